"""Update rules of the fused step (fabric_amd/train_step.py) beyond the reference's plain SGD (train.py:55): momentum / Nesterov SGD,
Adam and AdamW with weight decay (train.py:56 is the reference's commented-out `optim.Adam(..., weight_decay=1e-2)`), following
torch 2.10's single-tensor formulas (include/bidate_hip.h: bdn_sgd_momentum_step, bdn_adam_step).

The step keeps its optimizer state in flat float32 buffers in the backward-order FlatLayout of the parameters (fabric_amd/parallel.py).
torch.optim keys the same state by the index of the parameter in ``model.parameters()``.  The conversions between the two
(``flat_to_torch`` / ``torch_to_flat``) are plain torch and run on any device, so they can be checked without a GPU.

Two layer-wise adaptive rules go beyond torch.optim, which ships neither: 'lamb' (You et al., ICLR 2020) and 'lars' (You, Gitman, Ginsburg
2017), include/bidate_hip.h: bdn_lamb_step, bdn_lars_step.  Each is a family of its own; its param_group is AdamW's / SGD's with a key
'layer_adapt' and the rule's own hyperparameters added, so that a saved state identifies its rule.
"""
import math

import torch

KINDS = ('sgd', 'adam', 'adamw', 'lamb', 'lars')
LAYERWISE = ('lamb', 'lars')
STATE_KEYS = {'sgd': ('momentum_buffer',), 'adam': ('exp_avg', 'exp_avg_sq'), 'lamb': ('exp_avg', 'exp_avg_sq'), 'lars': ('momentum_buffer',)}
_FAMILY = {'sgd': 'sgd', 'adam': 'adam', 'adamw': 'adam', 'lamb': 'lamb', 'lars': 'lars'}
_STEPPED = ('adam', 'lamb')          # families whose per-parameter state carries a step count
DEFAULT_BETAS = (0.9, 0.999)


def _family(kind):
    return _FAMILY[kind]


class OptimConfig:
    """Validated hyperparameters of one update rule.  ``weight_decay=None`` is torch's default: 0 for sgd and adam, 1e-2 for adamw.
    Unsupported torch options (amsgrad, maximize) and settings torch itself rejects raise ValueError.

    'lamb' takes betas, eps, weight_decay (decoupled, default 0) and refuses momentum / dampening / nesterov; 'lars' takes momentum,
    dampening, nesterov, weight_decay and refuses betas other than the default.  Both take max_trust (None or 0: no clamp on the trust
    ratio) and adapt_1d (False: tensors of ndim <= 1 -- biases, BatchNorm weight and bias -- take ratio 1, the usual practice); 'lars'
    also trust_coef and lars_eps.  For the other kinds these four keep their defaults and are not used."""

    def __init__(self, kind='sgd', lr=1e-3, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=None, betas=DEFAULT_BETAS,
                 eps=1e-8, amsgrad=False, maximize=False, trust_coef=1e-3, lars_eps=1e-8, max_trust=None, adapt_1d=False):
        if kind not in KINDS:
            raise ValueError(f'optimizer {kind!r}: expected one of {KINDS}')
        if amsgrad:
            raise ValueError('amsgrad is not supported by the fused step')
        if maximize:
            raise ValueError('maximize is not supported by the fused step')
        if weight_decay is None:
            weight_decay = 1e-2 if kind == 'adamw' else 0.0
        if max_trust is None:
            max_trust = 0.0
        for name, v in (('lr', lr), ('momentum', momentum), ('dampening', dampening), ('weight_decay', weight_decay), ('eps', eps),
                        ('trust_coef', trust_coef), ('lars_eps', lars_eps), ('max_trust', max_trust)):
            if isinstance(v, bool) and name in ('trust_coef', 'lars_eps', 'max_trust'):
                raise ValueError(f'invalid {name}: {v!r} (must be a finite number >= 0)')
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f'invalid {name}: {v!r} (must be a finite number >= 0)')
        if not isinstance(adapt_1d, (bool, int)):
            raise ValueError(f'invalid adapt_1d: {adapt_1d!r} (must be a bool)')
        if kind in ('sgd', 'lars'):
            if nesterov and (momentum <= 0 or dampening != 0):
                raise ValueError('nesterov needs momentum > 0 and zero dampening')
        elif momentum != 0 or dampening != 0 or nesterov:
            raise ValueError(f'momentum / dampening / nesterov belong to sgd, not {kind}')
        betas = tuple(float(b) for b in betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'invalid betas {betas!r}: two values in [0, 1)')
        if kind == 'lars' and betas != DEFAULT_BETAS:
            raise ValueError(f'betas belong to adam / adamw / lamb, not lars (got {betas!r})')
        if kind not in LAYERWISE and (trust_coef != 1e-3 or lars_eps != 1e-8 or max_trust != 0 or adapt_1d):
            raise ValueError(f'trust_coef / lars_eps / max_trust / adapt_1d belong to lamb and lars, not {kind}')
        if kind == 'lamb' and (trust_coef != 1e-3 or lars_eps != 1e-8):
            raise ValueError('trust_coef / lars_eps belong to lars, not lamb')
        self.kind, self.lr = kind, float(lr)
        self.momentum, self.dampening, self.nesterov = float(momentum), float(dampening), bool(nesterov)
        self.weight_decay, self.betas, self.eps = float(weight_decay), betas, float(eps)
        self.trust_coef, self.lars_eps, self.max_trust, self.adapt_1d = float(trust_coef), float(lars_eps), float(max_trust), bool(adapt_1d)

    @property
    def family(self):
        return _family(self.kind)

    @property
    def plain(self):
        """optim.SGD(lr) itself: the reference's rule, run by bdn_sgd_step with no state."""
        return self.kind == 'sgd' and self.momentum == 0 and self.weight_decay == 0

    def state_keys(self):
        """Names of the per-parameter state buffers this rule keeps (none for SGD without momentum)."""
        if self.kind in ('sgd', 'lars'):
            return STATE_KEYS[self.kind] if self.momentum != 0 else ()
        return STATE_KEYS[self.family]

    @property
    def stepped(self):
        """The per-parameter state carries a step count (Adam's families and LAMB)."""
        return self.family in _STEPPED

    def param_group(self, params):
        """torch 2.10's param_group for this rule (``params``: parameter indices)."""
        if self.kind in ('sgd', 'lars'):
            g = dict(lr=self.lr, momentum=self.momentum, dampening=self.dampening, weight_decay=self.weight_decay,
                     nesterov=self.nesterov, maximize=False, foreach=None, differentiable=False, fused=None)
        else:
            g = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, amsgrad=False, maximize=False,
                     foreach=None, capturable=False, differentiable=False, fused=None,
                     decoupled_weight_decay=self.kind in ('adamw', 'lamb'))
        if self.kind in LAYERWISE:
            g.update(layer_adapt=self.kind, max_trust=self.max_trust, adapt_1d=self.adapt_1d)
        if self.kind == 'lars':
            g.update(trust_coef=self.trust_coef, lars_eps=self.lars_eps)
        g['params'] = list(params)
        return g

    @classmethod
    def from_param_group(cls, group):
        """The rule a torch SGD / Adam / AdamW param_group describes ('betas' marks the Adam family, decoupled_weight_decay AdamW), or,
        with a key 'layer_adapt', the LAMB / LARS rule that param_group() wrote."""
        la = group.get('layer_adapt')
        if la is not None:
            if la not in LAYERWISE:
                raise ValueError(f"unrecognised layer_adapt {la!r} in the optimizer param_group: expected one of {LAYERWISE}")
            extra = dict(max_trust=group.get('max_trust', 0.0) or None, adapt_1d=group.get('adapt_1d', False),
                         amsgrad=group.get('amsgrad', False), maximize=group.get('maximize', False))
            if la == 'lamb':
                return cls('lamb', lr=group['lr'], weight_decay=group.get('weight_decay', 0.0), betas=group.get('betas', DEFAULT_BETAS),
                           eps=group.get('eps', 1e-8), **extra)
            return cls('lars', lr=group['lr'], momentum=group.get('momentum', 0.0), dampening=group.get('dampening', 0.0),
                       nesterov=group.get('nesterov', False), weight_decay=group.get('weight_decay', 0.0),
                       trust_coef=group.get('trust_coef', 1e-3), lars_eps=group.get('lars_eps', 1e-8), **extra)
        if 'betas' in group:
            kind = 'adamw' if group.get('decoupled_weight_decay', False) else 'adam'
            return cls(kind, lr=group['lr'], weight_decay=group.get('weight_decay', 0.0), betas=group['betas'],
                       eps=group.get('eps', 1e-8), amsgrad=group.get('amsgrad', False), maximize=group.get('maximize', False))
        if 'momentum' in group:
            return cls('sgd', lr=group['lr'], momentum=group['momentum'], dampening=group.get('dampening', 0.0),
                       nesterov=group.get('nesterov', False), weight_decay=group.get('weight_decay', 0.0),
                       maximize=group.get('maximize', False))
        raise ValueError(f'unrecognised optimizer param_group (keys {sorted(group)}): expected torch.optim SGD, Adam or AdamW')

    def __eq__(self, other):
        return isinstance(other, OptimConfig) and vars(self) == vars(other)

    def __repr__(self):
        return 'OptimConfig(' + ', '.join(f'{k}={v!r}' for k, v in vars(self).items()) + ')'


def check_accumulate(k):
    """The fused step's `accumulate`: an int >= 1 (bool is refused: it is an int to Python only)."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f'invalid accumulate: {k!r} (must be an integer >= 1)')
    return k


def check_max_grad_norm(x):
    """The fused step's `max_grad_norm`: None (no clipping, nothing measured), a number > 0, or float('inf') (measure only)."""
    if x is None:
        return None
    if isinstance(x, bool) or not isinstance(x, (int, float)) or math.isnan(x) or x <= 0:
        raise ValueError(f"invalid max_grad_norm: {x!r} (must be a number > 0, float('inf') to measure without clipping, or None)")
    return float(x)


def check_sam(rho=None, adaptive=False, eps=1e-12):
    """The fused step's sharpness-aware keywords -> (rho or None, adaptive, eps).  rho=None: off (the other two must then keep their
    defaults: they would shape a perturbation that is not made).  ValueError: rho not a finite number > 0, adaptive not a bool, eps not a
    finite number >= 0 (bools are refused as numbers: they are numbers to Python only)."""
    if not isinstance(adaptive, bool):
        raise ValueError(f'invalid sam_adaptive: {adaptive!r} (must be a bool)')
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or eps < 0:
        raise ValueError(f'invalid sam_eps: {eps!r} (must be a finite number >= 0)')
    if rho is None:
        if adaptive or eps != 1e-12:
            raise ValueError('sam_adaptive / sam_eps shape a perturbation that is not on: give sam_rho')
        return None, False, float(eps)
    if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not math.isfinite(rho) or rho <= 0:
        raise ValueError(f'invalid sam_rho: {rho!r} (must be a finite number > 0, or None)')
    return float(rho), adaptive, float(eps)


AVERAGES = ('ema', 'swa')


def check_ema(ema_decay=None, average='ema', ema_every=1, ema_start=0):
    """The fused step's weight-averaging keywords -> (on, decay or None, average, every, start).  The average is on when `ema_decay` is a
    number (average='ema': an exponential moving average, weight 1 - decay) or average='swa' (the equal-weight running mean, weight
    1 / (n_averaged + 1); it takes no decay).  ValueError: a decay outside [0, 1), ema_every < 1, ema_start < 0, an unknown average, or
    'swa' together with a decay (bools are refused everywhere: they are numbers to Python only)."""
    if average not in AVERAGES:
        raise ValueError(f'average {average!r}: expected one of {AVERAGES}')
    if ema_decay is not None:
        if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= ema_decay < 1.0:       # NaN fails both
            raise ValueError(f'invalid ema_decay: {ema_decay!r} (must be a number in [0, 1), or None)')
        if average == 'swa':
            raise ValueError(f"average='swa' is the equal-weight mean and takes no ema_decay (got {ema_decay!r})")
        ema_decay = float(ema_decay)
    if isinstance(ema_every, bool) or not isinstance(ema_every, int) or ema_every < 1:
        raise ValueError(f'invalid ema_every: {ema_every!r} (must be an integer >= 1)')
    if isinstance(ema_start, bool) or not isinstance(ema_start, int) or ema_start < 0:
        raise ValueError(f'invalid ema_start: {ema_start!r} (must be an integer >= 0)')
    return ema_decay is not None or average == 'swa', ema_decay, average, ema_every, ema_start


def average_weight(average, decay, n_averaged):
    """The lerp weight of the next averaging update, in double: 1 - decay (EMA) or 1 / (n_averaged + 1) (SWA), as
    torch.optim.swa_utils forms it; the kernels take it rounded to float32."""
    return 1.0 - decay if average == 'ema' else 1.0 / (n_averaged + 1)


def flat_to_torch(cfg, layout, names, flat_state, step):
    """torch.optim's ``state_dict()`` of the flat state: ``flat_state`` maps cfg.state_keys() to flat buffers in ``layout``, ``names``
    lists the parameter names in ``model.parameters()`` order, ``step`` is the number of updates applied.  Every tensor is a copy.
    With no update applied yet the state is empty, as torch's is."""
    state = {}
    keys = cfg.state_keys()
    if keys and step > 0:
        for i, k in enumerate(names):
            s = {key: layout.view(flat_state[key], k).clone() for key in keys}
            if cfg.stepped:
                s = {'step': torch.tensor(float(step), dtype=torch.float32), **s}
            state[i] = s
    return {'state': state, 'param_groups': [cfg.param_group(range(len(names)))]}


def torch_to_flat(sd, layout, names, device=None):
    """Inverse of flat_to_torch: (cfg, flat_state, step) from a torch SGD / Adam / AdamW ``state_dict()`` (or flat_to_torch's output).
    flat_state holds new zero-padded float32 buffers of ``layout.total`` elements on ``device``.  Raises ValueError on more than one
    param group, a parameter count or shape mismatch, or per-parameter state that is not uniform (present for some parameters only,
    or different step counts): the flat buffers hold one state for all parameters.  For SGD the returned step is 1 when momentum
    buffers are present (they hold a value) and 0 otherwise."""
    groups = sd['param_groups']
    if len(groups) != 1:
        raise ValueError(f'{len(groups)} param groups: the fused step has one set of hyperparameters')
    g = groups[0]
    cfg = OptimConfig.from_param_group(g)
    if len(g['params']) != len(names):
        raise ValueError(f'optimizer state covers {len(g["params"])} parameters, the model has {len(names)}')
    idx = {pid: j for j, pid in enumerate(g['params'])}
    states = sd['state']
    keys = cfg.state_keys()
    if device is None:
        device = next((v.device for s in states.values() for v in s.values() if torch.is_tensor(v) and v.dim() > 0), 'cpu')
    flat = {key: torch.zeros(layout.total, dtype=torch.float32, device=device) for key in keys}
    present = [pid for pid in g['params'] if states.get(pid)]
    if present and len(present) != len(names):
        raise ValueError(f'optimizer state for {len(present)} of {len(names)} parameters: the flat state needs all or none')
    if present and not keys:
        raise ValueError(f'optimizer state present, but {cfg.kind} with momentum {cfg.momentum} keeps none')
    steps = set()
    for pid in present:
        name = names[idx[pid]]
        s = states[pid]
        shape = layout.slices[name][2]
        if set(s) - {'step'} != set(keys):
            raise ValueError(f'parameter {pid} ({name}): state keys {sorted(s)}, expected {sorted(keys)}'
                             + (' and step' if cfg.stepped else ''))
        for key in keys:
            if tuple(s[key].shape) != shape:
                raise ValueError(f'parameter {pid} ({name}): {key} has shape {tuple(s[key].shape)}, the parameter {shape}')
            layout.view(flat[key], name).copy_(s[key].detach().to(device=device, dtype=torch.float32))
        if cfg.stepped:
            st = s.get('step')
            if st is None:
                raise ValueError(f'parameter {pid} ({name}): no step in the Adam state')
            steps.add(float(st))
    if len(steps) > 1:
        raise ValueError(f'parameters were stepped different numbers of times ({sorted(steps)}): the flat state needs one count')
    if cfg.stepped:
        step = int(steps.pop()) if steps else 0
    else:
        step = 1 if present else 0
    return cfg, flat, step


# ------------------------------------------------------------------ parameter groups and frozen parameters
MAX_GROUPS = 8            # include/bidate_hip.h: the per-group hyperparameters travel in the kernel arguments
FROZEN = -1               # the reserved group id of a frozen segment
GROUP_KEYS = ('lr', 'weight_decay')


def _number(name, v):
    if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
        raise ValueError(f'invalid {name}: {v!r} (must be a finite number >= 0)')
    return float(v)


class ParamGroups:
    """Validated parameter groups of the fused step over parameter NAMES (state-dict keys).

    ``names``: every parameter in ``model.parameters()`` order; ``groups``: a list of dicts ``{'params': [names], 'lr': ...,
    'weight_decay': ...}`` (a missing key takes cfg's value), or None for one group of every trainable parameter; ``frozen``: the
    names with requires_grad=False.  A frozen parameter may be listed in a group, as torch.optim allows (it keeps its place in the
    group's 'params' for the state exchange), but it is never updated and carries no state.  ``self.groups`` is a list of plain dicts
    that the step reads at every update, so ``groups[i]['lr'] = x`` works as it does on a torch optimizer.

    ValueError: more than MAX_GROUPS groups, an unknown name, a name listed twice, a trainable parameter in no group (torch would
    silently leave it untrained; here that is an error, never a silent freeze), or a per-group key other than lr / weight_decay whose
    value differs from the step's rule (momentum, dampening, nesterov, betas, eps are one per step)."""

    def __init__(self, cfg, names, groups=None, frozen=()):
        self.names = list(names)
        self.frozen = set(frozen)
        known = set(self.names)
        if self.frozen - known:
            raise ValueError(f'unknown frozen parameter(s) {sorted(self.frozen - known)}')
        if groups is None:
            groups = [{'params': [k for k in self.names if k not in self.frozen]}]
        groups = list(groups)
        if len(groups) > MAX_GROUPS:
            raise ValueError(f'{len(groups)} param groups: the fused step takes at most {MAX_GROUPS}')
        rule = cfg.param_group([])
        self.groups, self.group_of = [], {}
        for j, g in enumerate(groups):
            if 'params' not in g:
                raise ValueError(f"param group {j} has no 'params'")
            out = {'params': list(g['params']), 'lr': cfg.lr, 'weight_decay': cfg.weight_decay}
            for key, v in g.items():
                if key == 'params':
                    continue
                if key in GROUP_KEYS:
                    out[key] = _number(key, v)
                elif key not in rule:
                    raise ValueError(f'param group {j}: unknown key {key!r}')
                elif (tuple(v) if key == 'betas' else v) != rule[key]:
                    raise ValueError(f'param group {j}: per-group {key} = {v!r} differs from the step\'s {rule[key]!r}; only '
                                     f'lr and weight_decay may differ between groups')
            for k in out['params']:
                if k not in known:
                    raise ValueError(f'param group {j}: unknown parameter {k!r}')
                if k in self.group_of:
                    raise ValueError(f'parameter {k!r} appears in more than one param group (or twice in one)')
                self.group_of[k] = j
            self.groups.append(out)
        left = [k for k in self.names if k not in self.frozen and k not in self.group_of]
        if left:
            raise ValueError(f'{len(left)} trainable parameter(s) in no param group (first: {left[0]!r}): list them, or set '
                             f'requires_grad=False to freeze them')

    def trainable(self):
        """Names that are updated, in model.parameters() order."""
        return [k for k in self.names if k not in self.frozen]

    def group_id(self, name):
        return FROZEN if name in self.frozen else self.group_of[name]

    def hyper(self, key):
        """The current per-group values of 'lr' or 'weight_decay' (read from the live dicts)."""
        return [_number(key, g[key]) for g in self.groups]


def segment_table(layout, groups):
    """(ends, ids) of bdn_*_step_grouped's segment table for ``layout`` (FlatLayout: every tensor padded to a float4) and ``groups``
    (ParamGroups): the sorted segment ends in float4 units and the group id of each segment, FROZEN for frozen tensors.  The segments
    tile [0, layout.total / 4); adjacent tensors of one group share a segment."""
    ends, ids = [], []
    for i, k in enumerate(layout.order):
        end = (layout.slices[layout.order[i + 1]][0] if i + 1 < len(layout.order) else layout.total) // 4
        gid = groups.group_id(k)
        if ids and ids[-1] == gid:
            ends[-1] = end
        else:
            ends.append(end)
            ids.append(gid)
    return ends, ids


def tensor_table(layout, groups, adapt_1d=False):
    """(ends, lens, ids, adapt) of bdn_lamb_step's / bdn_lars_step's per-tensor table for ``layout`` and ``groups`` (ParamGroups): four int32
    torch tensors (CPU) with one entry per tensor in layout order -- the tensor's end in float4 units (they tile [0, layout.total / 4)),
    its real element count, its group id (FROZEN for a frozen tensor) and its adapt flag: 1 when the trust ratio applies, 0 (ratio 1)
    for a tensor of ndim <= 1 unless ``adapt_1d``.  ``ends`` holds uint32 values in int32 storage, as the segment table does."""
    ends, lens, ids, adapt = [], [], [], []
    for i, k in enumerate(layout.order):
        off, n, shape = layout.slices[k]
        ends.append((layout.slices[layout.order[i + 1]][0] if i + 1 < len(layout.order) else layout.total) // 4)
        lens.append(n)
        ids.append(groups.group_id(k))
        adapt.append(int(bool(adapt_1d) or len(shape) > 1))
    as32 = lambda v: torch.tensor(v, dtype=torch.int64).to(torch.int32)
    return as32(ends), as32(lens), as32(ids), as32(adapt)


def groups_to_torch(cfg, groups, layout, flat_state, step):
    """torch.optim's ``state_dict()`` of a grouped step: what ``torch.optim.{SGD,Adam,AdamW}`` built with the same param groups holds.
    One 'param_groups' entry per group with torch 2.10's keys; a parameter is identified by its index in ``model.parameters()``
    (torch's load_state_dict matches the entries of a group by position, so any optimizer whose groups list the same parameters in
    the same order loads it).  No state entry for a frozen parameter, as torch keeps none for a parameter whose grad is None.  Every
    tensor is a copy."""
    index = {k: i for i, k in enumerate(groups.names)}
    state = {}
    keys = cfg.state_keys()
    if keys and step > 0:
        for k in groups.trainable():
            s = {key: layout.view(flat_state[key], k).clone() for key in keys}
            if cfg.stepped:
                s = {'step': torch.tensor(float(step), dtype=torch.float32), **s}
            state[index[k]] = s
    out = []
    for g in groups.groups:
        pg = cfg.param_group([index[k] for k in g['params']])
        pg['lr'], pg['weight_decay'] = float(g['lr']), float(g['weight_decay'])
        out.append(pg)
    return {'state': state, 'param_groups': out}


def torch_to_groups(sd, groups, layout, device=None):
    """Inverse of groups_to_torch: (cfg, per-group [{'lr', 'weight_decay'}] or None, flat_state, step) from the ``state_dict()`` of a torch
    SGD / Adam / AdamW built with the same param groups as ``groups`` (ParamGroups), or groups_to_torch's output.  As in torch, the
    saved entries are matched to the step's by POSITION (k-th parameter of the j-th group), whatever ids the file uses, and the saved
    hyperparameters replace the step's.  ValueError: another number of groups or of parameters in one, hyperparameters other than lr
    / weight_decay that differ between the saved groups, shapes that do not fit, state for only some of the trainable parameters, or
    different step counts.  State saved for a parameter that is frozen here is dropped."""
    saved = sd['param_groups']
    mine = groups.groups
    if len(saved) == 1 and len(saved[0]['params']) == len(groups.names) and [len(g['params']) for g in mine] != [len(groups.names)]:
        # an ungrouped state over every parameter in model.parameters() order (flat_to_torch's output): the state is taken by name; one
        # saved set of hyperparameters cannot describe the groups, which keep theirs (None is returned in their place)
        mine = None
    elif len(saved) != len(mine):
        raise ValueError(f'optimizer state has {len(saved)} param groups, the step has {len(mine)}')
    cfgs = [OptimConfig.from_param_group(g) for g in saved]
    cfg = cfgs[0]
    rule = {k: v for k, v in cfg.param_group([]).items() if k not in GROUP_KEYS + ('params',)}
    name_of = {}
    for j, (g, c) in enumerate(zip(saved, cfgs)):
        other = {k: v for k, v in c.param_group([]).items() if k not in GROUP_KEYS + ('params',)}
        if other != rule:
            diff = sorted(k for k in rule if rule[k] != other[k])
            raise ValueError(f'param group {j} differs from group 0 in {diff}: only lr and weight_decay may differ between groups')
        listed = groups.names if mine is None else mine[j]['params']
        if len(g['params']) != len(listed):
            raise ValueError(f'param group {j}: the optimizer state covers {len(g["params"])} parameters, the step\'s group {len(listed)}')
        for pid, k in zip(g['params'], listed):
            name_of[pid] = k
    states = sd['state']
    keys = cfg.state_keys()
    if device is None:
        device = next((v.device for s in states.values() for v in s.values() if torch.is_tensor(v) and v.dim() > 0), 'cpu')
    flat = {key: torch.zeros(layout.total, dtype=torch.float32, device=device) for key in keys}
    train = set(groups.trainable())
    present = [pid for pid, k in name_of.items() if k in train and states.get(pid)]
    n_train = sum(1 for k in name_of.values() if k in train)
    if present and len(present) != n_train:
        raise ValueError(f'optimizer state for {len(present)} of {n_train} trainable parameters: the flat state needs all or none')
    if present and not keys:
        raise ValueError(f'optimizer state present, but {cfg.kind} with momentum {cfg.momentum} keeps none')
    steps = set()
    for pid in present:
        name, s = name_of[pid], states[pid]
        shape = layout.slices[name][2]
        if set(s) - {'step'} != set(keys):
            raise ValueError(f'parameter {pid} ({name}): state keys {sorted(s)}, expected {sorted(keys)}'
                             + (' and step' if cfg.stepped else ''))
        for key in keys:
            if tuple(s[key].shape) != shape:
                raise ValueError(f'parameter {pid} ({name}): {key} has shape {tuple(s[key].shape)}, the parameter {shape}')
            layout.view(flat[key], name).copy_(s[key].detach().to(device=device, dtype=torch.float32))
        if cfg.stepped:
            if s.get('step') is None:
                raise ValueError(f'parameter {pid} ({name}): no step in the Adam state')
            steps.add(float(s['step']))
    if len(steps) > 1:
        raise ValueError(f'parameters were stepped different numbers of times ({sorted(steps)}): the flat state needs one count')
    if cfg.stepped:
        step = int(steps.pop()) if steps else 0
    else:
        step = 1 if present else 0
    return cfg, None if mine is None else [{'lr': c.lr, 'weight_decay': c.weight_decay} for c in cfgs], flat, step


# ------------------------------------------------------------------ averaged weights in torch.optim.swa_utils.AveragedModel's format
AVG_COUNT = 'n_averaged'
AVG_PREFIX = 'module.'


def avg_to_torch(layout, keys, flat_avg, buffers, n_averaged):
    """``AveragedModel(model).state_dict()`` of the flat average: 'n_averaged' (int64 scalar, on the CPU, where AveragedModel(model)
    keeps its count) and 'module.<key>' for every key of ``keys`` (the model's state_dict() order) -- a view of ``flat_avg`` in
    ``layout`` for a parameter, ``buffers[key]`` for a buffer.  Every tensor is a copy."""
    out = {AVG_COUNT: torch.tensor(int(n_averaged), dtype=torch.int64)}
    for k in keys:
        out[AVG_PREFIX + k] = (layout.view(flat_avg, k) if k in layout.slices else buffers[k]).clone()
    return out


def torch_to_avg(sd, layout, keys, buffers):
    """Inverse of avg_to_torch, checked before anything is written: (n_averaged, {key: tensor of sd}) for every key of ``keys``.
    ``buffers``: {key: a tensor of the expected shape} for the keys that are not parameters.  ValueError: no integer scalar
    'n_averaged', missing or unexpected keys, a wrong shape."""
    n = sd.get(AVG_COUNT)
    if not (torch.is_tensor(n) and n.numel() == 1 and not n.dtype.is_floating_point and n.dtype != torch.bool) and \
            not (isinstance(n, int) and not isinstance(n, bool)):
        raise ValueError(f"averaged state: {AVG_COUNT!r} must be an integer scalar (AveragedModel's update count)")
    if int(n) < 0:
        raise ValueError(f'averaged state: {AVG_COUNT} = {int(n)}')
    want = [AVG_PREFIX + k for k in keys]
    missing = [k for k in want if k not in sd]
    known = set(want)
    extra = [k for k in sd if k != AVG_COUNT and k not in known]
    if missing or extra:
        raise ValueError(f'averaged state: {len(missing)} missing key(s) {missing[:3]}, {len(extra)} unexpected key(s) {extra[:3]}')
    out = {}
    for k in keys:
        shape = layout.slices[k][2] if k in layout.slices else tuple(buffers[k].shape)
        v = sd[AVG_PREFIX + k]
        if not torch.is_tensor(v) or tuple(v.shape) != tuple(shape):
            raise ValueError(f'averaged state: {k} has shape {tuple(getattr(v, "shape", ()))}, the model {tuple(shape)}')
        out[k] = v.detach()
    return int(n), out


def is_averaged_state(sd):
    """An AveragedModel state dict: every key 'module.'-prefixed except an integer scalar 'n_averaged'."""
    if not isinstance(sd, dict) or AVG_COUNT not in sd or len(sd) < 2:
        return False
    n = sd[AVG_COUNT]
    if not (torch.is_tensor(n) and n.numel() == 1 and not n.dtype.is_floating_point and n.dtype != torch.bool):
        return False
    return all(isinstance(k, str) and k.startswith(AVG_PREFIX) for k in sd if k != AVG_COUNT)
