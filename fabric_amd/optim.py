"""Update rules of the fused step (fabric_amd/train_step.py) beyond the reference's plain SGD (train.py:55): momentum / Nesterov SGD,
Adam and AdamW with weight decay (train.py:56 is the reference's commented-out `optim.Adam(..., weight_decay=1e-2)`), following
torch 2.10's single-tensor formulas (include/bidate_hip.h: bdn_sgd_momentum_step, bdn_adam_step).

The step keeps its optimizer state in flat float32 buffers in the backward-order FlatLayout of the parameters (fabric_amd/parallel.py).
torch.optim keys the same state by the index of the parameter in ``model.parameters()``.  The conversions between the two
(``flat_to_torch`` / ``torch_to_flat``) are plain torch and run on any device, so they can be checked without a GPU.
"""
import math

import torch

KINDS = ('sgd', 'adam', 'adamw')
STATE_KEYS = {'sgd': ('momentum_buffer',), 'adam': ('exp_avg', 'exp_avg_sq')}


def _family(kind):
    return 'sgd' if kind == 'sgd' else 'adam'


class OptimConfig:
    """Validated hyperparameters of one update rule.  ``weight_decay=None`` is torch's default: 0 for sgd and adam, 1e-2 for adamw.
    Unsupported torch options (amsgrad, maximize) and settings torch itself rejects raise ValueError."""

    def __init__(self, kind='sgd', lr=1e-3, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=None, betas=(0.9, 0.999),
                 eps=1e-8, amsgrad=False, maximize=False):
        if kind not in KINDS:
            raise ValueError(f'optimizer {kind!r}: expected one of {KINDS}')
        if amsgrad:
            raise ValueError('amsgrad is not supported by the fused step')
        if maximize:
            raise ValueError('maximize is not supported by the fused step')
        if weight_decay is None:
            weight_decay = 1e-2 if kind == 'adamw' else 0.0
        for name, v in (('lr', lr), ('momentum', momentum), ('dampening', dampening), ('weight_decay', weight_decay), ('eps', eps)):
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f'invalid {name}: {v!r} (must be a finite number >= 0)')
        if kind == 'sgd':
            if nesterov and (momentum <= 0 or dampening != 0):
                raise ValueError('nesterov needs momentum > 0 and zero dampening')
        elif momentum != 0 or dampening != 0 or nesterov:
            raise ValueError(f'momentum / dampening / nesterov belong to sgd, not {kind}')
        betas = tuple(float(b) for b in betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'invalid betas {betas!r}: two values in [0, 1)')
        self.kind, self.lr = kind, float(lr)
        self.momentum, self.dampening, self.nesterov = float(momentum), float(dampening), bool(nesterov)
        self.weight_decay, self.betas, self.eps = float(weight_decay), betas, float(eps)

    @property
    def family(self):
        return _family(self.kind)

    @property
    def plain(self):
        """optim.SGD(lr) itself: the reference's rule, run by bdn_sgd_step with no state."""
        return self.kind == 'sgd' and self.momentum == 0 and self.weight_decay == 0

    def state_keys(self):
        """Names of the per-parameter state buffers this rule keeps (none for SGD without momentum)."""
        if self.kind == 'sgd':
            return STATE_KEYS['sgd'] if self.momentum != 0 else ()
        return STATE_KEYS['adam']

    def param_group(self, params):
        """torch 2.10's param_group for this rule (``params``: parameter indices)."""
        if self.kind == 'sgd':
            g = dict(lr=self.lr, momentum=self.momentum, dampening=self.dampening, weight_decay=self.weight_decay,
                     nesterov=self.nesterov, maximize=False, foreach=None, differentiable=False, fused=None)
        else:
            g = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, amsgrad=False, maximize=False,
                     foreach=None, capturable=False, differentiable=False, fused=None,
                     decoupled_weight_decay=self.kind == 'adamw')
        g['params'] = list(params)
        return g

    @classmethod
    def from_param_group(cls, group):
        """The rule a torch SGD / Adam / AdamW param_group describes ('betas' marks the Adam family, decoupled_weight_decay AdamW)."""
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


def flat_to_torch(cfg, layout, names, flat_state, step):
    """torch.optim's ``state_dict()`` of the flat state: ``flat_state`` maps cfg.state_keys() to flat buffers in ``layout``, ``names``
    lists the parameter names in ``model.parameters()`` order, ``step`` is the number of updates applied.  Every tensor is a copy.
    With no update applied yet the state is empty, as torch's is."""
    state = {}
    keys = cfg.state_keys()
    if keys and step > 0:
        for i, k in enumerate(names):
            s = {key: layout.view(flat_state[key], k).clone() for key in keys}
            if cfg.family == 'adam':
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
                             + (' and step' if cfg.family == 'adam' else ''))
        for key in keys:
            if tuple(s[key].shape) != shape:
                raise ValueError(f'parameter {pid} ({name}): {key} has shape {tuple(s[key].shape)}, the parameter {shape}')
            layout.view(flat[key], name).copy_(s[key].detach().to(device=device, dtype=torch.float32))
        if cfg.family == 'adam':
            st = s.get('step')
            if st is None:
                raise ValueError(f'parameter {pid} ({name}): no step in the Adam state')
            steps.add(float(st))
    if len(steps) > 1:
        raise ValueError(f'parameters were stepped different numbers of times ({sorted(steps)}): the flat state needs one count')
    if cfg.family == 'adam':
        step = int(steps.pop()) if steps else 0
    else:
        step = 1 if present else 0
    return cfg, flat, step
