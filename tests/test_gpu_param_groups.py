"""-m gpu: parameter groups and frozen parameters in the fused step (include/bidate_hip.h bdn_*_step_grouped; fabric_amd/optim.py;
TrainStep(param_groups=, bn=)).

The grouped kernels against the float64 restatement applied segment by segment (tests/param_groups_ref.py, pinned against CPU torch.optim
in tests/test_param_groups_cpu.py) and, with one group, bit for bit against the ungrouped kernels; frozen segments untouched; TrainStep
with groups against CUDA torch.optim with the same groups; a frozen encoder (no update, the trainable gradients bit-identical to a full
backward's, no encoder launches in backward); BatchNorm on running statistics against the autograd route; the default step on today's
entry points; data parallel; train.py's fine-tuning flags."""
import os
import subprocess
import sys

import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.optim import FROZEN
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.metrics import TverskyLoss
from oracle import filler
from tests import optim_ref as R
from tests.param_groups_ref import grouped_reference
from tests import guard
from tests.guard import guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
ENCODER = ('inc.', 'down1.', 'down2.', 'down3.', 'down4.')
_LR = 0.01


# ---------------------------------------------------------------- kernels
def _table(n, n_groups, frozen_every=0, seed=0):
    """A segment table over n floats (n % 4 == 0): cuts at random float4 boundaries, group ids cycling through the groups, every
    `frozen_every`-th segment frozen.  -> (ends, ids) in float4 units, and the same as [(start, stop, id)] in elements."""
    n4 = n // 4
    gen = torch.Generator().manual_seed(seed)
    n_seg = min(n4, max(n_groups, 11))
    cuts = sorted(set((torch.randperm(n4 - 1, generator=gen)[:n_seg - 1] + 1).tolist())) if n4 > 1 else []
    ends = cuts + [n4]
    ids = []
    for j in range(len(ends)):
        gid = FROZEN if frozen_every and j % frozen_every == 1 else j % n_groups
        if ids and ids[-1] == gid:                          # neighbours of one group would be merged by the host: keep them distinct
            gid = (gid + 1) % n_groups if n_groups > 1 else gid
        ids.append(gid)
    starts = [0] + ends[:-1]
    return ends, ids, [(4 * a, 4 * b, g) for a, b, g in zip(starts, ends, ids)]


def _dev_table(ends, ids):
    return (guard.guard(torch.tensor(ends, dtype=torch.int64).to(torch.int32), dev), guard.guard(torch.tensor(ids, dtype=torch.int32), dev))


def _call_grouped(kind, rule, p, g, state, tab, hyper, gs, step):
    st = _lib.stream_ptr()
    ends, ids = tab
    lr, wd = _lib.floats([h[0] for h in hyper]), _lib.floats([h[1] for h in hyper])
    t = (ends.data_ptr(), ids.data_ptr(), ends.numel(), len(hyper))
    if kind == 'sgd_plain':
        _lib.call('bdn_sgd_step_grouped', p.data_ptr(), g.data_ptr(), *t, lr, gs, p.numel(), st)
    elif kind == 'sgd':
        _lib.call('bdn_sgd_momentum_step_grouped', p.data_ptr(), g.data_ptr(), _lib.ptr(state.get('buf')), *t, lr, wd, gs,
                  rule.get('momentum', 0.0), rule.get('dampening', 0.0), int(rule.get('nesterov', False)), int(step == 1), p.numel(), st)
    else:
        b1, b2 = rule.get('betas', (0.9, 0.999))
        _lib.call('bdn_adam_step_grouped', p.data_ptr(), g.data_ptr(), state['m'].data_ptr(), state['v'].data_ptr(), *t, lr, wd, gs,
                  b1, b2, 1e-8, int(kind == 'adamw'), step, p.numel(), st)


_KERNEL_CASES = [
    ('sgd_plain', 'sgd_plain', dict(), 0.5),
    ('sgd_wd_only', 'sgd', dict(), 1.0),
    ('sgd_m', 'sgd', dict(momentum=0.9), 1.0),
    ('sgd_nesterov_damp0', 'sgd', dict(momentum=0.9, nesterov=True), 0.5),
    ('sgd_m_damp', 'sgd', dict(momentum=0.8, dampening=0.1), 1.0),
    ('adam', 'adam', dict(), 1.0),
    ('adamw', 'adamw', dict(betas=(0.8, 0.99)), 0.5),
]
_HYPER = [(0.01, 1e-2), (0.001, 0.0), (0.02, 1e-3), (0.005, 5e-2), (0.01, 0.0), (0.03, 1e-2), (0.002, 1e-4), (0.015, 2e-2)]


def _state(kind, rule, n, fill=0.0):
    if kind in ('adam', 'adamw'):
        return {'m': guard.full((n,), fill, device=dev), 'v': guard.full((n,), abs(fill), device=dev)}
    if rule.get('momentum', 0.0):
        return {'buf': guard.full((n,), float('nan'), device=dev)}           # the first step must not read it
    return {}


@pytest.mark.parametrize('n', [4, 1028, 4_000_004])
@pytest.mark.parametrize('n_groups', [1, 2, 8])
@pytest.mark.parametrize('name,kind,rule,gs', _KERNEL_CASES, ids=[c[0] for c in _KERNEL_CASES])
@guarded
def test_grouped_kernel_matches_float64_restatement(name, kind, rule, gs, n_groups, n):
    """Three steps on sizes that are no multiple of a block's 1024 vectors, 1 / 2 / 8 groups with their own lr and weight decay, some
    segments frozen: every element within R.ULPS of the restatement (frozen ones exactly as they were), from the kernel's own inputs."""
    hyper = _HYPER[:n_groups]
    if kind == 'sgd_plain':
        hyper = [(lr, 0.0) for lr, _ in hyper]
    ends, ids, segs = _table(n, n_groups, frozen_every=4, seed=n + n_groups)
    tab = _dev_table(ends, ids)
    gen = torch.Generator(device='cpu').manual_seed(n * 31 + len(name))
    p = guard.guard(torch.randn(n, generator=gen), dev)
    p[::7] *= 1e-3
    grads = [guard.guard(torch.randn(n, generator=gen) * (0.3 + it), dev) for it in range(3)]
    grads[1][::5] = 0.0
    state = _state(kind, rule, n)
    rkind = 'sgd' if kind == 'sgd_plain' else kind
    for it, g in enumerate(grads):
        p_in, s_in = p.clone(), {k: v.clone() for k, v in state.items()}
        _call_grouped(kind, rule, p, g, state, tab, hyper, gs, it + 1)
        torch.cuda.synchronize()
        if it == 0 and 'buf' in s_in:
            s_in['buf'] = torch.zeros_like(s_in['buf'])                       # NaN placeholders: frozen segments keep them, checked below
            frozen_mask = torch.zeros(n, dtype=torch.bool)
            for a, b, gid in segs:
                frozen_mask[a:b] = gid == FROZEN
            assert bool(torch.isnan(state['buf'].cpu()[frozen_mask]).all()) and not bool(torch.isnan(state['buf'].cpu()[~frozen_mask]).any())
            state['buf'][frozen_mask.to(dev)] = 0.0
        ref = grouped_reference(rkind, rule, segs, hyper, p_in.cpu(), g.cpu(), {k: v.cpu() for k, v in s_in.items()}, it + 1, gs)
        R.check(p, *ref['p'], f'{name} groups={n_groups} n={n} step {it} params')
        for key in state:
            R.check(state[key], *ref[key], f'{name} groups={n_groups} n={n} step {it} {key}')
        assert bool((p != p_in).any()), 'the step changed nothing'


@guarded
def test_nine_groups_are_refused():
    n = 64
    p, g, m, v = (guard.zeros(n, device=dev) for _ in range(4))
    tab = _dev_table([16], [0])
    nine = [(0.01, 0.0)] * 9
    for kind, rule in (('sgd_plain', {}), ('sgd', dict(momentum=0.9)), ('adam', {})):
        with pytest.raises(RuntimeError, match='9 groups'):
            _call_grouped(kind, rule, p, g, {'buf': m, 'm': m, 'v': v}, tab, nine, 1.0, 1)


@pytest.mark.parametrize('n', [1028, 13_401_156])
@guarded
def test_one_group_gives_the_bits_of_the_ungrouped_kernels(n):
    """One group over the whole buffer: the same device functions on the same inputs, so equality, not a tolerance."""
    st = _lib.stream_ptr()
    gen = torch.Generator(device='cpu').manual_seed(n)
    p0 = guard.guard(torch.randn(n, generator=gen), dev)
    grads = [guard.guard(torch.randn(n, generator=gen) * (0.3 + it), dev) for it in range(3)]
    tab = _dev_table([n // 4], [0])
    lr, wd, gs = 0.013, 1e-2, 0.5

    def run(grouped, kind, rule):
        p = guard.clone(p0)
        state = _state(kind, rule, n)
        for it, g in enumerate(grads):
            if grouped:
                _call_grouped(kind, rule, p, g, state, tab, [(lr, 0.0 if kind == 'sgd_plain' else wd)], gs, it + 1)
            elif kind == 'sgd_plain':
                _lib.call('bdn_sgd_step', p.data_ptr(), g.data_ptr(), lr, gs, n, st)
            elif kind == 'sgd':
                _lib.call('bdn_sgd_momentum_step', p.data_ptr(), g.data_ptr(), _lib.ptr(state.get('buf')), lr, gs, rule.get('momentum', 0.0),
                          rule.get('dampening', 0.0), wd, int(rule.get('nesterov', False)), int(it == 0), n, st)
            else:
                _lib.call('bdn_adam_step', p.data_ptr(), g.data_ptr(), state['m'].data_ptr(), state['v'].data_ptr(), lr, gs, 0.9, 0.999,
                          1e-8, wd, int(kind == 'adamw'), it + 1, n, st)
        torch.cuda.synchronize()
        return p, state

    for kind, rule in (('sgd_plain', {}), ('sgd', {}), ('sgd', dict(momentum=0.9)), ('sgd', dict(momentum=0.9, nesterov=True)),
                       ('sgd', dict(momentum=0.8, dampening=0.1)), ('adam', {}), ('adamw', {})):
        (pa, sa), (pb, sb) = run(False, kind, rule), run(True, kind, rule)
        assert torch.equal(pa, pb), (kind, rule, float((pa - pb).abs().max()))
        assert all(torch.equal(sa[k], sb[k]) for k in sa), (kind, rule)
        assert not torch.equal(pa, p0)


@pytest.mark.parametrize('kind,rule', [('sgd_plain', {}), ('sgd', dict(momentum=0.9)), ('adamw', {})], ids=['sgd', 'sgd_momentum', 'adamw'])
@guarded
def test_frozen_segments_are_neither_read_nor_written(kind, rule):
    """Frozen segments: parameters and state bit-identical after three steps, with their gradients NaN (a read would spread it) and,
    for the state, NaN placeholders of their own."""
    n = 300_004
    ends, ids, segs = _table(n, 3, frozen_every=3, seed=5)
    tab = _dev_table(ends, ids)
    mask = torch.zeros(n, dtype=torch.bool)
    for a, b, gid in segs:
        mask[a:b] = gid == FROZEN
    mask = mask.to(dev)
    assert bool(mask.any()) and not bool(mask.all())
    gen = torch.Generator(device='cpu').manual_seed(1)
    p = guard.guard(torch.randn(n, generator=gen), dev)
    state = _state(kind, rule, n)
    for t in state.values():
        t[~mask] = 0.0
        t[mask] = float('nan')
    p0, s0 = p.clone(), {k: v.clone() for k, v in state.items()}
    hyper = [(0.01, 0.0), (0.02, 0.0), (0.03, 0.0)] if kind == 'sgd_plain' else _HYPER[:3]
    for it in range(3):
        g = guard.guard(torch.randn(n, generator=gen), dev)
        g[mask] = float('nan')
        _call_grouped(kind, rule, p, g, state, tab, hyper, 1.0, it + 1)
    torch.cuda.synchronize()
    assert torch.equal(p[mask], p0[mask]) and not bool(torch.isnan(p).any())
    assert float((p[~mask] != p0[~mask]).float().mean()) > 0.9
    for k in state:
        assert bool(torch.isnan(state[k][mask]).all()) and not bool(torch.isnan(state[k][~mask]).any()), k


# ---------------------------------------------------------------- TrainStep with groups against CUDA torch.optim with the same groups
def _inputs(b=4, c=3, s=32, seed=3):
    return tuple(torch.from_numpy(v).to(dev) for v in filler.make_inputs(b, c, s, seed=seed))


_RULES = [
    ('sgd_momentum', dict(optimizer='sgd', momentum=0.9), lambda gs, lr: torch.optim.SGD(gs, lr=lr, momentum=0.9, foreach=False)),
    ('adamw', dict(optimizer='adamw'), lambda gs, lr: torch.optim.AdamW(gs, lr=lr, foreach=False)),
]


def _magnitude(opt, group, p, g, lr, it):
    s = opt.state.get(p, {})
    if 'betas' in group:
        return R.adam(p.detach(), g, s.get('exp_avg', torch.zeros_like(p)), s.get('exp_avg_sq', torch.zeros_like(p)), it + 1, group['lr'],
                      1.0, group['betas'], group['eps'], group['weight_decay'], group['decoupled_weight_decay'])[3]
    return R.sgd(p.detach(), g, s.get('momentum_buffer'), group['lr'], 1.0, group['momentum'], group['dampening'], group['weight_decay'],
                 group['nesterov'], first='momentum_buffer' not in s)[2]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('name,kw,make', _RULES, ids=[r[0] for r in _RULES])
def test_grouped_train_step_matches_torch_optim_on_its_own_gradients(name, kw, make, prec):
    """As test_train_step_matches_torch_optim_on_its_own_gradients, and with its bound (twice the kernel bound), for two groups:
    {weights: weight decay 1e-2} / {norms and biases: no decay, lr x 0.1}.  The second group's lr is changed through
    step.param_groups after the second step, as a scheduler would."""
    lr = 5e-3
    model = filler.fill_module(BiDateNet(3, 2, precision=prec)).to(dev).train()
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    w = [k for k, p in named if p.dim() > 1]
    nb = [k for k, p in named if p.dim() == 1]
    ts = TrainStep(model, lr=lr, param_groups=[{'params': w, 'weight_decay': 1e-2},
                                               {'params': [dict(named)[k] for k in nb], 'weight_decay': 0.0, 'lr': lr * 0.1}], **kw)
    assert [g['params'] for g in ts.param_groups] == [w, nb]
    q = {k: torch.nn.Parameter(p.detach().clone()) for k, p in named}
    opt = make([{'params': [q[k] for k in w], 'weight_decay': 1e-2}, {'params': [q[k] for k in nb], 'weight_decay': 0.0, 'lr': lr * 0.1}], lr)
    x1, x2, lbl = _inputs()
    for it in range(4):
        if it == 2:
            ts.param_groups[1]['lr'] = opt.param_groups[1]['lr'] = lr * 0.05
        with torch.no_grad():
            for k, p in named:
                q[k].copy_(p)
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        mags = {}
        for group, ks in zip(opt.param_groups, (w, nb)):
            for k in ks:
                q[k].grad = ts.grads[k].clone()
                mags[k] = _magnitude(opt, group, q[k], q[k].grad, lr, it)
        opt.step()
        for k, p in named:
            R.check(p, q[k].detach(), mags[k], f'{name} {prec} step {it} {k}', ulps=2 * R.ULPS)
    assert ts.opt_step == 4
    sd = ts.optimizer_state_dict()
    assert len(sd['param_groups']) == 2 and sd['param_groups'][1]['lr'] == lr * 0.05 and sd['param_groups'][1]['weight_decay'] == 0.0
    fresh = make([{'params': [q[k] for k in w]}, {'params': [q[k] for k in nb]}], 1.0)
    fresh.load_state_dict(sd)                                   # loads into torch.optim built with the same groups
    for k in names:
        for key, v in opt.state[q[k]].items():
            got = fresh.state[q[k]][key]
            assert float(got) == float(v) == 4.0 if key == 'step' else torch.allclose(got, v, rtol=1e-4, atol=1e-7), (k, key)
    ts.load_optimizer_state_dict(opt.state_dict())              # and torch's own state comes back in
    assert ts.opt_step == (4 if 'betas' in opt.param_groups[0] else 1)      # SGD's state carries no count: 1 = the buffers hold a value
    assert ts.param_groups[0]['weight_decay'] == 1e-2 and ts.param_groups[1]['lr'] == lr * 0.05


# ---------------------------------------------------------------- a frozen encoder
def _spy():
    calls = []
    orig = _lib.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    return calls, orig, spy


@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
def test_frozen_encoder_is_not_updated_and_launches_nothing_in_backward(prec):
    """Encoder frozen, AdamW with weight decay, 3 steps: every frozen tensor keeps its bits; at each step the trainable tensors'
    gradients are bit-identical to those of a full backward from the same weights and batch (same kernels, order and data); backward
    holds no bdn_enc_skip_bwd and only the decoder's weight- and data-gradient launches, the forward phase is the full step's."""
    x1, x2, lbl = _inputs(c=13, seed=5)
    model = filler.fill_module(BiDateNet(13, 2, precision=prec)).to(dev).train()
    for k, p in model.named_parameters():
        p.requires_grad_(not k.startswith(ENCODER))
    named = list(model.named_parameters())
    trainable = [k for k, p in named if p.requires_grad]
    ts = TrainStep(model, lr=1e-2, optimizer='adamw', weight_decay=5e-2, param_groups=[{'params': trainable}])
    full_model = filler.fill_module(BiDateNet(13, 2, precision=prec)).to(dev).train()
    full = TrainStep(full_model, lr=0.0)                        # lr 0: gradients only, its weights are set from the other model
    start = {k: p.detach().clone() for k, p in named}
    profiles = {}
    for it in range(3):
        full.flat_params.copy_(ts.flat_params)
        for k, v in model.state_dict().items():
            if 'running' in k or 'num_batches' in k:
                full_model.state_dict()[k].copy_(v)
        full_model.engine().invalidate_weights()
        for which, step in (('full', full), ('frozen', ts)):
            _lib.PROFILE = []
            try:
                step.step(x1, x2, lbl)
                torch.cuda.synchronize()
                profiles[which] = [(n, ph) for n, ph, *_ in _lib.PROFILE]
            finally:
                _lib.PROFILE = None
        for k in trainable:
            assert torch.equal(ts.grads[k], full.grads[k]), (it, k, float((ts.grads[k] - full.grads[k]).abs().max()))
    for k, p in named:
        if k.startswith(ENCODER):
            assert torch.equal(p.detach(), start[k]), k
        elif p.dim() > 1:
            assert not torch.equal(p.detach(), start[k]), k
    sd = ts.optimizer_state_dict()
    index = {k: i for i, (k, _) in enumerate(named)}
    assert set(sd['state']) == {index[k] for k in trainable}
    count = lambda prof, phase, *names: sum(1 for n, ph in prof if ph == phase and n in names)      # noqa: E731
    fz, fu = profiles['frozen'], profiles['full']
    assert [n for n, ph in fz if ph == 'fwd'] == [n for n, ph in fu if ph == 'fwd']
    wgrads = ('bdn_conv3x3_wgrad_ex', 'bdn_conv3x3_wgrad_bnbwd', 'bdn_conv3x3_wgrad')
    dgrads = ('bdn_conv3x3', 'bdn_conv3x3_dgrad_bs', 'bdn_conv3x3_dgrad_bb', 'bdn_conv3x3_x3src')
    assert count(fu, 'bwd', 'bdn_enc_skip_bwd') == 5 and count(fz, 'bwd', 'bdn_enc_skip_bwd') == 0
    assert count(fu, 'bwd', *wgrads) >= 18 and count(fz, 'bwd', 'bdn_conv3x3_wgrad_bnbwd') == 0
    assert count(fz, 'bwd', *wgrads) * 18 == count(fu, 'bwd', *wgrads) * 8, 'the 8 decoder layers of 18'
    assert count(fu, 'bwd', *dgrads) == 17 and count(fz, 'bwd', *dgrads) == 7, 'd4b ... d1b: d1a, the last trainable layer, has none'
    assert count(fz, 'bwd', 'bdn_upsample2x_bwd', 'bdn_upsample2x_bwd_bs') == 3


# ---------------------------------------------------------------- BatchNorm on running statistics
@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
def test_frozen_bn_step_matches_the_autograd_route(prec):
    """bn='frozen': BatchNorm buffers untouched after 3 steps; each step's gradients bit-identical to the autograd route's on an
    eval-mode module (the same engine.backward(bn_mode='running') on the same recomputed forward), conv biases included.

    The two routes differ in ONE launch, which is why the loss gradient is handed over instead of formed from `auto`'s own output: an
    eval-mode module's forward is the eval schedule (_forward_eval: BatchNorm folded into the convolutions), the fused step's loss sees
    the training-layout forward on the running statistics (forward(frozen=True), the one backward recomputes in both routes).  Their
    logits differ (MI355X, this input: up to 1.8e-4 in fp32, 1.1 in bf16), so the loss gradient differs before backward starts and the
    first weight gradient by 2e-7 (fp32) / 1.4e-3 (bf16).  On the SAME logits torch's TverskyLoss autograd and bdn_tversky give
    bit-identical loss gradients (the fused step's gradients below come from bdn_tversky's, the other route's from torch's), and
    from the same loss gradient every parameter gradient is bit-identical."""
    x1, x2, lbl = _inputs(c=13, seed=7)
    model = filler.fill_module(BiDateNet(13, 2, precision=prec)).to(dev).train()
    auto = filler.fill_module(BiDateNet(13, 2, precision=prec)).to(dev).eval()
    ts = TrainStep(model, lr=1e-3, optimizer='sgd', momentum=0.9, bn='frozen')
    assert ts.param_groups is None
    buffers = {k: v.clone() for k, v in model.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}
    assert len(buffers) == 54
    crit = TverskyLoss(alpha=0.1, beta=0.9)
    for it in range(3):
        with torch.no_grad():
            for (k, p), (_, a) in zip(model.named_parameters(), auto.named_parameters()):
                a.copy_(p)
                a.grad = None
        auto.engine().invalidate_weights()
        out = auto(x1, x2)
        fused = ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        seen = ts.last_logits.clone().requires_grad_(True)       # the logits the fused step's loss saw
        loss = crit(seen, lbl.long())
        loss.backward()
        assert abs(float(loss) - float(fused)) < 1e-6
        out.backward(seen.grad)
        torch.cuda.synchronize()
        for (k, a) in auto.named_parameters():
            assert torch.equal(ts.grads[k], a.grad), (it, k, float((ts.grads[k] - a.grad).abs().max()))
        bias = 'up4.conv.conv.0.bias'
        assert bool(ts.grads[bias].abs().sum() > 0), 'on running statistics the conv biases have gradients'
    for k, v in buffers.items():
        assert torch.equal(model.state_dict()[k], v), k


# ---------------------------------------------------------------- the default step is today's
def test_no_groups_nothing_frozen_takes_the_ungrouped_entry_points():
    x1, x2, lbl = _inputs(c=13, seed=5)
    calls, orig, spy = _spy()
    _lib.call = spy
    try:
        for kw, entry in ((dict(), 'bdn_sgd_step'), (dict(optimizer='sgd', momentum=0.9), 'bdn_sgd_momentum_step'),
                          (dict(optimizer='adamw'), 'bdn_adam_step')):
            del calls[:]
            model = filler.fill_module(BiDateNet(13, 2, precision='bf16')).to(dev).train()
            ts = TrainStep(model, lr=1e-2, **kw)
            assert ts.param_groups is None and ts.bn == 'batch'
            for _ in range(2):
                ts.step(x1, x2, lbl)
            torch.cuda.synchronize()
            assert calls.count(entry) == 2 and not any(n.endswith('_grouped') for n in calls), (entry, set(calls))
        del calls[:]
        model = filler.fill_module(BiDateNet(13, 2, precision='bf16')).to(dev).train()
        ts = TrainStep(model, lr=1e-2, optimizer='adamw', param_groups=[{'params': list(model.parameters())}])
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        assert calls.count('bdn_adam_step_grouped') == 1 and 'bdn_adam_step' not in calls
    finally:
        _lib.call = orig


def test_unlisted_trainable_parameter_raises_and_set_param_groups_rereads_flags():
    model = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()
    names = [k for k, _ in model.named_parameters()]
    with pytest.raises(ValueError, match='in no param group'):
        TrainStep(model, optimizer='adam', param_groups=[{'params': names[1:]}])
    with pytest.raises(ValueError, match='per-group betas'):
        TrainStep(model, optimizer='adam', param_groups=[{'params': names, 'betas': (0.5, 0.9)}])
    x1, x2, lbl = _inputs()
    ts = TrainStep(model, lr=1e-2, optimizer='adam')
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    keep = 'up4.conv.conv.0.weight'
    m_keep = ts.layout.view(ts.opt_state['exp_avg'], keep).clone()
    for k, p in model.named_parameters():
        p.requires_grad_(not k.startswith(ENCODER))
    ts.set_param_groups(None)                                   # the encoder is frozen from here on; lr still drives the one group
    inc = 'inc.conv.conv.0.weight'
    w0 = dict(model.named_parameters())[inc].detach().clone()
    assert torch.equal(ts.layout.view(ts.opt_state['exp_avg'], keep), m_keep) and not bool(ts.layout.view(ts.opt_state['exp_avg'], inc).any())
    ts.lr = 5e-3
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert torch.equal(dict(model.named_parameters())[inc].detach(), w0) and ts.opt_step == 2 and ts.param_groups[0]['lr'] == 5e-3
    assert not torch.equal(ts.layout.view(ts.opt_state['exp_avg'], keep), m_keep)


# ---------------------------------------------------------------- data parallel, in fresh child processes
_GLOO = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[3])
rank, world, bn = int(sys.argv[1]), int(sys.argv[2]), sys.argv[5]
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = sys.argv[4]
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
from fabric_amd import BiDateNet, _lib
from fabric_amd.train_step import TrainStep
from oracle import filler
ENCODER = ('inc.', 'down1.', 'down2.', 'down3.', 'down4.')
b, c, s, lr = 4, 3, 32, 0.05
x1, x2, lbl = (torch.from_numpy(v).cuda() for v in filler.make_inputs(b * world, c, s, seed=11))
sl = slice(rank * b, (rank + 1) * b)

def build(**kw):
    model = filler.fill_module(BiDateNet(c, 2, precision='fp32')).cuda().train()
    for k, p in model.named_parameters():
        p.requires_grad_(not k.startswith(ENCODER))
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    groups = [{'params': [k for k, p in named if p.dim() > 1]}, {'params': [k for k, p in named if p.dim() == 1], 'lr': lr * 0.1}]
    return TrainStep(model, lr=lr, param_groups=groups, bn=bn, n_buckets=3, **kw)

ts = build()
assert ts.world == world
released = []
orig = ts.bucketer.on_ready
def counting(keys):
    released.extend(keys)
    return orig(keys)
ts.bucketer.on_ready = counting
for _ in range(2):
    del released[:]
    ts.step(x1[sl], x2[sl], lbl[sl])
    assert sorted(released) == sorted(ts.layout.order), 'every key is reported ready exactly once per step'
torch.cuda.synchronize()
flat = ts.flat_params.cpu()
others = [torch.empty_like(flat) for _ in range(world)]
dist.all_gather(others, flat)
assert all(torch.equal(o, flat) for o in others), 'ranks diverged'
# single-process emulation: per-shard gradients from identical weights, summed in rank order, applied by the same grouped kernel
steps = [build(distributed=False) for _ in range(world)]
cur = steps[0].flat_params.clone()
ends, ids, n_seg = steps[0]._seg
for _ in range(2):
    g = torch.zeros_like(cur)
    for r, st in enumerate(steps):
        st.flat_params.copy_(cur)
        for gr in st.param_groups:
            gr['lr'] = 0.0
        st.model.engine().invalidate_weights()
        st.step(x1[r * b:(r + 1) * b], x2[r * b:(r + 1) * b], lbl[r * b:(r + 1) * b])
        g += st.flat_grads
    torch.cuda.synchronize()
    _lib.call('bdn_sgd_step_grouped', cur.data_ptr(), g.data_ptr(), ends.data_ptr(), ids.data_ptr(), n_seg, 2,
              _lib.floats([lr, lr * 0.1]), 1.0 / world, cur.numel(), _lib.stream_ptr())
torch.cuda.synchronize()
err = (cur.cpu() - flat).abs().max().item()
assert err < 5e-6, err
dist.barrier(); dist.destroy_process_group()
print('ok', rank, err)
'''


@pytest.mark.parametrize('bn', ['batch', 'frozen'])
def test_two_gloo_ranks_with_frozen_encoder_and_two_groups(tmp_path, bn):
    """Two ranks on one device (the pattern of tests/test_gpu_ddp.py, one attempt, a time limit): encoder frozen, two groups, plain SGD;
    once on batch statistics and once with bn='frozen' (whose conv-bias gradients are reduced).  No hang, every gradient key released
    once per step, rank-identical parameters equal to the single-process emulation with summed shard gradients within that file's
    bound (5e-6)."""
    script = tmp_path / 'groups_ddp_worker.py'
    script.write_text(_GLOO)
    port = str(39000 + (os.getpid() * 5 + (1 if bn == 'frozen' else 0)) % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', ROOT, port, bn], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=280)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(outs)
    assert all('ok' in o for o in outs)


# ---------------------------------------------------------------- train.py's fine-tuning flags
def test_train_cli_fine_tuning_flags(tmp_path):
    from fabric_amd.train import fine_tune_groups, make_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    from fabric_amd.utils.helpers import load_checkpoint
    bs = 8
    train_loader, _ = make_loaders(synthetic_onera(n_cities=6, bands=13, size=(360, 360)), ['city4', 'city5'], 90, 90, bs, True)
    per_epoch = len(train_loader)
    log = tmp_path / 'log'
    flags = ['--optimizer', 'adamw', '--freeze', 'inc', 'down1', '--no_decay_norm_bias', '--lr_scale', 'down2=0.1']
    common = [sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--batch_size', str(bs), '--num_workers', '0']
    r = subprocess.run(common + flags + ['--epochs', '1', '--log_dir', str(log)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sd = torch.load(log / 'optimizer_epoch_0.pt', weights_only=True)
    # the same groups on a fresh model, the way the command line builds them -> torch.optim.AdamW loads the file
    model = BiDateNet(13, 2)
    groups = fine_tune_groups(model, 1e-3, None, ['inc', 'down1'], True, [('down2', 0.1)])
    by = dict(model.named_parameters())
    frozen = [k for k, p in by.items() if not p.requires_grad]
    assert frozen and all(k.startswith(('inc.', 'down1.')) for k in frozen) and len(groups) == 4
    opt = torch.optim.AdamW([dict(g, params=[by[k] for k in g['params']]) for g in groups])
    opt.load_state_dict(sd)
    assert len(sd['param_groups']) == 4 and len(sd['state']) == 74 - len(frozen)
    assert sorted(g['weight_decay'] for g in sd['param_groups']) == [0.0, 0.0, 1e-2, 1e-2]
    ratios = sorted(g['lr'] for g in sd['param_groups'])
    assert abs(ratios[0] / ratios[-1] - 0.1) < 1e-9
    assert all(float(s['step']) == per_epoch for s in sd['state'].values())
    assert all(opt.state[by[k]] for k in by if k not in frozen) and not any(by[k] in opt.state and opt.state[by[k]] for k in frozen)
    ck = log / 'checkpoint_epoch_0.state_dict.pt'
    r = subprocess.run(common + flags + ['--epochs', '2', '--log_dir', str(log), '--resume', str(ck)], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert '"epoch": 1' in r.stdout and '"epoch": 0' not in r.stdout
    sd1 = torch.load(log / 'optimizer_epoch_1.pt', weights_only=True)
    assert all(float(s['step']) == 2 * per_epoch for s in sd1['state'].values())
    # --init_from the module.-prefixed state dict: a run from epoch 0 with those weights (everything frozen but outc, frozen BatchNorm:
    # the encoder and its running statistics come out as they went in)
    log2 = tmp_path / 'log2'
    r = subprocess.run(common + ['--optimizer', 'adamw', '--init_from', str(ck), '--epochs', '1', '--log_dir', str(log2), '--frozen_bn',
                                 '--freeze', 'inc', 'down1', 'down2', 'down3', 'down4'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert '"epoch": 0' in r.stdout
    a = load_checkpoint(str(ck)).state_dict()
    b = load_checkpoint(str(log2 / 'checkpoint_epoch_0.state_dict.pt')).state_dict()
    for k in a:
        same = torch.equal(a[k], b[k])
        if k.startswith(ENCODER) or 'running' in k or 'num_batches' in k:
            assert same, k
    assert not torch.equal(a['outc.conv.weight'], b['outc.conv.weight'])
    r = subprocess.run(common + ['--freeze', 'inc', '--loss_function', 'dice', '--epochs', '1'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and 'tversky' in r.stderr
