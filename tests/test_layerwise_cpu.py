"""CPU tests of the layer-wise adaptive rules (LAMB, LARS): the C ABI rows and argument refusals of bdn_lamb_step / bdn_lars_step,
OptimConfig for the new kinds, the per-tensor table, the state exchange, the float64 twin (tests/layerwise_ref.py) the GPU tests hold the
kernels to -- pinned here against CPU torch.optim with every ratio forced to 1, on a hand example and on the zero-norm / max_trust
branches -- and the learning-rate schedule (fabric_amd/schedule.py)."""
import ctypes
import math
import os
import re

import pytest
import torch

from fabric_amd import _lib
from fabric_amd import optim as O
from fabric_amd.optim import OptimConfig, ParamGroups
from fabric_amd.parallel import FlatLayout
from fabric_amd.schedule import LRSchedule

from tests import layerwise_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_VP = ctypes.c_void_p
_CTYPES = {'float*': _VP, 'const float*': _VP, 'void*': _VP, 'const uint32_t*': _VP, 'const int32_t*': _VP, 'float': ctypes.c_float,
           'int': ctypes.c_int, 'long long': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'double': ctypes.c_double}
_HOST = ('lr', 'weight_decay')                  # const float* that are HOST arrays: typed _hf so that the guard harness skips them


@pytest.mark.parametrize('name', ['bdn_lamb_step', 'bdn_lars_step', 'bdn_layerwise_workspace_bytes'])
def test_header_declaration_matches_signature_row(name):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\b(int|size_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())).rsplit(' ', 1) for p in m.group(2).split(',')]
    want = [_lib._hf if pname in _HOST else _CTYPES[ptype.strip()] for ptype, pname in params]
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_size_t)
    assert want == list(args), ([p for p in params], args)


def _lamb_args(**kw):
    a = dict(params=32, grads=32, m=32, v=32, ten_end=32, ten_len=32, ten_group=32, ten_adapt=32, n_tensors=1, n_groups=1,
             lr=_lib.floats([1e-3]), wd=_lib.floats([0.0]), gs=1.0, ds=None, b1=0.9, b2=0.999, eps=1e-8, max_trust=0.0, step=1, ws=32,
             trust=32, n=16, stream=None)
    a.update(kw)
    return list(a.values())


def _lars_args(**kw):
    a = dict(params=32, grads=32, buf=32, ten_end=32, ten_len=32, ten_group=32, ten_adapt=32, n_tensors=1, n_groups=1,
             lr=_lib.floats([1e-3]), wd=_lib.floats([0.0]), gs=1.0, ds=None, momentum=0.9, dampening=0.0, nesterov=0, first=1,
             trust_coef=1e-3, lars_eps=1e-8, max_trust=0.0, ws=32, trust=32, n=16, stream=None)
    a.update(kw)
    return list(a.values())


_REFUSED = [
    ('lamb', dict(params=None), 'null'), ('lamb', dict(m=None), 'null'), ('lamb', dict(ten_len=None), 'null'),
    ('lamb', dict(ten_adapt=None), 'null'), ('lamb', dict(lr=None), 'null'), ('lamb', dict(wd=None), 'null'), ('lamb', dict(ws=None), 'null'),
    ('lamb', dict(trust=None), 'null'), ('lamb', dict(v=40), 'aligned'), ('lamb', dict(ten_end=34), 'aligned'),
    ('lamb', dict(ds=34), 'aligned'), ('lamb', dict(ws=36), 'aligned'), ('lamb', dict(trust=34), 'aligned'), ('lamb', dict(n=18), 'multiple of 4'),
    ('lamb', dict(n_tensors=0), 'tensors'), ('lamb', dict(n_tensors=257), 'tensors'), ('lamb', dict(n_groups=0), 'groups'),
    ('lamb', dict(n_groups=9), 'groups'), ('lamb', dict(b1=1.0), 'betas'), ('lamb', dict(b2=-0.1), 'betas'), ('lamb', dict(eps=-1e-8), 'eps'),
    ('lamb', dict(max_trust=-1.0), 'max_trust'), ('lamb', dict(step=0), 'step'),
    ('lars', dict(grads=None), 'null'), ('lars', dict(ten_group=None), 'null'), ('lars', dict(buf=40), 'aligned'),
    ('lars', dict(n=6), 'multiple of 4'), ('lars', dict(n_tensors=300), 'tensors'), ('lars', dict(n_groups=-1), 'groups'),
    ('lars', dict(trust_coef=-1.0), 'trust_coef'), ('lars', dict(lars_eps=-1.0), 'lars_eps'), ('lars', dict(max_trust=float('nan')), 'max_trust'),
    ('lars', dict(nesterov=1, dampening=0.1), 'nesterov'), ('lars', dict(nesterov=1, momentum=0.0, buf=None), 'nesterov'),
    ('lars', dict(buf=None), 'momentum_buf'), ('lars', dict(momentum=0.0), 'momentum_buf'),
]


@pytest.mark.parametrize('rule,kw,word', _REFUSED, ids=[f'{r}-{"-".join(k)}-{i}' for i, (r, k, _) in enumerate(_REFUSED)])
def test_argument_errors_return_before_touching_a_device(rule, kw, word):
    """Fake non-null pointers: every refusal is BDN_E_ARG from the host checks, nothing reaches a device."""
    lib = _lib.load()
    rc = lib.bdn_lamb_step(*_lamb_args(**kw)) if rule == 'lamb' else lib.bdn_lars_step(*_lars_args(**kw))
    msg = lib.bdn_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


def test_n_zero_launches_nothing_and_workspace_size():
    lib = _lib.load()
    assert lib.bdn_lamb_step(*_lamb_args(n=0)) == 0 and lib.bdn_lars_step(*_lars_args(n=0)) == 0
    # one pair of doubles per (1024-vector chunk + tensor): fewer pieces than that exist
    assert lib.bdn_layerwise_workspace_bytes(4096 * 3 + 4, 7) == 16 * (4 + 7)
    assert lib.bdn_layerwise_workspace_bytes(0, 0) == 16


def test_config_for_the_new_kinds():
    assert O.KINDS == ('sgd', 'adam', 'adamw', 'lamb', 'lars')
    lamb, lars = OptimConfig('lamb'), OptimConfig('lars', momentum=0.9)
    assert lamb.family == 'lamb' and lars.family == 'lars' and OptimConfig('adamw').family == 'adam' and OptimConfig('sgd').family == 'sgd'
    assert lamb.state_keys() == ('exp_avg', 'exp_avg_sq') and lamb.stepped and not lars.stepped
    assert lars.state_keys() == ('momentum_buffer',) and OptimConfig('lars').state_keys() == ()
    assert not lamb.plain and not OptimConfig('lars').plain
    assert (lamb.trust_coef, lamb.lars_eps, lamb.max_trust, lamb.adapt_1d) == (1e-3, 1e-8, 0.0, False)
    assert lamb.weight_decay == 0.0 and lars.weight_decay == 0.0
    assert OptimConfig('lars', trust_coef=0.02, lars_eps=1e-6, max_trust=10, adapt_1d=True, momentum=0.9, nesterov=True).max_trust == 10.0
    for kw in (dict(kind='rmsprop'), dict(kind='lamb', momentum=0.9), dict(kind='lamb', dampening=0.1), dict(kind='lamb', nesterov=True),
               dict(kind='lars', betas=(0.8, 0.999)), dict(kind='lars', nesterov=True), dict(kind='lars', nesterov=True, momentum=0.9, dampening=0.1),
               dict(kind='lamb', max_trust=-1.0), dict(kind='lars', trust_coef=-1e-3), dict(kind='lars', lars_eps=float('nan')),
               dict(kind='lamb', trust_coef=0.5), dict(kind='adamw', max_trust=2.0), dict(kind='sgd', adapt_1d=True),
               dict(kind='lamb', betas=(1.0, 0.999)), dict(kind='lamb', amsgrad=True), dict(kind='lars', maximize=True),
               dict(kind='lamb', max_trust=True)):
        with pytest.raises(ValueError):
            OptimConfig(**kw)
    for c in (OptimConfig('lamb', lr=2e-3, weight_decay=0.01, betas=(0.8, 0.99), eps=1e-6, max_trust=10.0, adapt_1d=True),
              OptimConfig('lars', lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4, trust_coef=0.02, lars_eps=1e-6)):
        g = c.param_group([0, 1])
        assert g['layer_adapt'] == c.kind and g['params'] == [0, 1] and g['max_trust'] == c.max_trust and g['adapt_1d'] == c.adapt_1d
        assert OptimConfig.from_param_group(g) == c
    with pytest.raises(ValueError):
        OptimConfig.from_param_group(dict(lr=1e-3, layer_adapt='lion'))
    # a group without the key is torch's still
    assert OptimConfig.from_param_group(OptimConfig('adamw').param_group([])).kind == 'adamw'


def _layout():
    shapes = [('a', (1,)), ('b', (2,)), ('c', (3, 1)), ('d', (2, 2)), ('e', (64,)), ('f', (5, 3)), ('w', (4, 4, 3, 3))]
    return FlatLayout(shapes, [k for k, _ in shapes]), [k for k, _ in shapes]


def test_tensor_table():
    layout, names = _layout()
    cfg = OptimConfig('lamb')
    pg = ParamGroups(cfg, names, [{'params': ['a', 'b', 'c', 'f'], 'lr': 0.1}, {'params': ['d', 'e'], 'weight_decay': 0.0}], frozen=['w'])
    ends, lens, ids, adapt = O.tensor_table(layout, pg)
    assert all(t.dtype == torch.int32 and t.device.type == 'cpu' for t in (ends, lens, ids, adapt))
    assert ends.tolist() == [1, 2, 3, 4, 20, 24, 60] and ends[-1].item() * 4 == layout.total
    assert lens.tolist() == [1, 2, 3, 4, 64, 15, 144]
    assert ids.tolist() == [0, 0, 0, 1, 1, 0, O.FROZEN]
    assert adapt.tolist() == [0, 0, 1, 1, 0, 1, 1]                      # ndim <= 1 takes ratio 1
    assert O.tensor_table(layout, pg, adapt_1d=True)[3].tolist() == [1] * 7
    # the segment table of the grouped kernels merges neighbours; this one never does
    assert len(O.segment_table(layout, pg)[0]) < len(ends)


@pytest.mark.parametrize('cfg', [OptimConfig('lamb', lr=2e-3, weight_decay=0.01, max_trust=5.0),
                                 OptimConfig('lars', lr=0.1, momentum=0.9, nesterov=True, trust_coef=0.02)], ids=['lamb', 'lars'])
def test_state_round_trip_and_cross_family_refusal(cfg):
    layout, names = _layout()
    gen = torch.Generator().manual_seed(1)
    flat = {k: torch.zeros(layout.total) for k in cfg.state_keys()}
    for k in cfg.state_keys():
        for name in names:
            layout.view(flat[k], name).copy_(torch.randn(layout.slices[name][2], generator=gen))
    step = 3 if cfg.stepped else 1
    sd = O.flat_to_torch(cfg, layout, names, flat, step)
    assert sd['param_groups'][0]['layer_adapt'] == cfg.kind and len(sd['state']) == len(names)
    assert ('step' in sd['state'][0]) == cfg.stepped
    cfg2, flat2, step2 = O.torch_to_flat(sd, layout, names)
    assert cfg2 == cfg and step2 == step and all(torch.equal(flat[k], flat2[k]) for k in flat)
    sd2 = O.flat_to_torch(cfg2, layout, names, flat2, step2)
    assert sd2['param_groups'] == sd['param_groups']
    assert all(torch.equal(sd['state'][i][k], sd2['state'][i][k]) for i in sd['state'] for k in sd['state'][i])
    # with groups and a frozen tensor
    pg = ParamGroups(cfg, names, [{'params': ['a', 'b', 'c', 'w'], 'lr': 0.5}, {'params': ['d', 'e', 'f'], 'weight_decay': 0.25}], frozen=['w'])
    gsd = O.groups_to_torch(cfg, pg, layout, flat, step)
    assert [g['layer_adapt'] for g in gsd['param_groups']] == [cfg.kind] * 2 and names.index('w') not in gsd['state']
    cfg3, hyper, flat3, step3 = O.torch_to_groups(gsd, pg, layout)
    assert cfg3.kind == cfg.kind and step3 == step and hyper == [{'lr': 0.5, 'weight_decay': cfg.weight_decay}, {'lr': cfg.lr, 'weight_decay': 0.25}]
    for k in flat:
        for name in names:
            want = torch.zeros(layout.slices[name][2]) if name == 'w' else layout.view(flat[k], name)
            assert torch.equal(layout.view(flat3[k], name), want)
    # the family tells the rules apart: what TrainStep.load_optimizer_state_dict compares
    families = {OptimConfig.from_param_group(OptimConfig(k, **({'momentum': 0.9} if k in ('sgd', 'lars') else {})).param_group([])).family
                for k in O.KINDS}
    assert families == {'sgd', 'adam', 'lamb', 'lars'}


# ---------------------------------------------------------------- the twin
def _tensors(gen, shapes, scale=1.0):
    return [torch.randn(s, generator=gen, dtype=torch.float64) * scale for s in shapes]


def test_twin_with_unit_ratios_is_adamw():
    gen = torch.Generator().manual_seed(0)
    shapes = [(5, 3), (7,), (2, 2, 3)]
    ps = _tensors(gen, shapes)
    params = [p.clone().requires_grad_() for p in ps]
    opt = torch.optim.AdamW(params, lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05, foreach=False)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for step in range(1, 4):
        gs = _tensors(gen, shapes, 0.5 * step)
        for p, g in zip(params, gs):
            p.grad = g.clone()
        opt.step()
        out = L.lamb(ps, gs, ms, vs, step, [1e-2] * 3, [0.05] * 3, betas=(0.8, 0.99), eps=1e-6, ratios=[1.0] * 3)
        ps, ms, vs = out['p'], out['m'], out['v']
        for i, (a, b) in enumerate(zip(ps, params)):
            assert float((a - b.detach()).abs().max()) <= 1e-12 * float(b.detach().abs().max()), (step, i)
            assert torch.allclose(ms[i], opt.state[params[i]]['exp_avg'], rtol=1e-12, atol=0)
            assert torch.allclose(vs[i], opt.state[params[i]]['exp_avg_sq'], rtol=1e-12, atol=0)
            assert bool((out['p_mag'][i] >= a.abs() * (1 - 1e-12)).all()) and bool((out['u_mag'][i] >= out['u'][i].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('nesterov', [False, True])
def test_twin_with_unit_ratios_is_sgd_momentum(nesterov):
    gen = torch.Generator().manual_seed(1)
    shapes = [(5, 3), (7,)]
    ps = _tensors(gen, shapes)
    params = [p.clone().requires_grad_() for p in ps]
    opt = torch.optim.SGD(params, lr=0.1, momentum=0.9, nesterov=nesterov, weight_decay=1e-2, foreach=False)
    bufs = None
    for step in range(3):
        gs = _tensors(gen, shapes, 0.5 + step)
        for p, g in zip(params, gs):
            p.grad = g.clone()
        opt.step()
        out = L.lars(ps, gs, bufs, [0.1] * 2, [1e-2] * 2, momentum=0.9, nesterov=nesterov, first=step == 0, ratios=[1.0] * 2)
        ps, bufs = out['p'], out['buf']
        for i, (a, b) in enumerate(zip(ps, params)):
            assert float((a - b.detach()).abs().max()) <= 1e-12 * float(b.detach().abs().max()), (step, i)
            assert torch.allclose(bufs[i], opt.state[params[i]]['momentum_buffer'], rtol=1e-12, atol=0)


def test_twin_ratios_on_a_hand_example():
    p = [torch.tensor([3.0, 4.0], dtype=torch.float64), torch.tensor([[1.0, 2.0], [2.0, 0.0]], dtype=torch.float64)]
    g = [torch.tensor([0.5, -1.0], dtype=torch.float64), torch.tensor([[2.0, 0.0], [-1.0, 2.0]], dtype=torch.float64)]
    z = [torch.zeros_like(t) for t in p]
    wd, lr, b1, b2, eps = 0.1, 0.01, 0.9, 0.999, 1e-8
    out = L.lamb(p, g, z, z, 1, [lr] * 2, [wd] * 2, betas=(b1, b2), eps=eps)
    for i in range(2):
        m, v = (1 - b1) * g[i], (1 - b2) * g[i] ** 2
        u = (m / (1 - b1)) / (v.sqrt() / math.sqrt(1 - b2) + eps) + wd * p[i]
        wn, un = float(p[i].pow(2).sum().sqrt()), float(u.pow(2).sum().sqrt())
        assert out['wn'][i] == pytest.approx(wn, rel=1e-15) and out['xn'][i] == pytest.approx(un, rel=1e-14)
        assert out['ratio'][i] == pytest.approx(wn / un, rel=1e-14)
        assert torch.allclose(out['p'][i], p[i] - lr * (wn / un) * u, rtol=1e-14, atol=0)
    assert out['wn'] == [5.0, 3.0]
    tc, le = 0.02, 1e-3
    out = L.lars(p, g, None, [lr] * 2, [wd] * 2, momentum=0.9, first=True, trust_coef=tc, lars_eps=le)
    for i, (wn, gn) in enumerate([(5.0, math.sqrt(1.25)), (3.0, 3.0)]):
        local = tc * wn / (gn + wd * wn + le)
        assert out['xn'][i] == pytest.approx(gn, rel=1e-15) and out['ratio'][i] == pytest.approx(local, rel=1e-14)
        d = local * (g[i] + wd * p[i])
        assert torch.allclose(out['buf'][i], d, rtol=1e-14, atol=0) and torch.allclose(out['p'][i], p[i] - lr * d, rtol=1e-14, atol=0)


def test_twin_zero_norm_clamp_adapt_and_frozen_branches():
    assert L.lamb_ratio(0.0, 2.0) == 1.0 and L.lamb_ratio(2.0, 0.0) == 1.0 and L.lamb_ratio(6.0, 2.0) == 3.0
    assert L.lamb_ratio(6.0, 2.0, max_trust=2.5) == 2.5 and L.lamb_ratio(6.0, 2.0, max_trust=10.0) == 3.0
    assert L.lamb_ratio(6.0, 2.0, adapt=False) == 1.0
    assert L.lars_ratio(0.0, 2.0, 0.1, 0.0, 0.0) == 1.0 and L.lars_ratio(2.0, 0.0, 0.1, 0.0, 0.0) == 1.0
    assert L.lars_ratio(4.0, 2.0, 0.5, 0.0, 0.0) == 1.0 and L.lars_ratio(4.0, 1.0, 0.5, 0.25, 0.0) == 1.0
    assert L.lars_ratio(4.0, 1.0, 0.5, 0.25, 0.0, max_trust=0.75) == 0.75 and L.lars_ratio(4.0, 1.0, 0.5, 0.25, 0.0, adapt=False) == 1.0
    assert L.lamb_ratio(0.0, 2.0, max_trust=0.5) == 0.5                       # the clamp comes after the zero-norm branch, as specified
    p = [torch.zeros(3, dtype=torch.float64), 3 * torch.ones(4, dtype=torch.float64), torch.ones(2, dtype=torch.float64)]
    g = [torch.ones(3, dtype=torch.float64), torch.ones(4, dtype=torch.float64), torch.ones(2, dtype=torch.float64)]
    z = [torch.zeros_like(t) for t in p]
    out = L.lamb(p, g, z, z, 1, [0.1] * 3, [0.0] * 3, max_trust=2.0, frozen={2})
    assert out['ratio'][0] == 1.0 and out['wn'][0] == 0.0                    # ||p|| == 0
    assert out['ratio'][1] == 2.0 and out['wn'][1] == 6.0                     # 6 / 2 clamped
    assert out['ratio'][2] == 0.0 and torch.equal(out['p'][2], p[2]) and out['wn'][2] == 0.0      # frozen: untouched, {0, 0, 0}
    out = L.lars(p, [torch.zeros(3, dtype=torch.float64)] + g[1:], None, [0.1] * 3, [0.0] * 3, adapt=[1, 0, 1])
    assert out['ratio'][0] == 1.0 and out['ratio'][1] == 1.0 and out['buf'] == [None] * 3


# ---------------------------------------------------------------- the schedule
class _Step:
    def __init__(self, groups=None):
        self.lr, self.param_groups = 0.5, groups


def test_schedule_warmup_cosine_and_resume_position():
    s = LRSchedule(0.4, 100, warmup_updates=4, schedule='cosine', lr_min=0.04)
    assert [s.lr(u) for u in range(4)] == pytest.approx([0.1, 0.2, 0.3, 0.4]) and s.lr(3) == 0.4
    assert s.lr(99) == pytest.approx(0.04, rel=1e-12) and s.lr(150) == pytest.approx(0.04, rel=1e-12)
    assert s.lr(51) == pytest.approx(0.22, rel=1e-12)                      # half way between the end of the warmup and the last update
    assert all(s.lr(u) >= s.lr(u + 1) for u in range(3, 99))
    c = LRSchedule(0.4, 101, schedule='cosine')
    assert c.lr(0) == 0.4 and c.lr(50) == pytest.approx(0.2, rel=1e-12) and c.lr(100) == pytest.approx(0.0, abs=1e-16)
    w = LRSchedule(0.4, 10, warmup_updates=5)
    assert w.lr(0) == pytest.approx(0.08) and w.lr(4) == 0.4 and w.lr(9) == 0.4
    # the position comes from (epoch, batch): a run resumed at epoch 2 continues where epoch 1 ended
    assert LRSchedule.updates_per_epoch(10, 4) == 3 and LRSchedule.updates_per_epoch(8, 4) == 2
    assert [LRSchedule.position(0, i, 10, 4) for i in (0, 3, 4, 9)] == [0, 0, 1, 2]
    assert LRSchedule.position(2, 0, 10, 4) == 6 == LRSchedule.position(1, 9, 10, 4) + 1
    short = LRSchedule(0.4, 2, warmup_updates=4, schedule='cosine')          # a run that ends inside its warmup
    assert [short.lr(u) for u in range(2)] == pytest.approx([0.1, 0.2])
    groups = [{'lr': 9.0}, {'lr': 9.0}]
    st = _Step(groups)
    LRSchedule(0.4, 100, 4, 'cosine', 0.04, group_lrs=[0.4, 0.04]).apply(st, 1)
    assert st.lr == pytest.approx(0.2) and [g['lr'] for g in groups] == pytest.approx([0.2, 0.02])
    for kw in (dict(schedule='linear'), dict(warmup_updates=-1), dict(lr_min=0.5), dict(lr_min=-0.1),
               dict(warmup_updates=1.5)):
        with pytest.raises(ValueError):
            LRSchedule(0.4, 100, **kw)


def test_default_schedule_is_a_no_op():
    s = LRSchedule(0.4, 100)
    assert s.is_default and s.factor(0) == 1.0 and s.factor(99) == 1.0
    groups = [{'lr': 7.0}]
    st = _Step(groups)
    s.apply(st, 5)
    assert st.lr == 0.5 and groups == [{'lr': 7.0}]                         # nothing is written, not even an equal value
    assert not LRSchedule(0.4, 100, 1).is_default and not LRSchedule(0.4, 100, schedule='cosine').is_default


def test_train_cli_refuses_the_layerwise_rules_without_the_fused_step():
    from fabric_amd import train
    for extra in (['--optimizer', 'lamb'], ['--optimizer', 'lars'], ['--lr_warmup_updates', '4'], ['--lr_schedule', 'cosine']):
        with pytest.raises(SystemExit, match='fused step'):
            train.main(['--synthetic', '--loss_function', 'dice'] + extra)
    with pytest.raises(SystemExit, match='lamb'):
        train.main(['--synthetic', '--optimizer', 'lamb', '--momentum', '0.9'])
