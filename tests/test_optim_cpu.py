"""CPU tests of the fused step's update rules (fabric_amd/optim.py): the C ABI rows, configuration checks, the flat <-> torch.optim state
conversion, and the float64 restatement (tests/optim_ref.py) the GPU tests hold the kernels to, pinned here against CPU torch.optim."""
import ctypes
import os
import re

import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.engine import param_order
from fabric_amd.optim import OptimConfig, flat_to_torch, torch_to_flat
from fabric_amd.parallel import FlatLayout

from tests import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'float': ctypes.c_float,
           'int': ctypes.c_int, 'long long': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'double': ctypes.c_double}


@pytest.mark.parametrize('name', ['bdn_sgd_momentum_step', 'bdn_adam_step'])
def test_header_declaration_matches_signature_row(name):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')
    types = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())).rsplit(' ', 1)[0].strip() for p in params]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int
    assert [_CTYPES[t] for t in types] == list(args), (types, args)
    assert ctypes.sizeof(ctypes.c_longlong) == ctypes.sizeof(ctypes.c_int64)


def test_argument_errors_return_before_touching_a_device():
    lib = _lib.load()
    assert lib.bdn_adam_step(None, None, None, None, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, 0, 1, 16, None) != 0
    assert b'null' in lib.bdn_last_error()
    assert lib.bdn_adam_step(16, 16, 16, 16, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, 0, 0, 16, None) != 0
    assert b'step' in lib.bdn_last_error()
    assert lib.bdn_adam_step(16, 16, 16, 16, 1e-3, 1.0, 1.0, 0.999, 1e-8, 0.0, 0, 1, 16, None) != 0
    assert lib.bdn_adam_step(16, 16, 16, 20, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, 0, 1, 16, None) != 0
    assert b'aligned' in lib.bdn_last_error()
    assert lib.bdn_sgd_momentum_step(16, 16, None, 1e-3, 1.0, 0.9, 0.0, 0.0, 0, 1, 16, None) != 0       # momentum without a buffer
    assert lib.bdn_sgd_momentum_step(16, 16, 32, 1e-3, 1.0, 0.0, 0.0, 0.0, 0, 1, 16, None) != 0        # a buffer without momentum
    assert lib.bdn_sgd_momentum_step(16, 16, 32, 1e-3, 1.0, 0.9, 0.1, 0.0, 1, 1, 16, None) != 0        # nesterov with dampening
    assert b'nesterov' in lib.bdn_last_error()
    assert lib.bdn_sgd_momentum_step(16, 16, None, 1e-3, 1.0, 0.0, 0.0, 0.0, 0, 1, 0, None) == 0        # n == 0 launches nothing


def test_config_defaults_and_validation():
    assert OptimConfig().plain and OptimConfig('sgd', momentum=0, weight_decay=0).plain
    assert OptimConfig('sgd').state_keys() == ()
    assert not OptimConfig('sgd', weight_decay=1e-4).plain and OptimConfig('sgd', weight_decay=1e-4).state_keys() == ()
    assert OptimConfig('sgd', momentum=0.9).state_keys() == ('momentum_buffer',)
    assert OptimConfig('adam').weight_decay == 0.0 and OptimConfig('sgd').weight_decay == 0.0
    assert OptimConfig('adamw').weight_decay == 1e-2                                  # torch.optim.AdamW's default
    assert OptimConfig('adamw', weight_decay=0.0).weight_decay == 0.0
    assert OptimConfig('adam').state_keys() == ('exp_avg', 'exp_avg_sq')
    for kw in (dict(kind='rmsprop'), dict(kind='adam', amsgrad=True), dict(maximize=True), dict(nesterov=True),
               dict(nesterov=True, momentum=0.9, dampening=0.1), dict(lr=-1e-3), dict(momentum=-0.5), dict(weight_decay=-1e-2),
               dict(kind='adam', eps=-1e-8), dict(kind='adam', betas=(1.0, 0.999)), dict(kind='adam', betas=(0.9, -0.1)),
               dict(kind='adam', momentum=0.9), dict(kind='adamw', nesterov=True), dict(lr=float('nan'))):
        with pytest.raises(ValueError):
            OptimConfig(**kw)


@pytest.mark.parametrize('make', [lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4),
                                  lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.8, dampening=0.2),
                                  lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-2),
                                  lambda ps: torch.optim.AdamW(ps, lr=1e-3, betas=(0.8, 0.99), eps=1e-6)],
                         ids=['sgd_nesterov_wd', 'sgd_dampening', 'adam_wd', 'adamw'])
def test_torch_state_round_trips_through_the_flat_layout(make):
    """torch.optim state of a CPU BiDateNet(13, 2) after 3 steps -> flat backward-order buffers -> torch format: equal to the original,
    and it loads into a fresh torch optimizer of the same kind."""
    torch.manual_seed(0)
    model = BiDateNet(13, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(13))
    opt = make(model.parameters())
    for _ in range(3):
        for p in model.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    sd = opt.state_dict()
    cfg, flat, step = torch_to_flat(sd, layout, names)
    assert all(v.shape == (layout.total,) and v.dtype == torch.float32 for v in flat.values())
    assert set(flat) == set(cfg.state_keys()) and step == (3 if cfg.family == 'adam' else 1)
    back = flat_to_torch(cfg, layout, names, flat, step)
    g0, g1 = sd['param_groups'][0], back['param_groups'][0]
    assert set(g0) == set(g1) and all(g0[k] == g1[k] for k in g0), (g0, g1)
    assert set(back['state']) == set(sd['state'])
    for i, s in sd['state'].items():
        assert set(s) == set(back['state'][i])
        for k, v in s.items():
            w = back['state'][i][k]
            assert w.dtype == v.dtype and w.shape == v.shape and w.device == v.device and torch.equal(w, v), (i, k)
            if v.dim():
                assert w.data_ptr() != v.data_ptr()
    # a copy, not a view of the flat buffers
    k0 = next(iter(flat))
    flat[k0].add_(1.0)
    assert not torch.equal(back['state'][0][k0], layout.view(flat[k0], names[0]))
    fresh = make(BiDateNet(13, 2).parameters())
    fresh.load_state_dict(back)
    for i, s in sd['state'].items():
        for k, v in s.items():
            assert torch.equal(fresh.state_dict()['state'][i][k], v)


def test_conversion_rejects_mismatches():
    model = BiDateNet(3, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(3))
    opt = torch.optim.Adam(model.parameters())
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    sd = opt.state_dict()
    with pytest.raises(ValueError, match='parameters'):
        torch_to_flat(sd, layout, names[:-1])
    bad = {'state': dict(sd['state']), 'param_groups': sd['param_groups']}
    bad['state'][0] = dict(bad['state'][0], exp_avg=torch.zeros(3))
    with pytest.raises(ValueError, match='shape'):
        torch_to_flat(bad, layout, names)
    bad['state'] = {k: v for k, v in sd['state'].items() if k != 5}
    with pytest.raises(ValueError, match='all or none'):
        torch_to_flat(bad, layout, names)
    bad['state'] = dict(sd['state'])
    bad['state'][1] = dict(bad['state'][1], step=torch.tensor(7.0))
    with pytest.raises(ValueError, match='different numbers'):
        torch_to_flat(bad, layout, names)
    two = {'state': {}, 'param_groups': [dict(sd['param_groups'][0], params=[0]), dict(sd['param_groups'][0], params=[1])]}
    with pytest.raises(ValueError, match='param groups'):
        torch_to_flat(two, layout, names)
    ams = {'state': {}, 'param_groups': [dict(sd['param_groups'][0], amsgrad=True)]}
    with pytest.raises(ValueError, match='amsgrad'):
        torch_to_flat(ams, layout, names)
    fresh = torch_to_flat(torch.optim.Adam(model.parameters()).state_dict(), layout, names)     # no step taken: zero state, step 0
    assert fresh[2] == 0 and all(not bool(v.any()) for v in fresh[1].values())


_RULES = [
    ('sgd_momentum', dict(momentum=0.9)),
    ('sgd_dampening', dict(momentum=0.9, dampening=0.1)),
    ('sgd_nesterov_wd', dict(momentum=0.9, nesterov=True, weight_decay=1e-2)),
    ('sgd_wd', dict(weight_decay=1e-2)),
    ('adam', dict()),
    ('adam_wd', dict(weight_decay=1e-2)),
    ('adamw', dict(weight_decay=1e-2)),
]


@pytest.mark.parametrize('rule,kw', _RULES, ids=[r for r, _ in _RULES])
def test_float64_restatement_matches_cpu_torch_optim(rule, kw):
    """5 steps of CPU torch.optim (foreach=False: the single-tensor formulas) against the float64 restatement, each step from torch's own
    float32 parameters and state, within the bound tests/test_gpu_optim.py holds the kernels to."""
    torch.manual_seed(1)
    n = 4099
    p = torch.nn.Parameter(torch.randn(n))
    lr = 0.05
    if rule.startswith('sgd'):
        opt = torch.optim.SGD([p], lr=lr, foreach=False, **kw)
    else:
        opt = (torch.optim.AdamW if rule == 'adamw' else torch.optim.Adam)([p], lr=lr, foreach=False, **kw)
    for it in range(5):
        g = torch.randn(n) * (0.5 + it)
        p0 = p.detach().clone()
        st = {k: v.clone() for k, v in opt.state[p].items()} if opt.state[p] else {}
        p.grad = g.clone()
        opt.step()
        if rule.startswith('sgd'):
            mom = kw.get('momentum', 0.0)
            rp, rb, mp, mb = R.sgd(p0, g, st.get('momentum_buffer'), lr, momentum=mom, dampening=kw.get('dampening', 0.0),
                                   weight_decay=kw.get('weight_decay', 0.0), nesterov=kw.get('nesterov', False), first=it == 0)
            if mom:
                R.check(opt.state[p]['momentum_buffer'], rb, mb, f'{rule} step {it} buf')
        else:
            m0 = st.get('exp_avg', torch.zeros(n))
            v0 = st.get('exp_avg_sq', torch.zeros(n))
            rp, rm, rv, mp, mm, mv = R.adam(p0, g, m0, v0, it + 1, lr, weight_decay=kw.get('weight_decay', 0.0), decoupled=rule == 'adamw')
            R.check(opt.state[p]['exp_avg'], rm, mm, f'{rule} step {it} m')
            R.check(opt.state[p]['exp_avg_sq'], rv, mv, f'{rule} step {it} v')
            assert float(opt.state[p]['step']) == it + 1
        R.check(p, rp, mp, f'{rule} step {it} p')
