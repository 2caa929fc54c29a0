"""CPU tests of the fused step's parameter groups (fabric_amd/optim.py: ParamGroups, segment_table, groups_to_torch, torch_to_groups):
the C ABI rows of the grouped update kernels, the segment table, the rejections, the state exchange with torch.optim built with the same
groups, and the float64 restatement of the grouped update (tests/optim_ref.py's rules applied segment by segment) that
tests/test_gpu_param_groups.py holds the kernels to, pinned here against CPU torch.optim."""
import ctypes
import os
import re

import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.engine import param_order
from fabric_amd.optim import (FROZEN, MAX_GROUPS, OptimConfig, ParamGroups, flat_to_torch, groups_to_torch, segment_table,
                              torch_to_groups)
from fabric_amd.parallel import FlatLayout

from tests import optim_ref as R
from tests.param_groups_ref import grouped_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODER = ('inc.', 'down1.', 'down2.', 'down3.', 'down4.')

_CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'const uint32_t*': ctypes.c_void_p,
           'const int32_t*': ctypes.c_void_p, 'float': ctypes.c_float, 'int': ctypes.c_int, 'long long': ctypes.c_int64,
           'size_t': ctypes.c_size_t, 'double': ctypes.c_double}
GROUPED = ['bdn_sgd_step_grouped', 'bdn_sgd_momentum_step_grouped', 'bdn_adam_step_grouped']


def _model(c):
    torch.manual_seed(0)
    model = BiDateNet(c, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    return model, named, names, FlatLayout([(k, p.shape) for k, p in named], param_order(c))


def is_norm_or_bias(k, named):
    return dict(named)[k].dim() == 1


# ---------------------------------------------------------------- the C ABI
@pytest.mark.parametrize('name', GROUPED)
def test_header_declaration_matches_signature_row(name):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')
    types = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())).rsplit(' ', 1)[0].strip() for p in params]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int
    assert [_CTYPES[t] for t in types] == list(args), (types, args)


def test_argument_errors_return_before_touching_a_device():
    lib = _lib.load()
    one, wd = _lib.floats([1e-3]), _lib.floats([0.0])
    nine = _lib.floats([1e-3] * 9)
    adam = lambda *a: lib.bdn_adam_step_grouped(*a)        # noqa: E731
    tail = (1.0, 0.9, 0.999, 1e-8, 0, 1, 16, None)
    assert adam(None, None, None, None, 16, 16, 1, 1, one, wd, *tail) != 0 and b'null' in lib.bdn_last_error()
    assert adam(16, 16, 16, 16, 16, 16, 1, 9, nine, nine, *tail) != 0 and b'9 groups' in lib.bdn_last_error()
    assert adam(16, 16, 16, 16, 16, 16, 1, 0, one, wd, *tail) != 0 and b'groups' in lib.bdn_last_error()
    assert adam(16, 16, 16, 16, 16, 16, 257, 1, one, wd, *tail) != 0 and b'segments' in lib.bdn_last_error()
    assert adam(16, 16, 16, 20, 16, 16, 1, 1, one, wd, *tail) != 0 and b'aligned' in lib.bdn_last_error()
    assert adam(16, 16, 16, 16, 16, 16, 1, 1, one, wd, 1.0, 0.9, 0.999, 1e-8, 0, 0, 16, None) != 0 and b'step' in lib.bdn_last_error()
    assert adam(16, 16, 16, 16, 16, 16, 1, 1, one, wd, 1.0, 0.9, 0.999, 1e-8, 0, 1, 18, None) != 0 and b'multiple of 4' in lib.bdn_last_error()
    assert lib.bdn_sgd_step_grouped(16, 16, 16, 16, 1, 9, nine, 1.0, 16, None) != 0 and b'9 groups' in lib.bdn_last_error()
    sgdm = lib.bdn_sgd_momentum_step_grouped
    assert sgdm(16, 16, 32, 16, 16, 1, 9, nine, nine, 1.0, 0.9, 0.0, 0, 1, 16, None) != 0 and b'9 groups' in lib.bdn_last_error()
    assert sgdm(16, 16, None, 16, 16, 1, 1, one, wd, 1.0, 0.9, 0.0, 0, 1, 16, None) != 0            # momentum without a buffer
    assert sgdm(16, 16, 32, 16, 16, 1, 1, one, wd, 1.0, 0.9, 0.1, 1, 1, 16, None) != 0 and b'nesterov' in lib.bdn_last_error()
    assert sgdm(16, 16, None, 16, 16, 1, 1, one, wd, 1.0, 0.0, 0.0, 0, 1, 0, None) == 0             # n == 0 launches nothing


# ---------------------------------------------------------------- the segment table
def _groupings(named, names):
    enc = [k for k in names if k.startswith(ENCODER)]
    dec = [k for k in names if not k.startswith(ENCODER)]
    nb = [k for k in names if is_norm_or_bias(k, named)]
    w = [k for k in names if not is_norm_or_bias(k, named)]
    mid = names[len(names) // 2]
    return {
        'one_group': ([{'params': names}], set()),
        'norms_biases_vs_weights': ([{'params': w, 'weight_decay': 1e-2}, {'params': nb, 'weight_decay': 0.0, 'lr': 1e-4}], set()),
        'encoder_decoder': ([{'params': enc, 'lr': 1e-4}, {'params': dec}], set()),
        'encoder_frozen': ([{'params': dec}], set(enc)),
        'encoder_frozen_two_groups': ([{'params': [k for k in dec if k in w]}, {'params': [k for k in dec if k in nb]}], set(enc)),
        'one_tensor_frozen': ([{'params': [k for k in names if k != mid]}], {mid}),
        'implicit_group': (None, set(enc)),
    }


@pytest.mark.parametrize('c', [13, 3])
@pytest.mark.parametrize('which', ['one_group', 'norms_biases_vs_weights', 'encoder_decoder', 'encoder_frozen',
                                   'encoder_frozen_two_groups', 'one_tensor_frozen', 'implicit_group'])
def test_segment_table_tiles_the_layout(c, which):
    _, named, names, layout = _model(c)
    groups, frozen = _groupings(named, names)[which]
    pg = ParamGroups(OptimConfig('adamw', lr=1e-3), names, groups, frozen)
    ends, ids = segment_table(layout, pg)
    assert len(ends) == len(ids) <= 256
    assert layout.total % 4 == 0 and ends[-1] == layout.total // 4, 'the segments end where the buffer ends'
    assert all(a < b for a, b in zip(ends, ends[1:])) and ends[0] > 0, 'sorted, none empty'
    assert all(a != b for a, b in zip(ids, ids[1:])), 'same-group neighbours are merged'
    assert all(g == FROZEN or 0 <= g < len(pg.groups) for g in ids)
    starts = [0] + ends[:-1]
    for k in names:                                                    # every tensor lies in exactly one segment, of its group
        off, n, _ = layout.slices[k]
        assert off % 4 == 0
        v0, v1 = off // 4, (off + n + 3) // 4
        hit = [j for j, (a, b) in enumerate(zip(starts, ends)) if a <= v0 and v1 <= b]
        assert len(hit) == 1, k
        want = FROZEN if k in frozen else next(j for j, g in enumerate(pg.groups) if k in g['params'])
        assert ids[hit[0]] == want == pg.group_id(k), k
    if which == 'one_group':
        assert ids == [0] and ends == [layout.total // 4]
    if which == 'encoder_frozen':
        assert FROZEN in ids and 0 in ids


# ---------------------------------------------------------------- the rejections
def test_group_rejections():
    _, named, names, _ = _model(3)
    cfg = OptimConfig('adamw', lr=1e-3)
    with pytest.raises(ValueError, match='at most 8'):
        ParamGroups(cfg, names, [{'params': [k]} for k in names[:MAX_GROUPS + 1]] + [{'params': names[MAX_GROUPS + 1:]}])
    with pytest.raises(ValueError, match='unknown parameter'):
        ParamGroups(cfg, names, [{'params': names + ['no.such.weight']}])
    with pytest.raises(ValueError, match='more than one param group'):
        ParamGroups(cfg, names, [{'params': names}, {'params': names[:1]}])
    with pytest.raises(ValueError, match='more than one param group'):
        ParamGroups(cfg, names, [{'params': names + names[:1]}])
    with pytest.raises(ValueError, match='in no param group'):
        ParamGroups(cfg, names, [{'params': names[1:]}])
    ParamGroups(cfg, names, [{'params': names[1:]}], frozen=names[:1])                     # frozen: it needs no group
    ParamGroups(cfg, names, [{'params': names}], frozen=names[:1])                         # ... and may be listed in one, as in torch
    with pytest.raises(ValueError, match='per-group betas'):
        ParamGroups(cfg, names, [{'params': names[:5]}, {'params': names[5:], 'betas': (0.8, 0.999)}])
    with pytest.raises(ValueError, match='per-group eps'):
        ParamGroups(cfg, names, [{'params': names, 'eps': 1e-6}])
    with pytest.raises(ValueError, match='per-group momentum'):
        ParamGroups(OptimConfig('sgd', momentum=0.9), names, [{'params': names, 'momentum': 0.5}])
    with pytest.raises(ValueError, match='unknown key'):
        ParamGroups(cfg, names, [{'params': names, 'warmup': 3}])
    with pytest.raises(ValueError, match='invalid lr'):
        ParamGroups(cfg, names, [{'params': names, 'lr': -1.0}])
    ok = ParamGroups(cfg, names, [{'params': names, 'betas': (0.9, 0.999), 'eps': 1e-8, 'amsgrad': False}])   # the rule's own values pass
    assert ok.groups[0]['lr'] == 1e-3 and ok.groups[0]['weight_decay'] == 1e-2            # missing keys: the step's


# ---------------------------------------------------------------- state exchange with torch.optim built with the same groups
_MAKERS = [
    ('sgd_momentum', OptimConfig('sgd', lr=0.1, momentum=0.9, nesterov=True),
     lambda gs: torch.optim.SGD(gs, lr=0.1, momentum=0.9, nesterov=True)),
    ('adam', OptimConfig('adam', lr=1e-3), lambda gs: torch.optim.Adam(gs, lr=1e-3)),
    ('adamw', OptimConfig('adamw', lr=1e-3, betas=(0.8, 0.99)), lambda gs: torch.optim.AdamW(gs, lr=1e-3, betas=(0.8, 0.99))),
]


def _three_groups(model, named, names):
    """weights of the decoder / weights of the encoder (lower lr) / norms and biases (no decay); `inc` frozen but still listed, one
    more tensor frozen and listed nowhere."""
    frozen = {k for k in names if k.startswith('inc.')} | {'down1.mpconv.1.conv.0.weight'}
    for k, p in named:
        p.requires_grad_(k not in frozen)
    listed = [k for k in names if k != 'down1.mpconv.1.conv.0.weight']
    g0 = [k for k in listed if not is_norm_or_bias(k, named) and not k.startswith(ENCODER)]
    g1 = [k for k in listed if not is_norm_or_bias(k, named) and k.startswith(ENCODER)]
    g2 = [k for k in listed if is_norm_or_bias(k, named)]
    groups = [{'params': g0, 'weight_decay': 1e-2}, {'params': g1, 'lr': 1e-4, 'weight_decay': 1e-2},
              {'params': g2, 'weight_decay': 0.0}]
    return groups, frozen


@pytest.mark.parametrize('name,cfg,make', _MAKERS, ids=[m[0] for m in _MAKERS])
def test_grouped_torch_state_round_trips_through_the_flat_layout(name, cfg, make):
    """torch.optim with three groups and frozen parameters, 3 steps on random gradients -> flat buffers -> torch format.  The result
    identifies a parameter by its index in model.parameters() (torch by its position in the concatenated groups; load_state_dict of
    either side matches by position inside each group), so entries are compared through that correspondence: tensor for tensor, key for
    key, and no entry for a frozen parameter.  It loads into a fresh optimizer of the same construction."""
    model, named, names, layout = _model(13)
    groups, frozen = _three_groups(model, named, names)
    by = dict(named)
    tg = lambda: [dict(g, params=[by[k] for k in g['params']]) for g in groups]        # noqa: E731
    opt = make(tg())
    for _ in range(3):
        for k, p in named:
            p.grad = torch.randn_like(p) if k not in frozen else None
        opt.step()
    sd = opt.state_dict()
    pg = ParamGroups(cfg, names, groups, frozen)
    cfg2, hyper, flat, step = torch_to_groups(sd, pg, layout)
    assert cfg2.kind == cfg.kind and step == (3 if cfg.family == 'adam' else 1)
    assert [h['lr'] for h in hyper] == [g['lr'] for g in sd['param_groups']]
    assert [h['weight_decay'] for h in hyper] == [g['weight_decay'] for g in sd['param_groups']]
    back = groups_to_torch(cfg2, pg, layout, flat, step)
    index = {k: i for i, k in enumerate(names)}
    assert len(back['param_groups']) == len(sd['param_groups']) == 3
    n_state = 0
    for g_t, g_b, g in zip(sd['param_groups'], back['param_groups'], groups):
        assert set(g_t) == set(g_b)
        assert all(g_t[key] == g_b[key] for key in g_t if key != 'params'), (g_t, g_b)
        assert g_b['params'] == [index[k] for k in g['params']]
        for pid_t, pid_b, k in zip(g_t['params'], g_b['params'], g['params']):
            if k in frozen:
                assert pid_t not in sd['state'] and pid_b not in back['state'], k
                continue
            s_t, s_b = sd['state'][pid_t], back['state'][pid_b]
            assert set(s_t) == set(s_b)
            n_state += 1
            for key, v in s_t.items():
                w = s_b[key]
                assert w.dtype == v.dtype and w.shape == v.shape and torch.equal(w, v), (k, key)
    assert n_state == len(back['state']) == len(sd['state']) == len(names) - len(frozen)
    fresh = make(tg())
    fresh.load_state_dict(back)
    for k, p in named:
        if k in frozen:
            assert p not in fresh.state or not fresh.state[p]
            continue
        for key, v in opt.state[p].items():
            assert torch.equal(fresh.state[p][key], v), (k, key)
    for g_f, g_t in zip(fresh.param_groups, opt.param_groups):
        assert g_f['lr'] == g_t['lr'] and g_f['weight_decay'] == g_t['weight_decay']


def test_exchange_rejections_and_ungrouped_state():
    model, named, names, layout = _model(3)
    cfg = OptimConfig('adam', lr=1e-3)
    opt = torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=1e-3)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    sd = opt.state_dict()
    # today's single-group optimizer_state_dict() (flat_to_torch) loads into a grouped step with one group: hyperparameters adopted
    one = ParamGroups(cfg, names, [{'params': names}])
    flat0 = {k: torch.zeros(layout.total) for k in cfg.state_keys()}
    for i, k in enumerate(names):
        for key in flat0:
            layout.view(flat0[key], k).copy_(sd['state'][i][key])
    single = flat_to_torch(OptimConfig.from_param_group(sd['param_groups'][0]), layout, names, flat0, 2)
    cfg2, hyper, flat, step = torch_to_groups(single, one, layout)
    assert step == 2 and hyper == [{'lr': 2e-3, 'weight_decay': 1e-3}] and all(torch.equal(flat[k], flat0[k]) for k in flat0)
    # ... and into a step with other groups, which keep their hyperparameters (None in their place); frozen parameters' state is dropped
    two = ParamGroups(cfg, names, [{'params': names[2:40]}, {'params': names[40:], 'lr': 5e-4}], frozen=names[:2])
    cfg3, hyper, flat, step = torch_to_groups(single, two, layout)
    assert hyper is None and step == 2
    assert not bool(layout.view(flat['exp_avg'], names[0]).any()) and torch.equal(layout.view(flat['exp_avg'], names[5]), sd['state'][5]['exp_avg'])
    by = dict(named)
    grouped = torch.optim.Adam([{'params': [by[k] for k in names[2:40]]}, {'params': [by[k] for k in names[40:]], 'lr': 5e-4}]).state_dict()
    with pytest.raises(ValueError, match='param groups'):
        torch_to_groups(grouped, one, layout)
    with pytest.raises(ValueError, match='covers'):
        torch_to_groups(grouped, ParamGroups(cfg, names, [{'params': names[2:41]}, {'params': names[41:]}], frozen=names[:2]), layout)
    bad = {'state': {}, 'param_groups': [grouped['param_groups'][0], dict(grouped['param_groups'][1], betas=(0.5, 0.999))]}
    with pytest.raises(ValueError, match='differs from group 0'):
        torch_to_groups(bad, two, layout)
    part = {'state': {0: sd['state'][2]}, 'param_groups': grouped['param_groups']}
    with pytest.raises(ValueError, match='all or none'):
        torch_to_groups(part, two, layout)


# ---------------------------------------------------------------- the float64 restatement of the grouped update
_RULES = [('sgd_momentum', 'sgd', dict(momentum=0.9)), ('sgd_nesterov', 'sgd', dict(momentum=0.9, nesterov=True)), ('sgd_plain', 'sgd', dict()),
          ('adam', 'adam', dict()), ('adamw', 'adamw', dict())]


@pytest.mark.parametrize('name,kind,rule', _RULES, ids=[r[0] for r in _RULES])
def test_grouped_restatement_matches_cpu_torch_optim(name, kind, rule):
    """5 steps of CPU torch.optim (foreach=False) with three groups (lr and weight decay differ) and one parameter without a gradient,
    against the restatement applied segment by segment, each step from torch's own float32 parameters and state, within R.ULPS."""
    torch.manual_seed(2)
    sizes = [1028, 512, 2052, 260]
    ps = [torch.nn.Parameter(torch.randn(n)) for n in sizes]
    hyper = [(0.05, 1e-2), (0.005, 0.0), (0.02, 1e-3)]
    gid = [0, 1, FROZEN, 2]
    tgroups = [{'params': [ps[0]], 'lr': 0.05, 'weight_decay': 1e-2}, {'params': [ps[1], ps[2]], 'lr': 0.005, 'weight_decay': 0.0},
               {'params': [ps[3]], 'lr': 0.02, 'weight_decay': 1e-3}]
    if kind == 'sgd':
        opt = torch.optim.SGD(tgroups, lr=1.0, foreach=False, **rule)
    else:
        opt = (torch.optim.AdamW if kind == 'adamw' else torch.optim.Adam)(tgroups, lr=1.0, foreach=False, **rule)
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    segs = [(offs[i], offs[i + 1], gid[i]) for i in range(4)]
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])      # noqa: E731
    keys = {'sgd': {'buf': 'momentum_buffer'} if rule.get('momentum') else {}}.get(kind, {'m': 'exp_avg', 'v': 'exp_avg_sq'})
    for it in range(5):
        gs = [torch.randn(n) * (0.5 + it) for n in sizes]
        p0 = cat(ps).clone()
        st0 = {k: cat([opt.state[p].get(tk, torch.zeros_like(p)) for p in ps]).clone() for k, tk in keys.items()}
        for p, g, i in zip(ps, gs, gid):
            p.grad = g.clone() if i != FROZEN else None
        opt.step()
        ref = grouped_reference(kind, rule, segs, hyper, p0, cat(gs), st0, it + 1)
        R.check(cat(ps), *ref['p'], f'{name} step {it} p')
        for k, tk in keys.items():
            R.check(cat([opt.state[p].get(tk, torch.zeros_like(p)) for p in ps]), *ref[k], f'{name} step {it} {tk}')
        assert torch.equal(ps[2].detach(), p0[offs[2]:offs[3]]) and not opt.state[ps[2]]
