"""-m gpu: the kernels between backward and the update (include/bidate_hip.h bdn_grad_accumulate, bdn_grad_norm, bdn_*_step_grouped_ex),
on guard-banded buffers.

bdn_grad_accumulate bit for bit against torch's float32 copy_ / add_; bdn_grad_norm against the float64 norm of the same float32 data
(tests/grad_clip_ref.py, pinned against CPU clip_grad_norm_ in tests/test_grad_clip_cpu.py), with frozen segments NaN-filled so that a
read of them poisons the result, on ill-conditioned data, and twice for its bits; the _ex update rules against the float64 restatement
of tests/optim_ref.py with the product of the two float32 scale factors, and bit for bit against the plain grouped entry points at a
coefficient of 1."""
import math

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.optim import FROZEN
from tests import grad_clip_ref as G
from tests import guard
from tests import optim_ref as R
from tests.guard import guarded
from tests.param_groups_ref import grouped_reference

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
EPS32 = G.EPS32
CHUNK = 16384            # floats per stage-1 partial of bdn_grad_norm (4096 float4 vectors per block)


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize('n', [1, 3, 4, 1023, 4_000_003])
@guarded
def test_accumulate_copies_and_adds_like_torch(n):
    gen = torch.Generator(device='cpu').manual_seed(n)
    a, b, c = (torch.randn(n, generator=gen) * 10.0 ** k for k in (0, 3, -3))
    acc = guard.full((n,), float('nan'), device=dev)          # add = 0 must not read it
    ga, gb, gc = (guard.guard(t, dev) for t in (a, b, c))
    st = _lib.stream_ptr()
    _lib.call('bdn_grad_accumulate', acc.data_ptr(), ga.data_ptr(), n, 0, st)
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), a)
    _lib.call('bdn_grad_accumulate', acc.data_ptr(), gb.data_ptr(), n, 1, st)
    _lib.call('bdn_grad_accumulate', gc.data_ptr(), acc.data_ptr(), n, 1, st)          # the last micro-step: g = g + acc
    torch.cuda.synchronize()
    want = a.clone().add_(b)
    assert torch.equal(acc.cpu(), want)
    assert torch.equal(gc.cpu(), c.clone().add_(want))
    assert torch.equal(ga.cpu(), a) and torch.equal(gb.cpu(), b), 'a source was written'


@guarded
def test_accumulate_on_a_sub_range_leaves_the_rest_alone():
    n, a, b = 40_000, 1028, 33_796                            # a, b multiples of 4; neither the range nor its ends are block multiples
    gen = torch.Generator(device='cpu').manual_seed(5)
    src = torch.full((n,), float('nan'))
    src[a:b] = torch.randn(b - a, generator=gen)
    inner = torch.randn(b - a, generator=gen)
    dst = torch.full((n,), float('nan'))
    dst[a:b] = inner
    gs, gd = guard.guard(src, dev), guard.guard(dst, dev)
    _lib.call('bdn_grad_accumulate', gd.data_ptr() + 4 * a, gs.data_ptr() + 4 * a, b - a, 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = gd.cpu()
    assert torch.equal(out[a:b], inner + src[a:b])
    assert bool(torch.isnan(out[:a]).all()) and bool(torch.isnan(out[b:]).all())
    _lib.call('bdn_grad_accumulate', gd.data_ptr() + 4 * a, gs.data_ptr() + 4 * a, b - a, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = gd.cpu()
    assert torch.equal(out[a:b], src[a:b]) and bool(torch.isnan(out[:a]).all()) and bool(torch.isnan(out[b:]).all())


# ---------------------------------------------------------------- norm
def _table(n, variant, seed=0):
    """-> (device table or None, [(start, stop, id)] in elements or None).  'groups': ~11 segments cut at random float4 boundaries, ids
    cycling through three groups; 'frozen': the same with the first and the last segment frozen (a buffer too short for three segments:
    one segment, frozen); 'short': 'groups' with the middle segment frozen and the last end 5 vectors short of n / 4 (fewer where the last
    segment is shorter than 6 vectors), so that the vectors behind it belong to no segment and do not count."""
    if variant == 'none':
        return None, None
    n4 = n // 4
    gen = torch.Generator().manual_seed(seed + n)
    n_seg = min(n4, 11)
    cuts = sorted(set((torch.randperm(n4 - 1, generator=gen)[:n_seg - 1] + 1).tolist())) if n4 > 1 else []
    ends = cuts + [n4]
    ids = [j % 3 for j in range(len(ends))]
    if variant == 'frozen':
        ids[0] = ids[-1] = FROZEN
    if variant == 'short':
        ends[-1] = max(n4 - 5, (cuts[-1] if cuts else 0) + 1)
        if len(ids) > 2:
            ids[len(ids) // 2] = FROZEN
    starts = [0] + ends[:-1]
    tab = (guard.guard(torch.tensor(ends, dtype=torch.int64).to(torch.int32), dev), guard.guard(torch.tensor(ids, dtype=torch.int32), dev))
    return tab, [(4 * a, 4 * b, g) for a, b, g in zip(starts, ends, ids)]


def _norm(g, tab, grad_scale, max_norm, ws=None):
    n = g.numel()
    if ws is None:
        ws = guard.alloc_bytes(_lib.load().bdn_grad_norm_workspace_bytes(n), dev)
    out = guard.full((2,), float('nan'), device=dev)
    t = (None, None, 0) if tab is None else (tab[0].data_ptr(), tab[1].data_ptr(), tab[0].numel())
    _lib.call('bdn_grad_norm', g.data_ptr(), *t, grad_scale, max_norm, ws.data_ptr(), out.data_ptr(), n, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_coef(out, max_norm):
    """out[1] within one float32 ulp of torch's formula applied to the returned out[0]."""
    want = G.coef32(out[0], max_norm)
    if math.isnan(float(want)):
        assert math.isnan(float(out[1]))
    else:
        assert abs(float(out[1]) - float(want)) <= float(np.spacing(np.float32(abs(want)))), (out, want)


# 4: one vector.  1020 / 1024: one vector short of, and exactly, one pass of a block's 256 lanes.  16388: one vector past the first partial
# chunk (CHUNK floats per block).  4_000_004: 244 whole chunks and a ragged last block of 577 vectors.
@pytest.mark.parametrize('variant', ['none', 'groups', 'frozen', 'short'])
@pytest.mark.parametrize('n', [4, 1020, 1024, CHUNK + 4, 4_000_004])
@guarded
def test_norm_matches_float64_and_skips_frozen_segments(n, variant):
    assert n % 4 == 0 and (n <= CHUNK or n % CHUNK != 0)
    gen = torch.Generator(device='cpu').manual_seed(n + len(variant))
    g = torch.randn(n, generator=gen) * 3.0
    tab, segs = _table(n, variant)
    if variant in ('frozen', 'short'):
        for a, b, gid in segs:
            if gid == FROZEN:
                g[a:b] = float('nan')                         # a read of a frozen vector poisons the norm
        g[segs[-1][1]:] = float('nan')                        # and so does a read behind the table's end ('short')
        assert variant == 'short' or (bool(torch.isnan(g[:4]).all()) and bool(torch.isnan(g[-4:]).all()))
        assert variant == 'frozen' or n < CHUNK or bool(torch.isnan(g[-20:]).all())
    gs = 0.5
    ref = G.norm(g, segs, gs)
    assert math.isfinite(ref)
    max_norm = ref / 2 if ref > 0 else 1.0                    # the clip is active
    gd = guard.guard(g, dev)
    out = _norm(gd, tab, gs, max_norm)
    print(f'n={n} {variant}: norm {out[0]!r} (float64 {ref!r}, rel err {abs(float(out[0]) - ref) / max(ref, 1e-300):.3e}), coef {out[1]!r}')
    assert abs(float(out[0]) - ref) <= 2 * EPS32 * ref, (out, ref)
    _check_coef(out, max_norm)
    if ref > 0:
        assert 0.49 < float(out[1]) < 0.51
    else:
        assert float(out[0]) == 0.0 and float(out[1]) == 1.0  # everything frozen: nothing read, norm 0, no clipping
    again = _norm(gd, tab, gs, max_norm)
    assert out.tobytes() == again.tobytes(), 'a repeat run differs'
    assert torch.equal(gd.cpu().view(torch.int32), g.view(torch.int32)), 'the gradients were written'


@pytest.mark.parametrize('case', ['huge', 'tiny', 'nan', 'inf_max_norm', 'zeros'])
@guarded
def test_norm_on_ill_conditioned_data(case):
    n = 2 * CHUNK + 1028                                      # three partials, the last one ragged
    g = torch.zeros(n)
    max_norm = 1.0
    if case == 'huge':
        g.fill_(1e25)                                         # squares overflow float32; the norm, 1e25 sqrt(n), does not
    elif case == 'tiny':
        g.fill_(1e-30)                                        # squares underflow float32 to 0; the norm must not be 0
        max_norm = 1e-30
    elif case == 'nan':
        g = torch.randn(n, generator=torch.Generator().manual_seed(1))
        g[CHUNK + 77] = float('nan')
    elif case == 'inf_max_norm':
        g = torch.randn(n, generator=torch.Generator().manual_seed(2)) * 100.0
        max_norm = float('inf')
    out = _norm(guard.guard(g, dev), None, 1.0, max_norm)
    print(f'{case}: norm {out[0]!r} coef {out[1]!r}')
    if case == 'nan':
        assert math.isnan(float(out[0])) and math.isnan(float(out[1])), out
        return
    ref = G.norm(g)
    assert abs(float(out[0]) - ref) <= 2 * EPS32 * ref, (out, ref)
    _check_coef(out, max_norm)
    if case in ('huge', 'tiny'):
        assert float(out[0]) > 0 and math.isfinite(float(out[0])) and 0 < float(out[1]) < 1
    elif case == 'inf_max_norm':
        assert float(out[1]) == 1.0 and float(out[0]) > 1000
    else:
        assert float(out[0]) == 0.0 and float(out[1]) == 1.0


# ---------------------------------------------------------------- the _ex update rules
# the rules of tests/test_gpu_optim.py's _KERNEL_CASES (name, rule, grad_scale), and plain SGD for bdn_sgd_step_grouped_ex
_KERNEL_CASES = [
    ('sgd_plain', dict(kind='sgd_plain'), 0.5),
    ('sgd_m', dict(kind='sgd', momentum=0.9), 1.0),
    ('sgd_m_damp', dict(kind='sgd', momentum=0.9, dampening=0.1), 0.5),
    ('sgd_nesterov', dict(kind='sgd', momentum=0.9, nesterov=True), 1.0),
    ('sgd_nesterov_wd', dict(kind='sgd', momentum=0.9, nesterov=True, weight_decay=1e-2), 0.5),
    ('sgd_m_wd', dict(kind='sgd', momentum=0.8, weight_decay=1e-2), 1.0),
    ('sgd_wd_only', dict(kind='sgd', weight_decay=1e-2), 0.5),
    ('adam', dict(kind='adam'), 1.0),
    ('adam_l2', dict(kind='adam', weight_decay=1e-2), 0.5),
    ('adamw', dict(kind='adamw', weight_decay=1e-2), 1.0),
    ('adamw_gs', dict(kind='adamw', weight_decay=1e-2, betas=(0.8, 0.99)), 0.5),
]
_LRS, _WD_FACTORS = (0.01, 0.001, 0.02), (1.0, 0.0, 2.0)        # three groups: their own lr, and the rule's weight decay x 1, 0, 2


def _call(case, ex, p, g, state, tab, hyper, gs, ds, step):
    st = _lib.stream_ptr()
    lr, wd = _lib.floats([h[0] for h in hyper]), _lib.floats([h[1] for h in hyper])
    t = (tab[0].data_ptr(), tab[1].data_ptr(), tab[0].numel(), len(hyper))
    sfx, extra = ('_ex', (ds.data_ptr(),)) if ex else ('', ())
    kind = case['kind']
    if kind == 'sgd_plain':
        _lib.call('bdn_sgd_step_grouped' + sfx, p.data_ptr(), g.data_ptr(), *t, lr, gs, *extra, p.numel(), st)
    elif kind == 'sgd':
        _lib.call('bdn_sgd_momentum_step_grouped' + sfx, p.data_ptr(), g.data_ptr(), _lib.ptr(state.get('buf')), *t, lr, wd, gs, *extra,
                  case.get('momentum', 0.0), case.get('dampening', 0.0), int(case.get('nesterov', False)), int(step == 1), p.numel(), st)
    else:
        b1, b2 = case.get('betas', (0.9, 0.999))
        _lib.call('bdn_adam_step_grouped' + sfx, p.data_ptr(), g.data_ptr(), state['m'].data_ptr(), state['v'].data_ptr(), *t, lr, wd, gs,
                  *extra, b1, b2, 1e-8, int(kind == 'adamw'), step, p.numel(), st)


def _fresh_state(case, n):
    if case['kind'] in ('adam', 'adamw'):
        return {'m': guard.zeros(n, device=dev), 'v': guard.zeros(n, device=dev)}
    if case.get('momentum', 0.0):
        return {'buf': guard.full((n,), float('nan'), device=dev)}          # the first step must not read it
    return {}


@pytest.mark.parametrize('ds', [1.0, 0.37])
@pytest.mark.parametrize('name,case,gs', _KERNEL_CASES, ids=[c[0] for c in _KERNEL_CASES])
@guarded
def test_ex_update_takes_the_device_scale(name, case, gs, ds):
    """Three steps, three groups and a frozen segment (NaN gradients), n no multiple of a block's 1024 vectors: every element within
    R.ULPS + 1 of the restatement with grad_scale replaced by the float64 product of the two float32 factors (the kernel rounds that
    product once more); frozen elements keep their bits; with a device scale of 1.0 the bits are the plain grouped entry point's."""
    n = 300_004
    wd0 = case.get('weight_decay', 0.0)
    hyper = [(lr, wd0 * f) for lr, f in zip(_LRS, _WD_FACTORS)]
    n4 = n // 4
    gen = torch.Generator(device='cpu').manual_seed(len(name) * 131 + int(ds * 100))
    cuts = sorted(set((torch.randperm(n4 - 1, generator=gen)[:10] + 1).tolist()))
    ends = cuts + [n4]
    ids = [FROZEN if j == 4 else j % 3 for j in range(len(ends))]
    segs = [(4 * a, 4 * b, gid) for a, b, gid in zip([0] + ends[:-1], ends, ids)]
    tab = (guard.guard(torch.tensor(ends, dtype=torch.int64).to(torch.int32), dev), guard.guard(torch.tensor(ids, dtype=torch.int32), dev))
    mask = torch.zeros(n, dtype=torch.bool)
    for a, b, gid in segs:
        mask[a:b] = gid == FROZEN
    assert bool(mask.any())
    p = guard.guard(torch.randn(n, generator=gen), dev)
    p[::7] *= 1e-3
    grads = []
    for it in range(3):
        g = torch.randn(n, generator=gen) * (0.3 + it)
        g[mask] = float('nan')
        grads.append(guard.guard(g, dev))
    dsd = guard.full((1,), ds, device=dev)
    state = _fresh_state(case, n)
    twin_p, twin_state = (guard.clone(p), _fresh_state(case, n)) if ds == 1.0 else (None, None)
    scale = float(np.float32(gs)) * float(np.float32(ds))     # the float64 product of the two float32 factors
    rkind = 'sgd' if case['kind'] == 'sgd_plain' else case['kind']
    for it, g in enumerate(grads):
        p_in, s_in = p.clone(), {k: v.clone() for k, v in state.items()}
        _call(case, True, p, g, state, tab, hyper, gs, dsd, it + 1)
        torch.cuda.synchronize()
        if it == 0 and 'buf' in s_in:
            s_in['buf'] = torch.zeros_like(s_in['buf'])
            assert bool(torch.isnan(state['buf'].cpu()[mask]).all()) and not bool(torch.isnan(state['buf'].cpu()[~mask]).any())
        gg = g.cpu().clone()
        gg[mask] = 0.0
        s_ref = {k: torch.where(mask, torch.zeros(()), v.cpu()) for k, v in s_in.items()}
        ref = grouped_reference(rkind, case, segs, hyper, p_in.cpu(), gg, s_ref, it + 1, scale)
        R.check(p, *ref['p'], f'{name} ds={ds} step {it} params', ulps=R.ULPS + 1)
        for key in state:
            got = torch.where(mask.to(dev), torch.zeros((), device=dev), state[key])
            R.check(got, *ref[key], f'{name} ds={ds} step {it} {key}', ulps=R.ULPS + 1)
        assert torch.equal(p.cpu()[mask], p_in.cpu()[mask]) and bool((p != p_in).any())
        if twin_p is not None:
            _call(case, False, twin_p, g, twin_state, tab, hyper, gs, None, it + 1)
            torch.cuda.synchronize()
            assert torch.equal(twin_p, p), f'{name} step {it}: a device scale of 1.0 changed the bits'
            for key in state:
                assert torch.equal(twin_state[key].view(torch.int32), state[key].view(torch.int32)), (name, it, key)
