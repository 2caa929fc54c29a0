"""-m gpu: bdn_mad_centre / _moments / _solve / _chi2 / _mask (include/bidate_hip.h; fabric_amd.utils.mad) through the C ABI on guard-banded
buffers, with a workspace of exactly the queried size born as 0xFF and outputs born as NaN, against tests/mad_ref.py.  Every entry runs
twice and must give the same bits.  The reduction tree and the Jacobi sweeps legitimately differ from numpy's and LAPACK's, so the
comparison with the twin is within bounds:

  centre, moments   the header's bound n 2^-53 sum |term|, times 4 for the twin's own rounding (derived, not measured); n_valid exact.
  solve             rho 1e-10, var 2e-10, mean 1e-12 of the band's scale (expectations: everything is float64 on well-conditioned blocks).
                    a and b only for variates whose rho lies more than 1e-3 from its neighbours in the twin: a singular vector moves by
                    (error of K) / gap, about 1e-13 / 1e-3, and Lx^-T scales it by at most the size of a, so 1e-8 max |a_i|.
  a whole run       rho RHO_TOL, var twice that; mean 2^-24 of the largest value (the weights of the later iterations are float32 rasters
                    that may differ from the twin's in the last bit at some pixels, and a weighted mean moves by at most that share of the
                    largest value); a, b AB_REL and the variates VARIATES_REL (relative to |M_i| + sqrt(var_i)), both for the separated
                    variates; chi2 CHI2_ULP float32 ulp; proba PROBA_ULP float32 ulp plus 8 * 2^-53 (1 - Q is formed in double from a Q
                    whose absolute error is a few 2^-53, however small the difference).  The expectation was rho 1e-10 and 2 ulp; each
                    bound is the larger of the expectation and ten times the largest error measured on an MI355X over the cases below:
                    MEASURED holds those figures, DESIGN.md section 25 discusses them.

Shapes: the smallest that can still go wrong -- 1 x 1 (too few pixels), 37 x 53 with n_b in {1, 2, 3, 13} (one block of tiles, the last
tile partial), 97 x 131 with n_b = 13 (199 tiles, the last one partial), bands [4, 1] of a 5-band stack."""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from gpu_util import dev, st
from tests import guard
from tests import mad_ref as MR
from tests import sched_stress as ss
from tests.guard import guarded

pytestmark = pytest.mark.gpu
EXV = 9
U = 2.0 ** -53
# the largest errors measured on an MI355X over the whole-run cases of this file (test_a_whole_run prints them)
MEASURED = {'rho': 3.9e-12, 'chi2_ulp': 1.0, 'proba_ulp': 1.0, 'variates_rel': 1.1e-7, 'ab_rel': 2.5e-10}
RHO_TOL = max(1e-10, 10 * MEASURED['rho'])
CHI2_ULP = max(2.0, 10 * MEASURED['chi2_ulp'])
PROBA_ULP = max(2.0, 10 * MEASURED['proba_ulp'])
VARIATES_REL = max(2.0 ** -22, 10 * MEASURED['variates_rel'])       # the expectation: 2 float32 ulp, relative to |M_i| + sqrt(var_i)
AB_REL = max(1e-8, 10 * MEASURED['ab_rel'])                         # the expectation: that of a single solve


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


class Scene:
    """The two dates, the band list and the exclude raster on the device, guarded."""

    def __init__(self, d1, d2, bands, ex=None):
        self.h_d1, self.h_d2, self.bands, self.h_ex = d1, d2, list(bands), ex
        self.C, self.H, self.W = d1.shape
        self.nb = len(bands)
        self.d1, self.d2 = dev(torch.from_numpy(d1)), dev(torch.from_numpy(d2))
        self.band_t = dev(torch.tensor(self.bands), torch.int32)
        self.ex = None if ex is None else dev(torch.from_numpy(ex), torch.uint8)
        self.args = (self.d1.data_ptr(), self.d2.data_ptr(), self.band_t.data_ptr(), self.nb, _lib.ptr(self.ex), EXV if ex is not None else 0)
        self.shape = (self.C, self.H, self.W)

    def ws(self):
        return guard.alloc_bytes(_lib.load().bdn_mad_workspace_bytes(self.nb, self.H, self.W), label='mad workspace')

    def twin_kw(self):
        return dict(exclude=self.h_ex, exclude_value=EXV if self.h_ex is not None else None)


def _centre(s, stream=None):
    cen, nv = guard.empty(2 * s.nb, dtype=torch.float64), guard.empty(1, dtype=torch.int64)
    _lib.call('bdn_mad_centre', *s.args, cen.data_ptr(), nv.data_ptr(), s.ws().data_ptr(), *s.shape, st() if stream is None else stream)
    return cen, nv


def _moments(s, cen, weight=None, state=None, mom=None, stream=None):
    mom = guard.empty(MR.moment_doubles(s.nb), dtype=torch.float64) if mom is None else mom
    _lib.call('bdn_mad_moments', *s.args, _lib.ptr(weight), cen.data_ptr(), _lib.ptr(state), mom.data_ptr(), s.ws().data_ptr(), *s.shape,
              st() if stream is None else stream)
    return mom


def _solve(s, mom, cen, nv, first, tol, state=None, min_var=1e-9, stream=None):
    state = guard.empty(MR.state_doubles(s.nb), dtype=torch.float64) if state is None else state
    _lib.call('bdn_mad_solve', mom.data_ptr(), cen.data_ptr(), nv.data_ptr(), s.nb, 1 if first else 0, float(tol), float(min_var), state.data_ptr(),
              st() if stream is None else stream)
    return state


def _chi2(s, state, out=None, stream=None):
    chi2, proba, var = out if out is not None else (guard.empty(s.H, s.W), guard.empty(2, s.H, s.W), guard.empty(s.nb, s.H, s.W))
    _lib.call('bdn_mad_chi2', *s.args, state.data_ptr(), chi2.data_ptr(), proba.data_ptr(), var.data_ptr(), *s.shape, st() if stream is None else stream)
    return chi2, proba, var


def _mask(s, proba, thr, out_bad):
    m = guard.empty(s.H, s.W, dtype=torch.uint8)
    _lib.call('bdn_mad_mask', proba.data_ptr(), *s.args, float(thr), out_bad, m.data_ptr(), *s.shape, st())
    return m


def _run(s, iters, tol, stream=None):
    """The driver's sequence by hand: (chi2, proba, variates, state), every buffer born as 0xFF (NaN)."""
    cen, nv = _centre(s, stream)
    mom = guard.empty(MR.moment_doubles(s.nb), dtype=torch.float64)
    state = guard.empty(MR.state_doubles(s.nb), dtype=torch.float64)
    out = (guard.empty(s.H, s.W), guard.empty(2, s.H, s.W), guard.empty(s.nb, s.H, s.W))
    for it in range(iters):
        _moments(s, cen, None if it == 0 else out[1], None if it == 0 else state, mom, stream)
        _solve(s, mom, cen, nv, it == 0, tol, state, stream=stream)
        _chi2(s, state, out, stream)
    return out + (state,)


def _ulp32(got, want):
    """|got - want| in units of the float32 spacing at want."""
    want = want.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _data(kind):
    """(d1, d2, bands, exclude or None, weight or None) of a named case.  Shared: never modified."""
    r = np.random.default_rng(99)
    if kind.startswith('37x53/'):
        nb = int(kind.split('/')[1])
        d1, d2, _ = MR.scene(nb, nb, 37, 53)
        return d1, d2, list(range(nb)), None, None
    if kind == '97x131':
        d1, d2, _ = MR.scene(7, 13, 97, 131)
        return d1, d2, list(range(13)), None, None
    if kind == 'subset':
        d1, d2, _ = MR.scene(5, 5, 37, 53)
        return d1, d2, [4, 1], None, None
    if kind == 'exclude':
        d1, d2, _ = MR.scene(6, 3, 37, 53)
        return d1, d2, [0, 1, 2], np.where(r.random((37, 53)) < 0.1, EXV, 0).astype(np.uint8), None
    if kind == 'nonfinite':
        d1, d2, _ = MR.scene(8, 3, 37, 53)
        d2 = d2.copy()
        k = r.choice(37 * 53, 60, replace=False)
        d2[1].reshape(-1)[k] = r.choice([np.nan, np.inf, -np.inf], 60)          # one band of one date only
        return d1, d2, [0, 1, 2], None, None
    if kind == 'weight':
        d1, d2, _ = MR.scene(9, 3, 37, 53)
        w = r.random((37, 53)).astype(np.float32)
        w[r.random((37, 53)) < 0.3] = 0
        return d1, d2, [0, 1, 2], None, w
    if kind == 'offset':
        d1, d2, _ = MR.scene(10, 3, 37, 53, offset=1000.0)
        return d1, d2, [0, 1, 2], None, None
    raise KeyError(kind)


CASES = ['37x53/1', '37x53/2', '37x53/3', '37x53/13', '97x131', 'subset', 'exclude', 'nonfinite', 'weight', 'offset']
RUNS = ['37x53/1', '37x53/2', '37x53/3', '37x53/13', '97x131', 'subset', 'exclude', 'nonfinite', 'offset']


# ---------------------------------------------------------------- centre and moments
@pytest.mark.parametrize('kind', CASES)
@guarded
def test_centre_and_moments_within_the_derived_bound(kind):
    d1, d2, bands, ex, w = _data(kind)
    s = Scene(d1, d2, bands, ex)
    nb = s.nb
    runs = [_centre(s) for _ in range(2)]
    assert _same(*runs)
    cen, nv = runs[0]
    want_c, n, abs_c = MR.centre_ref(d1, d2, bands, with_abs=True, **s.twin_kw())
    got_c = cen.cpu().numpy()
    assert int(nv.item()) == n > 0
    bound = 4 * n * U * abs_c / n + U * np.abs(want_c)
    print(f'{kind}: centre largest error / bound = {(np.abs(got_c - want_c) / bound).max():.3g}')
    assert (np.abs(got_c - want_c) <= bound).all()
    if kind == 'offset':
        assert (np.abs(got_c) > 990).all()
    w_d = None if w is None else dev(torch.from_numpy(w))
    moms = [_moments(s, cen, w_d) for _ in range(2)]
    assert _same(moms, moms[::-1]) and torch.equal(_bits(moms[0]), _bits(moms[1]))
    got = MR.unpack_moments(moms[0].cpu().numpy(), nb)
    s0, s1, s2, (a0, a1, a2), nval = MR.moments_ref(d1, d2, bands, got_c, w, with_abs=True, **s.twin_kw())
    assert nval == n
    worst = 0.0
    for g, want, a in ((got[0], s0, a0), (got[1], s1, a1), (got[2], s2, a2)):
        err, bnd = np.abs(np.asarray(g) - want), 4 * n * U * np.asarray(a)
        assert (err <= bnd).all(), (kind, float(np.max(err / np.maximum(bnd, 1e-300))))
        worst = max(worst, float(np.max(err / np.maximum(bnd, 1e-300))))
    print(f'{kind}: moments largest error / bound = {worst:.3g}')
    if w is not None:
        assert got[0] < 0.6 * n                              # the zeros took part as zeros


@guarded
def test_a_band_outside_the_stack_and_a_single_pixel():
    d1, d2, _, _, _ = _data('37x53/3')
    s = Scene(d1, d2, [0, 3, 1])                             # 3 is outside a 3-band stack
    cen, nv = _centre(s)
    assert int(nv.item()) == 0 and (cen.cpu().numpy() == 0).all()
    out = _run(s, 2, 0.0)
    state = MR.unpack_state(out[3].cpu().numpy(), 3)
    assert state['ok'] == 0 and state['n_valid'] == 0 and state['converged'] == 1 and state['iter'] == 1 and state['skip'] == 1
    assert all(torch.isnan(t).all() for t in out[:3])
    one = Scene(np.array([[[2.5]]], np.float32), np.array([[[1.5]]], np.float32), [0])
    runs = [_run(one, 1, 0.0) for _ in range(2)]
    assert _same(*runs)
    state = MR.unpack_state(runs[0][3].cpu().numpy(), 1)
    assert state['ok'] == 0 and state['n_valid'] == 1 and state['S0'] == 1.0 and all(torch.isnan(t).all() for t in runs[0][:3])
    m = _mask(one, runs[0][1], 0.5, 7)
    assert m.cpu().numpy().tolist() == [[0]]


# ---------------------------------------------------------------- the solve
@pytest.mark.parametrize('kind', CASES)
@guarded
def test_solve_against_the_twin_on_the_device_moments(kind):
    d1, d2, bands, ex, w = _data(kind)
    s = Scene(d1, d2, bands, ex)
    nb = s.nb
    cen, nv = _centre(s)
    mom = _moments(s, cen, None if w is None else dev(torch.from_numpy(w)))
    states = [_solve(s, mom, cen, nv, True, 1e-3) for _ in range(2)]
    assert torch.equal(_bits(states[0]), _bits(states[1]))
    got = MR.unpack_state(states[0].cpu().numpy(), nb)
    want = MR.solve_ref(*MR.unpack_moments(mom.cpu().numpy(), nb), cen.cpu().numpy(), int(nv.item()), nb, None, 1e-3, 1e-9)
    assert (got['iter'], got['ok'], got['converged'], got['skip'], got['n_valid']) == (1, 1, 0, 0, want['n_valid']) and got['delta'] == np.inf
    assert got['S0'] == want['S0'] and np.array_equal(got['centre'], want['centre'])
    e_rho, e_var = np.abs(got['rho'] - want['rho']).max(), np.abs(got['var'] - want['var']).max()
    scale = np.sqrt(np.abs(np.diag(MR.unpack_moments(mom.cpu().numpy(), nb)[2])) / want['S0']) + np.abs(want['mean'])
    e_mean = (np.abs(got['mean'] - want['mean']) / scale).max()
    rho = want['rho']
    sep = np.minimum(np.abs(np.diff(rho, prepend=np.inf)), np.abs(np.diff(rho, append=-np.inf))) > 1e-3
    assert sep.any(), 'the case keeps no separated variate'
    e_ab = max(float((np.abs(got[k][sep] - want[k][sep]).max(1) / np.abs(want[k][sep]).max(1)).max()) for k in ('a', 'b'))
    print(f'{kind}: rho {e_rho:.3g} var {e_var:.3g} mean {e_mean:.3g} a,b {e_ab:.3g} on {int(sep.sum())} of {nb} variates')
    assert (np.diff(got['rho']) <= 0).all() and (got['rho'] <= 1).all() and (got['rho'] >= 0).all()
    assert e_rho <= 1e-10 and e_var <= 2e-10 and e_mean <= 1e-12 and e_ab <= 1e-8
    # the variates have unit weighted variance and correlation rho
    _, _, s2 = MR.unpack_moments(mom.cpu().numpy(), nb)
    mz = mom.cpu().numpy()[1:1 + 2 * nb] / want['S0']
    cov = s2 / want['S0'] - np.outer(mz, mz)
    for i in range(nb):
        a, b = got['a'][i], got['b'][i]
        assert abs(a @ cov[:nb, :nb] @ a - 1) < 1e-9 and abs(b @ cov[nb:, nb:] @ b - 1) < 1e-9 and abs(a @ cov[:nb, nb:] @ b - got['rho'][i]) < 1e-9


# ---------------------------------------------------------------- a whole run
@pytest.mark.parametrize('kind', RUNS)
@guarded
def test_a_whole_run(kind):
    d1, d2, bands, ex, _ = _data(kind)
    s = Scene(d1, d2, bands, ex)
    runs = [_run(s, 6, 0.0) for _ in range(2)]
    assert _same(*runs)
    chi2, proba, var, state = (t.cpu().numpy() for t in runs[0])
    want = MR.irmad_ref(d1, d2, bands, iters=6, tol=0.0, **s.twin_kw())
    got = MR.unpack_state(state, s.nb)
    ws = want['state']
    assert (got['iter'], got['ok'], got['converged'], got['skip'], got['n_valid']) == (6, 1, 0, 0, ws['n_valid'])
    valid = want['valid']
    assert (chi2[~valid] == 0).all() and (proba[0][~valid] == 1).all() and (proba[1][~valid] == 0).all() and (var[:, ~valid] == 0).all()
    e_rho = np.abs(got['rho'] - ws['rho']).max()
    e_chi = _ulp32(chi2, want['chi2'])[valid].max()
    e_p = max(float(((np.abs(proba[k].astype(np.float64) - want['proba'][k].astype(np.float64)) - 8 * U).clip(0) /
                     np.spacing(np.abs(want['proba'][k])).astype(np.float64))[valid].max()) for k in (0, 1))
    e_delta = abs(got['delta'] - ws['delta'])
    sd = np.sqrt(np.maximum(ws['var'], 1e-9))[:, None]
    e_var = float((np.abs(var.astype(np.float64) - want['variates'].astype(np.float64))[:, valid] / (np.abs(want['variates'][:, valid]) + sd)).max())
    # the rest of the final state, and the variates: a_i, b_i and with them M_i are defined up to (error of K) / gap, so they are compared
    # for the variates whose rho lies more than 1e-3 from its neighbours in the twin, as in the solve test
    rho = ws['rho']
    sep = np.minimum(np.abs(np.diff(rho, prepend=np.inf)), np.abs(np.diff(rho, append=-np.inf))) > 1e-3
    assert sep.any(), 'the case keeps no separated variate'
    e_sep = float((np.abs(var.astype(np.float64) - want['variates'].astype(np.float64))[:, valid] / (np.abs(want['variates'][:, valid]) + sd))[sep].max())
    e_svar = np.abs(got['var'] - ws['var']).max()
    e_mean = np.abs(got['mean'] - ws['mean']).max()
    e_ab = max(float((np.abs(got[k][sep] - ws[k][sep]).max(1) / np.abs(ws[k][sep]).max(1)).max()) for k in ('a', 'b'))
    print(f'{kind}: MEASURE rho {e_rho:.3g} chi2_ulp {e_chi:.3g} proba_ulp {e_p:.3g} delta {e_delta:.3g} variates_rel {e_var:.3g} '
          f'(separated: {e_sep:.3g}, {int(sep.sum())} of {s.nb}) var {e_svar:.3g} mean {e_mean:.3g} a,b {e_ab:.3g}')
    assert e_rho <= RHO_TOL and e_delta <= 2 * RHO_TOL and e_svar <= 2 * RHO_TOL
    assert e_chi <= CHI2_ULP and e_p <= PROBA_ULP
    assert e_sep <= VARIATES_REL and e_ab <= AB_REL
    assert e_mean <= 2.0 ** -24 * float(max(np.abs(d1[bands][np.isfinite(d1[bands])]).max(), np.abs(d2[bands][np.isfinite(d2[bands])]).max()))
    big = float(max(np.abs(d1[bands][np.isfinite(d1[bands])]).max(), np.abs(d2[bands][np.isfinite(d2[bands])]).max()))
    assert np.abs(got['centre'] - ws['centre']).max() <= 4 * ws['n_valid'] * U * big         # the centre test's bound, on the largest value
    assert abs(got['S0'] - ws['S0']) <= 2.0 ** -24 * ws['S0']                                # a sum of float32 weights, each within its last bit
    if kind == 'nonfinite':
        assert (~valid).sum() == 60
    if kind == 'exclude':
        assert 0 < (~valid).sum() == int((ex == EXV).sum())


# ---------------------------------------------------------------- early stop
@guarded
def test_the_run_stops_on_the_device_and_later_launches_change_nothing():
    d1, d2, bands, _, _ = _data('37x53/13')
    deltas = MR.irmad_ref(d1, d2, bands, iters=8, tol=0.0)['deltas']
    j = next(i for i in range(1, 7) if deltas[i] / deltas[i + 1] >= 1.6 ** 2)   # two successive deltas a factor 1.6 on either side of tol
    tol = float(np.sqrt(deltas[j] * deltas[j + 1]))
    assert deltas[j] / tol >= 1.6 and tol / deltas[j + 1] >= 1.6
    want = MR.irmad_ref(d1, d2, bands, iters=10, tol=tol)
    count = want['state']['iter']
    assert count == j + 2 and want['state']['converged'] == 1 and want['state']['skip'] == 1
    s = Scene(d1, d2, bands)
    long_run, short_run = _run(s, 10, tol), _run(s, count, tol)
    got = MR.unpack_state(long_run[3].cpu().numpy(), s.nb)
    assert (got['iter'], got['converged'], got['skip'], got['ok']) == (count, 1, 1, 1) and got['delta'] < tol
    short = MR.unpack_state(short_run[3].cpu().numpy(), s.nb)
    assert (short['iter'], short['converged'], short['skip']) == (count, 1, 0)
    for a, b in zip(long_run[:3], short_run[:3]):
        assert torch.equal(_bits(a), _bits(b))
    sa, sb = long_run[3].cpu().numpy().copy(), short_run[3].cpu().numpy().copy()
    sa[MR.SKIP] = sb[MR.SKIP] = 0                            # the skip flag is the one thing the later launches set
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))


# ---------------------------------------------------------------- degenerate inputs
@guarded
def test_a_date_against_itself():
    d1, _, bands, _, _ = _data('37x53/13')
    s = Scene(d1, d1.copy(), bands)
    chi2, proba, var, state = _run(s, 3, 0.0)
    got = MR.unpack_state(state.cpu().numpy(), s.nb)
    print(f'identical dates: 1 - rho {np.abs(1 - got["rho"]).max():.3g}, chi2 max {float(chi2.max()):.3g}')
    assert got['ok'] == 1 and np.abs(1 - got['rho']).max() <= 1e-10 and float(chi2.max()) <= 1e-12
    assert (proba[0] == 1).all() and float(proba[1].max()) <= 8 * U      # 1 - Q in double: a few 2^-53 at most
    assert not _mask(s, proba, 0.01, 0).any()


@pytest.mark.parametrize('what', ['constant band', 'all excluded'])
@guarded
def test_a_rank_deficient_date_and_an_empty_scene_fail(what):
    d1, d2, bands, _, _ = _data('37x53/3')
    ex = None
    if what == 'constant band':
        d2 = d2.copy()
        d2[1] = 4.25
    else:
        ex = np.full((37, 53), EXV, np.uint8)
    s = Scene(d1, d2, bands, ex)
    runs = [_run(s, 3, 0.0) for _ in range(2)]
    assert _same(*runs)
    chi2, proba, var, state = runs[0]
    got = MR.unpack_state(state.cpu().numpy(), 3)
    assert (got['ok'], got['converged'], got['iter'], got['skip']) == (0, 1, 1, 1) and np.isnan(got['rho']).all() and np.isnan(got['a']).all()
    assert all(torch.isnan(t).all() for t in (chi2, proba, var))
    m = _mask(s, proba, 0.5, 0).cpu().numpy()
    assert not m.any()
    want = MR.irmad_ref(d1, d2, bands, iters=3, tol=0.0, **s.twin_kw())['state']
    assert (want['ok'], want['iter'], want['skip']) == (0, 1, 1)


# ---------------------------------------------------------------- invariances
@guarded
def test_swapping_the_dates_permuting_the_bands_and_gains_of_two():
    d1, d2, bands, _, _ = _data('37x53/3')
    base = _run(Scene(d1, d2, bands), 6, 0.0)
    perm = [2, 0, 1]
    gains = np.array([2.0, 0.5, 8.0], np.float32)[:, None, None]
    for name, sc in (('swapped', Scene(d2, d1, bands)), ('permuted, scaled', Scene(d1, (d2 * gains).astype(np.float32), perm))):
        got = _run(sc, 6, 0.0)
        r0, r1 = (MR.unpack_state(t[3].cpu().numpy(), 3)['rho'] for t in (base, got))
        e_chi = _ulp32(got[0].cpu().numpy(), base[0].cpu().numpy()).max()
        print(f'{name}: rho {np.abs(r0 - r1).max():.3g} chi2_ulp {e_chi:.3g}')
        assert np.abs(r0 - r1).max() <= 2 * RHO_TOL and e_chi <= 2 * CHI2_ULP + 1


# ---------------------------------------------------------------- the mask
@guarded
def test_mask_is_the_twin_on_the_device_proba():
    d1, d2, bands, _, _ = _data('nonfinite')
    ex = np.where(np.random.default_rng(3).random((37, 53)) < 0.1, EXV, 0).astype(np.uint8)
    s = Scene(d1, d2, bands, ex)
    _, proba, _, _ = _run(s, 3, 0.0)
    valid = MR.valid_mask(d1, d2, bands, ex, EXV)
    p0 = proba[0].cpu().numpy()
    for thr, bad in ((0.01, 0), (0.95, 1), (0.5, 200), (0.0, 3), (1.0, 0)):
        masks = [_mask(s, proba, thr, bad) for _ in range(2)]
        assert torch.equal(masks[0], masks[1])
        want = MR.mask_ref(p0, valid, thr, bad)
        assert np.array_equal(masks[0].cpu().numpy(), want), (thr, bad)
    assert 0 < MR.mask_ref(p0, valid, 0.95, 0).sum() < valid.sum() and (~valid).sum() > 60
    nan = guard.full((2, 37, 53), float('nan'), dtype=torch.float32)
    got = _mask(s, nan, 0.5, 5).cpu().numpy()
    assert np.array_equal(got, np.where(valid, 0, 5).astype(np.uint8))


# ---------------------------------------------------------------- schedule stress
@guarded
def test_a_lagging_side_stream_gives_the_bits_of_the_synchronised_run():
    d1, d2, bands, ex, _ = _data('exclude')
    s = Scene(d1, d2, bands, ex)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    e0.record(); torch.cuda._sleep(4_000_000); e1.record()
    torch.cuda.synchronize()
    rate = 4_000_000 / (e0.elapsed_time(e1) * 1e3)           # _sleep cycles per microsecond
    with ss.Perturb(ss.sync()):
        e0.record()
        ref = _run(s, 3, 0.0)
        e1.record()
    torch.cuda.synchronize()
    short = int(3 * e0.elapsed_time(e1) * 1e3 / 10 * rate)   # three times the mean of the ten entries
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ss.Perturb(ss.lag(side), short=short) as h, torch.cuda.stream(side):
        got = _run(s, 3, 0.0, stream=side.cuda_stream)
    side.synchronize()
    assert len(h.log) == 10 and [e[1] for e in h.log][:4] == ['bdn_mad_centre', 'bdn_mad_moments', 'bdn_mad_solve', 'bdn_mad_chi2'] and short > 0
    assert _same(ref, got)
