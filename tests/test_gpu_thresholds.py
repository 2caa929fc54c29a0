"""-m gpu: bdn_raster_hist, bdn_hist_threshold and bdn_raster_mask through the C ABI on guard-banded buffers against the numpy restatement
tests/thresholds_ref.py.  Outputs are born 0xFF (NaN); every entry runs twice and must give the same bits.

Shapes, the smallest that can go wrong: one pixel; 37 x 53 (the one-pixel path, one partial block); 64 x 64 (the four-pixel path); 97 x 131
(several blocks, one-pixel path); 96 x 128 with the raster one float past its allocation's start (a count that divides by four on a
pointer that does not); bins 2, 64, 1000 (no power of two), 4096 (the most).

Histogram and mask: bit-equal (integers, comparisons).  Selection: Rosin is integer arithmetic, its bin and counts are exact.  Otsu's,
Kittler's and EM's sums are formed in the restatement in the kernel's order, product by product, so the two differ only through log, exp
and what follows from them; a near-tie may therefore resolve differently, and the device's bin is held to this: its criterion IN THE
RESTATEMENT lies within the tolerance of the restatement's optimum.  Tolerances: the expectation is 1e-12 relative for Otsu and Kittler
and 1e-9 for EM (its iteration feeds log and exp back 30 times or more); each bound is the larger of that and ten times the largest error
measured on the MI355X over this file's cases (MEASURED, discussed in DESIGN.md section 26).  Kittler's J = 1 + ... is a sum of terms of
order 1 that may itself come close to 0, so its error is taken relative to max(|J|, 1); the error of a class mean or deviation is taken
relative to the largest |coordinate| (a mean may be 0)."""
import functools
import math

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from gpu_util import dev, st
from tests import guard
from tests import thresholds_ref as R
from tests.guard import guarded

pytestmark = pytest.mark.gpu

# the largest errors seen on the MI355X over the cases of this file (printed by the tests with -s)
MEASURED = {'otsu_crit': 0.0, 'kittler_crit': 1.8e-16, 'split_stats': 0.0, 'em_params': 0.0, 'em_loglik': 0.0}
OTSU_TOL = max(1e-12, 10 * MEASURED['otsu_crit'])
KITTLER_TOL = max(1e-12, 10 * MEASURED['kittler_crit'])
STATS_TOL = max(1e-12, 10 * MEASURED['split_stats'])
EM_TOL = max(1e-9, 10 * MEASURED['em_params'], 10 * MEASURED['em_loglik'])

SHAPES = {'1': (1, 1, 0), '37x53': (37, 53, 0), '64x64': (64, 64, 0), '97x131': (97, 131, 0), '96x128+1': (96, 128, 1)}
BINS = (2, 64, 1000, 4096)
EXV = 3
C = R.COL


def _bits(t):
    return t.contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _edges(n_bins, kind='linear'):
    """(edges float32, coord float64).  'linear': [-2, 6] (0 is an edge for 64 and 4096 bins); 'sqrt': [0, 40]; 'dup': linear with a run of
    equal edges (empty bins by construction)."""
    if kind == 'sqrt':
        return R.bin_edges(0.0, 40.0, n_bins, 'sqrt')
    e, c = R.bin_edges(-2.0, 6.0, n_bins)
    if kind == 'dup':
        e = e.copy()
        e[n_bins // 4:n_bins // 4 + 4] = e[n_bins // 4]
        e[-3:] = e[-1]
    return e, c


@functools.lru_cache(maxsize=None)
def _raster(shape, n_bins, kind='linear'):
    """(values float32 [HW], exclude uint8 [HW]): two modes inside the edges, with values exactly on edges, +-0, denormals, +-inf, NaN and
    the neighbours of the two ends planted at random places.  Shared: never modified."""
    h, w, _ = SHAPES[shape]
    n = h * w
    e, _ = _edges(n_bins, kind)
    r = np.random.default_rng(1000 * n_bins + n)
    if kind == 'sqrt':
        v = r.chisquare(4, n)
        tail = r.random(n) < 0.06
        v = np.where(tail, v + r.uniform(15, 45, n), v).astype(np.float32)
    else:
        v = np.where(r.random(n) < 0.85, r.normal(0.5, 0.8, n), r.normal(4.0, 0.6, n)).astype(np.float32)
    special = np.concatenate([e[r.integers(0, n_bins + 1, 12)], e[[0, -1, 1, n_bins - 1]],
                              np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf, np.nan, np.nan], np.float32),
                              np.nextafter(e[[0, -1]], np.float32(-np.inf)), np.nextafter(e[[0, -1]], np.float32(np.inf))]).astype(np.float32)
    if n == 1:
        v[0] = e[-1]
    else:
        k = min(n // 2, special.size)
        v[r.choice(n, k, replace=False)] = special[r.permutation(special.size)[:k]]
    ex = np.where(r.random(n) < 0.1, EXV, r.integers(0, 3, n)).astype(np.uint8)
    return v, ex


def _place(shape, v):
    """The raster on the device at the shape's float offset inside its guarded allocation: (keep-alive tensor, pointer)."""
    off = SHAPES[shape][2]
    buf = guard.empty(v.size + off)
    buf[off:].copy_(torch.from_numpy(v))
    return buf, buf.data_ptr() + 4 * off


def _place_u8(shape, ex):
    off = SHAPES[shape][2]
    buf = guard.empty(ex.size + 4 * off, dtype=torch.uint8)
    buf[4 * off:].copy_(torch.from_numpy(ex))
    return buf, buf.data_ptr() + 4 * off


def _hist(ptr, n, edges_t, n_bins, hist, ex_ptr=None, exv=0):
    _lib.call('bdn_raster_hist', ptr, ex_ptr, exv, edges_t.data_ptr(), n_bins, hist.data_ptr(), n, st())


def _as_u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------- the histogram
@pytest.mark.parametrize('n_bins', BINS)
@pytest.mark.parametrize('shape', list(SHAPES))
@guarded
def test_hist_is_the_twin_bit_for_bit(shape, n_bins):
    v, ex = _raster(shape, n_bins)
    e, _ = _edges(n_bins)
    buf, ptr = _place(shape, v)
    exb, ex_ptr = _place_u8(shape, ex)
    et = dev(torch.from_numpy(e))
    preset = np.full(n_bins + 3, 1 << 40, np.uint64)                  # 64-bit adds: the counts land above bit 32
    got = []
    for _ in range(2):
        h = dev(torch.from_numpy(preset.view(np.int64)), torch.int64)
        _hist(ptr, v.size, et, n_bins, h)
        _hist(ptr, v.size, et, n_bins, h, ex_ptr, EXV)                # a second, accumulating call with an exclude raster
        got.append(h)
    assert torch.equal(_bits(got[0]), _bits(got[1]))
    want = R.raster_hist(v, e, ex, EXV, hist=R.raster_hist(v, e, hist=preset))
    assert np.array_equal(_as_u64(got[0]), want)
    assert (want - preset).sum() == 2 * v.size


@pytest.mark.parametrize('shape', ['37x53', '64x64'])
@guarded
def test_hist_with_duplicate_edges_and_sqrt_spacing(shape):
    for kind, n_bins in (('dup', 64), ('sqrt', 1000)):
        v, ex = _raster(shape, n_bins, kind)
        e, _ = _edges(n_bins, kind)
        buf, ptr = _place(shape, v)
        exb, ex_ptr = _place_u8(shape, ex)
        h = guard.zeros(n_bins + 3, dtype=torch.int64)
        _hist(ptr, v.size, dev(torch.from_numpy(e)), n_bins, h, ex_ptr, EXV)
        want = R.raster_hist(v, e, ex, EXV)
        assert np.array_equal(_as_u64(h), want), kind
        if kind == 'dup':
            assert (want[n_bins // 4:n_bins // 4 + 3] == 0).all() and want[:n_bins].sum() > 0


@guarded
def test_hist_stays_inside_its_buffers_with_an_unsorted_table():
    """A device-side edge table is never validated: whatever it holds, every pixel is counted in exactly one cell and nothing outside the
    buffers is touched (the guards)."""
    r = np.random.default_rng(5)
    v, _ = _raster('97x131', 64)
    for n_bins in (2, 1000):
        e = r.normal(2, 3, n_bins + 1).astype(np.float32)
        e[r.integers(0, n_bins + 1, 3)] = (np.nan, np.inf, -np.inf)
        buf, ptr = _place('97x131', v)
        h = guard.zeros(n_bins + 3, dtype=torch.int64)
        _hist(ptr, v.size, dev(torch.from_numpy(e)), n_bins, h)
        assert int(h.sum().item()) == v.size and int(h[n_bins + 2].item()) == int((~np.isfinite(v)).sum())


# ---------------------------------------------------------------- the selection
def _select_dev(hist_np, coord, edges, methods=15, em_iters=100, em_tol=1e-9):
    """(table [4,16], thr [4]) of the device, run twice on fresh NaN-born outputs: the same bits."""
    ht = dev(torch.from_numpy(hist_np.view(np.int64)), torch.int64)
    ct, et = dev(torch.from_numpy(coord), torch.float64), dev(torch.from_numpy(edges))
    out = []
    for _ in range(2):
        table, thr = guard.empty(4, 16, dtype=torch.float64), guard.empty(4)
        _lib.call('bdn_hist_threshold', ht.data_ptr(), ct.data_ptr(), et.data_ptr(), coord.size, methods, em_iters, float(em_tol),
                  table.data_ptr(), thr.data_ptr(), st())
        out.append((table, thr))
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))
    return out[0][0].cpu().numpy(), out[0][1].cpu().numpy()


def _rel(got, want, floor=0.0):
    return abs(got - want) / max(abs(want), floor) if max(abs(want), floor) > 0 else abs(got - want)


def _check_selection(name, hist, coord, edges, em_iters=100, em_tol=1e-9):
    """Compare the device's table with the restatement's; returns the errors seen."""
    n_bins = coord.size
    want_t, want_thr = R.hist_threshold(hist, coord, edges, 15, em_iters, em_tol)
    got_t, got_thr = _select_dev(hist, coord, edges, 15, em_iters, em_tol)
    otsu, kit = R.criteria(hist, coord) if want_t[:, C['OK']].any() else (None, None)
    seen = dict.fromkeys(MEASURED, 0.0)
    c = hist[:n_bins].astype(np.int64)
    for row, m in enumerate(R.METHODS):
        g, w = got_t[row], want_t[row]
        assert g[C['OK']] == w[C['OK']], (name, m, g, w)
        if not w[C['OK']]:
            assert not g.any() and np.isnan(got_thr[row]), (name, m, g)           # zeros and a NaN threshold, nothing stale
            continue
        b = int(g[C['BIN']])
        assert 1 <= b <= n_bins - 1 and g[C['VALUE']] == edges[b] == got_thr[row], (name, m)
        assert (g[C['N0']], g[C['N1']], g[C['N']]) == (c[:b].sum(), c[b:].sum(), c.sum()), (name, m)
        assert g[C['BELOW']] == hist[n_bins] and g[C['ABOVE']] == hist[n_bins + 1], (name, m)
        same = b == int(w[C['BIN']])
        if m == 'rosin':
            assert same and g[C['CRIT']] == w[C['CRIT']], (name, g, w)
        elif m in ('otsu', 'kittler'):
            crit, tol, floor = (otsu, OTSU_TOL, 0.0) if m == 'otsu' else (kit, KITTLER_TOL, 1.0)
            best = crit[int(w[C['BIN']])]
            assert not np.isnan(crit[b]) and _rel(crit[b], best, floor) <= tol, (name, m, b, int(w[C['BIN']]))      # a tie within the tolerance
            err = _rel(g[C['CRIT']], crit[b], floor)
            seen[m + '_crit'] = max(seen[m + '_crit'], err)
            assert err <= tol, (name, m, err)
        if m != 'em' and same:
            for k in ('MEAN0', 'MEAN1', 'SD0', 'SD1', 'W1'):
                err = _rel(g[C[k]], w[C[k]], abs(coord).max() if k != 'W1' else 0.0)
                seen['split_stats'] = max(seen['split_stats'], err)
                assert err <= STATS_TOL, (name, m, k, err)
            assert g[C['ITERS']] == 0 and g[C['LOGLIK']] == 0
        if m == 'em':
            assert g[C['ITERS']] == w[C['ITERS']], (name, g[C['ITERS']], w[C['ITERS']])
            for k in ('MEAN0', 'MEAN1', 'SD0', 'SD1', 'W1'):
                err = _rel(g[C[k]], w[C[k]], abs(coord).max() if k != 'W1' else 0.0)
                seen['em_params'] = max(seen['em_params'], err)
                assert err <= EM_TOL, (name, k, err)
            err = _rel(g[C['LOGLIK']], w[C['LOGLIK']])
            seen['em_loglik'] = max(seen['em_loglik'], err)
            assert err <= EM_TOL and g[C['CRIT']] == g[C['LOGLIK']], (name, err)
            if not same:                                              # the two log posteriors cross between the two bins: a tie
                lo, hi = sorted((b, int(w[C['BIN']])))
                for i in range(lo, hi + 1):
                    l0 = math.log(1 - w[C['W1']]) - math.log(w[C['SD0']]) - 0.5 * ((coord[i] - w[C['MEAN0']]) / w[C['SD0']]) ** 2
                    l1 = math.log(w[C['W1']]) - math.log(w[C['SD1']]) - 0.5 * ((coord[i] - w[C['MEAN1']]) / w[C['SD1']]) ** 2
                    assert abs(l1 - l0) <= EM_TOL * (abs(l0) + abs(l1)), (name, b, int(w[C['BIN']]))
    print(f'{name}: ' + ' '.join(f'{k}={v:.2e}' for k, v in seen.items()))
    return seen


@functools.lru_cache(maxsize=None)
def _raster_case(shape, n_bins, kind):
    v, ex = _raster(shape, n_bins, kind)
    e, c = _edges(n_bins, kind)
    return R.raster_hist(v, e, ex, EXV), c, e


SELECT_CASES = {
    'equal gaussians': lambda: (R.mixture_hist([(0.5, 0.0), (0.5, 4.0)], R.bin_edges(-6, 10, 1024)[0]),) + R.bin_edges(-6, 10, 1024)[::-1],
    'unequal gaussians': lambda: (R.mixture_hist([(0.9, 0.0), (0.1, 6.0)], R.bin_edges(-6, 10, 1024)[0]),) + R.bin_edges(-6, 10, 1024)[::-1],
    '97x131/2': lambda: _raster_case('97x131', 2, 'linear'),
    '97x131/64': lambda: _raster_case('97x131', 64, 'linear'),
    '97x131/1000': lambda: _raster_case('97x131', 1000, 'linear'),
    '97x131/4096': lambda: _raster_case('97x131', 4096, 'linear'),
    '37x53/64 dup': lambda: _raster_case('37x53', 64, 'dup'),
    '97x131/1000 sqrt': lambda: _raster_case('97x131', 1000, 'sqrt'),
    '64x64/4096 sqrt': lambda: _raster_case('64x64', 4096, 'sqrt'),
}


@pytest.mark.parametrize('case', list(SELECT_CASES))
@guarded
def test_selection_against_the_twin(case):
    hist, coord, edges = SELECT_CASES[case]()
    _check_selection(case, hist, coord, edges)
    # the step budget: three steps are far from the fixed point, where em_tol = 0 would stop (|dL| <= 0 holds once L repeats bit for bit,
    # which the last bits of log and exp decide)
    _check_selection(case + ' (3 EM steps)', hist, coord, edges, em_iters=3, em_tol=0.0)


@guarded
def test_selection_of_a_subset_of_methods_and_of_nothing_to_split():
    e, c = R.bin_edges(0.0, 8.0, 8)
    two = np.zeros(11, np.uint64)
    two[[2, 5, 8, 9, 10]] = (40, 10, 3, 4, 5)
    for methods in (1, 2, 4, 8, 5, 10):
        got_t, got_thr = _select_dev(two, c, e, methods)
        want_t, want_thr = R.hist_threshold(two, c, e, methods)
        assert np.array_equal(got_t[:3], want_t[:3]) and np.array_equal(got_thr[:3], want_thr[:3], equal_nan=True), methods
        assert got_t[3][C['OK']] == want_t[3][C['OK']] == float(bool(methods & 8)) and np.allclose(got_t[3], want_t[3], rtol=EM_TOL, atol=0)
        for row in range(4):
            if not methods >> row & 1:
                assert not got_t[row].any() and np.isnan(got_thr[row])
    constant, empty, peak_last = np.zeros(11, np.uint64), np.zeros(11, np.uint64), np.zeros(11, np.uint64)
    constant[3], empty[10] = 50, 8
    peak_last[[1, 2, 7]] = (5, 6, 50)
    big = np.zeros(11, np.uint64)
    big[[1, 3, 6]] = (1 << 49, 5, 1)
    for name, hist in (('constant', constant), ('all excluded', empty), ('peak at the last occupied bin', peak_last), ('2^49', big)):
        _check_selection(name, hist, c, e)
    e2, c2 = R.bin_edges(0.0, 2.0, 2)
    _check_selection('two bins', np.array([30, 10, 0, 0, 0], np.uint64), c2, e2)


# ---------------------------------------------------------------- the mask
def _mask(ptr, n, thr_ptr, below, ex_ptr=None, exv=0, ex_out=0, out=None):
    out = guard.empty(n, dtype=torch.uint8) if out is None else out
    _lib.call('bdn_raster_mask', ptr, ex_ptr, exv, thr_ptr, below, ex_out, out.data_ptr(), n, st())
    return out


@pytest.mark.parametrize('shape', list(SHAPES))
@guarded
def test_mask_is_the_twin_bit_for_bit(shape):
    v, ex = _raster(shape, 64)
    e, _ = _edges(64)
    buf, ptr = _place(shape, v)
    exb, ex_ptr = _place_u8(shape, ex)
    thr = dev(torch.tensor([float(e[40]), 0.0, float('nan'), float('inf')]))
    for k, t in enumerate((e[40], np.float32(0.0), np.float32(np.nan), np.float32(np.inf))):
        for below in (0, 1):
            a, b = (_mask(ptr, v.size, thr.data_ptr() + 4 * k, below) for _ in range(2))
            assert torch.equal(a, b)
            assert np.array_equal(a.cpu().numpy(), R.raster_mask(v, t, bool(below))), (k, below)
            m = _mask(ptr, v.size, thr.data_ptr() + 4 * k, below, ex_ptr, EXV, 200)
            assert np.array_equal(m.cpu().numpy(), R.raster_mask(v, t, bool(below), ex, EXV, 200)), (k, below)
    assert not _mask(ptr, v.size, thr.data_ptr() + 8, 0).any() and not _mask(ptr, v.size, thr.data_ptr() + 8, 1).any()      # a NaN threshold


@pytest.mark.parametrize('shape,n_bins,kind', [('97x131', 1000, 'sqrt'), ('64x64', 64, 'linear'), ('96x128+1', 4096, 'linear')])
@guarded
def test_the_chain_on_the_device_and_the_count_of_ones(shape, n_bins, kind):
    """Histogram, selection and mask with no host read between them: the ones of every method's mask are the histogram's tail."""
    v, ex = _raster(shape, n_bins, kind)
    e, c = _edges(n_bins, kind)
    buf, ptr = _place(shape, v)
    exb, ex_ptr = _place_u8(shape, ex)
    et, ct = dev(torch.from_numpy(e)), dev(torch.from_numpy(c), torch.float64)
    h = guard.zeros(n_bins + 3, dtype=torch.int64)
    table, thr = guard.empty(4, 16, dtype=torch.float64), guard.empty(4)
    _hist(ptr, v.size, et, n_bins, h, ex_ptr, EXV)
    _lib.call('bdn_hist_threshold', h.data_ptr(), ct.data_ptr(), et.data_ptr(), n_bins, 15, 100, 1e-9, table.data_ptr(), thr.data_ptr(), st())
    masks = [_mask(ptr, v.size, thr.data_ptr() + 4 * k, 0, ex_ptr, EXV, 0) for k in range(4)]
    t, counts = table.cpu().numpy(), _as_u64(h).astype(np.int64)
    assert t[:, C['OK']].sum() >= 3
    for k in range(4):
        if t[k][C['OK']]:
            b = int(t[k][C['BIN']])
            assert int(masks[k].sum().item()) == counts[b:n_bins].sum() + counts[n_bins + 1] == t[k][C['N1']] + t[k][C['ABOVE']], R.METHODS[k]
            assert np.array_equal(masks[k].cpu().numpy(), R.raster_mask(v, e[b], False, ex, EXV, 0))
        else:
            assert not masks[k].any()
