"""-m gpu: fabric_amd.utils.morphology and the bdn_cc_mark / bdn_cc_select / bdn_d2_mask / bdn_threshold_pair / bdn_mask_not entries
against the host restatement tests/morph_ref.py.  Every comparison is of exact bits; there is no tolerance anywhere.  The shapes are the
smallest at which these kernels can go wrong: one pixel, one row, one column, one tile (T = bdn_cc_tile() = 64), 65 x 129 (W % 4 != 0: the
one-pixel path, tile seams both ways, bdn_edt's wide-row path), 130 x 68 (W % 4 == 0: the four-pixel path) and 67 x 128 (bdn_edt's last LDS
width).  The raw entries run on guard-banded buffers born 0xFF (tests/guard.py): a mark or workspace that is read before it is written, or
a byte written out of bounds, fails the test."""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd._lib import call, ptr
from fabric_amd.utils import morphology as M
from gpu_util import st
from tests import cc_ref
from tests import guard
from tests import morph_ref as R
from tests.guard import guarded

pytestmark = pytest.mark.gpu

T = _lib.load().bdn_cc_tile()
SHAPES = [(1, 1), (1, 70), (70, 1), (T, T), (T + 1, 2 * T + 1), (2 * T + 2, T + 4), (T + 3, 2 * T)]
IDS = [f'{h}x{w}' for h, w in SHAPES]
INT_MAX = (1 << 31) - 1


@functools.lru_cache(maxsize=None)
def _patterns(shape):
    out = cc_ref.patterns(*shape, tile=T)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _seed(shape):
    """A sparse seed raster: about 1 % of the pixels, on and off any mask."""
    s = (np.random.default_rng(shape[0] * 977 + shape[1]).random(shape) < 0.01).astype(np.uint8)
    s.setflags(write=False)
    return s


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _same(got, want, what):
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), what


def _twice_and_in_place(fn, src, want, what, alias=0):
    """fn(*src) twice gives the same bits, equal to `want`; with out= the aliased input it gives them again."""
    a = fn(*src)
    _same(a, want, what)
    assert torch.equal(fn(*src), a), what
    again = [t.clone() for t in src]
    r = fn(*again, out=again[alias])
    assert r is again[alias] and torch.equal(r, a), what + ' (in place)'


# ---------------------------------------------------------------- reconstruction
@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_reconstruct_clear_border_fill_holes(shape, conn):
    seed_np = _seed(shape)
    seed = _cuda(seed_np)
    for name, m_np in _patterns(shape).items():
        m = _cuda(m_np)
        _twice_and_in_place(lambda a, b, out=None: M.reconstruct(a, b, conn, out=out), (m, seed), R.reconstruct(m_np, seed_np, conn), name)
        s2 = seed.clone()                                                           # out = the seed raster
        _same(M.reconstruct(m, s2, conn, out=s2), R.reconstruct(m_np, seed_np, conn), name)
        _twice_and_in_place(lambda a, out=None: M.clear_border(a, conn, out=out), (m,), R.clear_border(m_np, conn), name)
        _twice_and_in_place(lambda a, out=None: M.fill_holes(a, None, conn, out=out), (m,), R.fill_holes(m_np, None, conn), name)
        for k in (1, 3):
            _same(M.fill_holes(m, k, conn), R.fill_holes(m_np, k, conn), (name, k))
    # foreground is == 1 only: other byte values are background for every function
    odd_np = (np.random.default_rng(5).integers(0, 4, shape) * 85).astype(np.uint8)                     # 0, 85, 170, 255
    odd_np[_patterns(shape)['random 0.5'] == 1] = 1
    odd = _cuda(odd_np)
    _same(M.reconstruct(odd, seed, conn), R.reconstruct(odd_np, seed_np, conn), 'odd bytes')
    _same(M.fill_holes(odd, None, conn), R.fill_holes(odd_np, None, conn), 'odd bytes')
    _same(M.clear_border(odd, conn), R.clear_border(odd_np, conn), 'odd bytes')


def test_seed_in_the_farthest_tile():
    """A ring through four tiles: its root is its top-left pixel in tile (0, 0), its only seed the bottom-right corner in tile (1, 1).  A
    second ring has no seed on it, one seed lies on background right beside it."""
    h = w = 2 * T + 2
    m = np.zeros((h, w), np.uint8)
    for lo, hi in ((10, 2 * T - 8), (30, 2 * T - 30)):
        m[lo, lo:hi + 1] = m[hi, lo:hi + 1] = 1
        m[lo:hi + 1, lo] = m[lo:hi + 1, hi] = 1
    seed = np.zeros_like(m)
    seed[2 * T - 8, 2 * T - 8] = 1                      # on the outer ring
    seed[29, 40] = 1                                    # background, one pixel above the inner ring
    for conn in (4, 8):
        got = M.reconstruct(_cuda(m), _cuda(seed), conn).cpu().numpy()
        assert np.array_equal(got, R.reconstruct(m, seed, conn))
        assert got[10, 10] == 1 and got.sum() == 4 * (2 * T - 18) and got[30, 30] == 0
    seed[:] = 0
    seed[5, 5] = 1                                      # a seed outside the mask does not count
    assert not M.reconstruct(_cuda(m), _cuda(seed)).any()


def test_hole_border_cases():
    def ring(n, lo, hi):
        a = np.zeros((n, n), np.uint8)
        a[lo, lo:hi + 1] = a[hi, lo:hi + 1] = 1
        a[lo:hi + 1, lo] = a[lo:hi + 1, hi] = 1
        return a
    # a pocket that touches the image edge at one pixel is no hole
    m = ring(9, 0, 6)
    m[0, 3] = 0
    for conn in (4, 8):
        got = M.fill_holes(_cuda(m), None, conn).cpu().numpy()
        assert np.array_equal(got, m) and np.array_equal(got, R.fill_holes(m, None, conn))
    # a pocket joined to the outside only diagonally: a hole under 8-connectivity (background 4), not under 4 (background 8)
    m = ring(9, 1, 6)
    m[1, 1] = 0
    got8, got4 = M.fill_holes(_cuda(m), None, 8).cpu().numpy(), M.fill_holes(_cuda(m), None, 4).cpu().numpy()
    assert got8[2:6, 2:6].all() and got8[1, 1] == 0 and np.array_equal(got4, m)
    assert np.array_equal(got8, R.fill_holes(m, None, 8)) and np.array_equal(got4, R.fill_holes(m, None, 4))
    # a hole inside an object inside a hole: both are filled, the object stays
    m = ring(15, 1, 13) | ring(15, 4, 10)
    m[7, 7] = 1
    got = M.fill_holes(_cuda(m)).cpu().numpy()
    assert got[1:14, 1:14].all() and got.sum() == 13 * 13 and np.array_equal(got, R.fill_holes(m))
    # max_area at exactly the hole's area and one below
    m = ring(9, 1, 6)                                   # one hole of 16 pixels
    for conn in (4, 8):
        at, below = M.fill_holes(_cuda(m), 16, conn).cpu().numpy(), M.fill_holes(_cuda(m), 15, conn).cpu().numpy()
        assert at[2:6, 2:6].all() and np.array_equal(below, m)
        assert np.array_equal(at, R.fill_holes(m, 16, conn)) and np.array_equal(below, R.fill_holes(m, 15, conn))


# ---------------------------------------------------------------- hysteresis
@pytest.mark.parametrize('pos_class', [0, 1])
@pytest.mark.parametrize('shape', [(T + 1, 2 * T + 1), (2 * T + 2, T + 4)], ids=['65x129', '130x68'])
def test_hysteresis_mask(shape, pos_class):
    h, w = shape
    r = np.random.default_rng(11)
    # a smooth field, so that weak regions hang on strong ones; then the special values
    f = r.random((h + 8, w + 8)).astype(np.float32)
    f = sum(f[dy:dy + h, dx:dx + w] for dy in range(9) for dx in range(9)) / np.float32(81)
    p = ((f - f.min()) / (f.max() - f.min())).astype(np.float32)
    low, high = float(np.quantile(p, 0.5)), float(np.quantile(p, 0.8))
    p[0, 0], p[0, 1 % w], p[h - 1, w - 1] = np.nan, np.inf, -np.inf
    p[h // 2, w // 2], p[h // 2, w // 2 + 1] = np.float32(high), np.float32(low)                        # exactly at the thresholds
    proba_np = np.stack([p, 1 - p] if pos_class == 0 else [1 - p, p]).astype(np.float32)
    proba = _cuda(proba_np)
    for conn in (4, 8):
        want = R.hysteresis_mask(proba_np, low, high, pos_class, conn)
        weak, strong = R.threshold_pair(proba_np, low, high, pos_class)
        assert weak.sum() > want.sum() > strong.sum() > 0                                               # the reconstruction decides something
        got = M.hysteresis_mask(proba, low, high, pos_class, conn)
        _same(got, want, conn)
        assert got[h // 2, w // 2] == 1 and got[0, 0] == 0
        assert torch.equal(M.hysteresis_mask(proba, low, high, pos_class, conn), got)
        out = torch.full((h, w), 0xFF, dtype=torch.uint8, device='cuda')
        assert M.hysteresis_mask(proba, low, high, pos_class, conn, out=out) is out and torch.equal(out, got)
    # low == high: the bits of bdn_threshold_mask at that threshold
    for t in (0.0, low, high, 1.0):
        plain = torch.empty(h, w, dtype=torch.uint8, device='cuda')
        call('bdn_threshold_mask', ptr(proba), pos_class, t, ptr(plain), 2, h * w, st())
        assert torch.equal(M.hysteresis_mask(proba, t, t, pos_class), plain), t
    assert np.array_equal(proba.cpu().numpy(), proba_np, equal_nan=True)


# ---------------------------------------------------------------- disc morphology
def _radii(shape):
    return (0, 1, 2, 4, 5, 25, shape[0] ** 2 + shape[1] ** 2 + 1)


@pytest.mark.parametrize('k', range(7), ids=['r0', 'r1', 'r2', 'r4', 'r5', 'r25', 'rbig'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_disc_morphology(shape, k):
    r2 = _radii(shape)[k]
    for name, m_np in _patterns(shape).items():
        m = _cuda(m_np)
        er_np, di_np = R.binary_erosion(m_np, r2), R.binary_dilation(m_np, r2)
        _twice_and_in_place(lambda a, out=None: M.binary_dilation(a, r2, out=out), (m,), di_np, (name, 'dilation'))
        _twice_and_in_place(lambda a, out=None: M.binary_erosion(a, r2, out=out), (m,), er_np, (name, 'erosion'))
        op_np, cl_np = R.binary_dilation(er_np, r2), R.binary_erosion(di_np, r2)
        _twice_and_in_place(lambda a, out=None: M.binary_opening(a, r2, out=out), (m,), op_np, (name, 'opening'))
        _twice_and_in_place(lambda a, out=None: M.binary_closing(a, r2, out=out), (m,), cl_np, (name, 'closing'))
        op, cl = M.binary_opening(m, r2), M.binary_closing(m, r2)
        assert bool((op <= m).all()) and bool((m <= cl).all()), name
        if r2 == 0:
            assert torch.equal(op, m) and torch.equal(cl, m) and torch.equal(M.binary_dilation(m, 0), m) and torch.equal(M.binary_erosion(m, 0), m)
    if k == 0:                                          # radius2 = 0 returns the input's 0 / 1 image
        odd_np = (np.random.default_rng(6).integers(0, 4, shape) * 85 + 1).astype(np.uint8)              # 1, 86, 171, 0 (256 wraps)
        for fn in (M.binary_dilation, M.binary_erosion, M.binary_opening, M.binary_closing):
            _same(fn(_cuda(odd_np), 0), (odd_np == 1).astype(np.uint8), fn.__name__)


# ---------------------------------------------------------------- the C ABI on guard-banded buffers
def _g(a):
    return guard.guard(torch.from_numpy(np.ascontiguousarray(a)))


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
@guarded
def test_mark_and_select_on_guarded_buffers(shape, conn):
    H, W = shape
    seed_np = _seed(shape) * 3                                       # seed_value 3
    seed = _g(seed_np)
    base_np = (np.random.default_rng(9).integers(0, 3, shape)).astype(np.uint8)                         # 0, 1, 2: only 1 counts
    for name in ('random 0.5', 'random 0.593', 'spiral', 'serpentine', 'foreground', 'background', 'checkerboard'):
        m_np = _patterns(shape)[name]
        labels, area, counts = guard.empty(H, W, dtype=torch.int32), guard.empty(H, W, dtype=torch.int32), guard.empty(4, dtype=torch.int32)
        ws = guard.alloc_bytes(_lib.load().bdn_cc_workspace_bytes(H, W))
        call('bdn_cc_label', ptr(_g(m_np)), 1, None, 0, conn, H, W, ptr(labels), ptr(area), ptr(counts), ptr(ws), st())
        lab_np, area_np = labels.cpu().numpy(), area.cpu().numpy()
        assert counts.tolist()[2] == 0 and np.array_equal(lab_np, cc_ref.label(m_np == 1, conn)), name
        marks = {}
        for sd, border in ((seed, 0), (None, 1), (seed, 1), (None, 0)):
            mark = guard.empty(H, W, dtype=torch.int32)               # born 0xFF
            call('bdn_cc_mark', ptr(labels), ptr(sd), 3, border, ptr(mark), H, W, st())
            want = R.mark(lab_np, None if sd is None else seed_np, 3, bool(border))
            assert np.array_equal(mark.cpu().numpy(), want), (name, sd is None, border)
            zeroed = guard.zeros(H, W, dtype=torch.int32)
            call('bdn_cc_mark', ptr(labels), ptr(sd), 3, border, ptr(zeroed), H, W, st())
            assert torch.equal(zeroed, mark)
            marks[(sd is None, border)] = (mark, want)
        mark, mark_np = marks[(False, 1)]
        big = int(area_np.max())
        for mk, keep, ar, lo, hi, base in ((mark, 1, None, 1, INT_MAX, None), (mark, 0, None, 1, INT_MAX, None), (None, 1, area, 2, max(big - 1, 2), None),
                                           (mark, 0, area, 1, 3, base_np), (None, 0, None, 1, INT_MAX, base_np), (mark, 1, area, 1, INT_MAX, base_np)):
            out = guard.empty(H, W, dtype=torch.uint8)
            b = None if base is None else _g(base)
            call('bdn_cc_select', ptr(labels), ptr(mk), keep, ptr(ar), lo, hi, ptr(b), ptr(out), H, W, st())
            want = R.select(lab_np, None if mk is None else mark_np, keep, None if ar is None else area_np, lo, hi, base)
            assert np.array_equal(out.cpu().numpy(), want), (name, mk is None, keep, ar is None, lo, hi, base is None)
            if b is not None:                                        # out may alias base
                call('bdn_cc_select', ptr(labels), ptr(mk), keep, ptr(ar), lo, hi, ptr(b), ptr(b), H, W, st())
                assert torch.equal(b, out)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
@guarded
def test_streaming_entries_on_guarded_buffers(shape):
    H, W = shape
    n = H * W
    r = np.random.default_rng(H * 31 + W)
    d2_np = r.integers(0, 40, shape).astype(np.int32)
    d2_np[0, 0], d2_np[-1, -1] = INT_MAX, 26
    d2 = _g(d2_np)
    for r2 in (0, 25, 26, INT_MAX - 1):
        for greater in (0, 1):
            out = guard.empty(H, W, dtype=torch.uint8)
            call('bdn_d2_mask', ptr(d2), r2, greater, ptr(out), n, st())
            assert np.array_equal(out.cpu().numpy(), ((d2_np > r2) if greater else (d2_np <= r2)).astype(np.uint8)), (r2, greater)
    p_np = r.random((3, H, W)).astype(np.float32)
    p_np[1].flat[0], p_np[1].flat[n // 2], p_np[1].flat[n - 1] = np.nan, 0.25, 0.75
    p = _g(p_np)
    for pos in (0, 1, 2):
        lo, hi = guard.empty(H, W, dtype=torch.uint8), guard.empty(H, W, dtype=torch.uint8)
        call('bdn_threshold_pair', ptr(p), pos, 0.25, 0.75, ptr(lo), ptr(hi), 3, n, st())
        want_lo, want_hi = R.threshold_pair(p_np, 0.25, 0.75, pos)
        assert np.array_equal(lo.cpu().numpy(), want_lo) and np.array_equal(hi.cpu().numpy(), want_hi), pos
    src_np = r.integers(0, 3, shape).astype(np.uint8)
    out = guard.empty(H, W, dtype=torch.uint8)
    call('bdn_mask_not', ptr(_g(src_np)), ptr(out), n, st())
    assert np.array_equal(out.cpu().numpy(), (src_np != 1).astype(np.uint8))


@guarded
def test_one_pixel_path_at_a_width_that_is_a_multiple_of_four():
    """Pointers that are not 16 / 4-byte aligned take the one-pixel path whatever the width."""
    H, W = 6, 8
    m_np = _patterns((T, T))['random 0.5'][:H, :W]
    lab_np = cc_ref.label(m_np == 1, 8)
    buf = guard.empty(H * W + 1, dtype=torch.int32)
    labels = buf[1:].view(H, W)                                      # 4-byte aligned only
    labels.copy_(torch.from_numpy(lab_np))
    mark = guard.empty(H, W, dtype=torch.int32)
    call('bdn_cc_mark', ptr(labels), None, 0, 1, ptr(mark), H, W, st())
    assert np.array_equal(mark.cpu().numpy(), R.mark(lab_np, None, 1, True))
    obuf = guard.empty(H * W + 1, dtype=torch.uint8)
    out = obuf[1:].view(H, W)
    call('bdn_cc_select', ptr(labels), ptr(mark), 0, None, 1, INT_MAX, None, ptr(out), H, W, st())
    assert np.array_equal(out.cpu().numpy(), R.select(lab_np, R.mark(lab_np, None, 1, True), False)) and obuf[0].item() == 0xFF
    call('bdn_d2_mask', ptr(labels), 5, 1, ptr(out), H * W, st())
    assert np.array_equal(out.cpu().numpy(), (lab_np > 5).astype(np.uint8)) and obuf[0].item() == 0xFF
    src = guard.guard(torch.from_numpy(np.ascontiguousarray(m_np)))
    call('bdn_mask_not', ptr(src), ptr(out), H * W, st())
    assert np.array_equal(out.cpu().numpy(), (m_np != 1).astype(np.uint8)) and obuf[0].item() == 0xFF


def test_bad_arguments_launch_nothing():
    lib = _lib.load()
    H, W = 4, 8
    i32 = lambda: torch.full((H, W), -1, dtype=torch.int32, device='cuda')              # noqa: E731
    u8 = lambda: torch.full((H, W), 0xFF, dtype=torch.uint8, device='cuda')             # noqa: E731
    labels, mark, out, lo, hi = i32(), i32(), u8(), u8(), u8()
    proba = torch.rand(2, H, W, device='cuda')
    s = st()
    for h, w in ((0, 8), (4, 0), (-1, 8), (46341, 46341)):
        assert lib.bdn_cc_mark(ptr(labels), None, 1, 1, ptr(mark), h, w, s) == -1
        assert lib.bdn_cc_select(ptr(labels), ptr(mark), 1, None, 1, INT_MAX, None, ptr(out), h, w, s) == -1
    for low, high in ((0.6, 0.5), (-0.1, 0.5), (0.5, 1.1), (float('nan'), 0.5), (0.5, float('nan'))):
        assert lib.bdn_threshold_pair(ptr(proba), 1, low, high, ptr(lo), ptr(hi), 2, H * W, s) == -1
    assert lib.bdn_threshold_pair(ptr(proba), 1, 0.2, 0.5, ptr(lo), ptr(hi), 2, 0, s) == -1
    assert lib.bdn_d2_mask(ptr(labels), -1, 0, ptr(out), H * W, s) == -1 and lib.bdn_d2_mask(ptr(labels), 1, 0, ptr(out), 0, s) == -1
    assert lib.bdn_mask_not(ptr(lo), ptr(out), 0, s) == -1
    torch.cuda.synchronize()
    assert bool((mark == -1).all()) and all(bool((t == 0xFF).all()) for t in (out, lo, hi))
    with pytest.raises(RuntimeError, match='threshold_pair'):
        call('bdn_threshold_pair', ptr(proba), 1, 0.6, 0.5, ptr(lo), ptr(hi), 2, H * W, s)
