"""-m gpu: bdn_cc_label / bdn_cc_compact / bdn_cc_stats / bdn_cc_filter through the C ABI on guard-banded buffers whose payloads are born
0xFF, against the host restatement tests/cc_ref.py.  Every comparison is of exact integers; every case asserts counts[2] == 0.  The
shapes straddle the tile edge T (read from the library): one tile, 1-wide rasters, T x T, (T + 1) x (T - 1), several tiles with seams in
both directions at a width that takes the scalar path, a W % 4 == 0 shape for the vector path, and one larger raster."""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd._lib import call, ptr
from gpu_util import st
from tests import cc_ref as R
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu

T = _lib.load().bdn_cc_tile()
SHAPES = [(T // 2 + 3, T - 5), (1, 1), (1, 5), (5, 1), (7, 13), (T, T), (T + 1, T - 1), (2 * T + 3, 3 * T + 1), (96, 200), (517, 1030)]
PATTERNS = ['background', 'foreground', 'random 0.1', 'random 0.5', 'random 0.593', 'random 0.9', 'checkerboard', 'diagonals', 'spiral',
            'serpentine', 'rows', 'columns', 'reach back', 'corner']


@functools.lru_cache(maxsize=None)
def _patterns(shape):
    return R.patterns(*shape, tile=T)


@functools.lru_cache(maxsize=None)
def _ref(shape, pattern, conn):
    """(labels, area, (n, n_fg), compact) of the host restatement; shared by the tests, never modified."""
    lab = R.label(_patterns(shape)[pattern] == 1, conn)
    out = (lab, R.areas(lab), R.counts(lab), R.compact(lab))
    for a in (out[0], out[1], out[3]):
        a.setflags(write=False)
    return out


def _g(a):
    return guard.guard(torch.from_numpy(np.ascontiguousarray(a)))


def _label(src, conn, H, W, fg=1, excl=None, exv=0, want_area=True, ws=None):
    labels = guard.empty(H, W, dtype=torch.int32)
    area = guard.empty(H, W, dtype=torch.int32) if want_area else None
    counts = guard.empty(4, dtype=torch.int32)
    ws = guard.alloc_bytes(_lib.load().bdn_cc_workspace_bytes(H, W)) if ws is None else ws
    call('bdn_cc_label', ptr(src), fg, ptr(excl), exv, conn, H, W, ptr(labels), ptr(area), ptr(counts), ptr(ws), st())
    return labels, area, counts, ws


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@guarded
def test_label_compact_stats_filter(shape, pattern, conn):
    H, W = shape
    m = _patterns(shape)[pattern]
    lab, area_ref, (n, n_fg), comp_ref = _ref(shape, pattern, conn)
    src = _g(m)
    labels, area, counts, ws = _label(src, conn, H, W)
    c = counts.tolist()
    assert c[2] == 0 and c[3] == 0 and (c[0], c[1]) == (n, n_fg), c
    assert np.array_equal(labels.cpu().numpy(), lab)
    assert np.array_equal(area.cpu().numpy(), area_ref)                      # every element, the zeros included
    # without areas: the same labels, area untouched (NULL)
    l2, _, c2, _ = _label(src, conn, H, W, want_area=False)
    assert torch.equal(l2, labels) and c2.tolist() == c

    # compact = the rank of the roots; counts[0] = n, the other words stay
    comp = guard.empty(H, W, dtype=torch.int32)
    cc = guard.full((4,), 7, dtype=torch.int32)
    call('bdn_cc_compact', ptr(labels), H, W, ptr(comp), ptr(cc), ptr(ws), st())
    assert np.array_equal(comp.cpu().numpy(), comp_ref)
    assert cc.tolist() == [n, 7, 7, 7]

    # statistics: with and without `other`, an excluded value, padding rows, and a table shorter than n (the guard bands prove the skip)
    other_np = np.random.default_rng(5).integers(0, 3, (H, W)).astype(np.uint8)
    other = _g(other_np)
    for n_max, oth, exv in ((n + 2, other, -1), (n + 2, None, -1), (n + 2, other, 0)) + (((n - 1, other, -1),) if n > 1 else ()):
        table = guard.empty(n_max, 8, dtype=torch.int32)
        call('bdn_cc_stats', ptr(comp), n_max, ptr(oth), 2, exv, H, W, ptr(table), st())
        want = R.stats_table(comp_ref, n_max, None if oth is None else other_np, 2, exv)
        assert np.array_equal(table.cpu().numpy(), want), (n_max, oth is None, exv)

    # filter by area, into a fresh mask and in place
    biggest = int(area_ref.max())
    for k in (1, 2, 5, biggest, biggest + 1):
        want = R.filter_mask(lab, area_ref, k)
        out = guard.empty(H, W, dtype=torch.uint8)
        call('bdn_cc_filter', ptr(src), ptr(labels), ptr(area), k, ptr(out), H, W, st())
        assert np.array_equal(out.cpu().numpy(), want), k
        inplace = guard.clone(src)
        call('bdn_cc_filter', ptr(inplace), ptr(labels), ptr(area), k, ptr(inplace), H, W, st())
        assert np.array_equal(inplace.cpu().numpy(), want), k


@pytest.mark.parametrize('conn', [4, 8])
@guarded
def test_exclusion_cuts_a_component_and_fg_value(conn):
    H, W = T + 9, 2 * T + 6
    m = np.zeros((H, W), np.uint8)
    m[5, 3:W - 3] = 7                                      # one bar across the tile border ...
    m[T + 2, :] = 7
    m[0, 0] = 1                                            # (another value: background when fg_value = 7)
    ex = np.full((H, W), 3, np.uint8)
    ex[4:7, T - 1:T + 1] = 255                             # ... cut in two at the border by the exclusion
    fg = R.foreground(m, 7, ex, 255)
    lab = R.label(fg, conn)
    assert R.counts(lab)[0] == 3 and R.counts(R.label(m == 7, conn))[0] == 2
    labels, area, counts, _ = _label(_g(m), conn, H, W, fg=7, excl=_g(ex), exv=255)
    assert counts.tolist() == [3, int(fg.sum()), 0, 0]
    assert np.array_equal(labels.cpu().numpy(), lab) and np.array_equal(area.cpu().numpy(), R.areas(lab))
    # an exclusion value that does not occur changes nothing
    labels, _, counts, _ = _label(_g(m), conn, H, W, fg=7, excl=_g(ex), exv=9)
    assert counts.tolist()[:3] == [2, int((m == 7).sum()), 0] and np.array_equal(labels.cpu().numpy(), R.label(m == 7, conn))


@guarded
def test_same_bits_every_time_and_for_any_workspace():
    shape, conn = (517, 1030), 4
    H, W = shape
    lab, area_ref, (n, n_fg), _ = _ref(shape, 'random 0.593', conn)
    src = _g(_patterns(shape)['random 0.593'])
    nbytes = _lib.load().bdn_cc_workspace_bytes(H, W)
    runs = []
    for fill in (None, None, None, 0xFF, 0x00):            # three runs on fresh workspaces, then a 0xFF-born and a zeroed one
        ws = guard.alloc_bytes(nbytes)
        if fill is not None:
            ws.fill_(fill)
        labels, area, counts, _ = _label(src, conn, H, W, ws=ws)
        assert counts.tolist() == [n, n_fg, 0, 0]
        runs.append((labels, area))
    for labels, area in runs[1:]:
        assert torch.equal(labels, runs[0][0]) and torch.equal(area, runs[0][1])
    assert np.array_equal(runs[0][0].cpu().numpy(), lab) and np.array_equal(runs[0][1].cpu().numpy(), area_ref)


@guarded
def test_misaligned_pointers_take_the_scalar_kernels():
    """W % 4 == 0 with src, exclude, other and out_mask one byte off a 4-byte boundary: the dispatch falls back to the one-pixel kernels."""
    shape, conn = (96, 200), 8
    H, W = shape
    m = _patterns(shape)['random 0.5']
    ex = (np.random.default_rng(9).random(shape) < 0.1).astype(np.uint8)
    lab = R.label(R.foreground(m, 1, ex, 1), conn)
    area_ref, (n, n_fg), comp_ref = R.areas(lab), R.counts(lab), R.compact(lab)

    def off1(a):                                          # a copy of `a` that starts one byte into a guarded payload
        buf = guard.empty(a.size + 1, dtype=torch.uint8)
        buf[1:].copy_(torch.from_numpy(a.ravel()))
        assert buf[1:].data_ptr() % 4 == 1
        return buf[1:]
    src, excl = off1(m), off1(ex)
    labels, area, counts, ws = _label(src, conn, H, W, excl=excl, exv=1)
    assert counts.tolist() == [n, n_fg, 0, 0]
    assert np.array_equal(labels.cpu().numpy(), lab) and np.array_equal(area.cpu().numpy(), area_ref)
    comp = guard.empty(H, W, dtype=torch.int32)
    call('bdn_cc_compact', ptr(labels), H, W, ptr(comp), None, ptr(ws), st())
    other = off1(ex)
    table = guard.empty(n, 8, dtype=torch.int32)
    call('bdn_cc_stats', ptr(comp), n, ptr(other), 0, -1, H, W, ptr(table), st())
    assert np.array_equal(table.cpu().numpy(), R.stats_table(comp_ref, n, ex, 0))
    out = guard.empty(H * W + 1, dtype=torch.uint8)
    call('bdn_cc_filter', ptr(src), ptr(labels), ptr(area), 5, ptr(out[1:]), H, W, st())
    assert np.array_equal(out[1:].cpu().numpy().reshape(H, W), R.filter_mask(lab, area_ref, 5)) and int(out[0]) == 0xFF
