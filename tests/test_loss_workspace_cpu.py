"""CPU tests of the criterion workspace sizes (csrc/loss.hip): the four size queries against a restatement, written here from the comments
above the entry points, of overlap_plan's rule and of the one workspace layout they share

    [focal block partials, double, nfp of them, padded to 16 bytes][sums n][part nblk*n][pcounts gx*gy*{4,5}][tail]

with tail = the focal gradient scale padded to 16 bytes (_masked, _topk) or 8 floats of slack (bdn_overlap_loss, bdn_criterion).  The
expected values come from that documentation alone, never from a second call into the library.  The queries are host-only.

One point where the queries differ, recorded here as it is: bdn_overlap_workspace_bytes does not test B*H*W < 2^31 (bdn_overlap_loss itself
refuses such a shape); the three bdn_criterion*_workspace_bytes return 0 there."""
import itertools

import pytest

from fabric_amd import _lib

GRID = list(itertools.product([1, 3, 64], [(1, 1), (8, 8), (40, 72), (90, 90), (128, 128), (5, 300)], [2, 3, 8], [0, 1]))
HUGE = (1 << 15, 2, 1 << 8, 1 << 8)                 # B*H*W = 2^31


def _ceil(a, b):
    return -(-a // b)


def _up16(v):
    return _ceil(v, 16) * 16


def _plan(B, ncls, H, W, reduce_w):
    """overlap_plan: a block is RL row lanes x CW columns, CW the power of two >= W capped at 256; about 256 row blocks."""
    CW = 1
    while CW < W and CW < 256:
        CW *= 2
    RL = 256 // CW
    rows = B * H
    rpb = max(RL, _ceil(rows, 256))
    gx, gy = _ceil(W, CW), _ceil(rows, rpb)
    return dict(gx=gx, gy=gy, nblk=gx * gy if reduce_w else gy, n=3 * ncls * (1 if reduce_w else W))


def _layout_end(p, nfp, ncnt, has_gscale):
    fpart = _up16(8 * nfp)
    sums, part, pcounts = 4 * p['n'], 4 * p['nblk'] * p['n'], 4 * ncnt * p['gx'] * p['gy']
    return fpart + sums + part + pcounts + (16 if has_gscale else 4 * 8)


def _overlap(B, ncls, H, W, rw):
    return _layout_end(_plan(B, ncls, H, W, rw), 0, 4, False)


def _criterion(B, ncls, H, W, rw):
    p = _plan(B, ncls, H, W, rw)
    return max(_layout_end(p, p['gx'] * p['gy'], 4, False), 8 * 1024)          # or bdn_focal's 1024 doubles (the single-term shortcut)


def _masked(B, ncls, H, W, rw):
    p = _plan(B, ncls, H, W, rw)
    return _layout_end(p, p['gx'] * p['gy'], 5, True)


def _topk(B, ncls, H, W, rw):
    """... [gscale, 16 B][state 3 x 4 int64][hist 2048 + 2048 + 1024][chunk tie counts][pterm npix f32][kept npix u8], every part padded
    to 16 bytes; the kept-term partials in front are one double per block of the sum pass (at most 512 blocks of whole 256-pixel chunks)."""
    npix = B * H * W
    nchunks = _ceil(npix, 256)
    nsb = _ceil(nchunks, _ceil(nchunks, 512))
    state = _up16(_layout_end(_plan(B, ncls, H, W, rw), nsb, 5, True))
    tie = state + 8 * 12 + 4 * 5120
    pterm = _up16(tie + 4 * nchunks)
    kept = _up16(pterm + 4 * npix)
    return _up16(kept + npix)


QUERIES = [('bdn_overlap_workspace_bytes', _overlap), ('bdn_criterion_workspace_bytes', _criterion),
           ('bdn_criterion_masked_workspace_bytes', _masked), ('bdn_criterion_topk_workspace_bytes', _topk)]


@pytest.mark.parametrize('name,restated', QUERIES)
def test_size_query_equals_the_documented_layout(name, restated):
    query = getattr(_lib.load(), name)
    for B, (H, W), ncls, rw in GRID:
        assert query(B, ncls, H, W, rw) == restated(B, ncls, H, W, rw), (name, B, ncls, H, W, rw)


@pytest.mark.parametrize('name,restated', QUERIES)
def test_size_query_returns_zero_for_an_invalid_shape(name, restated):
    query = getattr(_lib.load(), name)
    for rw in (0, 1):
        assert query(1, 1, 8, 8, rw) == 0 and query(1, 9, 8, 8, rw) == 0 and query(0, 2, 8, 8, rw) == 0, name
        B, ncls, H, W = HUGE
        if name == 'bdn_overlap_workspace_bytes':      # the one query without the 2^31 test (module docstring): its layout's size
            assert query(B, ncls, H, W, rw) == restated(B, ncls, H, W, rw)
        else:
            assert query(B, ncls, H, W, rw) == 0, name
