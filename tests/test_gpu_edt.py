"""-m gpu: bdn_edt (include/bidate_hip.h; fabric_amd.utils.distance.distance_transform_sq) through the C ABI on guard-banded buffers, with
a workspace of exactly the queried size (0xFF-filled).  Everything is integers: every comparison is exact equality with
tests/edt_ref.d2_ref (scipy-derived; pinned to the brute force by tests/test_edt_cpu.py).

Shapes: the small ones of the issue, and the kernel's own boundaries -- the row pass keeps its stack in LDS up to W = 128 and in the
workspace above ((64, 128) below it, (65, 129) above, (130, 257) well above), one wave of 64 rows per block (N * H = 192 rows: whole blocks;
195, 201, 390: a tail), columns in blocks of 256 threads (N * W = 279, 387, 771), the row pass reads g eight columns at a time (W = 1, 5,
13, 93: tails)."""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import distance
from gpu_util import dev, st
from tests import edt_ref as ER
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (5, 1), (7, 13), (64, 128), (65, 129), (67, 93), (130, 257)]
LIMITS = [1, 5, 26, ER.LIMIT]
N = 3
GROUPS = [ER.PATTERNS[i:i + N] for i in range(0, len(ER.PATTERNS), N)]


@functools.lru_cache(maxsize=None)
def _case(shape, group, equal, with_valid):
    """(src uint8 [N,H,W], valid uint8 [N,H,W] or None, unlimited reference int64 [N,H,W]).  Shared: never modified."""
    h, w = shape
    src = np.stack([ER.pattern(p, h, w) for p in GROUPS[group]])
    valid = None
    if with_valid:
        valid = np.where(np.random.default_rng(group * 7 + h).random(src.shape) < 0.1, 9, 0).astype(np.uint8)
    ref = np.stack([ER.d2_ref(ER.sites(src[i], 1, bool(equal), None if valid is None else valid[i], 9)) for i in range(N)])
    return torch.from_numpy(src), None if valid is None else torch.from_numpy(valid), torch.from_numpy(ref)


def _run(src_d, valid_d, equal, limit, ws=None, site_value=1, invalid_value=9):
    n, h, w = src_d.shape
    if ws is None:
        ws = guard.alloc_bytes(_lib.load().bdn_edt_workspace_bytes(n, h, w), label='edt workspace')
    out = guard.full((n, h, w), -7, dtype=torch.int32)
    _lib.call('bdn_edt', src_d.data_ptr(), site_value, int(equal), _lib.ptr(valid_d), invalid_value if valid_d is not None else 0, limit,
              out.data_ptr(), ws.data_ptr(), n, h, w, st())
    return out


@pytest.mark.parametrize('with_valid', [False, True])
@pytest.mark.parametrize('equal', [1, 0])
@pytest.mark.parametrize('shape', SHAPES)
@guarded
def test_edt_is_exact(shape, equal, with_valid):
    for group in range(len(GROUPS)):
        src, valid, ref = _case(shape, group, equal, with_valid)
        src_d, valid_d = dev(src, torch.uint8), None if valid is None else dev(valid, torch.uint8)
        for limit in LIMITS:
            got = _run(src_d, valid_d, equal, limit).cpu().long()
            want = ref.clamp(max=limit)
            bad = int((got != want).sum())
            assert bad == 0, (shape, GROUPS[group], equal, with_valid, limit, bad)


@guarded
def test_edt_large_case():
    """1030 x 2051: many blocks of rows, the workspace stack, distances of hundreds of pixels."""
    h, w = 1030, 2051
    r = np.random.default_rng(5)
    src = (r.random((1, h, w)) < 0.0005).astype(np.uint8)
    src[0, :, 1200:] = 0                                    # a wide empty stretch: long parabolas
    src[0, 400:700, 100:900] = 0
    ref = torch.from_numpy(ER.d2_ref(src[0] == 1))
    got = _run(dev(torch.from_numpy(src), torch.uint8), None, 1, ER.LIMIT)[0].cpu().long()
    assert int(ref.max()) > 500 ** 2
    assert torch.equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize('shape', [(67, 93), (130, 257)])
@guarded
def test_edt_same_bits_from_any_workspace(shape):
    src, valid, ref = _case(shape, 3, 1, True)
    src_d, valid_d = dev(src, torch.uint8), dev(valid, torch.uint8)
    nbytes = _lib.load().bdn_edt_workspace_bytes(N, *shape)
    outs = []
    for fill in (0xFF, 0x00, 0xFF):
        ws = guard.alloc_bytes(nbytes, label='edt workspace').fill_(fill)
        outs.append(_run(src_d, valid_d, 1, ER.LIMIT, ws=ws))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0].cpu().long(), ref)


def test_distance_transform_sq_public_surface():
    h, w = 67, 93
    m = torch.from_numpy(ER.pattern('rand2', h, w))
    ref = torch.from_numpy(ER.d2_ref(m.numpy() == 1))
    got = distance.distance_transform_sq(m.cuda())
    assert got.dtype == torch.int32 and tuple(got.shape) == (h, w) and torch.equal(got.cpu().long(), ref)
    got = distance.distance_transform_sq(m.cuda()[None].contiguous(), max_dist=3)
    assert tuple(got.shape) == (1, h, w) and torch.equal(got[0].cpu().long(), ref.clamp(max=10))
    valid = torch.from_numpy(np.where(np.random.default_rng(1).random((h, w)) < 0.1, 255, 0).astype(np.uint8))
    ref = torch.from_numpy(ER.d2_ref(ER.sites(m.numpy(), 1, False, valid.numpy(), 255)))
    out = torch.empty(h, w, dtype=torch.int32, device='cuda')
    assert distance.distance_transform_sq(m.cuda(), equal=False, valid=valid.cuda(), invalid_value=255, out=out) is out
    assert torch.equal(out.cpu().long(), ref)
    with pytest.raises(RuntimeError, match='no CPU path'):
        distance.distance_transform_sq(m)


@pytest.mark.parametrize('ignore, max_dist', [(None, None), (255, None), (255, 3)])
def test_signed_distance_is_exact(ignore, max_dist):
    h, w = 33, 65
    r = np.random.default_rng(3)
    small = r.integers(0, 3, (4, 5, 9))                     # 8 x 8 blocks: distances up to tens of pixels, roots of many non-squares
    lab = np.repeat(np.repeat(small, 8, axis=1), 8, axis=2)[:, :h, :w].astype(np.uint8)
    lab[1][lab[1] == 2] = 0                                 # class 2 absent from image 1
    lab[2][:] = 2                                           # class 2 fills image 2
    if ignore is not None:
        lab[r.random(lab.shape) < 0.2] = ignore
        lab[3][:] = ignore                                  # no valid pixel
    want = np.stack([ER.phi_ref(lab[i], 2, ignore, max_dist) for i in range(4)])
    got = distance.signed_distance(torch.from_numpy(lab).cuda(), 2, ignore_index=ignore, max_dist=max_dist).cpu().numpy()
    assert np.array_equal(got, want)
    assert not want[1].any() and not want[2].any() and want[0].any()
