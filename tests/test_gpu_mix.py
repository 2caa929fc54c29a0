"""bdn_mix_patches and bdn_patch_label_counts on the device, through the C ABI on guard-banded buffers, against tests/mix_ref.py.  Outputs
are compared as uint32 / uint8 bit patterns: mixing moves bits and computes nothing.

Shapes are the smallest at which the kernel can go wrong: S = 5 (far below one 64 x 64 tile, and below the largest margin), 64 (exactly
one tile), 65 (a second tile of one row / column), 130 (a ragged 3 x 3 of tiles); C = 1 (fewer planes than plane groups) and 13; four
recipients and three donor rows in one call."""
import numpy as np
import pytest
import torch

from fabric_amd import _lib
from tests import guard
from tests import mix_ref as M
from tests.guard import guarded
from tests.test_gpu_augment import _special

pytestmark = pytest.mark.gpu

N, ROWS = 4, 7


def _inputs(S, C, seed):
    """float32 [ROWS][C][S][S] x 2 with NaN payloads, +-inf, -0.0 and denormals, as uint32 bit patterns."""
    r = np.random.default_rng(seed)
    return _special(r, (ROWS, C, S, S)).view(np.uint32), _special(r, (ROWS, C, S, S)).view(np.uint32)


def _run(plan, d1, d2, labels, mode, paste_label=1, margin=0, want_mask=True):
    """One bdn_mix_patches call on guarded copies -> (d1, d2 as uint32, labels, mask_out or None), whole buffers."""
    C, S = d1.shape[1], d1.shape[2]
    plan = np.ascontiguousarray(plan, np.int32)
    plan_dev = guard.guard(torch.from_numpy(plan))
    g1, g2 = guard.guard(torch.from_numpy(d1.view(np.float32))), guard.guard(torch.from_numpy(d2.view(np.float32)))
    gl = guard.guard(torch.from_numpy(labels))
    mask = guard.full((N, S, S), 77, dtype=torch.uint8) if want_mask else None
    _lib.call('bdn_mix_patches', _lib.host_int32(plan), plan_dev.data_ptr(), N, ROWS, C, S, M.MODES[mode], paste_label, margin, g1.data_ptr(),
              g2.data_ptr(), gl.data_ptr(), _lib.ptr(mask), _lib.stream_ptr())
    torch.cuda.synchronize()
    return (g1.cpu().numpy().view(np.uint32), g2.cpu().numpy().view(np.uint32), gl.cpu().numpy(), mask.cpu().numpy() if want_mask else None)


def _check(got, plan, d1, d2, labels, mode, paste_label=1, margin=0):
    o1, o2, ol, mask = got
    donor_rows = [int(p[2]) if p[0] else 0 for p in plan]                  # an unmixed sample: any row, under an all-zero mask
    masks = np.stack([M.mask(p, labels[r], mode, paste_label, margin) for p, r in zip(plan, donor_rows)])
    if mask is not None:
        assert np.array_equal(mask, masks), np.argwhere(mask != masks)[:5]
    for name, out, src in (('date 1', o1, d1), ('date 2', o2, d2), ('labels', ol, labels)):
        assert np.array_equal(out[N:], src[N:]), f'{name}: a donor row changed'
        want = M.mix(src[:N], src[donor_rows], masks)
        assert np.array_equal(out[:N], want), (name, np.argwhere(out[:N] != want)[:5])
        for k, p in enumerate(plan):
            if not p[0]:
                assert np.array_equal(out[k], src[k]), f'{name}: unmixed sample {k} changed'
    return masks


def box_plan(S):
    """Sample 0 unmixed; 1 a box on the top and right borders (crossing the tile seam at S = 130); 2 the whole patch; 3 a box on the bottom
    and right borders that crosses the seam at S = 65 and shares donor row 5 with sample 2.  Donor row 6 is used by nobody."""
    h1, w1, h3 = max(1, 3 * S // 4), max(1, S // 3), S // 2 + 1
    return np.array([(0, 0, -1, 0, 0, 0, 0, 0), (1, 11, 4, 0, S - w1, h1, w1, 0), (1, 12, 5, 0, 0, S, S, 0), (1, 12, 5, S - h3, S - h3, h3, h3, 0)],
                    np.int32)


@pytest.mark.parametrize('C', [1, 13])
@pytest.mark.parametrize('S', [5, 64, 65, 130])
@guarded
def test_boxes_move_the_donors_bits(S, C):
    d1, d2 = _inputs(S, C, 10 * S + C)
    labels = np.random.default_rng(S).integers(0, 256, (ROWS, S, S)).astype(np.uint8)
    plan = box_plan(S)
    got = _run(plan, d1, d2, labels, 'box')
    masks = _check(got, plan, d1, d2, labels, 'box')
    assert not masks[0].any() and masks[2].all() and masks[1][0, S - 1] and masks[3][S - 1, S - 1] and 0 < masks[1].sum() < S * S
    quiet = _run(plan, d1, d2, labels, 'box', want_mask=False)                # mask_out is optional: the same bits without it
    assert all(np.array_equal(a, b) for a, b in zip(quiet[:3], got[:3]))


def object_labels(S, seed):
    """Recipient rows random bytes; donor row 4: paste pixels (1) at both far corners and, from S = 65 on, on either side of the tile seam
    (columns 63 / 64 and rows 63 / 64), among bytes 0, 2 and 255; row 5: no byte 1 at all; row 6: about 3 % of byte 1."""
    r = np.random.default_rng(seed)
    labels = r.integers(0, 256, (ROWS, S, S)).astype(np.uint8)
    other = np.array([0, 2, 255], np.uint8)
    labels[4:] = other[r.integers(0, 3, (3, S, S))]
    labels[4, 0, 0] = labels[4, S - 1, S - 1] = 1
    if S > 64:
        labels[4, 10, 63] = labels[4, 30, 64] = labels[4, 63, 20] = labels[4, 64, 40] = 1
    labels[6][r.uniform(0, 1, (S, S)) < 0.03] = 1
    labels[6, S // 2, S // 2] = 1
    return labels


OBJECT_PLAN = [(1, 21, 4, 0, 0), (0, 0, -1, 0, 0), (1, 22, 5, 0, 0), (1, 23, 6, 0, 0)]


@pytest.mark.parametrize('margin', [0, 1, 16])
@pytest.mark.parametrize('C', [1, 13])
@pytest.mark.parametrize('S', [5, 64, 65, 130])
@guarded
def test_objects_are_pasted_with_their_margin(S, C, margin):
    d1, d2 = _inputs(S, C, 10 * S + C + 1)
    labels = object_labels(S, S + margin)
    assert (labels[4:] == 255).any() and not (labels[5] == 1).any()
    plan = np.array([(on, i, row, 0, 0, S * on, S * on, 0) for on, i, row, _, _ in OBJECT_PLAN], np.int32)
    got = _run(plan, d1, d2, labels, 'object', 1, margin)
    masks = _check(got, plan, d1, d2, labels, 'object', 1, margin)
    assert masks[0][0, 0] and masks[0][S - 1, S - 1] and not masks[1].any() and masks[3].any()
    assert not masks[2].any(), 'a donor without paste_label leaves the recipient untouched'
    if margin == 0:
        assert np.array_equal(masks[0], labels[4] == 1) and (got[2][0][masks[0] == 1] == 1).all()
    elif margin >= S:
        assert masks[0].all() and masks[3].all()
    else:
        assert masks[0].sum() > (labels[4] == 1).sum() and (got[2][0][masks[0] == 1] != 1).any()          # the ring carries the donor's labels


@guarded
def test_another_paste_label_and_a_plan_without_mixed_samples():
    S, C = 65, 2
    d1, d2 = _inputs(S, C, 3)
    labels = object_labels(S, 9)
    plan = np.array([(on, i, row, 0, 0, S * on, S * on, 0) for on, i, row, _, _ in OBJECT_PLAN], np.int32)
    masks = _check(_run(plan, d1, d2, labels, 'object', 255, 2), plan, d1, d2, labels, 'object', 255, 2)
    assert masks[2].any() and not masks[1].any()
    none = np.array([(0, 0, -1, 0, 0, 0, 0, 0)] * N, np.int32)
    for mode in ('box', 'object'):
        assert not _check(_run(none, d1, d2, labels, mode, 1, 16), none, d1, d2, labels, mode, 1, 16).any()


# ---------------------------------------------------------------- bdn_patch_label_counts
@pytest.mark.parametrize('S', [1, 16])
@guarded
def test_patch_label_counts_against_numpy(S):
    r = np.random.default_rng(5)
    shapes = [(40, 52), (70, 33)]
    values = np.array([0, 1, 2, 255], np.uint8)
    labels = [values[r.integers(0, 4, s)] for s in shapes]
    dev_l = [guard.guard(torch.from_numpy(l)) for l in labels]
    dev_i = [guard.zeros((2, 1) + s) for s in shapes]
    table = guard.guard(torch.from_numpy(np.array([[i.data_ptr(), l.data_ptr(), h | (w << 32)] for i, l, (h, w) in zip(dev_i, dev_l, shapes)],
                                                  np.int64)))
    hw = np.array(shapes, np.int32)
    desc = []
    for c, (H, W) in enumerate(shapes):                      # the four corners, the middle of the four borders, and the interior
        for row in (0, (H - S) // 2, H - S):
            for col in (0, (W - S) // 2, W - S):
                desc.append((c, row, col, len(desc) % 8))    # sym is ignored
    desc = np.array(desc, np.int32)
    desc_dev = guard.guard(torch.from_numpy(desc))
    for value in (1, 255, 7):                                # 7 is absent
        counts = guard.full((len(desc),), -5, dtype=torch.int32)
        _lib.call('bdn_patch_label_counts', table.data_ptr(), _lib.host_int32(hw), len(shapes), _lib.host_int32(desc), desc_dev.data_ptr(),
                  len(desc), S, value, counts.data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        want = [int((labels[c][i:i + S, j:j + S] == value).sum()) for c, i, j, _ in desc]
        assert counts.cpu().tolist() == want
        assert (value == 7) == (sum(want) == 0)
