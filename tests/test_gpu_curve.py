"""-m gpu: bdn_score_hist / bdn_score_curve / bdn_threshold_mask through the C ABI on guard-banded buffers (tests/guard.py; outputs are
born 0xFF = NaN), against the integer / float64 restatement tests/curve_ref.py.  The histogram is compared as integers with the bincount
of the kernel's own exported scores (exact on every input), the scores with the float64 softmax at the bar tests/test_gpu_scene_blend.py
holds the same expression to, the curve bit for bit (single correctly rounded divisions of exact integers) and the average precision
within 1e-12 (at most 4096 terms <= 1 summed in double: worst case ~4.5e-13)."""
import math

import numpy as np
import pytest
import torch

from fabric_amd._lib import call, ptr
from gpu_util import st
from tests import curve_ref as CR
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 90, 77), (1, 8, 16, 300), (2, 3, 1, 5), (4, 2, 32, 32)]      # scalar / vector loads x two classes / any: all four kernels
BINS = (2, 64, 1024, 4096)
MASKS = ('none', 'random', 'image', 'all')
SCORE_TOL = 2e-6
AP_TOL = 1e-12
IGN = 255


def _inputs(shape, mask, seed=0, label_max=None):
    B, C, H, W = shape
    r = np.random.default_rng(seed + 17 * B + C + H)
    logits = (3 * r.standard_normal(shape)).astype(np.float32)
    labels = r.integers(0, label_max or C, (B, H, W)).astype(np.uint8)
    if mask == 'random':
        labels[r.random((B, H, W)) < 0.3] = IGN
    elif mask == 'image':
        labels[B // 2] = IGN
    elif mask == 'all':
        labels[:] = IGN
    return logits, labels


def _hist(x, labels, n_bins, pos=1, ignore=-1, is_logits=1, hist=None, want_scores=True):
    """One bdn_score_hist on guarded device tensors x [n,ncls,...] and labels [n,...]; hist starts at zero unless given."""
    n, ncls = x.shape[:2]
    hw = math.prod(x.shape[2:])
    hist = guard.zeros(2, n_bins, dtype=torch.int64) if hist is None else hist
    scores = guard.empty(n, hw) if want_scores else None
    call('bdn_score_hist', ptr(x), is_logits, ptr(labels), ignore, pos, n, ncls, hw, n_bins, ptr(hist), ptr(scores), st())
    return hist, scores


def _curve(hist, n_bins):
    curve, summary = guard.empty(4, n_bins, dtype=torch.float64), guard.empty(8, dtype=torch.float64)
    call('bdn_score_curve', ptr(hist), n_bins, ptr(curve), ptr(summary), st())
    return curve.cpu().numpy(), summary.cpu().numpy()


def _assert_curve(hist_np, curve, summary, what=''):
    """The kernel's curve and summary of `hist_np` against curve_ref: everything bit-equal but the average precision."""
    c, want = CR.curve(hist_np), CR.summary_vector(hist_np)
    assert np.array_equal(curve[0], c['TP'].astype(np.float64)) and np.array_equal(curve[1], c['FP'].astype(np.float64)), what
    assert np.array_equal(curve[2], c['P']) and np.array_equal(curve[3], c['R']), what
    print(f'{what}: i_best {summary[2]:.0f} F {summary[0]!r} AP {summary[5]!r} ref {want[5]!r} |dAP|={abs(summary[5] - want[5]):.3e}')
    assert summary[2] == want[2], (what, summary, want)
    for k in (0, 1, 3, 4, 6, 7):
        assert summary[k] == want[k], (what, k, summary, want)
    assert abs(summary[5] - want[5]) <= AP_TOL, what


# ---------------------------------------------------------------- 1. the histogram, the scores and the curve of the kernel's own histogram
@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_hist_scores_and_curve(shape, mask):
    B, C, H, W = shape
    pos = 5 if C == 8 else 1
    logits, labels = _inputs(shape, mask)
    ignore = -1 if mask == 'none' else IGN
    x, lb = guard.guard(torch.from_numpy(logits)), guard.guard(torch.from_numpy(labels))
    ref = CR.softmax_scores(logits, pos).reshape(B, -1)
    ign = labels.reshape(B, -1) == ignore
    for n_bins in BINS:
        hist, scores = _hist(x, lb, n_bins, pos, ignore)
        s = scores.cpu().numpy()
        assert np.isfinite(s).all() and (s[ign] == 0).all() and not np.signbit(s[ign]).any()
        err = np.abs(s.astype(np.float64) - ref)[~ign]
        print(f'{shape} {mask} n_bins={n_bins}: max |score - float64 softmax| = {err.max() if err.size else 0.0:.3e}')
        assert err.size == 0 or err.max() <= SCORE_TOL
        h = hist.cpu().numpy()
        assert np.array_equal(h, CR.histogram(s, labels, n_bins, pos, None if ignore < 0 else ignore))
        assert h.sum() == (~ign).sum()
        curve, summary = _curve(hist, n_bins)
        _assert_curve(h, curve, summary, f'{shape} {mask} {n_bins}')
    h2, _ = _hist(x, lb, 64, pos, ignore, want_scores=False)                 # without the export: the same counts
    assert torch.equal(h2, _hist(x, lb, 64, pos, ignore)[0])


@pytest.mark.parametrize('shape', [(5, 2, 251, 263), (3, 2, 600, 600), (2, 3, 520, 516)], ids=str)
@guarded
def test_hist_grid_stride_across_images(shape):
    """More items than the grid has threads (a block per 4 x 256 items): the grid-stride loop, whose steps cross image boundaries."""
    B, C, H, W = shape
    logits, labels = _inputs(shape, 'random')
    x, lb = guard.guard(torch.from_numpy(logits)), guard.guard(torch.from_numpy(labels))
    hist, scores = _hist(x, lb, 1024, 1, IGN)
    s = scores.cpu().numpy()
    ign = labels.reshape(B, -1) == IGN
    assert (s[ign] == 0).all()
    assert np.abs(s.astype(np.float64) - CR.softmax_scores(logits, 1).reshape(B, -1))[~ign].max() <= SCORE_TOL
    assert np.array_equal(hist.cpu().numpy(), CR.histogram(s, labels, 1024, 1, IGN))


# ---------------------------------------------------------------- 2. skew: the wave-aggregation path
@pytest.mark.parametrize('shape', [(4, 2, 32, 32), (3, 2, 90, 77), (1, 8, 16, 300)], ids=str)
@guarded
def test_skewed_inputs(shape):
    B, C, H, W = shape
    npix = B * H * W
    zeros = guard.zeros(*shape)
    neg = guard.zeros(B, H, W, dtype=torch.uint8)
    for n_bins in BINS:
        hist, scores = _hist(zeros, neg, n_bins)                             # every pixel in one (label, bin) cell: s = 1 / ncls
        want = np.zeros((2, n_bins), np.int64)
        want[0, CR.bins(np.float32([1.0 / C]), n_bins)[0]] = npix
        assert np.array_equal(hist.cpu().numpy(), want) and bool((scores == 1.0 / C).all())
    # two values: class pos_class wins by 4 on every 7th pixel, which is also the positive one; then on pixels that are not
    r = np.random.default_rng(3)
    logits = np.zeros(shape, np.float32)
    hot = (np.arange(npix) % 7 == 0).reshape(B, H, W)
    logits[:, 1][hot] = 4.0
    for labels in (hot.astype(np.uint8), (r.random((B, H, W)) < 0.03).astype(np.uint8)):
        x, lb = guard.guard(torch.from_numpy(logits)), guard.guard(torch.from_numpy(labels))
        hist, scores = _hist(x, lb, 1024)
        h = hist.cpu().numpy()
        assert np.array_equal(h, CR.histogram(scores.cpu().numpy(), labels, 1024))
        assert np.count_nonzero(h) <= 4 and h.sum() == npix and h[1].sum() == labels.sum()


# ---------------------------------------------------------------- 3. bin edges, through the probability input
@pytest.mark.parametrize('hw', [4 * 700, 2801], ids=['vector', 'scalar'])
@pytest.mark.parametrize('n_bins', BINS)
@guarded
def test_bin_edges(n_bins, hw):
    ks = np.unique(np.concatenate([[1, 2, n_bins // 2, n_bins - 1, n_bins], np.random.default_rng(n_bins).integers(1, n_bins + 1, 600)]))[:640]
    edge = (ks / n_bins).astype(np.float32)
    below = np.nextafter(edge, np.float32(0))
    special = np.float32([0.0, -0.0, 1.0, np.nan, -1.0, 2.0, np.inf, -np.inf, 1e-45, np.nextafter(np.float32(1), np.float32(0))])
    s = np.resize(np.concatenate([edge, below, special]), hw).astype(np.float32)
    want_bin = np.resize(np.concatenate([np.minimum(ks, n_bins - 1), ks - 1, [0, 0, n_bins - 1, 0, 0, n_bins - 1, n_bins - 1, 0, 0, n_bins - 1]]), hw)
    assert np.array_equal(CR.bins(s, n_bins), want_bin)                      # the header's rule, spelled out, agrees with curve_ref
    labels = (np.arange(hw) % 3 == 0).astype(np.uint8)
    x = np.full((1, 2, hw), np.nan, np.float32)                              # the other class's plane is never used
    x[0, 1] = s
    hist, scores = _hist(guard.guard(torch.from_numpy(x)), guard.guard(torch.from_numpy(labels[None])), n_bins, is_logits=0)
    assert np.array_equal(scores.cpu().numpy().view(np.int32).reshape(-1), s.view(np.int32))          # as it is, NaN and -0 included
    want = np.zeros((2, n_bins), np.int64)
    np.add.at(want, (labels.astype(np.int64), want_bin), 1)
    assert np.array_equal(hist.cpu().numpy(), want)


# ---------------------------------------------------------------- 4. accumulation
@guarded
def test_additivity_and_accumulation():
    shape = (4, 2, 90, 77)
    logits, labels = _inputs(shape, 'random', seed=5)
    x, lb = guard.guard(torch.from_numpy(logits)), guard.guard(torch.from_numpy(labels))
    whole, _ = _hist(x, lb, 1024, 1, IGN)
    parts = guard.zeros(2, 1024, dtype=torch.int64)
    _hist(x[:1], lb[:1], 1024, 1, IGN, hist=parts)
    _hist(x[1:], lb[1:], 1024, 1, IGN, hist=parts)
    assert torch.equal(whole, parts)
    start = torch.from_numpy(np.random.default_rng(1).integers(0, 1 << 41, (2, 1024)))
    acc = guard.guard(start)
    _hist(x, lb, 1024, 1, IGN, hist=acc)
    assert torch.equal(acc.cpu(), start + whole.cpu())                       # added to, not overwritten
    again, _ = _hist(x, lb, 1024, 1, IGN)
    assert torch.equal(again, whole)                                         # the same bits on every run


@pytest.mark.parametrize('shape', [(3, 2, 90, 77), (2, 3, 16, 300)], ids=str)
@guarded
def test_nonfinite_logits_at_ignored_pixels_change_nothing(shape):
    logits, labels = _inputs(shape, 'random', seed=7)
    dirty = logits.copy()
    ign = labels == IGN
    for c, v in zip(range(shape[1]), (np.nan, np.inf, -np.inf)):
        dirty[:, c][ign] = v
    lb = guard.guard(torch.from_numpy(labels))
    h0, s0 = _hist(guard.guard(torch.from_numpy(logits)), lb, 256, 1, IGN)
    h1, s1 = _hist(guard.guard(torch.from_numpy(dirty)), lb, 256, 1, IGN)
    assert torch.equal(h0, h1) and torch.equal(s0, s1) and bool(torch.isfinite(s1).all())


@guarded
def test_labels_beyond_the_classes_are_negatives_and_pos_class_zero():
    shape = (2, 3, 16, 300)
    logits, labels = _inputs(shape, 'none', seed=9, label_max=6)             # labels 3, 4, 5 name no class
    x, lb = guard.guard(torch.from_numpy(logits)), guard.guard(torch.from_numpy(labels))
    for pos in (0, 1, 2):
        hist, scores = _hist(x, lb, 64, pos)
        h = hist.cpu().numpy()
        assert np.array_equal(h, CR.histogram(scores.cpu().numpy(), labels, 64, pos))
        assert h[1].sum() == (labels == pos).sum() and h[0].sum() == (labels != pos).sum()
        assert np.abs(scores.cpu().numpy().astype(np.float64) - CR.softmax_scores(logits, pos).reshape(2, -1)).max() <= SCORE_TOL
    two, l2 = _inputs((4, 2, 32, 32), 'random', seed=11)
    hist, scores = _hist(guard.guard(torch.from_numpy(two)), guard.guard(torch.from_numpy(l2)), 1024, 0, IGN)
    assert np.array_equal(hist.cpu().numpy(), CR.histogram(scores.cpu().numpy(), l2, 1024, 0, IGN))
    assert np.abs(scores.cpu().numpy().astype(np.float64) - CR.softmax_scores(two, 0).reshape(4, -1))[l2.reshape(4, -1) != IGN].max() <= SCORE_TOL


def test_hist_past_two_to_the_31():
    """Plane 1 of a [1, 2, 2^30 + 4] probability map ends behind element 2^31: 64-bit indexing (plain tensors: 4.3 GB are read)."""
    hw, n_bins = (1 << 30) + 4, 64
    x = torch.empty(1, 2, hw, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    x[0, 1].uniform_(generator=g)
    x[0, 1, -4:] = torch.tensor([0.0, 1.0, 0.999, 0.5], device='cuda')
    labels = (torch.rand(hw, device='cuda', generator=g) < 0.03).to(torch.uint8)
    hist = torch.zeros(2, n_bins, dtype=torch.int64, device='cuda')
    call('bdn_score_hist', ptr(x), 0, ptr(labels), -1, 1, 1, 2, hw, n_bins, ptr(hist), None, st())
    want = torch.zeros(2 * n_bins, dtype=torch.int64, device='cuda')
    step = 1 << 28
    for i in range(0, hw, step):
        s, l = x[0, 1, i:i + step], labels[i:i + step]
        b = torch.where(s >= 1, torch.full_like(s, n_bins - 1), s * n_bins).to(torch.int64) + n_bins * (l == 1)
        want += torch.bincount(b, minlength=2 * n_bins)
    assert torch.equal(hist.reshape(-1), want) and int(hist.sum()) == hw


# ---------------------------------------------------------------- 5. the curve on host-made histograms
def _crafted():
    out = {}
    for n in BINS:
        r = np.random.default_rng(n)
        out[f'zero-{n}'] = np.zeros((2, n), np.int64)
        h = np.zeros((2, n), np.int64); h[0] = r.integers(0, 1000, n)
        out[f'no positives-{n}'] = h
        h = np.zeros((2, n), np.int64); h[1] = r.integers(0, 1000, n)
        out[f'no negatives-{n}'] = h
        h = np.zeros((2, n), np.int64); h[:, n // 2] = (5, 9)
        out[f'one bin-{n}'] = h
        h = np.zeros((2, n), np.int64); h[1, n - 1] = 3; h[0, 0] = 4
        out[f'F ties across empty bins-{n}'] = h                            # F = 1 on 1..n-1: the first wins
        h = (r.integers(0, 1 << 40, (2, n)) * (r.random((2, n)) < 0.6)).astype(np.int64)
        out[f'2^40-{n}'] = h
        skew = np.zeros((2, n), np.int64)
        skew[0] = (1e9 * np.exp(-np.arange(n) / (n / 16))).astype(np.int64); skew[1] = (3e7 * np.linspace(0.05, 1, n) ** 2).astype(np.int64)
        out[f'skew-{n}'] = skew
    return out


@pytest.mark.parametrize('name,hist', list(_crafted().items()), ids=list(_crafted()))
@guarded
def test_curve_on_crafted_histograms(name, hist):
    n = hist.shape[1]
    curve, summary = _curve(guard.guard(torch.from_numpy(hist)), n)
    _assert_curve(hist, curve, summary, name)
    if name.startswith('zero'):
        assert not summary.any() and not curve.any()
    if name.startswith('F ties'):
        assert summary[2] == 1 and summary[0] == 1.0
    only = guard.empty(8, dtype=torch.float64)                               # without the curve output
    call('bdn_score_curve', ptr(guard.guard(torch.from_numpy(hist))), n, None, ptr(only), st())
    assert np.array_equal(only.cpu().numpy(), summary)


# ---------------------------------------------------------------- 6. the thresholded mask
@pytest.mark.parametrize('ncls,hw,pos', [(2, 90 * 77, 1), (3, 64 * 64, 2), (2, 5, 0), (2, 4 * 600001, 1)])
@guarded
def test_threshold_mask(ncls, hw, pos):
    r = np.random.default_rng(hw)
    p = r.random((ncls, hw)).astype(np.float32)
    p[pos, 5::97] = np.nan
    p[pos, 1::2][: hw // 8] = p[pos, 0]                                      # the threshold below is on a value the map holds many times
    g = guard.guard(torch.from_numpy(p))
    for t in (float(p[pos, 0]), 0.0, 1.0, 0.5, float(np.nextafter(p[pos, 0], np.float32(2)))):
        mask = guard.empty(hw, dtype=torch.uint8)
        call('bdn_threshold_mask', ptr(g), pos, t, ptr(mask), ncls, hw, st())
        with np.errstate(invalid='ignore'):
            assert np.array_equal(mask.cpu().numpy(), (p[pos] >= np.float32(t)).astype(np.uint8)), t
