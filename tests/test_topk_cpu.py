"""CPU tests of top-k hard-pixel mining: the float64 restatement tests/topk_ref.py is pinned to tests/ignore_ref.py (at ppm = 1 000 000
the two are the same function) and to torch's own topk over F.cross_entropy (gamma = 0), the integer selection rule select() is checked on
hand-made ties / signed zeros / +inf, and the parts of the feature that need no device: Criterion(topk=), criterion_from_opt, the
--loss_topk checks of the training CLI, bdn_criterion_topk's declaration, argument checks and workspace size."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fabric_amd import _lib
from fabric_amd.criterion import Criterion
from tests import ignore_ref as IR
from tests import topk_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2, 9, 7), (2, 5, 4, 33), (2, 3, 1, 5)]
TOL = 1e-12


def _inputs(shape, seed=3, frac=0.3, ignore=255):
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy(3 * r.standard_normal(shape))
    lbl = torch.from_numpy(r.integers(0, C, (B, H, W)))
    mask = torch.from_numpy(r.random((B, H, W)) < frac)
    return logits, torch.where(mask, torch.full_like(lbl, ignore), lbl), mask


def _class_alpha(C):
    return [0.25, 0.75] if C == 2 else [round(0.1 + 0.8 * k / (C - 1), 3) for k in range(C)]


def _criteria(C, topk, ignore=255):
    kw = dict(ignore_index=ignore, topk=topk)
    out = [Criterion(w_overlap=0.0, w_focal=1.0, gamma=g, class_alpha=_class_alpha(C) if a else None, size_average=sa, **kw)
           for g in (0.0, 2.0) for a in (False, True) for sa in (True, False)]
    for reduce in ('columns', 'image'):
        out.append(Criterion.parse('focal+dice', focal_gamma=2.0, weights=(0.25, 2), reduce=reduce, **kw))
        out.append(Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=_class_alpha(C),
                                   reduce=reduce, **kw))
    return out


# ---------------------------------------------------------------- the restatement against what it is built on
@pytest.mark.parametrize('ignore', [255, None])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_every_pixel_kept_is_the_masked_criterion(shape, ignore):
    logits, labels, _ = _inputs(shape, frac=0.3 if ignore is not None else 0.0)
    for c in _criteria(shape[1], 1.0, ignore):
        plain = Criterion(c.w_overlap, c.alpha, c.beta, c.eps, c.reduce, c.w_focal, c.gamma, c.class_alpha, c.size_average,
                          ignore_index=255)             # (no pixel carries 255 when ignore is None)
        a, b = TR.reference(c, logits, labels), IR.reference(plain, logits, labels)
        assert a['K'] == int(a['valid'].sum()) and bool(a['kept'].equal(a['valid']))
        for k in ('loss', 'overlap', 'focal'):
            assert abs(a[k] - b[k]) <= TOL, (k, a[k], b[k])
        for k in ('dloss', 'doverlap', 'dfocal'):
            assert (a[k] - b[k]).abs().max().item() <= TOL, k


@pytest.mark.parametrize('f', [0.25, 0.1, 1e-6])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_gamma_zero_is_the_mean_of_torch_topk_over_cross_entropy(shape, f):
    logits, labels, mask = _inputs(shape)
    c = Criterion(w_overlap=0.0, w_focal=1.0, gamma=0.0, ignore_index=255, topk=f)
    x = logits.clone().requires_grad_(True)
    ce = F.cross_entropy(x, labels, reduction='none', ignore_index=255).reshape(-1)[~mask.reshape(-1)]
    K = max(1, int(ce.numel()) * TR.ppm_of(f) // 1_000_000)
    want = torch.topk(ce, K)[0].mean()
    (dwant,) = torch.autograd.grad(want, x)
    got = TR.reference(c, logits, labels)
    assert got['K'] == K
    assert abs(got['loss'] - float(want.detach())) <= TOL and (got['dloss'] - dwant).abs().max().item() <= TOL
    assert abs(got['threshold'] - float(torch.topk(ce.detach(), K)[0][-1])) <= TOL
    assert not got['dloss'][mask[:, None].expand_as(logits)].any()


def test_the_gradient_is_zero_off_the_kept_set_and_the_overlap_term_reaches_every_valid_pixel():
    shape = (3, 2, 9, 7)
    logits, labels, mask = _inputs(shape)
    c = Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255, topk=0.25)
    r = TR.reference(c, logits, labels)
    kept = r['kept'].reshape(shape[0], 1, *shape[2:]).expand_as(logits)
    valid = (~mask)[:, None].expand_as(logits)
    assert r['K'] == max(1, int((~mask).sum()) * 250_000 // 1_000_000) == int(r['kept'].sum())
    assert not r['dfocal'][~kept].any() and r['dfocal'][kept].abs().min() > 0
    assert r['doverlap'][valid & ~kept].abs().min() > 0 and not r['dloss'][~valid].any()


# ---------------------------------------------------------------- K and the selection rule, in integers
def test_kept_count_arithmetic():
    M = 1_000_000
    assert [TR.kept_count(0, p) for p in (1, 250_000, M)] == [0, 0, 0]
    assert [TR.kept_count(1, p) for p in (1, 250_000, M)] == [1, 1, 1]
    assert [TR.kept_count(3, p) for p in (1, 250_000, 333_334, 666_667, M)] == [1, 1, 1, 2, 3]
    assert [TR.kept_count(999_999, p) for p in (1, 2, 250_000, 999_999, M)] == [1, 1, 249_999, 999_998, 999_999]
    n = 2 ** 31 - 1
    assert [TR.kept_count(n, p) for p in (1, 250_000, 999_999, M)] == [2147, 536_870_911, 2_147_481_499, n]
    assert n * M < 2 ** 63                                  # the kernel's 64-bit product cannot overflow
    assert TR.ppm_of(0.25) == 250_000 and TR.ppm_of(1.0) == M and TR.ppm_of(1e-6) == 1 and TR.ppm_of(0.1) == 100_000


def test_keys_are_monotone_and_total():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    v = np.array([-inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.nextafter(np.float32(1), np.float32(2)), 3e38, inf], dtype=np.float32)
    k = TR.keys(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()          # strictly ascending, -0 < +0 included
    assert TR.keys(np.array([nan]))[0] > k[-1]              # a (positive) NaN has a place too: above +inf
    assert k.min() >= 0 and k.max() < 2 ** 32


def test_select_on_ties_signed_zeros_and_infinity():
    v = np.array([1.0, 2.0, 1.0, 1.0, 0.5, 2.0, 1.0], dtype=np.float32)
    ok = np.ones(7, bool)
    assert TR.select(v, ok, 0).tolist() == [False] * 7
    assert TR.select(v, ok, 1).tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert TR.select(v, ok, 2).tolist() == [0, 1, 0, 0, 0, 1, 0]
    assert TR.select(v, ok, 4).tolist() == [1, 1, 1, 0, 0, 1, 0]           # the first two of the four ties at 1.0
    assert TR.select(v, ok, 7).all()
    ok[0] = False                                                          # an ignored pixel is never kept, whatever it holds
    assert TR.select(v, ok, 4).tolist() == [0, 1, 1, 1, 0, 1, 0]
    z = np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    assert TR.select(z, np.ones(4, bool), 1).tolist() == [0, 1, 0, 0]      # +0 ranks above -0
    assert TR.select(z, np.ones(4, bool), 3).tolist() == [1, 1, 0, 1]
    w = np.array([5.0, np.inf, 3e38, -np.inf], dtype=np.float32)
    assert TR.select(w, np.ones(4, bool), 1).tolist() == [0, 1, 0, 0] and TR.select(w, np.ones(4, bool), 3).tolist() == [1, 1, 1, 0]
    zeros = np.zeros((2, 3, 4), dtype=np.float32)                          # all equal: the first K valid pixels in index order
    valid = np.ones(24, bool); valid[[0, 5]] = False
    assert np.nonzero(TR.select(zeros, valid, 5))[0].tolist() == [1, 2, 3, 4, 6]


def test_select_agrees_with_the_float64_sort_on_random_values():
    r = np.random.default_rng(0)
    v = (r.standard_normal(5000) * np.exp(r.standard_normal(5000) * 3)).astype(np.float32)
    v[r.integers(0, 5000, 800)] = v[r.integers(0, 5000, 800)]              # ties
    valid = r.random(5000) < 0.7
    idx = np.nonzero(valid)[0]
    for K in (0, 1, 17, idx.size // 4, idx.size):
        order = idx[np.argsort(-v[idx].astype(np.float64), kind='stable')]
        want = np.zeros(5000, bool); want[order[:K]] = True
        assert (TR.select(v, valid, K) == want).all(), K


# ---------------------------------------------------------------- Criterion
def test_criterion_topk_validation_and_repr():
    assert Criterion().topk is None and 'topk' not in repr(Criterion())
    c = Criterion.parse('focal+dice', focal_gamma=2.0, topk=0.25, ignore_index=255)
    assert c.topk == 0.25 and c.topk_ppm == 250_000 and repr(c).endswith('ignore_index=255, topk=0.25)')
    assert Criterion.parse('focal', focal_gamma=0.0, topk=1).topk_ppm == 1_000_000
    assert Criterion(w_focal=1.0, topk=1e-6).topk_ppm == 1
    for bad in (0, 0.0, -0.1, 1.0000001, 2, 1e-7, float('nan'), 'x', True):
        with pytest.raises(ValueError):
            Criterion(w_focal=1.0, topk=bad)
    with pytest.raises(ValueError, match='focal'):
        Criterion(topk=0.5)                                                # the default criterion has no focal weight
    for name in ('tversky', 'dice', 'jaccard'):
        with pytest.raises(ValueError, match='focal'):
            Criterion.parse(name, topk=0.5)
    with pytest.raises(ValueError, match='class'):
        Criterion(w_focal=1.0, class_alpha=[1.5, -0.5], topk=0.5)
    with pytest.raises(ValueError, match='class'):
        Criterion(w_focal=1.0, class_alpha=1.5, topk=0.5)                  # [1.5, -0.5]
    assert Criterion(w_focal=1.0, class_alpha=[1.5, -0.5]).class_alpha == (1.5, -0.5)       # without topk: as before
    with pytest.raises(RuntimeError, match='no CPU path'):
        c.evaluate(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))


def test_criterion_from_opt_carries_loss_topk():
    from fabric_amd.utils.helpers import criterion_from_opt
    opt = types.SimpleNamespace(loss_function='focal+dice', focal_gamma=2.0, loss_topk=0.1, ignore_label=255)
    c = criterion_from_opt(opt)
    assert c.topk == 0.1 and c.topk_ppm == 100_000 and c.ignore_index == 255
    del opt.loss_topk
    assert criterion_from_opt(opt).topk is None
    opt.loss_topk, opt.loss_function = 0.1, 'dice'
    with pytest.raises(ValueError, match='focal'):
        criterion_from_opt(opt)


def _train(*args):
    return subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', *args], cwd=ROOT, capture_output=True,
                          text=True, timeout=600)


def test_cli_loss_topk_needs_a_focal_term_the_fused_step_and_a_fraction():
    r = _train('--fused_step', 'true', '--loss_function', 'dice', '--loss_topk', '0.25')
    assert r.returncode != 0 and 'focal term' in r.stderr, r.stderr[-500:]
    r = _train('--loss_function', 'focal', '--focal_gamma', '2', '--loss_topk', '0.25')
    assert r.returncode != 0 and '--fused_step true' in r.stderr, r.stderr[-500:]
    for bad in ('0', '1.5', '-0.25'):
        r = _train('--fused_step', 'true', '--loss_function', 'focal+dice', '--focal_gamma', '2', '--loss_topk', bad)
        assert r.returncode != 0 and '0 < F <= 1' in r.stderr, (bad, r.stderr[-500:])


# ---------------------------------------------------------------- the C ABI without a device
def test_topk_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+bdn_criterion_topk\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'bdn_criterion_topk not declared'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES['bdn_criterion_topk']
    assert res is ctypes.c_int and len(args) == len(params) == 25
    for p, a in zip(params, args):
        want = ctypes.c_void_p if '*' in p else ctypes.c_float if p.startswith('float') else ctypes.c_int
        assert a is want, (p, a)
    assert [p.split()[-1].lstrip('*') for p in params][12:20] == ['topk_ppm', 'ws', 'loss', 'terms', 'counts', 'dlogits', 'pixel_terms', 'kept']
    assert re.search(r'\bsize_t\s+bdn_criterion_topk_workspace_bytes\s*\(\s*int B, int ncls, int H, int W, int reduce_w\)\s*;', hdr)
    assert _lib.SIGNATURES['bdn_criterion_topk_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert 'utils/metrics.py:8-48' in hdr[hdr.index('top-k hard-pixel mining'):hdr.index('bdn_criterion_topk_workspace_bytes(int B')]
    lib = _lib.load()
    assert lib.bdn_criterion_topk and lib.bdn_criterion_topk_workspace_bytes


def _crit(**over):
    """bdn_criterion_topk with fake non-null pointers: every argument check returns before anything touches a device."""
    lib = _lib.load()
    a = dict(logits=16, labels=16, ignore_label=255, w_overlap=1.0, alpha=0.5, beta=0.5, eps=1e-7, reduce_w=0, w_focal=1.0, gamma=2.0,
             class_alpha=None, size_average=1, topk_ppm=250_000, ws=16, loss=16, terms=None, counts=None, dlogits=None, pixel_terms=None,
             kept=None, B=1, ncls=2, H=4, W=4, stream=None)
    a.update(over)
    rc = lib.bdn_criterion_topk(*a.values())
    return rc, lib.bdn_last_error().decode()


def test_topk_argument_errors_return_before_touching_a_device():
    for v in (-2, 256):
        rc, msg = _crit(ignore_label=v)
        assert rc == -1 and 'ignore_label' in msg, (v, rc, msg)
    for v in (0, -1, 1_000_001):
        rc, msg = _crit(topk_ppm=v)
        assert rc == -1 and 'topk_ppm' in msg, (v, rc, msg)
    rc, msg = _crit(w_focal=0.0)
    assert rc == -1 and 'w_focal' in msg
    rc, msg = _crit(w_overlap=-1.0)
    assert rc == -1
    rc, msg = _crit(gamma=-1.0)
    assert rc == -1 and 'gamma' in msg
    rc, msg = _crit(ncls=9)
    assert rc == -2
    rc, msg = _crit(B=1 << 16, H=1 << 8, W=1 << 7)
    assert rc == -2 and '2^31' in msg
    rc, msg = _crit(ws=8)
    assert rc == -1 and 'aligned' in msg
    rc, msg = _crit(loss=None)
    assert rc == -1 and 'null' in msg


def test_topk_workspace_size():
    lib = _lib.load()
    ws, masked = lib.bdn_criterion_topk_workspace_bytes, lib.bdn_criterion_masked_workspace_bytes
    assert ws(0, 2, 4, 4, 0) == 0 and ws(1, 1, 4, 4, 0) == 0 and ws(1, 9, 4, 4, 0) == 0 and ws(1 << 16, 2, 1 << 8, 1 << 7, 0) == 0
    for shape in ((3, 2, 90, 77), (1, 8, 16, 300), (2, 3, 1, 5), (64, 2, 128, 128)):
        B, C, H, W = shape
        for rw in (0, 1):
            n = ws(B, C, H, W, rw)
            npix = B * H * W
            # a float and a byte per pixel, an int per 256 pixels, the histograms and the select's state; beside them no more than the
            # masked criterion's parts, at most 512 block partials and padding
            own = 5 * npix + 4 * ((npix + 255) // 256) + 4 * 5120 + 96
            assert n % 16 == 0 and own < n <= masked(B, C, H, W, rw) + own + 8 * 512 + 256
