"""CPU tests of the Lovasz-Softmax term: the float64 restatement tests/lovasz_ref.py is pinned to the set-function definition (the Jaccard
loss of every prefix of mispredicted pixels, by brute force), to torch autograd through sort, gather and cumsum (the paper's published
lovasz_grad), to 1 - IoU on hard predictions and to the ignore rule; the integer ordering rule is checked on hand-made ties, infinities and
NaN; and the parts of the feature that need no device: Criterion(w_lovasz=), Criterion.parse, criterion_from_opt, the training CLI's checks,
bdn_lovasz_softmax's declaration, argument checks and workspace size."""
import ctypes
import itertools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd import criterion as CR
from fabric_amd.criterion import Criterion
from tests import lovasz_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2, 9, 7), (2, 5, 4, 33), (2, 3, 1, 5)]
TOL = 1e-12


def _inputs(shape, seed=3, frac=0.3, ignore=255, absent=None):
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy(3 * r.standard_normal(shape))
    lbl = torch.from_numpy(r.integers(0, C, (B, H, W)))
    if absent is not None:
        lbl = torch.where(lbl == absent, torch.full_like(lbl, (absent + 1) % C), lbl)
    mask = torch.from_numpy(r.random((B, H, W)) < frac)
    return logits, torch.where(mask, torch.full_like(lbl, ignore), lbl), mask


# ---------------------------------------------------------------- the coefficients against the set function
def _jaccard_loss(fg, M):
    """The Jaccard loss of the set M of mispredicted pixels: a mispredicted foreground pixel leaves the intersection, a mispredicted
    background pixel joins the union; the empty set has loss 0 (also without foreground)."""
    if not M:
        return 0.0
    G = sum(fg)
    inter = G - sum(1 for i in M if fg[i])
    union = G + sum(1 for i in M if not fg[i])
    return 1.0 - inter / union


def test_coefficients_are_the_increments_of_the_jaccard_set_function():
    for N in range(1, 9):
        for fg in itertools.product((False, True), repeat=N):            # every foreground pattern along the order, G = 0 and G = N included
            g = LR.coefficients(np.array(fg))
            want = [_jaccard_loss(fg, range(r + 1)) - _jaccard_loss(fg, range(r)) for r in range(N)]
            assert np.abs(g - np.array(want)).max() <= 1e-15, (fg, g, want)
            assert (g >= 0).all() and g.sum() <= 1.0 + 1e-15                # what makes the extension 1-Lipschitz in the max norm of the errors
    assert LR.coefficients(np.zeros(5, bool)).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert LR.coefficients(np.ones(4, bool)).tolist() == [0.25] * 4
    assert LR.coefficients(np.zeros(0, bool)).size == 0


@pytest.mark.parametrize('classes', ['present', 'all'])
def test_the_term_is_the_lovasz_extension_by_brute_force(classes):
    """N <= 8 valid pixels, three classes of which one may be absent: L_c = sum over the order of err times the set function's increment."""
    r = np.random.default_rng(11)
    for case in range(200):
        N = int(r.integers(1, 9))
        logits = torch.from_numpy(2 * r.standard_normal((1, 3, 1, N)))
        labels = torch.from_numpy(r.integers(0, 3 if case % 2 else 2, (1, 1, N)))
        p = torch.softmax(logits.double(), 1)[0, :, 0].numpy()
        L, inc = [], []
        for c in range(3):
            fg = (labels.reshape(-1).numpy() == c)
            err = np.abs(fg - p[c])
            order = sorted(range(N), key=lambda i: (-err[i], i))
            fgs = [bool(fg[i]) for i in order]
            L.append(sum(err[i] * (_jaccard_loss(fgs, range(k + 1)) - _jaccard_loss(fgs, range(k))) for k, i in enumerate(order)))
            inc.append(classes == 'all' or fg.any())
        want = sum(l for l, i in zip(L, inc) if i) / sum(inc)
        got = LR.evaluate(logits, labels, None, classes)
        assert abs(got['term'] - want) <= TOL and got['included'].tolist() == inc and np.abs(got['class_terms'] - L).max() <= TOL


# ---------------------------------------------------------------- the closed-form gradient against autograd over the paper's formulation
def _lovasz_autograd(logits, labels, ignore, classes):
    """The paper's lovasz_softmax_flat over torch.sort / cumsum on `logits`' graph (float64)."""
    B, C, H, W = logits.shape
    x = logits.reshape(B, C, -1).permute(0, 2, 1).reshape(-1, C)
    t = labels.reshape(-1)
    keep = t != ignore if ignore is not None else torch.ones_like(t, dtype=torch.bool)
    p, t = torch.softmax(x[keep], 1), t[keep]
    if p.numel() == 0:
        return logits.sum() * 0.0
    losses = []
    for c in range(C):
        fg = (t == c).double()
        if classes == 'present' and fg.sum() == 0:
            continue
        err = (fg - p[:, c]).abs()
        es, perm = torch.sort(err, descending=True, stable=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1 - fs).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac))
    return torch.stack(losses).mean() if losses else logits.sum() * 0.0


@pytest.mark.parametrize('classes', ['present', 'all'])
@pytest.mark.parametrize('ignore', [255, None])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_closed_form_gradient_is_autograd_through_sort_and_cumsum(shape, ignore, classes):
    for absent in (None, 1):
        logits, labels, mask = _inputs(shape, frac=0.3 if ignore is not None else 0.0, absent=absent)
        x = logits.clone().requires_grad_(True)
        want = _lovasz_autograd(x, labels, ignore, classes)
        (dwant,) = torch.autograd.grad(want, x)
        got = LR.evaluate(logits, labels, ignore, classes)
        assert abs(got['term'] - float(want.detach())) <= TOL, (got['term'], float(want))
        assert (got['dlogits'] - dwant).abs().max().item() <= TOL
        assert got['m'] == (shape[1] if classes == 'all' or absent is None else shape[1] - 1)
        assert not got['dlogits'][mask[:, None].expand_as(logits)].any() and got['dlogits'].abs().max() > 0


def test_hard_predictions_give_one_minus_iou():
    shape = (2, 3, 6, 5)
    _, labels, _ = _inputs(shape, frac=0.0)
    r = np.random.default_rng(5)
    pred = torch.from_numpy(r.integers(0, 3, labels.shape))
    logits = 120.0 * torch.nn.functional.one_hot(pred, 3).permute(0, 3, 1, 2).double() - 60.0      # softmax is exactly one-hot in float64
    iou = [float(((pred == c) & (labels == c)).sum()) / float(((pred == c) | (labels == c)).sum()) for c in range(3)]
    got = LR.evaluate(logits, labels)
    assert abs(got['term'] - np.mean([1 - v for v in iou])) <= TOL
    assert np.abs(got['class_terms'] - (1 - np.array(iou))).max() <= TOL


@pytest.mark.parametrize('classes', ['present', 'all'])
def test_ignored_pixels_and_their_logits_change_nothing(classes):
    shape = (3, 2, 9, 7)
    logits, labels, mask = _inputs(shape)
    a = LR.evaluate(logits, labels, 255, classes)
    bad = logits.clone()
    bad[mask[:, None].expand_as(bad)] = float('nan')
    b = LR.evaluate(bad, labels, 255, classes)
    assert a['term'] == b['term'] and torch.equal(a['dlogits'], b['dlogits'])
    # the valid pixels alone, as one row: the same term and the same gradient at those pixels
    keep = ~mask.reshape(-1)
    x = logits.reshape(3, 2, -1).permute(0, 2, 1).reshape(-1, 2)[keep].t().reshape(1, 2, 1, -1)
    c = LR.evaluate(x, labels.reshape(-1)[keep].reshape(1, 1, -1), None, classes)
    assert abs(a['term'] - c['term']) <= TOL
    da = a['dlogits'].reshape(3, 2, -1).permute(0, 2, 1).reshape(-1, 2)[keep]
    assert (da - c['dlogits'][0, :, 0].t()).abs().max().item() <= TOL
    every = LR.evaluate(logits, torch.full_like(labels, 255), 255, classes)          # no valid pixel
    assert every['term'] == 0.0 and not every['dlogits'].any() and every['m'] == 0
    out = LR.evaluate(logits, torch.full_like(labels, 7), None, 'present')           # labels outside the classes: foreground of no class
    assert out['term'] == 0.0 and out['m'] == 0 and not out['dlogits'].any()
    assert LR.evaluate(logits, torch.full_like(labels, 7), None, 'all')['term'] > 0


# ---------------------------------------------------------------- the ordering rule, in integers
def test_order_from_errors_on_ties_infinity_and_nan():
    v = np.array([0.5, 1.0, 0.5, 0.0, 1.0, 0.5], dtype=np.float32)
    ok = np.ones(6, bool)
    assert LR.order_from_errors(v, ok).tolist() == [1, 4, 0, 2, 5, 3]
    ok[4] = False
    o = LR.order_from_errors(v, ok)
    assert o.tolist() == [1, 0, 2, 5, 3] and LR.ranks_of(o, 6).tolist() == [1, 0, 2, 4, -1, 3]
    w = np.array([0.25, np.inf, np.nan, 1.0, np.nan], dtype=np.float32)
    assert LR.order_from_errors(w, np.ones(5, bool)).tolist() == [2, 4, 1, 3, 0]          # a (positive) NaN sits above +inf; ties by index
    same = np.full(9, 0.5, dtype=np.float32)
    assert LR.order_from_errors(same, np.ones(9, bool)).tolist() == list(range(9))
    r = np.random.default_rng(0)
    e = r.random(4000).astype(np.float32)
    e[r.integers(0, 4000, 600)] = e[r.integers(0, 4000, 600)]
    valid = r.random(4000) < 0.7
    idx = np.nonzero(valid)[0]
    assert (LR.order_from_errors(e, valid) == idx[np.argsort(-e[idx].astype(np.float64), kind='stable')]).all()


# ---------------------------------------------------------------- Criterion
def test_names_and_parse():
    assert CR.NAMES == ('tversky', 'dice', 'jaccard', 'focal', 'focal+tversky', 'focal+dice', 'focal+jaccard')
    assert CR.COMPOUND == ('focal+tversky', 'focal+dice', 'focal+jaccard') and CR.LOVASZ_NAMES == ('lovasz', 'focal+lovasz')
    c = Criterion.parse('lovasz')
    assert (c.w_overlap, c.w_focal, c.w_lovasz, c.lovasz_classes) == (0.0, 0.0, 1.0, 'present') and c._lovasz_only
    c = Criterion.parse('focal+lovasz', focal_gamma=2.0, weights=(0.25, 2), ignore_index=255, lovasz_classes='all', focal_alpha=0.25)
    assert (c.w_overlap, c.w_focal, c.w_lovasz, c.gamma, c.lovasz_classes, c.ignore_index) == (0.0, 0.25, 2.0, 2.0, 'all', 255)
    assert c.class_alpha == (0.25, 0.75) and not c._lovasz_only and "w_lovasz=2.0, lovasz_classes='all'" in repr(c)
    assert Criterion.parse('focal+lovasz', focal_gamma=0).gamma == 0.0 and Criterion.parse('focal+lovasz').gamma == 0.0       # CE + Lovasz
    assert Criterion.parse('focal+lovasz', focal_gamma=0.0, topk=0.25).topk_ppm == 250_000
    for bad in ('lovasz+focal', 'lovasz+dice', 'focal+lovasz+dice', 'Lovasz'):
        with pytest.raises(ValueError, match='unknown criterion'):
            Criterion.parse(bad, focal_gamma=2.0)
    with pytest.raises(ValueError, match='focal'):
        Criterion.parse('lovasz', topk=0.5)                                 # top-k ranks the focal term


def test_constructor_validation_and_defaults():
    d = Criterion()
    assert d.w_lovasz == 0.0 and d.lovasz_classes == 'present' and 'lovasz' not in repr(d)
    c = Criterion(w_overlap=0.5, alpha=1.0, beta=1.0, w_focal=1.0, gamma=2.0, w_lovasz=0.75, ignore_index=255, topk=0.25)
    assert (c.w_overlap, c.w_focal, c.w_lovasz) == (0.5, 1.0, 0.75)
    assert Criterion(w_overlap=0.0, w_lovasz=1.0)._lovasz_only
    for bad in (-1.0, -1e-9, float('nan')):
        with pytest.raises(ValueError, match='>= 0'):
            Criterion(w_lovasz=bad)
    for bad in ('some', None, 'ALL', 1):
        with pytest.raises(ValueError, match='lovasz_classes'):
            Criterion(w_lovasz=1.0, lovasz_classes=bad)
    with pytest.raises(ValueError, match='criterion weights are both zero'):
        Criterion(w_overlap=0.0, w_focal=0.0, w_lovasz=0.0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        Criterion.parse('lovasz').evaluate(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))


def test_criterion_from_opt_carries_the_lovasz_options():
    from fabric_amd.utils.helpers import criterion_from_opt
    opt = types.SimpleNamespace(loss_function='focal+lovasz', focal_gamma=0.0, loss_weights=[0.5, 2.0], ignore_label=255, lovasz_classes='all')
    c = criterion_from_opt(opt)
    assert (c.w_focal, c.w_lovasz, c.lovasz_classes, c.ignore_index, c.w_overlap) == (0.5, 2.0, 'all', 255, 0.0)
    del opt.lovasz_classes
    opt.loss_function = 'lovasz'
    c = criterion_from_opt(opt)
    assert c._lovasz_only and c.lovasz_classes == 'present' and c.w_lovasz == 1.0
    opt.loss_function = 'focal+dice'
    assert criterion_from_opt(opt).w_lovasz == 0.0


def _train(*args):
    return subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', *args], cwd=ROOT, capture_output=True,
                          text=True, timeout=600)


def test_cli_lovasz_needs_the_fused_step_a_gamma_and_a_known_classes_mode():
    for name in ('lovasz', 'focal+lovasz'):
        r = _train('--loss_function', name, '--focal_gamma', '0')
        assert r.returncode != 0 and '--fused_step true' in r.stderr, r.stderr[-500:]
    r = _train('--fused_step', 'true', '--loss_function', 'focal+lovasz')
    assert r.returncode != 0 and '--focal_gamma' in r.stderr, r.stderr[-500:]
    r = _train('--fused_step', 'true', '--loss_function', 'lovasz', '--lovasz_classes', 'some')
    assert r.returncode != 0 and 'lovasz_classes' in r.stderr, r.stderr[-500:]
    r = _train('--fused_step', 'true', '--loss_function', 'lovasz+focal', '--focal_gamma', '0')
    assert r.returncode != 0 and 'lovasz+focal' in r.stderr, r.stderr[-500:]
    r = _train('--fused_step', 'true', '--loss_function', 'lovasz', '--loss_topk', '0.25')
    assert r.returncode != 0 and 'focal term' in r.stderr, r.stderr[-500:]


# ---------------------------------------------------------------- the C ABI without a device
def test_lovasz_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+bdn_lovasz_softmax\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'bdn_lovasz_softmax not declared'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES['bdn_lovasz_softmax']
    assert res is ctypes.c_int and len(args) == len(params) == 17
    for p, a in zip(params, args):
        want = ctypes.c_void_p if '*' in p else ctypes.c_float if p.startswith('float') else ctypes.c_int
        assert a is want, (p, a)
    assert [p.split()[-1].lstrip('*') for p in params] == ['logits', 'labels', 'ignore_label', 'classes_all', 'weight', 'accumulate', 'ws', 'loss',
                                                           'term', 'dlogits', 'pixel_errors', 'ranks', 'B', 'ncls', 'H', 'W', 'stream']
    assert re.search(r'\bsize_t\s+bdn_lovasz_workspace_bytes\s*\(\s*int B, int ncls, int H, int W\)\s*;', hdr)
    assert _lib.SIGNATURES['bdn_lovasz_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    doc = hdr[hdr.index('the Lovasz-Softmax term'):hdr.index('bdn_lovasz_workspace_bytes(int B')]
    assert 'utils/helpers.py:303-312' in doc and 'CVPR 2018' in doc
    assert 'Lov' in open(os.path.join(ROOT, 'PAPERS.md')).read()
    lib = _lib.load()
    assert lib.bdn_lovasz_softmax and lib.bdn_lovasz_workspace_bytes


def _call(**over):
    """bdn_lovasz_softmax with fake non-null pointers: every argument check returns before anything touches a device."""
    lib = _lib.load()
    a = dict(logits=16, labels=16, ignore_label=255, classes_all=0, weight=1.0, accumulate=0, ws=16, loss=16, term=None, dlogits=None,
             pixel_errors=None, ranks=None, B=1, ncls=2, H=4, W=4, stream=None)
    a.update(over)
    rc = lib.bdn_lovasz_softmax(*a.values())
    return rc, lib.bdn_last_error().decode()


def test_lovasz_argument_errors_return_before_touching_a_device():
    for v in (-2, 256):
        rc, msg = _call(ignore_label=v)
        assert rc == -1 and 'ignore_label' in msg, (v, rc, msg)
    rc, msg = _call(weight=-1.0)
    assert rc == -1 and 'weight' in msg
    rc, msg = _call(weight=float('nan'))
    assert rc == -1 and 'weight' in msg
    for v in (1, 9):
        rc, msg = _call(ncls=v)
        assert rc == -2 and 'ncls' in msg
    rc, msg = _call(B=0)
    assert rc == -2
    rc, msg = _call(B=1 << 16, H=1 << 8, W=1 << 7)
    assert rc == -2 and '2^31' in msg
    rc, msg = _call(ws=8)
    assert rc == -1 and 'aligned' in msg
    for name in ('logits', 'labels', 'ws', 'loss'):
        rc, msg = _call(**{name: None})
        assert rc == -1 and 'null' in msg, name


def test_lovasz_workspace_size():
    ws = _lib.load().bdn_lovasz_workspace_bytes
    assert ws(1, 1, 4, 4) == 0 and ws(1, 9, 4, 4) == 0 and ws(0, 2, 4, 4) == 0 and ws(1 << 16, 2, 1 << 8, 1 << 7) == 0
    assert ws(1, 2, 0, 4) == 0 and ws(1, 2, 4, -1) == 0
    assert ws((1 << 16) - 1, 2, 1 << 8, 1 << 7) > 0                            # just below 2^31 pixels
    for shape in ((3, 2, 90, 77), (1, 8, 16, 300), (4, 2, 32, 32), (2, 3, 1, 5), (2, 2, 128, 128), (64, 2, 128, 128)):
        B, C, H, W = shape
        n, npix = ws(B, C, H, W), B * H * W
        tiles = (npix + 4095) // 4096
        # two buffers of 8-byte (key, payload) pairs per class (rows padded to 4 pixels); per class and tile of 4096 pixels 256 digit counts
        # and a foreground count (rows padded to 4 tiles) and a double; 256 digit totals per class; a valid count per tile; sixteen totals,
        # eight scales, padding
        own = 16 * C * npix
        more = 48 * C + (tiles + 3) * C * (1024 + 4) + tiles * (8 * C + 4) + 1024 * C + 64 + 32 + 48
        assert n % 16 == 0 and own <= n <= own + more, (shape, n, own, more)
