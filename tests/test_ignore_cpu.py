"""CPU tests of the ignore label: the float64 restatement tests/ignore_ref.py is pinned to the oracle's own loss functions
(oracle/bidate_oracle.py) by identities that hold exactly in real arithmetic (bar 1e-12 in float64), and the parts of the feature that
need no device: Criterion(ignore_index=), the --ignore_label checks of the training CLI, bdn_criterion_masked's declaration, argument
checks and workspace size, synthetic_onera(ignore_frac=)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import Criterion
from oracle import bidate_oracle as O
from tests import criterion_ref as CR
from tests import ignore_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2, 9, 7), (2, 5, 4, 33), (2, 3, 1, 5)]
TOL = 1e-12


def _inputs(shape, seed=3, frac=0.3, ignore=255):
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy(3 * r.standard_normal(shape))
    lbl = torch.from_numpy(r.integers(0, C, (B, H, W)))
    mask = torch.from_numpy(r.random((B, H, W)) < frac)
    if ignore < C:                                          # ignoring a real class: its pixels are the mask
        return logits, lbl, lbl == ignore
    return logits, torch.where(mask, torch.full_like(lbl, ignore), lbl), mask


def _class_alpha(C):
    return [0.25, 0.75] if C == 2 else [round(0.1 + 0.8 * k / (C - 1), 3) for k in range(C)]


def _overlap_criteria(reduce, ignore=255):
    return [Criterion.parse(n, tversky_alpha=0.1, tversky_beta=0.9, reduce=reduce, ignore_index=ignore) for n in ('tversky', 'dice', 'jaccard')]


def _focal_criteria(C, ignore=255):
    return [Criterion(w_overlap=0.0, w_focal=1.0, gamma=g, class_alpha=_class_alpha(C) if a else None, size_average=sa, ignore_index=ignore)
            for g in (0.0, 2.0) for a in (False, True) for sa in (True, False)]


def _grad(fn, x):
    x = x.detach().clone().requires_grad_(True)
    v = fn(x)
    return float(v.detach()), torch.autograd.grad(v, x)[0]


def _close(a, b, what):
    err = abs(a - b) if isinstance(a, float) else (a - b).abs().max().item()
    assert err <= TOL, (what, err)


# ---------------------------------------------------------------- 1. no pixel ignored: the oracle's function
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_no_pixel_ignored_is_the_oracle_function(shape):
    logits, lbl, _ = _inputs(shape, frac=0.0)
    for reduce, labels in (('columns', lbl), ('image', lbl[:, None])):
        for c in _overlap_criteria(reduce):
            ref = IR.reference(c, logits, lbl)
            v, g = _grad(lambda x: CR.overlap_fn(c)(x, labels), logits)
            _close(ref['loss'], v, (c, 'loss'))
            _close(ref['dloss'], g, (c, 'grad'))
    for c in _focal_criteria(shape[1]):
        ref = IR.reference(c, logits, lbl)
        v, g = _grad(lambda x: O.focal_loss(x, lbl, c.gamma, list(c.class_alpha) if c.class_alpha else None, c.size_average), logits)
        _close(ref['loss'], v, (c, 'loss'))
        _close(ref['dloss'], g, (c, 'grad'))
    c = Criterion.parse('focal+dice', focal_gamma=2.0, weights=(0.25, 2), ignore_index=255)
    ref, ref0 = IR.reference(c, logits, lbl), CR.reference(Criterion.parse('focal+dice', focal_gamma=2.0, weights=(0.25, 2)), logits, lbl)
    _close(ref['loss'], ref0['loss'], 'compound loss')
    _close(ref['dloss'], ref0['dloss'], 'compound grad')
    assert IR.counts(logits, lbl, 255) == CR.counts(logits, lbl) + [lbl.numel()]


# ---------------------------------------------------------------- 2. / 3. any mask: the oracle's function on the compacted valid pixels
def _compact(logits, lbl, valid):
    """-> ([1,C,1,Nv] logits, [Nv] labels, scatter(g [1,C,1,Nv]) -> [B,C,H,W] with zeros at the ignored pixels)."""
    B, C, H, W = logits.shape
    idx = valid.reshape(-1).nonzero().view(-1)
    flat = logits.permute(1, 0, 2, 3).reshape(C, -1)

    def scatter(g):
        out = torch.zeros(C, B * H * W, dtype=g.dtype)
        out[:, idx] = g.reshape(C, -1)
        return out.reshape(C, B, H, W).permute(1, 0, 2, 3)
    return flat[:, idx].reshape(1, C, 1, -1), lbl.reshape(-1)[idx], scatter


@pytest.mark.parametrize('ignore', [255, 0])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_image_reduction_and_focal_are_the_oracle_on_the_compacted_pixels(shape, ignore):
    logits, lbl, mask = _inputs(shape, ignore=ignore)
    assert mask.any() and not mask.all()
    cl, ct, scatter = _compact(logits, lbl, ~mask)
    for c in _overlap_criteria('image', ignore):
        ref = IR.reference(c, logits, lbl)
        v, g = _grad(lambda x: CR.overlap_fn(c)(x, ct.view(1, 1, 1, -1)), cl)
        _close(ref['loss'], v, (c, 'loss'))
        _close(ref['dloss'], scatter(g), (c, 'grad'))
        assert (ref['dloss'][mask[:, None].expand_as(logits)] == 0).all()
    for c in _focal_criteria(shape[1], ignore):
        ref = IR.reference(c, logits, lbl)
        v, g = _grad(lambda x: O.focal_loss(x, ct, c.gamma, list(c.class_alpha) if c.class_alpha else None, c.size_average), cl)
        _close(ref['loss'], v, (c, 'loss'))
        _close(ref['dloss'], scatter(g), (c, 'grad'))
        assert (ref['dloss'][mask[:, None].expand_as(logits)] == 0).all()
    # ... and what the ignored logits hold does not matter, inf and NaN included
    bad = logits.clone()
    poison = torch.tensor([1e30, float('inf'), -float('inf'), float('nan')], dtype=logits.dtype)
    bad[mask[:, None].expand_as(logits)] = poison.repeat(logits.numel())[:int(mask.sum()) * shape[1]]
    c = Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, ignore_index=ignore)
    a, b = IR.reference(c, logits, lbl), IR.reference(c, bad, lbl)
    assert a['loss'] == b['loss'] and torch.equal(a['dloss'], b['dloss']) and IR.counts(logits, lbl, ignore) == IR.counts(bad, lbl, ignore)


# ---------------------------------------------------------------- 4. columns, the same rows ignored in every image: rows removed
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_column_reduction_with_whole_rows_ignored_is_the_oracle_without_those_rows(shape):
    """Rows 1, 4, 7, ... of every image are ignored (none at H = 1, where the identity is that of no ignored pixel)."""
    logits, lbl, _ = _inputs(shape, frac=0.0)
    H = shape[2]
    rows = torch.zeros(H, dtype=torch.bool)
    rows[1::3] = True
    keep = (~rows).nonzero().view(-1)
    masked = lbl.clone()
    masked[:, rows] = 255
    for c in _overlap_criteria('columns'):
        ref = IR.reference(c, logits, masked)
        v, g = _grad(lambda x: CR.overlap_fn(c)(x, lbl[:, keep]), logits[:, :, keep])
        full = torch.zeros_like(logits)
        full[:, :, keep] = g
        _close(ref['loss'], v, (c, 'loss'))
        _close(ref['dloss'], full, (c, 'grad'))
        assert (ref['dloss'][:, :, rows] == 0).all()


# ---------------------------------------------------------------- 5. all ignored
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_all_ignored_gives_overlap_one_focal_zero_and_no_gradient(shape):
    logits, lbl, _ = _inputs(shape)
    lbl = torch.full_like(lbl, 255)
    for reduce in ('columns', 'image'):
        for sa in (True, False):
            c = Criterion(1.0, 0.5, 0.5, 5e-8, reduce, w_focal=1.0, gamma=2.0, size_average=sa, ignore_index=255)
            ref = IR.reference(c, logits, lbl)
            assert ref['overlap'] == 1.0 and ref['focal'] == 0.0 and ref['loss'] == 1.0 and not ref['dloss'].any()
    assert IR.counts(logits, lbl, 255) == [0, 0, 0, 0, 0]


# ---------------------------------------------------------------- Criterion
def test_criterion_ignore_index_validation_and_repr():
    assert Criterion().ignore_index is None and 'ignore_index' not in repr(Criterion())
    c = Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255)
    assert c.ignore_index == 255 and repr(c).endswith('ignore_index=255)')
    assert Criterion(ignore_index=0).ignore_index == 0 and Criterion.parse('tversky', ignore_index=7).ignore_index == 7
    for bad in (-1, 256, 1.5, 'x', True):
        with pytest.raises((ValueError, TypeError)):
            Criterion(ignore_index=bad)
    with pytest.raises(ValueError, match='0..255'):
        Criterion.parse('dice', ignore_index=300)
    with pytest.raises(RuntimeError, match='no CPU path'):
        Criterion(ignore_index=255).evaluate(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))


def test_criterion_from_opt_carries_the_ignore_label():
    import types
    from fabric_amd.utils.helpers import criterion_from_opt
    opt = types.SimpleNamespace(loss_function='tversky', tversky_alpha=0.1, tversky_beta=0.9, ignore_label=255)
    assert criterion_from_opt(opt).ignore_index == 255
    del opt.ignore_label
    assert criterion_from_opt(opt).ignore_index is None


# ---------------------------------------------------------------- the CLI's checks (refused while the options are read: no step runs)
def _train(*args):
    return subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', *args], cwd=ROOT, capture_output=True,
                          text=True, timeout=600)


def test_cli_ignore_label_needs_the_fused_step_and_a_byte():
    r = _train('--ignore_label', '255')
    assert r.returncode != 0 and '--fused_step true' in r.stderr, r.stderr[-500:]
    r = _train('--ignore_label', '255', '--loss_function', 'dice')
    assert r.returncode != 0 and '--fused_step true' in r.stderr, r.stderr[-500:]
    r = _train('--fused_step', 'true', '--ignore_label', '256')
    assert r.returncode != 0 and '0..255' in r.stderr, r.stderr[-500:]
    r = _train('--fused_step', 'true', '--ignore_label', '-1')
    assert r.returncode != 0 and '0..255' in r.stderr, r.stderr[-500:]


def test_batch_accuracy_divides_by_the_valid_count():
    from fabric_amd.train import batch_accuracy
    assert batch_accuracy([1, 2, 3, 50], 200) == 25.0
    assert batch_accuracy([1, 2, 3, 50, 100], 200) == 50.0
    assert batch_accuracy([0, 0, 0, 0, 0], 200) == 0.0


# ---------------------------------------------------------------- the entry point: declared, exported, checked
_CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'const uint8_t*': ctypes.c_void_p,
           'int32_t*': ctypes.c_void_p, 'float': ctypes.c_float, 'int': ctypes.c_int}


def test_masked_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+bdn_criterion_masked\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'bdn_criterion_masked not declared'
    types = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())).rsplit(' ', 1)[0].strip() for p in m.group(1).split(',')]
    res, args = _lib.SIGNATURES['bdn_criterion_masked']
    assert res is ctypes.c_int and [_CTYPES[t] for t in types] == list(args), (types, args)
    assert re.search(r'\bsize_t\s+bdn_criterion_masked_workspace_bytes\s*\(\s*int B, int ncls, int H, int W, int reduce_w\)\s*;', hdr)
    assert _lib.SIGNATURES['bdn_criterion_masked_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    # the existing signatures do not change: the masked entry is bdn_criterion's plus the label
    assert args[:2] + args[3:] == _lib.SIGNATURES['bdn_criterion'][1]
    lib = _lib.load()
    assert lib.bdn_criterion_masked and lib.bdn_criterion_masked_workspace_bytes


def _crit(**kw):
    a = dict(logits=16, labels=16, ignore_label=255, w_overlap=1.0, alpha=0.5, beta=0.5, eps=1e-7, reduce_w=0, w_focal=1.0, gamma=2.0,
             class_alpha=None, size_average=1, ws=16, loss=16, terms=None, counts=None, dlogits=None, B=2, ncls=2, H=8, W=8, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    lib = _lib.load()
    rc = lib.bdn_criterion_masked(*a.values())
    return rc, lib.bdn_last_error()


def test_masked_argument_errors_return_before_touching_a_device():
    for name in ('logits', 'labels', 'ws', 'loss'):
        rc, msg = _crit(**{name: None})
        assert rc != 0 and b'null pointer' in msg, name
    for v in (-1, 256, 1 << 20):
        rc, msg = _crit(ignore_label=v)
        assert rc != 0 and b'0..255' in msg, v
    rc, msg = _crit(w_overlap=0.0, w_focal=0.0)
    assert rc != 0 and b'both weights are zero' in msg
    for kw in (dict(w_overlap=-1.0), dict(w_focal=-0.5), dict(w_overlap=float('nan'))):
        rc, msg = _crit(**kw)
        assert rc != 0 and b'negative weight' in msg, kw
    rc, msg = _crit(gamma=-1.0)
    assert rc != 0 and b'negative gamma' in msg
    for ncls in (1, 9):
        rc, msg = _crit(ncls=ncls)
        assert rc != 0 and b'ncls' in msg, ncls
    rc, msg = _crit(B=1 << 15, H=1 << 8, W=1 << 8)                                # B*H*W = 2^31
    assert rc != 0 and b'2^31' in msg
    rc, msg = _crit(B=0)
    assert rc != 0 and b'bad shape' in msg
    rc, msg = _crit(ws=24)
    assert rc != 0 and b'aligned' in msg


def test_masked_workspace_size():
    lib = _lib.load()
    ws = lib.bdn_criterion_masked_workspace_bytes
    for shape in [(64, 2, 128, 128), (3, 2, 90, 77), (1, 8, 16, 300), (2, 3, 1, 5), (2, 2, 1, 1)]:
        B, C, H, W = shape
        for reduce_w in (0, 1):
            n = ws(B, C, H, W, reduce_w)
            assert 0 < n <= lib.bdn_criterion_workspace_bytes(B, C, H, W, reduce_w) + 4096, shape
    assert ws(0, 2, 8, 8, 0) == 0 and ws(2, 1, 8, 8, 0) == 0 and ws(2, 9, 8, 8, 0) == 0 and ws(2, 2, 0, 8, 0) == 0 and ws(2, 2, 8, -1, 1) == 0
    assert ws(1 << 15, 2, 1 << 8, 1 << 8, 0) == 0                                 # B*H*W = 2^31


# ---------------------------------------------------------------- synthetic data with unlabelled regions
def test_synthetic_onera_ignore_frac():
    from fabric_amd.utils.dataloaders import synthetic_onera
    a, b = synthetic_onera(n_cities=2, size=(120, 100)), synthetic_onera(n_cities=2, size=(120, 100), ignore_frac=0.0)
    c = synthetic_onera(n_cities=2, size=(120, 100), ignore_frac=0.2)
    r = np.random.default_rng(0)                            # today's arrays: the first draw of the function as it always was
    assert np.array_equal(a['city0']['images'][0], r.standard_normal((13, 120, 100)).astype(np.float32))
    for k in a:
        assert np.array_equal(a[k]['images'], b[k]['images']) and np.array_equal(a[k]['labels'], b[k]['labels'])
        assert a[k]['labels'].max() == 1
        m = c[k]['labels'] == 255
        assert np.array_equal(a[k]['images'], c[k]['images']) and np.array_equal(a[k]['labels'][~m], c[k]['labels'][~m])
        assert 0.2 <= m.mean() < 0.5 and m[:, 0].all() and set(np.unique(c[k]['labels'])) <= {0, 1, 255}
    d = synthetic_onera(n_cities=1, size=(120, 100), ignore_frac=0.1, ignore_value=7)
    assert set(np.unique(d['city0']['labels'])) <= {0, 1, 7}
