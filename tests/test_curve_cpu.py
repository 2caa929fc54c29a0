"""CPU tests of the score curve: the host restatement tests/curve_ref.py is pinned to brute force (score >= float32(i / n_bins) counted per
threshold, F.argmax()) and to sklearn's average_precision_score / precision_recall_curve on the bin-quantised scores; then the parts of
the feature that need no device: the declarations of bdn_score_hist / bdn_score_curve / bdn_threshold_mask against _lib.SIGNATURES, every
argument check of the three (fake non-null pointers: each returns before anything touches a device), ScoreCurve's and threshold='s
validation and the --val_curve_bins / --scene_threshold checks of the training CLI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score, precision_recall_curve

from fabric_amd import _lib
from fabric_amd.utils import metrics as M
from tests import curve_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = (2, 64, 1024, 4096)
AP_TOL = 1e-12          # at most 4096 terms, each <= 1, summed in double: worst case 4096 * 2^-53 ~ 4.5e-13


def _scores(n_bins, n=6000, seed=0):
    """float32 scores in [0, 1] and one above: random ones, exact bin edges k / n_bins and their lower neighbours, 0, 1 and 2."""
    r = np.random.default_rng(seed + n_bins)
    s = r.random(n).astype(np.float32) ** 3                                   # skewed towards 0, like change probabilities
    k = r.integers(0, n_bins + 1, 400)
    edge = (k / n_bins).astype(np.float32)
    s = np.concatenate([s, edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(2)), np.float32([0, 1, 2, 1e-45, 1e-30])])
    labels = (r.random(s.size) < 0.2 + 0.5 * np.minimum(s, 1)).astype(np.uint8)
    return s.astype(np.float32), labels


# ---------------------------------------------------------------- the restatement against brute force
@pytest.mark.parametrize('n_bins', BINS)
def test_bins_are_the_thresholds(n_bins):
    s, _ = _scores(n_bins)
    b = CR.bins(s, n_bins)
    assert b.min() >= 0 and b.max() == n_bins - 1
    for i in sorted({0, 1, n_bins // 2, n_bins - 1} | set(np.random.default_rng(1).integers(0, n_bins, 40).tolist())):
        assert np.array_equal(b >= i, s >= np.float32(i / n_bins)), i


def test_bins_of_the_values_outside_the_unit_interval():
    s = np.float32([np.nan, -1.0, -0.0, 0.0, 2.0, np.inf, -np.inf, 1.0, np.nextafter(np.float32(1), np.float32(0))])
    for n in BINS:
        assert CR.bins(s, n).tolist() == [0, 0, 0, 0, n - 1, n - 1, 0, n - 1, n - 1]
    assert CR.bins(np.float32([0.5, 0.25, 0.75, np.nextafter(np.float32(0.5), np.float32(0))]), 2).tolist() == [1, 0, 1, 0]


@pytest.mark.parametrize('ignore', [None, 255])
@pytest.mark.parametrize('n_bins', BINS)
def test_curve_is_the_brute_force_count(n_bins, ignore):
    s, l = _scores(n_bins)
    if ignore is not None:
        l = np.where(np.random.default_rng(2).random(l.size) < 0.3, ignore, l).astype(np.uint8)
    h = CR.histogram(s, l, n_bins, 1, ignore)
    c = CR.curve(h)
    valid = np.ones(l.size, bool) if ignore is None else l != ignore
    assert h.sum() == valid.sum() and h[1].sum() == (l == 1).sum()
    n_pos = int((l == 1).sum())
    F = np.zeros(n_bins)
    for i in range(n_bins):
        pred = s >= np.float32(i / n_bins)
        tp, fp = int((pred & valid & (l == 1)).sum()), int((pred & valid & (l != 1)).sum())
        assert (tp, fp) == (c['TP'][i], c['FP'][i]), i
        assert c['P'][i] == (tp / (tp + fp) if tp + fp else 0.0) and c['R'][i] == tp / n_pos
        F[i] = 2 * tp / (2 * tp + fp + n_pos - tp)
    assert np.array_equal(F, c['F'])
    sm = CR.summary(h)
    assert sm['i_best'] == int(F.argmax()) and sm['F_best'] == F.max() and sm['t_best'] == sm['i_best'] / n_bins
    assert (sm['n_pos'], sm['n_neg']) == (n_pos, int((valid & (l != 1)).sum()))
    assert sm['P_best'] == c['P'][sm['i_best']] and sm['R_best'] == c['R'][sm['i_best']]


def test_degenerate_histograms_and_the_tie_rule():
    z = CR.summary(np.zeros((2, 8), np.int64))
    assert z == {'F_best': 0.0, 't_best': 0.0, 'i_best': 0, 'P_best': 0.0, 'R_best': 0.0, 'AP': 0.0, 'n_pos': 0, 'n_neg': 0}
    h = np.zeros((2, 8), np.int64); h[0, 3] = 5                               # no positives
    assert CR.summary(h)['i_best'] == 0 and CR.summary(h)['AP'] == 0.0 and CR.summary(h)['n_neg'] == 5
    h = np.zeros((2, 8), np.int64); h[1, 5] = 7                               # no negatives: F = 1 for every threshold up to bin 5
    s = CR.summary(h)
    assert (s['i_best'], s['F_best'], s['AP'], s['P_best'], s['R_best']) == (0, 1.0, 1.0, 1.0, 1.0)
    h = np.zeros((2, 8), np.int64); h[0, 1] = 4; h[1, 6] = 3                  # F = 1 on 2..6 (empty bins between): the first wins
    assert CR.summary(h)['i_best'] == 2 and CR.summary(h)['t_best'] == 0.25
    big = np.zeros((2, 4), np.int64); big[0] = [1 << 40, 3, 1 << 39, 0]; big[1] = [5, 1 << 40, 0, (1 << 40) + 1]
    c = CR.curve(big)
    assert c['TP'][0] == (1 << 41) + 6 and c['FP'][0] == (1 << 40) + (1 << 39) + 3


# ---------------------------------------------------------------- the restatement against sklearn
@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('n_bins', BINS)
def test_average_precision_and_curve_match_sklearn(n_bins, seed):
    s, l = _scores(n_bins, seed=seed)
    h = CR.histogram(s, l, n_bins)
    q = CR.bins(s, n_bins) / n_bins                                           # the bin-quantised scores, exact in float64
    got = CR.summary(h)['AP']
    want = average_precision_score(l, q)
    print(f'n_bins={n_bins} seed={seed}: AP {got!r} sklearn {want!r} |d|={abs(got - want):.3e}')
    assert abs(got - want) <= AP_TOL
    p, r, t = precision_recall_curve(l, q)
    c = CR.curve(h)
    idx = np.rint(t * n_bins).astype(np.int64)                                # sklearn's thresholds: the distinct quantised scores
    assert np.array_equal(idx / n_bins, t)
    assert np.abs(c['P'][idx] - p[:-1]).max() <= 1e-15 and np.abs(c['R'][idx] - r[:-1]).max() <= 1e-15
    assert (p[-1], r[-1]) == (1.0, 0.0)


# ---------------------------------------------------------------- Python surface without a device
def test_score_curve_and_threshold_validation():
    sc = M.ScoreCurve()
    assert (sc.n_bins, sc.pos_class, sc.ignore_index) == (1024, 1, None)
    for bad in (0, 1, 3, 100, 8192, 2.0, True, '64', None):
        with pytest.raises(ValueError, match='n_bins'):
            M.ScoreCurve(n_bins=bad)
    for bad in (-1, 256, 1.0, True):
        with pytest.raises(ValueError, match='pos_class'):
            M.ScoreCurve(pos_class=bad)
        with pytest.raises(ValueError, match='ignore_index'):
            M.ScoreCurve(ignore_index=bad)
    with pytest.raises(RuntimeError, match='no CPU path'):
        sc.update(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU path'):
        sc.update_proba(torch.zeros(2, 4, 4), torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='differ'):
        sc.merge(M.ScoreCurve(n_bins=64))
    assert M.check_threshold(None) == (None, 1) and M.check_threshold(0.25, 0, 3) == (0.25, 0)
    assert M.check_threshold(0) == (0.0, 1) and M.check_threshold(1) == (1.0, 1)
    for bad in (-0.01, 1.0001, float('nan'), float('inf'), '0.5', True, [0.5]):
        with pytest.raises(ValueError, match='threshold'):
            M.check_threshold(bad)
    for bad in (-1, 2, 1.0, True, None):
        with pytest.raises(ValueError, match='pos_class'):
            M.check_threshold(0.5, bad, 2)
    import inspect
    from fabric_amd.utils.inference import predict_scene_blended
    sig = inspect.signature(predict_scene_blended).parameters
    assert sig['threshold'].default is None and sig['pos_class'].default == 1


def test_cli_curve_flag_checks():
    from fabric_amd.train import check_curve_flags
    assert check_curve_flags(0, 'argmax', 0) == 'argmax' and check_curve_flags(256, 'argmax', 0) == 'argmax'
    assert check_curve_flags(256, 'val', 64) == 'val' and check_curve_flags(0, '0.35', 64) == 0.35
    for n in (1, 3, 100, 8192, -2):
        with pytest.raises(ValueError, match='val_curve_bins'):
            check_curve_flags(n, 'argmax', 0)
    with pytest.raises(ValueError, match='--val_curve_bins N'):
        check_curve_flags(0, 'val', 64)
    with pytest.raises(ValueError, match='scene_stride'):
        check_curve_flags(256, 'val', 0)
    for bad in ('1.5', '-0.1', 'nan', 'best'):
        with pytest.raises(ValueError, match='scene_threshold'):
            check_curve_flags(0, bad, 64)
    r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', '--scene_stride', '64', '--scene_threshold', 'val'],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and '--val_curve_bins N' in r.stderr, r.stderr[-500:]


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


@pytest.mark.parametrize('name,n_args', [('bdn_score_hist', 12), ('bdn_score_curve', 5), ('bdn_threshold_mask', 7)])
def test_curve_entry_points_are_declared_and_exported(name, n_args):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(params) == n_args
    for p, a in zip(params, args):
        assert a is _ctype(p), (p, a)
    assert params[-1] == 'void* stream'
    sec = hdr[hdr.index('threshold-free validation'):hdr.index('int bdn_score_hist(')]
    for cite in ('train.py:96-106', 'train.py:151-158', 'train.py:199'):
        assert cite in sec
    assert 'do not depend on arrival order' in sec
    assert getattr(_lib.load(), name)


def _call(name, defaults, over):
    lib = _lib.load()
    a = dict(defaults)
    a.update(over)
    rc = getattr(lib, name)(*a.values())
    return rc, lib.bdn_last_error().decode()


_HIST = dict(x=64, x_is_logits=1, labels=64, ignore_label=-1, pos_class=1, n_img=1, ncls=2, HW=16, n_bins=64, hist=64, scores_out=None, stream=None)
_CURVE = dict(hist=64, n_bins=64, curve_out=None, summary=64, stream=None)
_MASK = dict(proba=64, pos_class=1, threshold=0.5, mask=64, ncls=2, HW=16, stream=None)


def test_score_hist_argument_errors_return_before_touching_a_device():
    for v in (0, 1, 3, 100, 8192, -4):
        rc, msg = _call('bdn_score_hist', _HIST, dict(n_bins=v))
        assert rc == -1 and 'n_bins' in msg, (v, rc, msg)
    for v in (-1, 2, 300):
        rc, msg = _call('bdn_score_hist', _HIST, dict(pos_class=v))
        assert rc == -1 and 'pos_class' in msg, (v, rc, msg)
    rc, msg = _call('bdn_score_hist', _HIST, dict(pos_class=8, ncls=8))
    assert rc == -1 and 'pos_class' in msg
    for v in (-2, 256):
        rc, msg = _call('bdn_score_hist', _HIST, dict(ignore_label=v))
        assert rc == -1 and 'ignore_label' in msg, (v, rc, msg)
    for v in (1, 0, -3, 257):
        rc, msg = _call('bdn_score_hist', _HIST, dict(ncls=v))
        assert rc == -2 and 'ncls' in msg, (v, rc, msg)
    for k in ('x', 'labels', 'hist'):
        rc, msg = _call('bdn_score_hist', _HIST, {k: None})
        assert rc == -1 and 'null' in msg, (k, rc, msg)
    for over in (dict(n_img=0), dict(HW=0), dict(HW=-5), dict(n_img=1 << 20, HW=1 << 21)):
        rc, msg = _call('bdn_score_hist', _HIST, over)
        assert rc == -2, (over, rc, msg)
    rc, msg = _call('bdn_score_hist', _HIST, dict(x_is_logits=2))
    assert rc == -1 and 'x_is_logits' in msg
    rc, msg = _call('bdn_score_hist', _HIST, dict(hist=68))
    assert rc == -1 and 'aligned' in msg


def test_score_curve_argument_errors_return_before_touching_a_device():
    for v in (0, 1, 3, 100, 8192, -4):
        rc, msg = _call('bdn_score_curve', _CURVE, dict(n_bins=v))
        assert rc == -1 and 'n_bins' in msg, (v, rc, msg)
    for k in ('hist', 'summary'):
        rc, msg = _call('bdn_score_curve', _CURVE, {k: None})
        assert rc == -1 and 'null' in msg, (k, rc, msg)
    rc, msg = _call('bdn_score_curve', _CURVE, dict(curve_out=68))
    assert rc == -1 and 'aligned' in msg


def test_threshold_mask_argument_errors_return_before_touching_a_device():
    for v in (-0.001, 1.001, float('nan'), float('inf'), -float('inf')):
        rc, msg = _call('bdn_threshold_mask', _MASK, dict(threshold=v))
        assert rc == -1 and 'threshold' in msg, (v, rc, msg)
    for v in (-1, 2):
        rc, msg = _call('bdn_threshold_mask', _MASK, dict(pos_class=v))
        assert rc == -1 and 'pos_class' in msg, (v, rc, msg)
    for v in (1, 0, 257):
        rc, msg = _call('bdn_threshold_mask', _MASK, dict(ncls=v))
        assert rc == -2 and 'ncls' in msg, (v, rc, msg)
    for k in ('proba', 'mask'):
        rc, msg = _call('bdn_threshold_mask', _MASK, {k: None})
        assert rc == -1 and 'null' in msg, (k, rc, msg)
    for v in (0, -1):
        rc, msg = _call('bdn_threshold_mask', _MASK, dict(HW=v))
        assert rc == -2, (v, rc, msg)
