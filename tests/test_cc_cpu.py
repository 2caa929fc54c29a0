"""CPU tests of the connected-component feature: the host restatement tests/cc_ref.py is pinned to scipy.ndimage.label (compact labels, both
connectivities), np.bincount (areas), scipy.ndimage.find_objects (boxes) and brute force (filter, object scores); then the parts that
need no device: the declarations of the bdn_cc_* entries against _lib.SIGNATURES, every argument check of every C entry (fake non-null
pointers: each returns BDN_E_ARG before anything touches a device), check_cc_args, check_object_flags and the training CLI's flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import objects as O
from tests import cc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 5), (5, 1), (7, 13), (67, 93)]


def _structure(ndi, conn):
    return ndi.generate_binary_structure(2, 1 if conn == 4 else 2)


# ---------------------------------------------------------------- the restatement against scipy / numpy / brute force
@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('shape', SHAPES)
def test_compact_labels_are_scipys(shape, conn):
    ndi = pytest.importorskip('scipy.ndimage')
    for name, m in R.patterns(*shape, tile=64).items():
        lab = R.label(m == 1, conn)
        want, n = ndi.label(m, _structure(ndi, conn))
        assert np.array_equal(R.compact(lab), want), name
        assert R.counts(lab) == (n, int(m.sum())), name
        # canonical labels: 1 + the smallest linear index of the component
        for k in range(1, min(n, 20) + 1):
            assert (lab[want == k] == np.flatnonzero(want.ravel() == k)[0] + 1).all(), (name, k)
        assert (lab[m == 0] == 0).all()


@pytest.mark.parametrize('conn', [4, 8])
def test_areas_and_boxes(conn):
    ndi = pytest.importorskip('scipy.ndimage')
    H, W = 67, 93
    r = np.random.default_rng(3)
    other = r.integers(0, 3, (H, W)).astype(np.uint8)
    for name, m in R.patterns(H, W, tile=64).items():
        lab = R.label(m == 1, conn)
        comp = R.compact(lab)
        n = int(comp.max())
        area = R.areas(lab)
        cnt = np.bincount(comp.ravel(), minlength=n + 1)[1:]
        roots = np.flatnonzero(lab.ravel() == np.arange(1, H * W + 1))
        assert np.array_equal(area.ravel()[roots], cnt), name
        assert area.sum() == m.sum() and np.count_nonzero(area) == n
        t = R.stats_table(comp, n + 2, other, 2)
        assert np.array_equal(t[:n, 0], cnt) and (t[:, 6:] == 0).all()
        for k, sl in enumerate(ndi.find_objects(comp)):
            assert tuple(t[k, 1:5]) == (sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1), (name, k)
            assert t[k, 5] == int(((comp == k + 1) & (other == 2)).sum())
        assert (t[n:] == [0, H, W, -1, -1, 0, 0, 0]).all()
        assert (R.stats_table(comp, n + 2)[:, 5] == 0).all()
        if n > 1:                                          # labels above n_max are skipped
            assert np.array_equal(R.stats_table(comp, n - 1, other, 2), t[:n - 1])
        # an excluded pixel adds to no column
        te = R.stats_table(comp, n + 2, other, 2, 0)
        assert np.array_equal(te[:n, 0], np.bincount(comp[other != 0].ravel(), minlength=n + 1)[1:]) and np.array_equal(te[:, 5], t[:, 5])


@pytest.mark.parametrize('conn', [4, 8])
def test_filter_is_brute_force(conn):
    ndi = pytest.importorskip('scipy.ndimage')
    for name, m in R.patterns(40, 51, tile=64).items():
        want_lab, n = ndi.label(m, _structure(ndi, conn))
        size = np.bincount(want_lab.ravel())
        biggest = int(size[1:].max()) if n else 0
        for k in (1, 2, 5, biggest, biggest + 1):
            want = ((want_lab > 0) & (size[want_lab] >= k)).astype(np.uint8)
            assert np.array_equal(R.remove_small(m, max(k, 1), conn), want), (name, k)


def _brute_scores(pred, truth, pos, ign, conn, min_area, min_overlap, ndi):
    p = (pred == 1) & (truth != ign if ign is not None else True)
    lp, n_p = ndi.label(p, _structure(ndi, conn))
    keep = [k for k in range(1, n_p + 1) if (lp == k).sum() >= min_area]
    kept = np.isin(lp, keep)
    lt, n_t = ndi.label(truth == pos, _structure(ndi, conn))
    ph = sum(int(((lp == k) & (truth == pos)).sum()) >= min_overlap for k in keep)
    th = sum(int(((lt == k) & kept).sum()) >= min_overlap for k in range(1, n_t + 1))
    return len(keep), n_t, ph, th


@pytest.mark.parametrize('ign', [None, 255])
@pytest.mark.parametrize('conn', [4, 8])
def test_object_scores_are_brute_force(conn, ign):
    ndi = pytest.importorskip('scipy.ndimage')
    r = np.random.default_rng(11)
    H, W = 48, 61
    blobs = ndi.binary_dilation(r.random((H, W)) < 0.02, iterations=2)
    truth = blobs.astype(np.uint8)
    if ign is not None:
        truth[r.random((H, W)) < 0.15] = ign
    pred = (np.roll(blobs, 2, 1) | (r.random((H, W)) < 0.03)).astype(np.uint8)
    for min_area in (1, 4):
        for min_overlap in (1, 3):
            got = R.object_scores(pred, truth, 1, ign, conn, min_area, min_overlap)
            n_p, n_t, ph, th = _brute_scores(pred, truth, 1, ign, conn, min_area, min_overlap, ndi)
            assert (got['objects_pred'], got['objects_true'], got['pred_hit'], got['true_hit']) == (n_p, n_t, ph, th)
            assert got['object_precision'] == ph / n_p and got['object_recall'] == th / n_t
            assert got['object_f1'] == pytest.approx(2 * ph / n_p * th / n_t / (ph / n_p + th / n_t), abs=1e-15)


def test_object_scores_of_empty_rasters_are_zero():
    z, one = np.zeros((9, 11), np.uint8), np.zeros((9, 11), np.uint8)
    one[2:4, 3:6] = 1
    for pred, truth in ((z, one), (one, z), (z, z)):
        s = R.object_scores(pred, truth)
        assert s['object_precision'] == 0.0 and s['object_recall'] == 0.0 and s['object_f1'] == 0.0
        assert all(np.isfinite(v) for v in s.values())
    s = R.object_scores(one, one)
    assert (s['objects_pred'], s['objects_true'], s['object_f1']) == (1, 1, 1.0)
    ign = one.copy()
    ign[:] = 255                                           # everything ignored: no predicted object survives
    assert R.object_scores(one, ign, ignore_index=255)['objects_pred'] == 0


# ---------------------------------------------------------------- Python surface without a device
def test_check_cc_args():
    m = torch.zeros(5, 7, dtype=torch.uint8)
    assert O.check_cc_args(m) == (5, 7) and O.check_cc_args(m, 4, 0, m, 255, 3) == (5, 7)
    for bad in (torch.zeros(5, 7), torch.zeros(5, dtype=torch.uint8), torch.zeros(2, 5, 7, dtype=torch.uint8), np.zeros((5, 7), np.uint8),
                torch.zeros(0, 7, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='mask'):
            O.check_cc_args(bad)
    with pytest.raises(ValueError, match='contiguous'):
        O.check_cc_args(torch.zeros(7, 5, dtype=torch.uint8).t())
    with pytest.raises(ValueError, match='2\\^31 - 2'):
        O.check_cc_args(torch.empty(46341, 46341, dtype=torch.uint8, device='meta'))
    assert O.check_cc_args(torch.empty(2, (1 << 30) - 1, dtype=torch.uint8, device='meta')) == (2, (1 << 30) - 1)
    for bad in (3, 0, 6, 8.0, True, '8', None):
        with pytest.raises(ValueError, match='connectivity'):
            O.check_cc_args(m, bad)
    for bad in (-1, 256, 1.0, True):
        with pytest.raises(ValueError, match='fg_value'):
            O.check_cc_args(m, 8, bad)
        with pytest.raises(ValueError, match='exclude_value'):
            O.check_cc_args(m, 8, 1, m, bad)
    with pytest.raises(ValueError, match='exclude_value'):
        O.check_cc_args(m, 8, 1, m, None)
    for bad in (torch.zeros(5, 6, dtype=torch.uint8), torch.zeros(5, 7, dtype=torch.int32)):
        with pytest.raises(ValueError, match='exclude'):
            O.check_cc_args(m, 8, 1, bad, 0)
    for bad in (0, -3, 2.0, True, None):
        with pytest.raises(ValueError, match='min_area'):
            O.check_cc_args(m, min_area=bad)
    # the public functions validate first, then refuse host tensors: there is no CPU path
    for fn, args in ((O.label_components, (m,)), (O.remove_small_objects, (m, 2)), (O.object_scores, (m, m)),
                     (O.component_table, (torch.zeros(5, 7, dtype=torch.int32), 3))):
        with pytest.raises(RuntimeError, match='no CPU path'):
            fn(*args)
    with pytest.raises(ValueError, match='connectivity'):
        O.label_components(m, 5)
    with pytest.raises(ValueError, match='min_area'):
        O.remove_small_objects(m, 0)
    with pytest.raises(ValueError, match='min_overlap'):
        O.object_scores(m, m, min_overlap=0)
    with pytest.raises(ValueError, match='labels'):
        O.component_table(m, 3)
    import fabric_amd.utils as U
    for name in ('label_components', 'remove_small_objects', 'component_table', 'object_scores', 'check_cc_args'):
        assert getattr(U, name) is getattr(O, name)
    import inspect
    from fabric_amd.utils.inference import predict_scene_blended
    sig = inspect.signature(predict_scene_blended).parameters
    assert sig['min_area'].default is None and sig['connectivity'].default == 8


def test_cli_object_flag_checks():
    from fabric_amd.train import check_object_flags
    assert check_object_flags(0, False, 8, 0) is None and check_object_flags(0, True, 4, 16) is None
    assert check_object_flags(5, False, 8, 64) == 5 and check_object_flags(1, True, 8, 64) == 1
    for args in ((5, False, 8, 0), (0, True, 8, 0), (2, True, 4, -1)):
        with pytest.raises(ValueError, match='--scene_stride N > 0'):
            check_object_flags(*args)
    with pytest.raises(ValueError, match='scene_min_area'):
        check_object_flags(-1, False, 8, 16)
    for c in (0, 3, 6):
        with pytest.raises(ValueError, match='scene_connectivity'):
            check_object_flags(0, False, c, 16)
    for flags in (['--scene_min_area', '4'], ['--scene_objects', 'true']):
        r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1'] + flags,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and '--scene_stride N > 0' in r.stderr, r.stderr[-500:]


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


@pytest.mark.parametrize('name,res,n_args', [('bdn_cc_workspace_bytes', 'size_t', 2), ('bdn_cc_tile', 'int', 0), ('bdn_cc_label', 'int', 12),
                                             ('bdn_cc_compact', 'int', 7), ('bdn_cc_filter', 'int', 8), ('bdn_cc_stats', 'int', 9)])
def test_cc_entry_points_are_declared_and_exported(name, res, n_args):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\b' + res + r'\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',') if p.strip() != 'void']
    rt, args = _lib.SIGNATURES[name]
    assert rt is (ctypes.c_size_t if res == 'size_t' else ctypes.c_int) and len(args) == len(params) == n_args
    for p, a in zip(params, args):
        assert a is _ctype(p), (p, a)
    if n_args > 2:
        assert params[-1] == 'void* stream'
    sec = hdr[hdr.index('connected components of a scene mask'):hdr.index('size_t bdn_cc_workspace_bytes(')]
    for cite in ('scipy.ndimage.label + np.bincount', 'device-to-host copy', 'train.py:199', 'do not depend on arrival order'):
        assert cite in sec
    assert getattr(_lib.load(), name)
    assert 'cc.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()


def _call(name, defaults, over):
    lib = _lib.load()
    a = dict(defaults)
    a.update(over)
    rc = getattr(lib, name)(*a.values())
    return rc, lib.bdn_last_error().decode()


_LABEL = dict(src=64, fg_value=1, exclude=None, exclude_value=0, connectivity=8, H=4, W=4, labels=64, area=64, counts=64, workspace=64, stream=None)
_COMPACT = dict(labels=64, H=4, W=4, compact=128, counts=None, workspace=64, stream=None)
_FILTER = dict(src_mask=64, labels=64, area=64, min_area=2, out_mask=64, H=4, W=4, stream=None)
_STATS = dict(compact=64, n_max=4, other=None, other_value=1, other_exclude_value=-1, H=4, W=4, table=64, stream=None)
_BAD_SHAPES = (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(H=1, W=(1 << 31) - 1), dict(H=46341, W=46341))


def test_workspace_bytes_and_tile():
    lib = _lib.load()
    T = lib.bdn_cc_tile()
    assert T >= 8 and T & (T - 1) == 0
    for h, w in ((1, 1), (7, 13), (517, 1030), (2, (1 << 30) - 1)):
        n = lib.bdn_cc_workspace_bytes(h, w)
        assert n >= 4 * h * w and n % 16 == 0, (h, w, n)
    for over in _BAD_SHAPES:
        assert lib.bdn_cc_workspace_bytes(over.get('H', 4), over.get('W', 4)) == 0, over


def test_cc_label_argument_errors_return_before_touching_a_device():
    for v in (3, 0, -8, 16):
        rc, msg = _call('bdn_cc_label', _LABEL, dict(connectivity=v))
        assert rc == -1 and 'connectivity' in msg, (v, rc, msg)
    for over in _BAD_SHAPES:
        rc, msg = _call('bdn_cc_label', _LABEL, over)
        assert rc == -1 and '2^31 - 2' in msg, (over, rc, msg)
    for k in ('src', 'labels', 'counts', 'workspace'):
        rc, msg = _call('bdn_cc_label', _LABEL, {k: None})
        assert rc == -1 and 'null' in msg, (k, rc, msg)
    for v in (-1, 256, 1000):
        rc, msg = _call('bdn_cc_label', _LABEL, dict(fg_value=v))
        assert rc == -1 and 'fg_value' in msg, (v, rc, msg)
        rc, msg = _call('bdn_cc_label', _LABEL, dict(exclude=64, exclude_value=v))
        assert rc == -1 and 'exclude_value' in msg, (v, rc, msg)
    for over in (dict(labels=66), dict(area=65), dict(counts=70), dict(workspace=72)):
        rc, msg = _call('bdn_cc_label', _LABEL, over)
        assert rc == -1 and 'aligned' in msg, (over, rc, msg)


def test_cc_compact_argument_errors_return_before_touching_a_device():
    for over in _BAD_SHAPES:
        rc, msg = _call('bdn_cc_compact', _COMPACT, over)
        assert rc == -1 and '2^31 - 2' in msg, (over, rc, msg)
    for k in ('labels', 'compact', 'workspace'):
        rc, msg = _call('bdn_cc_compact', _COMPACT, {k: None})
        assert rc == -1 and 'null' in msg, (k, rc, msg)
    for over in (dict(labels=66), dict(compact=130), dict(counts=70), dict(workspace=72)):
        rc, msg = _call('bdn_cc_compact', _COMPACT, over)
        assert rc == -1 and 'aligned' in msg, (over, rc, msg)
    rc, msg = _call('bdn_cc_compact', _COMPACT, dict(compact=64))
    assert rc == -1 and 'alias' in msg


def test_cc_filter_argument_errors_return_before_touching_a_device():
    for over in _BAD_SHAPES:
        rc, msg = _call('bdn_cc_filter', _FILTER, over)
        assert rc == -1 and '2^31 - 2' in msg, (over, rc, msg)
    for k in ('labels', 'area', 'out_mask'):
        rc, msg = _call('bdn_cc_filter', _FILTER, {k: None})
        assert rc == -1 and 'null' in msg, (k, rc, msg)
    for over in (dict(labels=66), dict(area=65)):
        rc, msg = _call('bdn_cc_filter', _FILTER, over)
        assert rc == -1 and 'aligned' in msg, (over, rc, msg)


def test_cc_stats_argument_errors_return_before_touching_a_device():
    for over in _BAD_SHAPES:
        rc, msg = _call('bdn_cc_stats', _STATS, over)
        assert rc == -1 and '2^31 - 2' in msg, (over, rc, msg)
    for k in ('compact', 'table'):
        rc, msg = _call('bdn_cc_stats', _STATS, {k: None})
        assert rc == -1 and 'null' in msg, (k, rc, msg)
    for v in (0, -1, 1 << 28):
        rc, msg = _call('bdn_cc_stats', _STATS, dict(n_max=v))
        assert rc == -1 and 'n_max' in msg, (v, rc, msg)
    for v in (-1, 256):
        rc, msg = _call('bdn_cc_stats', _STATS, dict(other=64, other_value=v))
        assert rc == -1 and 'other_value' in msg, (v, rc, msg)
    for v in (-2, 256):
        rc, msg = _call('bdn_cc_stats', _STATS, dict(other=64, other_exclude_value=v))
        assert rc == -1 and 'other_exclude_value' in msg, (v, rc, msg)
    for over in (dict(compact=66), dict(table=65)):
        rc, msg = _call('bdn_cc_stats', _STATS, over)
        assert rc == -1 and 'aligned' in msg, (over, rc, msg)
