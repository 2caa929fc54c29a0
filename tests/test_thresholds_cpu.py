"""CPU tests of the label-free thresholds: the declarations of the three new entries against _lib.SIGNATURES and every argument check of
theirs (fake non-null pointers: each returns BDN_E_ARG before anything touches a device), the Python-side refusals on meta tensors, and
the numpy restatement tests/thresholds_ref.py on analytic histograms (counts = rint(n (cdf(edge[i+1]) - cdf(edge[i]))), no sampling) and
on the degenerate ones."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import mad as MAD
from fabric_amd.utils import thresholds as T
from tests import thresholds_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BDN_E_ARG = -1
_NAN, _INF = float('nan'), float('inf')


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


@pytest.mark.parametrize('name,n_args', [('bdn_raster_hist', 8), ('bdn_hist_threshold', 10), ('bdn_raster_mask', 9)])
def test_entry_points_are_declared_and_exported(name, n_args):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    rt, args = _lib.SIGNATURES[name]
    assert rt is ctypes.c_int and len(args) == len(params) == n_args
    for p, a in zip(params, args):
        assert a is _ctype(p), (p, a)
    assert params[-1] == 'void* stream'
    sec = hdr[hdr.index('thresholds without labels'):hdr.index('int bdn_raster_hist(')]
    for cite in ('train.py:199', 'searchsorted', 'Kittler', 'Rosin', 'Bruzzone', name):
        assert cite in sec
    assert getattr(_lib.load(), name)
    assert 'thresh.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()


def test_header_columns_match_the_python_names():
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    for i, k in enumerate(R.COLS):
        assert re.search(r'#define BDN_THR_COL_' + k + r' ' + str(i) + r'\b', hdr), k
        assert T.COLUMNS[i] == k.lower()
    assert re.search(r'#define BDN_THR_COLS 16\b', hdr)
    for i, k in enumerate(T.METHODS):
        assert re.search(r'#define BDN_THR_' + k.upper() + r' ' + str(1 << i) + r'\b', hdr), k
        assert T.check_methods(k) == 1 << i == getattr(R, k.upper())
    assert T.check_methods(T.METHODS) == 15 and T.check_methods(['rosin', 'otsu']) == 5


_HIST = dict(raster=64, exclude=None, exclude_value=0, edges=128, n_bins=16, hist=256, HW=16, stream=None)
_SELECT = dict(hist=64, coord=128, edges=256, n_bins=16, methods=15, em_iters=100, em_tol=1e-9, table=512, thr=1024, stream=None)
_MASK = dict(raster=64, exclude=None, exclude_value=0, thr=128, below=0, excluded_out=0, mask=256, HW=16, stream=None)


@pytest.mark.parametrize('name,defaults,bad', [
    ('bdn_raster_hist', _HIST, (dict(raster=None), dict(edges=None), dict(hist=None), dict(raster=66), dict(edges=130), dict(hist=260),
                                dict(exclude_value=-1), dict(exclude_value=256), dict(n_bins=1), dict(n_bins=0), dict(n_bins=4097),
                                dict(HW=0), dict(HW=-4), dict(HW=(1 << 40) + 1))),
    ('bdn_hist_threshold', _SELECT, (dict(hist=None), dict(coord=None), dict(edges=None), dict(table=None), dict(thr=None), dict(hist=68),
                                     dict(coord=132), dict(table=516), dict(edges=258), dict(thr=1026), dict(n_bins=1), dict(n_bins=4097),
                                     dict(methods=0), dict(methods=16), dict(methods=-1), dict(em_iters=0), dict(em_iters=1001),
                                     dict(em_tol=-1e-9), dict(em_tol=_NAN), dict(em_tol=_INF))),
    ('bdn_raster_mask', _MASK, (dict(raster=None), dict(thr=None), dict(mask=None), dict(raster=66), dict(thr=130), dict(exclude_value=-1),
                                dict(exclude_value=256), dict(excluded_out=-1), dict(excluded_out=256), dict(below=2), dict(below=-1),
                                dict(HW=0), dict(HW=(1 << 40) + 1))),
])
def test_c_entries_refuse_bad_arguments_before_any_launch(name, defaults, bad):
    lib = _lib.load()
    for over in bad:
        a = dict(defaults)
        a.update(over)
        rc = getattr(lib, name)(*a.values())
        assert rc == BDN_E_ARG, (name, over, rc, lib.bdn_last_error().decode())


# ---------------------------------------------------------------- the Python-side refusals
def _meta(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_bin_edges_on_the_host():
    for spacing, lo, hi in (('linear', -6, 10), ('sqrt', 0.0, 400.0), ('sqrt', 0.5, 3.0), ('log', 1e-3, 50.0)):
        for n in (2, 64, 1000, 4096):
            edges, coord = T.bin_edges(lo, hi, n, spacing)
            want_e, want_c = R.bin_edges(lo, hi, n, spacing)
            assert edges.dtype == torch.float32 and coord.dtype == torch.float64 and edges.shape == (n + 1,) and coord.shape == (n,)
            e = edges.numpy()
            assert e[0] == np.float32(lo) and e[-1] == np.float32(hi) and (np.diff(e) >= 0).all() and (np.diff(coord.numpy()) > 0).all()
            # torch and numpy may round u_i = a + (b - a) i / n differently in the last bit (a fused multiply-add), and exp as well
            assert np.allclose(coord.numpy(), want_c, rtol=1e-15, atol=1e-15 * max(abs(want_c[0]), abs(want_c[-1])))
            if spacing == 'log':
                assert np.allclose(e, want_e, rtol=2e-7, atol=0)
            else:
                assert np.array_equal(e, want_e)
    e, c = T.bin_edges(-6, 10, 1024)
    assert e[512].item() == 2.0 and c[0].item() == -6 + 0.0078125
    for lo, hi, spacing in ((1.0, 1.0, 'linear'), (2.0, 1.0, 'linear'), (_NAN, 1.0, 'linear'), (0.0, _INF, 'linear'), (-_INF, 0.0, 'linear'),
                            (0.0, 1.0, 'log'), (-1.0, 1.0, 'log'), (-0.5, 1.0, 'sqrt')):
        with pytest.raises(ValueError, match='lo'):
            T.bin_edges(lo, hi, 16, spacing)
    for n in (1, 0, 4097, 16.0, True):
        with pytest.raises(ValueError, match='n_bins'):
            T.bin_edges(0.0, 1.0, n)
    with pytest.raises(ValueError, match='spacing'):
        T.bin_edges(0.0, 1.0, 16, 'cubic')
    with pytest.raises(ValueError, match='both'):
        T.bin_edges(0.0, torch.tensor(1.0), 16)
    e, c = T.bin_edges(_meta(), _meta(), 16, 'sqrt')              # 0-d tensors: built where they live, nothing is read
    assert e.device.type == 'meta' and e.shape == (17,) and c.shape == (16,) and c.dtype == torch.float64


def test_histogram_and_table_checks_on_meta_tensors():
    e, c = _meta(17), _meta(16, dtype=torch.float64)
    h = T.RasterHistogram(e, c)
    assert h.n_bins == 16 and h.counts.shape == (19,) and h.counts.dtype == torch.int64
    for bad_e, bad_c in ((_meta(17, dtype=torch.float64), c), (_meta(2), _meta(1, dtype=torch.float64)), (_meta(4098), _meta(4097, dtype=torch.float64)),
                         (_meta(17, 1), c), ('x', c)):
        with pytest.raises(ValueError, match='edges'):
            T.RasterHistogram(bad_e, bad_c)
    for bad_c in (_meta(16), _meta(15, dtype=torch.float64), None, torch.zeros(16, dtype=torch.float64)):
        with pytest.raises(ValueError, match='coord'):
            T.RasterHistogram(e, bad_c)
    r = _meta(5, 7)
    assert T.check_raster_args(r) == 35 and T.check_raster_args(r, _meta(5, 7, dtype=torch.uint8), 3, _meta(5, 7, dtype=torch.uint8), 255) == 35
    for bad in (_meta(5, 7, dtype=torch.float64), _meta(0), _meta(7, 5).t(), 'x'):
        with pytest.raises(ValueError, match='raster'):
            h.update(bad)
    for ex, v in ((_meta(5, 6, dtype=torch.uint8), 1), (_meta(5, 7), 1), (torch.zeros(5, 7, dtype=torch.uint8), 1), (None, 1)):
        with pytest.raises(ValueError, match='exclude'):
            h.update(r, ex, v)
    for v in (None, -1, 256, 1.0, True):
        with pytest.raises(ValueError, match='exclude_value'):
            h.update(r, _meta(5, 7, dtype=torch.uint8), v)
    for methods in ((), 'median', ('otsu', 'x'), None, 3):
        with pytest.raises(ValueError, match='method'):
            h.select(methods)
    for it in (0, 1001, 10.0, True):
        with pytest.raises(ValueError, match='em_iters'):
            h.select('em', em_iters=it)
    for tol in (-1e-9, _NAN, _INF, 'x', True):
        with pytest.raises(ValueError, match='em_tol'):
            h.select('em', em_tol=tol)
    with pytest.raises(ValueError, match='n_bins'):
        h.merge(T.RasterHistogram(_meta(9), _meta(8, dtype=torch.float64)))
    t = T.ThresholdTable(_meta(4), _meta(4, 16, dtype=torch.float64), e, c)
    with pytest.raises(ValueError, match='method'):
        t.mask(r, 'median')
    with pytest.raises(ValueError, match='below'):
        t.mask(r, 'otsu', below=1)
    for out in (_meta(5, 6, dtype=torch.uint8), _meta(5, 7), torch.zeros(5, 7, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='out'):
            t.mask(r, 'otsu', out=out)
    for v in (-1, 256, 1.0, True):
        with pytest.raises(ValueError, match='excluded_out'):
            t.mask(r, 'otsu', excluded_out=v)
    both = torch.zeros(64, dtype=torch.uint8)                     # out on the raster's own storage
    with pytest.raises(ValueError, match='share memory'):
        T.check_raster_args(both[:32].view(torch.float32), None, None, both[32:40])


def test_public_functions_validate_then_refuse_host_tensors():
    r = torch.zeros(5, 7)
    e, c = T.bin_edges(0.0, 1.0, 16)
    h = T.RasterHistogram(e, c)
    for fn in (lambda: h.update(r), lambda: h.select(), lambda: T.auto_threshold(r), lambda: T.auto_threshold(r, lo=0.0, hi=1.0),
               lambda: T.ThresholdTable(torch.zeros(4), torch.zeros(4, 16, dtype=torch.float64), e, c).mask(r, 'otsu')):
        with pytest.raises(RuntimeError, match='no CPU path'):
            fn()
    with pytest.raises(ValueError, match='method'):
        T.auto_threshold(r, 'median')
    with pytest.raises(ValueError, match='lo'):
        T.auto_threshold(r, lo=1.0, hi=0.0)
    with pytest.raises(ValueError, match='lo'):
        T.auto_threshold(r, lo='a')
    with pytest.raises(ValueError, match='spacing'):
        T.auto_threshold(r, spacing='x')
    import fabric_amd.utils as U
    for name in ('RasterHistogram', 'ThresholdTable', 'auto_threshold', 'bin_edges', 'auto_change_mask'):
        assert hasattr(U, name)


def test_auto_change_mask_checks():
    chi2, proba = _meta(5, 7), _meta(2, 5, 7)
    res = MAD.MadResult(chi2, proba, None, None, None, None, None, [0], None, 0)
    assert MAD.check_auto_mask_args(res) is chi2
    assert tuple(MAD.check_auto_mask_args(res, 'em', 'proba', 64, 'linear').shape) == (5, 7)
    sig = inspect.signature(MAD.auto_change_mask).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [('method', 'rosin'), ('on', 'chi2'), ('n_bins', 1024), ('spacing', 'sqrt'),
                                                            ('chi2_max', None), ('excluded_out', 0), ('out', None)]
    with pytest.raises(ValueError, match='MadResult'):
        MAD.auto_change_mask('x')
    for kw, match in ((dict(method='x'), 'method'), (dict(on='rho'), 'on must'), (dict(n_bins=1), 'n_bins'), (dict(spacing='log'), 'log'),
                      (dict(chi2_max=0.0), 'chi2_max'), (dict(chi2_max=_NAN), 'chi2_max'), (dict(on='proba', chi2_max=5.0), 'chi2_max'),
                      (dict(excluded_out=256), 'excluded_out'), (dict(out=_meta(5, 6, dtype=torch.uint8)), 'out')):
        with pytest.raises(ValueError, match=match):
            MAD.auto_change_mask(res, **kw)


def test_predict_scene_blended_auto_threshold_arguments():
    from fabric_amd.utils.inference import check_auto_threshold_args, predict_scene_blended
    sig = inspect.signature(predict_scene_blended).parameters
    assert sig['auto_threshold'].default is None and sig['threshold_out'].default is None
    assert check_auto_threshold_args() is None and check_auto_threshold_args('otsu', {}) is None
    with pytest.raises(ValueError, match='method'):
        check_auto_threshold_args('median')
    with pytest.raises(ValueError, match='by value'):
        check_auto_threshold_args('otsu', None, 0.5)
    with pytest.raises(ValueError, match='by value'):
        check_auto_threshold_args('otsu', None, None, 0.2)
    with pytest.raises(ValueError, match='threshold_out'):
        check_auto_threshold_args('otsu', [])
    with pytest.raises(ValueError, match='threshold_out'):
        check_auto_threshold_args(None, {})


def test_cli_flag_checks(tmp_path):
    import json
    from fabric_amd.train import check_auto_threshold_flags, checkpoint_entry
    assert check_auto_threshold_flags(None, None, None, 'argmax', 0) == (None, None)
    assert check_auto_threshold_flags(None, None, None, 0.5, 32) == (None, None)
    assert check_auto_threshold_flags('otsu', None, None, 'argmax', 32) == ('otsu', None)
    assert check_auto_threshold_flags(None, 'rosin', None, 'argmax', 32) == (None, {'method': 'rosin', 'iters': 30})
    assert check_auto_threshold_flags('em', 'kittler', 7, 'argmax', 32) == ('em', {'method': 'kittler', 'iters': 7})
    assert check_auto_threshold_flags(None, 'rosin', None, 'val', 32) == (None, {'method': 'rosin', 'iters': 30})      # the baseline has its own threshold
    for args, match in ((('median', None, None, 'argmax', 32), 'one of'), (('otsu', None, None, 0.5, 32), 'leave --scene_threshold at argmax'),
                        (('otsu', None, None, 'val', 32), 'leave --scene_threshold at argmax'), (('otsu', None, None, 'argmax', 0), '--scene_stride N > 0'),
                        ((None, 'mean', None, 'argmax', 32), 'one of'), ((None, 'rosin', None, 'argmax', 0), '--scene_stride N > 0'),
                        ((None, None, 5, 'argmax', 32), 'add --scene_mad_baseline'), ((None, 'rosin', 0, 'argmax', 32), '1..1000'),
                        ((None, 'rosin', 1001, 'argmax', 32), '1..1000')):
        with pytest.raises(ValueError, match=match):
            check_auto_threshold_flags(*args)
    # --resume: the checkpoint's settings come back unless the flag is given again
    kept = {'scene_auto_threshold': 'kittler', 'scene_mad_baseline': {'method': 'em', 'iters': 12}}
    assert check_auto_threshold_flags(None, None, None, 'argmax', 32, kept) == ('kittler', {'method': 'em', 'iters': 12})
    assert check_auto_threshold_flags('otsu', 'rosin', None, 'argmax', 32, kept) == ('otsu', {'method': 'rosin', 'iters': 12})
    assert check_auto_threshold_flags(None, None, 3, 'argmax', 32, kept)[1] == {'method': 'em', 'iters': 3}
    assert check_auto_threshold_flags(None, None, None, 'argmax', 32, {'scene_auto_threshold': None, 'scene_mad_baseline': None}) == (None, None)
    with pytest.raises(ValueError, match='leave --scene_threshold at argmax'):
        check_auto_threshold_flags(None, None, None, 0.4, 32, kept)
    (tmp_path / 'metadata_epoch_3.json').write_text(json.dumps(kept))
    ck = str(tmp_path / 'checkpoint_epoch_3.state_dict.pt')
    assert checkpoint_entry(ck, 'scene_auto_threshold') == 'kittler' and checkpoint_entry(ck, 'scene_mad_baseline') == kept['scene_mad_baseline']
    assert checkpoint_entry(ck, 'absent') is None and checkpoint_entry(str(tmp_path / 'checkpoint_epoch_4.state_dict.pt'), 'x') is None
    src = open(os.path.join(ROOT, 'fabric_amd', 'train.py')).read()
    for flag in ('--scene_auto_threshold', '--scene_mad_baseline', '--scene_mad_iters'):
        m = re.search(r"add_argument\('" + flag + r"', type=(\w+), default=(\w+)", src)
        assert m and m.group(2) == 'None', flag
    for key in ("run_meta['scene_auto_threshold']", "run_meta['scene_mad_baseline']"):
        assert key in src


# ---------------------------------------------------------------- the restatement on analytic histograms
N_BINS, LO, HI, N_PIX = 1024, -6, 10, 1e7
WIDTH = (HI - LO) / N_BINS


def _mixture_hist(parts, edges):
    return R.mixture_hist(parts, edges, N_PIX)


def _select(hist, edges, coord, **kw):
    return R.read_table(*R.hist_threshold(hist, coord, edges, **kw))


def _count_identity(hist, res, n_bins):
    """The number of values >= edges[t] is sum(c[t:]) + above: what the table's N1 says, for every method that found a split."""
    for m, d in res.items():
        if d['ok']:
            c = hist[:n_bins].astype(np.int64)
            assert d['n1'] == c[d['bin']:].sum() and d['n0'] == c[:d['bin']].sum() and d['n0'] + d['n1'] == d['n'] == c.sum(), m
            assert d['below'] == hist[n_bins] and d['above'] == hist[n_bins + 1]
            assert 1 <= d['bin'] <= n_bins - 1


def test_equal_gaussians_split_in_the_middle():
    edges, coord = R.bin_edges(LO, HI, N_BINS)
    hist = _mixture_hist([(0.5, 0.0), (0.5, 4.0)], edges)
    res = _select(hist, edges, coord)
    for m in ('otsu', 'kittler', 'em'):
        assert res[m]['ok'] and res[m]['bin'] == 512 and res[m]['thr'] == 2.0 == res[m]['value'], (m, res[m])
    assert res['rosin']['ok'] and 2.0 - 0.25 < res['rosin']['thr'] < 2.0                   # the corner of the right mode's left flank
    em = res['em']
    assert abs(em['mean0']) < 1e-3 and abs(em['mean1'] - 4) < 1e-3 and abs(em['sd0'] - 1) < 1e-3 and abs(em['sd1'] - 1) < 1e-3
    assert abs(em['w1'] - 0.5) < 1e-6 and 2 <= em['iters'] <= 100 and em['loglik'] == em['crit'] < 0
    _count_identity(hist, res, N_BINS)


def test_unequal_gaussians_against_the_bayes_threshold():
    edges, coord = R.bin_edges(LO, HI, N_BINS)
    hist = _mixture_hist([(0.9, 0.0), (0.1, 6.0)], edges)
    res = _select(hist, edges, coord)
    bayes = 3.0 + math.log(9.0) / 6.0
    assert res['kittler']['thr'] == 3.375 and abs(res['kittler']['thr'] - bayes) < WIDTH
    assert res['em']['ok'] and abs(res['em']['thr'] - bayes) < WIDTH, res['em']
    assert res['otsu']['thr'] == 2.984375 and res['rosin']['thr'] == 2.53125          # the restatement's values, pinned not judged
    em = res['em']
    assert abs(em['mean1'] - 6) < 1e-3 and abs(em['w1'] - 0.1) < 1e-4 and abs(em['sd0'] - 1) < 1e-3
    _count_identity(hist, res, N_BINS)
    only = _select(hist, edges, coord, methods=R.ROSIN)
    assert only['rosin'] == res['rosin'] and not only['otsu']['ok'] and math.isnan(only['otsu']['thr']) and only['otsu']['n'] == 0


def test_first_split_of_a_plateau():
    """Empty bins between the modes: every split inside the gap has the same two classes, so the criteria are flat there; 'first' is
    the gap's left end, the bin after the last occupied bin of the low mode."""
    edges, coord = R.bin_edges(0.0, 64.0, 64)
    hist = np.zeros(67, np.uint64)
    hist[[3, 4, 5]] = (100, 300, 100)
    hist[[40, 41, 42]] = (10, 30, 10)
    res = _select(hist, edges, coord)
    otsu, kit = R.criteria(hist, coord)
    assert len({otsu[t] for t in range(6, 41)}) == 1 and len({kit[t] for t in range(6, 41)}) == 1
    assert res['otsu']['bin'] == 6 and res['kittler']['bin'] == 6 and res['otsu']['thr'] == 6.0
    assert res['rosin']['ok'] and res['rosin']['bin'] == 6          # the first bin of the empty stretch is the farthest from the chord
    _count_identity(hist, res, 64)


def test_mask_count_is_the_histogram_tail():
    r = np.random.default_rng(11)
    chi2 = r.chisquare(4, 20000).astype(np.float32)
    chi2[:600] += r.uniform(30, 80, 600).astype(np.float32)          # a changed tail
    chi2[1000:1010] = (np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e4, 2e4, np.nan, 5e3)
    exclude = (r.random(20000) < 0.1).astype(np.uint8)
    for spacing, lo, hi in (('sqrt', 0.0, 60.0), ('linear', 0.0, 60.0), ('log', 0.05, 60.0)):
        edges, coord = R.bin_edges(lo, hi, 256, spacing)
        hist = R.raster_hist(chi2, edges, exclude, 1)
        assert hist.sum() == chi2.size and hist[258] == (exclude == 1).sum() + (~np.isfinite(chi2) & (exclude != 1)).sum()
        assert hist[257] > 0 and (spacing != 'log' or hist[256] > 0)
        res = _select(hist, edges, coord)
        _count_identity(hist, res, 256)
        assert any(d['ok'] for d in res.values())
        for m, d in res.items():
            mask = R.raster_mask(chi2, d['thr'], False, exclude, 1, 0)
            below = R.raster_mask(chi2, d['thr'], True, exclude, 1, 7)
            if d['ok']:
                assert mask.sum() == d['n1'] + d['above'], (spacing, m)
                assert (below == 1).sum() == d['n0'] + d['below'] and (below == 7).sum() == (exclude == 1).sum()
            else:
                assert mask.sum() == 0 and (below == 1).sum() == 0


def test_raster_hist_definition():
    edges = np.array([0.0, 1.0, 1.0, 2.0, 4.0], np.float32)          # a duplicate edge: bin 1 is empty by construction
    v = np.array([-1e-45, -0.0, 0.0, 1e-45, 0.999, 1.0, 1.5, 2.0, 3.9999, 4.0, np.nextafter(np.float32(4), np.float32(5)), np.nan, np.inf, -np.inf],
                 np.float32)
    h = R.raster_hist(v, edges)
    assert h.tolist() == [4, 0, 2, 3, 1, 1, 3]
    h2 = R.raster_hist(v, edges, np.arange(14) % 2, 1, hist=h)
    assert h2.sum() == 28 and h2[6] == 3 + 7 + 1                     # the odd positions, and the NaN at an even one
    m = R.raster_mask(v, 1.0)
    assert m.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    assert R.raster_mask(v, 1.0, True).tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert R.raster_mask(v, np.nan).sum() == 0 and R.raster_mask(v, np.nan, True).sum() == 0


# ---------------------------------------------------------------- degenerate histograms
def _failed(d):
    return not d['ok'] and math.isnan(d['thr']) and all(d[k] == 0 for k in T.COLUMNS[1:])


def test_degenerate_histograms():
    edges, coord = R.bin_edges(0.0, 8.0, 8)
    constant = R.raster_hist(np.full(50, 3.25, np.float32), edges)
    assert constant[3] == 50
    excluded = R.raster_hist(np.arange(8, dtype=np.float32), edges, np.ones(8, np.uint8), 1)
    assert excluded[:10].sum() == 0 and excluded[10] == 8
    for hist in (constant, excluded, np.zeros(11, np.uint64)):
        assert all(_failed(d) for d in _select(hist, edges, coord).values())
    two = np.zeros(11, np.uint64)
    two[[2, 5]] = (40, 10)
    res = _select(two, edges, coord)
    assert res['otsu']['ok'] and res['otsu']['bin'] == 3 and (res['otsu']['n0'], res['otsu']['n1']) == (40, 10)
    assert res['otsu']['mean0'] == 2.5 and res['otsu']['mean1'] == 5.5 and res['otsu']['sd0'] == 0 and res['otsu']['sd1'] == 0
    assert _failed(res['kittler'])                                   # single-bin classes have no variance
    assert res['rosin']['ok'] and res['rosin']['bin'] == 3           # p = 2, e = 5: the first of the empty bins between them
    assert res['em']['ok'] and 3 <= res['em']['bin'] <= 5 and res['em']['mean0'] == 2.5 and res['em']['mean1'] == 5.5
    assert res['em']['sd0'] == res['em']['sd1'] == math.sqrt(1 / 12)          # the variance floor of unit spacing
    e2, c2 = R.bin_edges(0.0, 2.0, 2)
    h2 = np.array([30, 10, 0, 0, 0], np.uint64)
    res = _select(h2, e2, c2)
    assert res['otsu']['ok'] and res['otsu']['bin'] == 1 and res['otsu']['thr'] == 1.0 and _failed(res['rosin']) and _failed(res['kittler'])
    peak_last = np.zeros(11, np.uint64)
    peak_last[[1, 2, 7]] = (5, 6, 50)
    res = _select(peak_last, edges, coord)
    assert _failed(res['rosin']) and res['otsu']['ok']
    adjacent = np.zeros(11, np.uint64)
    adjacent[[4, 5]] = (9, 3)                                        # e = p + 1: nothing strictly between them
    assert _failed(_select(adjacent, edges, coord)['rosin'])
    big = np.zeros(11, np.uint64)
    big[[1, 3, 6]] = (1 << 49, 5, 1)
    res = _select(big, edges, coord)
    assert _failed(res['rosin']) and res['otsu']['ok']               # a total at or above 2^49
