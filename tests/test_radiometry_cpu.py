"""-m "not gpu": what the radiometric matching pins without a device -- the declarations of the new entries against _lib.SIGNATURES, every
argument check of every new C entry (fake non-null pointers: BDN_E_ARG before anything touches a device), the workspace condition, the
argument checks of fabric_amd.utils.radiometry on meta tensors, the CLI flag checks, synthetic_onera(radiometry=), and the properties of
the numpy twin the GPU tests compare bits against (tests/radiometry_ref.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import radiometry as RM
from fabric_amd.utils.dataloaders import synthetic_onera
from tests import radiometry_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
P = 0x1000                                                  # a fake non-null, 16-byte aligned pointer: never dereferenced


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


ENTRIES = [('bdn_band_quantiles_workspace_bytes', 'size_t', 4), ('bdn_band_quantiles', 'int', 16), ('bdn_transfer_apply', 'int', 13),
           ('bdn_stretch_u8', 'int', 8)]


@pytest.mark.parametrize('name,res,n_args', ENTRIES)
def test_entry_points_are_declared_and_exported(name, res, n_args):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\b' + res + r'\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    rt, args = _lib.SIGNATURES[name]
    assert rt is (ctypes.c_size_t if res == 'size_t' else ctypes.c_int) and len(args) == len(params) == n_args
    for p, a in zip(params, args):
        assert a is _ctype(p), (p, a)
    if res == 'int':
        assert params[-1] == 'void* stream'
    assert getattr(_lib.load(), name)
    assert 'radiometry.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()
    sec = hdr[hdr.index('radiometric matching of the two dates'):hdr.index('size_t bdn_band_quantiles_workspace_bytes(')]
    for cite in ('h = p * (n - 1)', 'hi = min(lo + 1, n - 1)', 'value[b][q] = a + ((b - a) * t)', 'no float\n * atomics', 'it does not grow with H W',
                 'BDN_E_ARG\n * before anything touches a device', 'k = the last index with s_k <= x', 'A NaN (a NaN pixel', 'at most 128 MiB'):
        assert cite in sec, cite
    assert '#define BDN_EXTRAPOLATE_OFFSET 0' in hdr and '#define BDN_EXTRAPOLATE_SLOPE 1' in hdr and RM.EXTRAPOLATE == {'offset': 0, 'slope': 1}


def _rc(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.bdn_last_error().decode()


def _bad(name, good, i, v, msg):
    a = list(good)
    a[i] = v
    rc, err = _rc(name, *a)
    assert rc == E_ARG and msg in err, (name, i, v, rc, err)


def test_band_quantiles_argument_checks():
    #       scene bands n_b excl exv pos probs n_q value order count ws C  H   W   stream
    good = [P, P, 3, None, 0, 0, P, 5, P, P, P, P, 3, 33, 65, None]
    for i in (0, 1, 6, 8, 9, 10, 11):
        _bad('bdn_band_quantiles', good, i, None, 'null pointer')
    for i, v, msg in ((2, 0, 'band indices'), (2, 65, 'band indices'), (7, 0, 'probabilities'), (7, 1025, 'probabilities'), (7, -1, 'probabilities'),
                      (12, 0, 'bad scene'), (12, 65536, 'bad scene'), (13, 0, 'bad scene'), (14, -5, 'bad scene'), (13, 32768, 'bad scene'),
                      (14, 32768, 'bad scene'), (5, 2, 'positive_only'), (5, -1, 'positive_only'), (0, P + 2, 'aligned'), (1, P + 1, 'aligned'),
                      (6, P + 4, 'aligned'), (8, P + 4, 'aligned'), (9, P + 2, 'aligned'), (10, P + 4, 'aligned'), (11, P + 8, 'aligned')):
        _bad('bdn_band_quantiles', good, i, v, msg)
    a = list(good); a[3], a[4] = P, 256
    rc, err = _rc('bdn_band_quantiles', *a)
    assert rc == E_ARG and 'exclude_value' in err
    a[4] = -1
    assert _rc('bdn_band_quantiles', *a)[0] == E_ARG


def test_workspace_does_not_grow_with_the_scene():
    q = _lib.load().bdn_band_quantiles_workspace_bytes
    band = lambda nq: 16384 + nq * (24576 + 32)              # hist0 + map0, and per probability 2 slots of 12 KiB and 2 x 2 entries of 8 B
    assert q(13, 256, 10000, 10000) == q(13, 256, 500, 500) == q(13, 256, 32767, 32767) == q(13, 256, 1, 1) == 13 * band(256)
    assert q(13, 2, 10000, 10000) == 13 * band(2) < 1 << 20
    assert q(1, 1, 1, 1) == band(1) and q(2, 40, 7, 9) == 2 * q(1, 40, 7, 9)
    cap = 128 << 20
    for nb, nq in ((64, 1024), (64, 256), (13, 1024), (64, 1), (1, 1024), (21, 256), (22, 256)):
        g = max(1, min(nb, cap // band(nq)))                 # the bands of one group; the entry takes the groups one after another
        assert 0 < q(nb, nq, 500, 500) == g * band(nq) <= cap and q(nb, nq, 500, 500) % 16 == 0, (nb, nq)
    assert q(64, 1024, 9, 9) == 5 * band(1024) and q(22, 256, 9, 9) == 21 * band(256)
    for args in ((0, 8, 8, 8), (65, 8, 8, 8), (1, 0, 8, 8), (1, 1025, 8, 8), (1, 8, 0, 8), (1, 8, 8, 32768), (1, 8, 32768, 8), (1, 8, 8, -1)):
        assert q(*args) == 0, args


def test_transfer_apply_and_stretch_argument_checks():
    #       src out bands n_b s  t  K  extrapolate exact C H   W   stream
    good = [P, 2 * P, P, 3, P, P, 16, 0, None, 3, 33, 65, None]
    for i in (0, 1, 2, 4, 5):
        _bad('bdn_transfer_apply', good, i, None, 'null pointer')
    for i, v, msg in ((3, 0, 'band indices'), (3, 65, 'band indices'), (6, 1, 'knots'), (6, 1025, 'knots'), (7, 2, 'extrapolate'), (7, -1, 'extrapolate'),
                      (9, 0, 'bad scene'), (9, 65536, 'bad scene'), (10, 0, 'bad scene'), (11, 32768, 'bad scene'), (0, P + 2, 'aligned'),
                      (1, 2 * P + 1, 'aligned'), (2, P + 2, 'aligned'), (4, P + 2, 'aligned'), (5, P + 1, 'aligned')):
        _bad('bdn_transfer_apply', good, i, v, msg)
    #       src u16 cd out C H   W   stream
    good = [P, 0, P, P, 3, 33, 65, None]
    for i in (0, 2, 3):
        _bad('bdn_stretch_u8', good, i, None, 'null pointer')
    for i, v, msg in ((1, 2, 'src_is_u16'), (1, -1, 'src_is_u16'), (4, 0, 'bad scene'), (5, 0, 'bad scene'), (6, 32768, 'bad scene'), (0, P + 2, 'aligned'),
                      (2, P + 4, 'aligned')):
        _bad('bdn_stretch_u8', good, i, v, msg)
    a = list(good); a[1], a[0] = 1, P + 1                    # a uint16 source: 2-byte aligned
    rc, err = _rc('bdn_stretch_u8', *a)
    assert rc == E_ARG and 'aligned' in err


# ---------------------------------------------------------------- the Python surface without a device
def test_check_args_on_meta_tensors():
    a = torch.empty(3, 33, 65, device='meta')
    ex = torch.empty(33, 65, dtype=torch.uint8, device='meta')
    assert RM.check_quantile_args(a, [0.0, 0.5, 1.0]) == (3, 33, 65, [0, 1, 2], 3)
    assert RM.check_quantile_args(a, torch.empty(7, dtype=torch.float64, device='meta'), [2, 0], ex, 255, True) == (3, 33, 65, [2, 0], 7)
    for kw, msg in ((dict(probs=[]), 'probs'), (dict(probs=[1.5]), r'\[0, 1\]'), (dict(probs=[float('nan')]), r'\[0, 1\]'), (dict(probs=[-0.1]), r'\[0, 1\]'),
                    (dict(probs=[0.5] * 1025), 'probs'), (dict(probs='0.5'), 'probs'), (dict(probs=[[0.5]]), 'probs'),
                    (dict(probs=torch.empty(3, device='meta')), 'float64'), (dict(probs=torch.zeros(3, dtype=torch.float64)), 'probs is on'),
                    (dict(bands=[]), 'bands'), (dict(bands=[3]), 'bands'), (dict(bands=[-1]), 'bands'), (dict(bands=[1, 1]), 'twice'), (dict(bands='0'), 'bands'),
                    (dict(exclude=ex), 'exclude_value'), (dict(exclude=ex, exclude_value=256), 'exclude_value'),
                    (dict(exclude=ex.float(), exclude_value=0), 'exclude'), (dict(positive_only=1), 'positive_only'),
                    (dict(exclude=torch.empty(33, 64, dtype=torch.uint8, device='meta'), exclude_value=0), 'exclude')):
        with pytest.raises(ValueError, match=msg):
            RM.check_quantile_args(a, **dict(dict(probs=[0.5]), **kw))
    for bad in (a.double(), a[0], a.permute(0, 2, 1), torch.empty(0, 3, 3, device='meta'), np.zeros((3, 33, 65), np.float32)):
        with pytest.raises(ValueError, match='scene'):
            RM.check_quantile_args(bad, [0.5])
    with pytest.raises(ValueError, match='name a subset'):
        RM.check_quantile_args(torch.empty(65, 4, 4, device='meta'), [0.5])
    assert RM.check_fit_args(a, a) == (3, 33, 65, [0, 1, 2], 256, 0)
    assert RM.check_fit_args(a, a, [0.02, 0.98], 2, [1], ex, 9, 'slope') == (3, 33, 65, [1], 2, 1)
    for kw, msg in ((dict(knots=1), 'knots'), (dict(knots=1025), 'knots'), (dict(knots=2.0), 'knots'), (dict(probs=[0.5]), 'knots'),
                    (dict(probs=[0.9, 0.1]), 'nondecreasing'), (dict(extrapolate='clamp'), 'extrapolate'), (dict(bands=[5]), 'bands')):
        with pytest.raises(ValueError, match=msg):
            RM.check_fit_args(a, a, **kw)
    with pytest.raises(ValueError, match='d1'):
        RM.check_fit_args(a, torch.empty(3, 33, 64, device='meta'))
    with pytest.raises(ValueError, match='d1 is on'):
        RM.check_fit_args(a, torch.zeros(3, 33, 65))
    k = torch.empty(2, 16, device='meta')
    tr = RM.BandTransfer(k, k, torch.empty(2, 2, dtype=torch.int64, device='meta'), [2, 0], 'offset')
    assert RM.check_transfer_args(a, tr) == (3, 33, 65, 2, 16) and RM.check_transfer_args(a, tr, a) == (3, 33, 65, 2, 16)       # out may be d2
    for t, out, msg in ((RM.BandTransfer(k.double(), k, None, [2, 0], 'offset'), None, 'transfer.src'), (RM.BandTransfer(k, k[:1], None, [2, 0], 'offset'), None, 'transfer.dst'),
                        (RM.BandTransfer(k, k, None, [2, 3], 'offset'), None, 'bands'), (RM.BandTransfer(k, k, None, [2, 0], 'clamp'), None, 'extrapolate'),
                        (RM.BandTransfer(torch.empty(2, 1, device='meta'), torch.empty(2, 1, device='meta'), None, [2, 0], 'offset'), None, 'knots'),
                        (tr, torch.empty(3, 33, 64, device='meta'), 'out'), ((k, k), None, 'BandTransfer')):
        with pytest.raises(ValueError, match=msg):
            RM.check_transfer_args(a, t, out)
    c = torch.zeros(3, 33, 65)
    with pytest.raises(RuntimeError, match='no CPU path'):
        RM.band_quantiles(c, [0.5])
    with pytest.raises(RuntimeError, match='no CPU path'):
        RM.fit_transfer(c, c)
    with pytest.raises(RuntimeError, match='no CPU path'):
        RM.apply_transfer(c, RM.BandTransfer(torch.zeros(1, 2), torch.zeros(1, 2), None, [0], 'offset'))
    with pytest.raises(ValueError, match='lower'):
        RM.match_range(c, c, 0.9, 0.1)
    for kw, msg in ((dict(method='mean'), 'method'), (dict(ignore_label=256), 'ignore_label'), (dict(knots=1), 'knots'), (dict(method='range', lower=0.5, upper=0.5), 'lower')):
        with pytest.raises(ValueError, match=msg):
            RM.normalize_cities({}, **kw)
    with pytest.raises(ValueError, match='float32 or uint16'):
        RM.stretch_8bit(np.zeros((4, 4), np.float64))
    with pytest.raises(ValueError, match='percentiles'):
        RM.stretch_8bit(np.zeros((4, 4), np.float32), 2, 101)
    import fabric_amd.utils as U
    import fabric_amd.utils.dataloaders as D
    for name in ('band_quantiles', 'fit_transfer', 'apply_transfer', 'match_histograms', 'match_range', 'normalize_cities', 'check_quantile_args',
                 'check_fit_args', 'check_transfer_args'):
        assert getattr(U, name) is getattr(RM, name)
    assert D.stretch_8bit is RM.stretch_8bit
    assert RM.report_line('x', dict(method='range', bands=[0], count=[[1], [1]], p=[0.02, 0.5, 0.98], src=[[1, 2, 3]], dst=[[1, 2, 3]]))['city'] == 'x'


def test_cli_radiometric_flag_checks():
    from fabric_amd.train import check_radiometric_flags as chk
    assert chk(None) is None and chk('none') is None
    assert chk('histogram') == dict(method='histogram', knots=256, lower=0.02, upper=0.98, bands=None)
    ids = ['B02', 'B03', 'B04', 'B08']
    assert chk('range', None, [0.1, 0.9], ['B04', '0'], ids) == dict(method='range', knots=256, lower=0.1, upper=0.9, bands=[2, 0])
    assert chk('histogram', 64) == dict(method='histogram', knots=64, lower=0.02, upper=0.98, bands=None)
    assert chk(None, synthetic_radiometry=[1.3, 0.2], synthetic=True) is None
    kept = dict(method='range', knots=256, lower=0.1, upper=0.9, bands=[2, 0])
    assert chk(None, checkpoint=kept) == kept and chk('none', checkpoint=kept) is None and chk('histogram', checkpoint=kept)['method'] == 'histogram'
    for args, kw, msg in ((('sigma',), {}, '--radiometric sigma'), ((None, 64), {}, 'add'), (('none', None, [0.1, 0.9]), {}, 'add'),
                          ((None, None, None, ['0']), {}, 'add'), (('histogram', 1), {}, 'radiometric_knots 1'), (('histogram', 1025), {}, 'radiometric_knots'),
                          (('histogram', None, [0.1, 0.9]), {}, 'radiometric_range'), (('range', 64), {}, 'radiometric_knots'),
                          (('range', None, [0.9, 0.1]), {}, 'radiometric_range'), (('range', None, [0.0, 1.5]), {}, 'radiometric_range'),
                          (('range', None, None, ['13']), {}, 'radiometric_bands 13'), (('range', None, None, ['B05'], ids), {}, 'radiometric_bands B05'),
                          (('range', None, None, ['0', 'B02'], ids), {}, 'twice'), (('range', None, None, None, None, 65), {}, 'name a subset'),
                          ((None,), dict(synthetic_radiometry=[1.3, 0.2]), 'add --synthetic'),
                          ((None,), dict(synthetic_radiometry=[float('nan'), 0.2], synthetic=True), 'GAIN BIAS'),
                          ((None, 64), dict(checkpoint=kept), 'resumed'), ((None,), dict(checkpoint=dict(method='mean')), 'unknown')):
        with pytest.raises(ValueError, match=msg):
            chk(*args, **kw)
    for flags, msg in ((['--radiometric_knots', '64'], 'add --radiometric'), (['--radiometric', 'range', '--radiometric_range', '0.9', '0.1'], 'radiometric_range')):
        r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1'] + flags,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and msg in r.stderr, r.stderr[-500:]


def test_synthetic_radiometry():
    kw = dict(n_cities=2, bands=3, size=(40, 50), seed=3)
    base, same = synthetic_onera(**kw), synthetic_onera(radiometry=None, **kw)
    for c in base:
        for k in ('images', 'labels'):
            assert base[c][k].dtype == same[c][k].dtype and np.array_equal(base[c][k].view(np.uint8), same[c][k].view(np.uint8))
    moved = synthetic_onera(radiometry=(1.3, 0.2), **kw)
    for c in base:
        assert np.array_equal(moved[c]['labels'], base[c]['labels']) and np.array_equal(moved[c]['images'][0], base[c]['images'][0])
        want = np.float32(1.3) * base[c]['images'][1] + np.float32(0.2)
        assert moved[c]['images'].dtype == np.float32 and np.array_equal(moved[c]['images'][1], want) and moved[c]['images'].flags['C_CONTIGUOUS']
    with pytest.raises(ValueError, match='radiometry'):
        synthetic_onera(radiometry=(1.3,), **kw)


# ---------------------------------------------------------------- the twin
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _gamma(seed=0, shape=(97, 131)):
    return np.random.default_rng(seed).gamma(2.0, 1.0, shape).astype(np.float32)


def test_key_order_and_quantile_formula():
    v = np.array([3.0, -0.0, 0.0, -1.5, np.float32(1e-45), -np.float32(1e-45), 2.0], np.float32)
    s = RR.valid_sorted(v)
    assert s.tolist() == [-1.5, -np.float32(1e-45), -0.0, 0.0, np.float32(1e-45), 2.0, 3.0] and np.signbit(s[2]) and not np.signbit(s[3])
    assert np.array_equal(_bits(RR.unkeys(RR.keys(v))), _bits(v))
    value, order = RR.quantiles_sorted(s, [0.0, 0.25, 1.0, 0.5])
    assert value.tolist() == [-1.5, (-np.float64(np.float32(1e-45))) * 0.5, 3.0, 0.0] and order[1].tolist() == [-np.float32(1e-45), -0.0]
    assert order[0].tolist() == [-1.5, -np.float32(1e-45)] and order[2].tolist() == [3.0, 3.0]
    value, order, count = RR.quantiles_ref(np.full((2, 3, 3), np.nan, np.float32), [0.5])
    assert count.tolist() == [0, 0] and np.isnan(value).all() and np.isnan(order).all()
    x = np.array([[[-1.0, 0.0, 2.0, np.inf, 5.0]]], np.float32)
    assert RR.quantiles_ref(x, [1.0], positive_only=True)[2].tolist() == [2]
    assert RR.quantiles_ref(x, [1.0], exclude=np.array([[0, 0, 7, 0, 7]], np.uint8), exclude_value=7)[2].tolist() == [2]


def test_value_agrees_with_numpy_quantile():
    """value = a + (b - a) t against np.quantile(float64 data, method='linear'), which forms the same h = p (n - 1) and the same a, b and t
    but blends them as a + (b - a) t below t = 0.5 and as b - (b - a) (1 - t) from there on.  Each form rounds the difference, the product and the sum
    once, every intermediate is at most 2 max(|a|, |b|) in magnitude, so each lies within 3 * 2^-53 * 2 max(|a|, |b|) of the exact blend and the
    two within 12 * 2^-53 * max(|a|, |b|) of each other."""
    x = _gamma(1) - np.float32(1.5)
    probs = np.concatenate([np.linspace(0, 1, 257), [0.02, 0.98, 1 / 3]])
    value, order, count = RR.quantiles_ref(x[None], probs)
    want = np.quantile(x.astype(np.float64), probs, method='linear')
    bound = 12 * 2.0 ** -53 * np.abs(order[0].astype(np.float64)).max(axis=1)
    err = np.abs(value[0] - want)
    print(f'largest |value - np.quantile| / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}')
    assert count[0] == x.size and (err <= bound).all()


def test_matching_a_date_to_itself_returns_its_bits():
    x = np.stack([_gamma(2) - np.float32(2.0), np.round(_gamma(3) * 4) / 4]).astype(np.float32)
    x[0, 0, :4] = [np.nan, np.inf, -np.inf, -0.0]
    for method, kw in (('histogram', dict(knots=256)), ('histogram', dict(knots=7)), ('range', {})):
        out, s, t, n = RR.match_ref(x, x, method, **kw)
        assert np.array_equal(_bits(s), _bits(t)) and np.array_equal(_bits(out), _bits(x)), method


# The bound of "recover d1 from 1.3 d1 + 0.2": date 2 is y = fl(fl(1.3f x) + 0.2f).  Its knots are the images of date 1's knots under that
# monotone map, so inside the knots seg(y) = t0 + (y - s0) * ((t1 - t0) / (s1 - s0)) is evaluated on a chord of the affine map up to the
# roundings that formed y and s (each at most u |y|, u = 2^-24, twice: 2 u Y relative to the date-2 range Y, divided by the gain 1.3 on
# the way back) and the three roundings of seg itself (the difference y - s0 is exact or rounded once, the quotient once, the product
# once, the sum once: at most 4 u X on the date-1 range X).  With X = max |d1| and Y <= 1.3 X + 0.2 that is below (2 * (1.3 X + 0.2) / 1.3
# + 4 X) u <= 6.4 u X for X >= 1: a few ulp of the band's range.  (Measured on this band: about 1e-6 at X of about 13.)
def _recover_bound(x):
    X = float(np.abs(x).max())
    return (2 * (1.3 * X + 0.2) / 1.3 + 4 * X) * 2.0 ** -24


@pytest.mark.parametrize('method', ['range', 'histogram'])
def test_an_affine_change_is_recovered(method):
    d1 = _gamma(4)[None]
    d2 = (np.float32(1.3) * d1 + np.float32(0.2)).astype(np.float32)
    out, s, t, n = RR.match_ref(d2, d1, method)
    err = float(np.abs(out.astype(np.float64) - d1).max())
    print(f'{method}: largest |matched - d1| = {err:.3g}, bound {_recover_bound(d1):.3g}, max d1 {d1.max():.3g}')
    assert n.tolist() == [[d1.size], [d1.size]] and err <= _recover_bound(d1)


def test_a_band_of_30_values_has_repeated_knots_and_maps_exactly():
    r = np.random.default_rng(5)
    q = r.integers(0, 30, (1, 97, 131)).astype(np.float32)
    d2, d1 = q, (2 * q + 1).astype(np.float32)
    out, s, t, n = RR.match_ref(d2, d1, 'histogram', knots=256)
    assert (np.diff(s[0]) == 0).sum() > 200 and np.array_equal(t, 2 * s + 1)
    assert np.array_equal(out, d1)
    out, _, _, _ = RR.match_ref(d2, d1, 'range', lower=0.0, upper=1.0)
    assert np.array_equal(out, d1)


def test_transfer_rules_of_the_twin():
    s = np.array([1, 1, 2, 4, 4], np.float32)
    t = np.array([10, 10, 20, 30, 30], np.float32)
    x = np.array([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, np.nan, np.inf, -np.inf], np.float32)
    off = RR.transfer_band(x, s, t, RR.OFFSET)
    assert off[:7].tolist() == [9.5, 10.0, 15.0, 20.0, 25.0, 30.0, 32.0] and np.array_equal(_bits(off[7:]), _bits(x[7:]))
    assert np.array_equal(_bits(RR.transfer_band(x, s, t, RR.SLOPE)), _bits(off))          # zero-length end segments: the offset rule
    s2, t2 = np.array([1, 2, 4], np.float32), np.array([10, 20, 30], np.float32)
    assert RR.transfer_band(x, s2, t2, RR.SLOPE)[:7].tolist() == [5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 40.0]
    assert np.array_equal(_bits(RR.transfer_band(x, s2, np.array([10, np.nan, 30], np.float32))), _bits(x))
    assert np.array_equal(_bits(RR.transfer_band(x, s2, t2, exact=True)), _bits(x))
    z = np.array([-0.0, 0.0, -5.0], np.float32)
    assert np.array_equal(_bits(RR.transfer_band(z, np.array([1, 2], np.float32), np.array([1, 2], np.float32))), _bits(z))


def test_stretch_twin_against_the_formula():
    r = np.random.default_rng(6)
    for x in (r.integers(0, 4000, (40, 50)).astype(np.uint16), (r.gamma(2.0, 500.0, (40, 50)) * (r.random((40, 50)) > 0.1)).astype(np.float32)):
        x[:3] = 0
        pos = x[x > 0].astype(np.float64)
        c, d = np.quantile(pos, 0.02), np.quantile(pos, 0.98)
        t = (x.astype(np.float64) - c) * (255.0 / (d - c))
        t[t < 0] = 0
        t[t > 255] = 255
        got = RR.stretch_8bit_ref(x)
        # the twin's c, d are a + (b - a) t; numpy's blend may differ in the last bit (test_value_agrees_with_numpy_quantile): a pixel may
        # then land on the other side of an integer, by one
        diff = np.abs(got.astype(int) - t.astype(np.uint8).astype(int))
        assert got.dtype == np.uint8 and diff.max() <= 1 and (diff != 0).mean() < 1e-3
        v = RR.valid_sorted(x.astype(np.float32), positive_only=True)
        (c2, d2), _ = RR.quantiles_sorted(v, [0.02, 0.98])
        t2 = np.clip((x.astype(np.float64) - c2) * (255.0 / (d2 - c2)), 0, 255)
        assert np.array_equal(got, t2.astype(np.uint8)) and got[:3].max() == 0 and got.max() == 255
    # a constant band: d == c, the scale is +inf; values above c give 255, c itself (0 * inf = NaN) and everything below give 0
    assert RR.stretch_8bit_ref(np.full((4, 5), 7, np.uint16)).tolist() == [[0] * 5] * 4
    assert RR.stretch_ref(np.array([6.0, 7.0, 8.0, np.nan], np.float32), 7.0, 7.0).tolist() == [0, 0, 255, 0]
    # no value > 0: c and d are NaN, every byte is 0
    assert not RR.stretch_8bit_ref(np.zeros((4, 5), np.float32)).any()
    stack = np.stack([np.full((4, 5), 7, np.uint16), np.arange(20, dtype=np.uint16).reshape(4, 5)])
    assert np.array_equal(RR.stretch_8bit_ref(stack)[1], RR.stretch_8bit_ref(stack[1]))
