"""-m "not gpu": what the co-registration pins without a device -- the reference of the GPU tests (tests/register_ref.py) against a brute
force, the method on integer and sub-pixel shifts, the declarations of the new entries against _lib.SIGNATURES, every argument check of
every new C entry (fake non-null pointers: BDN_E_ARG before anything touches a device), the workspace condition, the argument checks of
fabric_amd.utils.registration on meta tensors, the CLI flag checks and synthetic_onera(misreg=)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import registration as RG
from fabric_amd.utils.dataloaders import synthetic_onera
from tests import register_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
P = 0x1000                                                  # a fake non-null, 16-byte aligned pointer: never dereferenced


# ---------------------------------------------------------------- the reference
def _tiny(seed, c, h, w, holes=True):
    r = np.random.default_rng(seed)
    d1 = r.standard_normal((c, h, w)).astype(np.float32)
    d2 = (d1 * np.float32(0.8) + r.standard_normal((c, h, w)).astype(np.float32)).astype(np.float32)
    ex = None
    if holes:
        d1[0, 1, 2], d2[0, 0, 0], d2[-1, h - 1, w - 1], d1[-1, 2, 1] = np.nan, np.inf, -np.inf, np.nan
        ex = (r.random((h, w)) < 0.15).astype(np.uint8) * 9
    return d1, d2, ex


@pytest.mark.parametrize('shape,R,cells', [((1, 1, 1), 1, (1, 1)), ((2, 5, 7), 2, (1, 1)), ((2, 5, 7), 2, (2, 3)), ((1, 6, 4), 3, (3, 2))])
def test_reference_is_the_brute_force(shape, R, cells):
    for holes in (False, True):
        d1, d2, ex = _tiny(3, *shape, holes=holes and shape[1] > 2)
        bands = list(range(shape[0]))[::-1]
        t, sabs = RR.table_ref(d1, d2, bands, R, cells[0], cells[1], ex, 9)
        assert np.array_equal(t, RR.table_brute(d1, d2, bands, R, cells[0], cells[1], ex, 9))
        assert (sabs >= np.abs(t) * (1 - 1e-12)).all() and np.array_equal(sabs[..., 0], t[..., 0])
        fast, _ = RR.table_ref(d1, d2, bands, R, cells[0], cells[1], ex, 9, exact=False)
        assert np.array_equal(fast[..., 0], t[..., 0]) and np.allclose(fast, t, rtol=1e-12, atol=1e-12)


def test_cells_add_up_to_the_whole_scene():
    r = np.random.default_rng(5)
    d1 = r.integers(-20, 21, (2, 11, 13)).astype(np.float32)          # small integers: every sum is exact in any order
    d2 = r.integers(-20, 21, (2, 11, 13)).astype(np.float32)
    d1[0, 3, 3] = np.nan
    whole, _ = RR.table_ref(d1, d2, [0, 1], 2, 1, 1)
    for cells in ((2, 3), (3, 1), (11, 13)):
        t, _ = RR.table_ref(d1, d2, [0, 1], 2, *cells)
        assert np.array_equal(RR.whole_table(t), whole[:, 0, 0]), cells
    # the counts: a shift loses the pixels whose date-2 tap leaves the scene, and the NaN pixel
    assert whole[1, 0, 0, 2, 2, 0] == 11 * 13 and whole[0, 0, 0, 2, 2, 0] == 11 * 13 - 1 and whole[1, 0, 0, 0, 4, 0] == 9 * 11


def _noise_pair(t, seed=0, shape=(3, 96, 120)):
    """date 2 = date 1 sampled at + t, times 1.3 plus 0.2 plus noise: the estimate is -t."""
    r = np.random.default_rng(seed)
    d1 = r.standard_normal(shape).astype(np.float32)
    d2 = RR.shift_bilinear(d1, *t) * np.float32(1.3) + np.float32(0.2) + np.float32(0.3) * r.standard_normal(shape).astype(np.float32)
    return d1, d2.astype(np.float32)


@pytest.mark.parametrize('t', [(0, 0), (1, -2), (-4, 4), (3, 0)])
def test_integer_shifts_are_recovered(t):
    d1, d2 = _noise_pair(t)
    rep, field = RR.estimate_ref(d1, d2, 4)
    dy, dx, ncc, ok = rep[-1]
    assert ok == 1 and (round(dy), round(dx)) == (-t[0], -t[1])
    # white noise: the neighbours of the peak are noise of about 1 / sqrt(pixels) = 0.005 against a peak of 0.97, so the parabola moves
    # the estimate by a few thousandths of a pixel; on the window border it is not formed
    assert abs(dy + t[0]) < 0.02 and abs(dx + t[1]) < 0.02
    if abs(t[0]) == 4:
        assert dy == -t[0] and dx == -t[1]
    assert 0.96 < ncc < 0.985
    assert np.array_equal(rep[0], rep[-1]) and np.array_equal(field[0, 0], rep[-1, :2].astype(np.float32))


# twice the largest error the committed reference makes on the committed seeds (measured: 0.0457 px at sigma 1, 0.0267 px at sigma 2);
# DESIGN.md section 23.  This pins the method (a parabola through NCC samples is biased towards the integer), not the kernels.
SUBPIXEL_BOUND = {1: 0.0914, 2: 0.0534}


@pytest.mark.parametrize('sigma', [1, 2])
def test_subpixel_shifts_are_recovered(sigma):
    from scipy import ndimage
    worst = 0.0
    for k, t in enumerate([(0.25, -0.5), (1.3, 2.7), (-2.5, 0.4), (0.5, 0.5)]):
        r = np.random.default_rng(100 * sigma + k)
        d1 = np.stack([ndimage.gaussian_filter(r.standard_normal((96, 120)), sigma) for _ in range(3)]).astype(np.float32)
        d1 /= d1.std()
        d2 = RR.shift_bilinear(d1, *t)
        rep, _ = RR.estimate_ref(d1, d2, 4)
        dy, dx, ncc, ok = rep[-1]
        assert ok == 1
        worst = max(worst, abs(dy + t[0]), abs(dx + t[1]))
    print(f'sigma {sigma}: worst sub-pixel error {worst:.4f} px')
    assert worst <= SUBPIXEL_BOUND[sigma]


def test_field_interpolation_and_resampling_reference():
    r = np.random.default_rng(2)
    src = r.standard_normal((2, 9, 11)).astype(np.float32)
    out, oob = RR.apply_ref(src, np.zeros((1, 1, 2), np.float32))
    assert np.array_equal(out.view(np.uint32), src.view(np.uint32)) and not oob.any()
    out, oob = RR.apply_ref(src, np.array([[[2, -3]]], np.float32))
    want = src[:, np.clip(np.arange(9) + 2, 0, 8)][:, :, np.clip(np.arange(11) - 3, 0, 10)]
    assert np.array_equal(out, want)
    assert np.array_equal(oob, ((np.arange(9)[:, None] + 2 > 8) | (np.arange(11)[None, :] - 3 < 0)).astype(np.uint8))
    out, oob = RR.apply_ref(src, np.array([[[0.5, 0.0]]], np.float32))
    assert np.array_equal(out[:, :-1], (np.float32(0.5) * src[:, :-1]) + (np.float32(0.5) * src[:, 1:])) and oob[-1].all() and not oob[:-1].any()
    # the field between cell centres: constant outside the outer centres, linear between them
    f = np.zeros((3, 2, 2), np.float32)
    f[:, :, 0] = [[0, 0], [1, 1], [3, 3]]
    s = RR.field_ref(f, 9, 11)                               # rows 0..2, 3..5, 6..8: centres 1, 4, 7
    assert np.array_equal(s[0][:, 0], np.array([0, 0, 1 / 3, 2 / 3, 1, 5 / 3, 7 / 3, 3, 3], np.float32)) and not s[1].any()
    assert np.array_equal(s[0][:, 0], s[0][:, -1])


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


ENTRIES = [('bdn_shift_corr_workspace_bytes', 'size_t', 6), ('bdn_shift_corr', 'int', 15), ('bdn_shift_peak', 'int', 9), ('bdn_shift_apply', 'int', 10)]


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
    assert 'register.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()
    sec = hdr[hdr.index('co-registration of the two dates'):hdr.index('size_t bdn_shift_corr_workspace_bytes(')]
    for cite in ('d2(y + dy, x + dx) ~ d1(y, x)', 'no atomics', 'BDN_E_ARG before anything touches a device', 'first maximum in raster order',
                 'top = ((1 - fx) * v00) + (fx * v01)', 'cy_i = 0.5f (r0_i + r1_i - 1)'):
        assert cite in sec, cite


def _rc(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.bdn_last_error().decode()


def _bad(name, good, i, v, msg):
    a = list(good)
    a[i] = v
    rc, err = _rc(name, *a)
    assert rc == E_ARG and msg in err, (name, i, v, rc, err)


def test_shift_corr_argument_checks():
    #       d1 d2 bands n_b excl exv R ny nx table ws C  H   W   stream
    good = [P, P, P, 3, None, 0, 4, 2, 3, P, P, 3, 33, 65, None]
    for i in (0, 1, 2, 9, 10):
        _bad('bdn_shift_corr', good, i, None, 'null pointer')
    for i, v, msg in ((3, 0, 'band indices'), (3, 65, 'band indices'), (6, 0, 'search radius'), (6, 17, 'search radius'), (6, -1, 'search radius'),
                      (7, 0, 'bad grid'), (8, 0, 'bad grid'), (7, 65, 'bad grid'), (8, 65, 'bad grid'), (7, 34, 'bad grid'), (12, 0, 'bad grid'),
                      (13, -5, 'bad grid'), (12, 32768, 'bad grid'), (13, 32768, 'bad grid'), (11, 0, 'channels'), (11, 65536, 'channels'),
                      (0, P + 2, 'aligned'), (1, P + 1, 'aligned'), (2, P + 2, 'aligned'), (9, P + 4, 'aligned'), (10, P + 8, 'aligned')):
        _bad('bdn_shift_corr', good, i, v, msg)
    a = list(good); a[13], a[8] = 2, 3                       # nx > W
    assert _rc('bdn_shift_corr', *a)[0] == E_ARG
    a = list(good); a[4], a[5] = P, 256
    rc, err = _rc('bdn_shift_corr', *a)
    assert rc == E_ARG and 'exclude_value' in err
    a[5] = -1
    assert _rc('bdn_shift_corr', *a)[0] == E_ARG


def test_workspace_does_not_grow_with_the_scene():
    q = _lib.load().bdn_shift_corr_workspace_bytes
    big = q(13, 10000, 10000, 8, 8, 8)
    assert 0 < big < 256 << 20                               # the condition: under 256 MiB for 13 bands, 10 000^2, R = 8, cells 8 x 8
    assert big == q(13, 500, 500, 8, 8, 8) == q(13, 32767, 32767, 8, 8, 8)
    assert q(1, 1, 1, 1, 1, 1) == 8 * 6 * 9 * 1024 and q(2, 40, 40, 16, 1, 1) == 2 * q(1, 40, 40, 16, 1, 1)
    assert q(13, 500, 500, 8, 1, 1) == 8 * 6 * 289 * 13 * 1024 < 256 << 20
    assert q(64, 500, 500, 16, 1, 1) == 8 * 6 * 1089 * 64 * 80 <= 256 << 20      # capped: P tables within 256 MiB where one table is
    assert q(1, 100, 100, 2, 64, 64) == 8 * 6 * 25 * 4096   # one partial per cell for a fine grid: the size of the table
    assert q(3, 97, 131, 8, 3, 2) % 16 == 0
    for args in ((0, 8, 8, 1, 1, 1), (65, 8, 8, 1, 1, 1), (1, 0, 8, 1, 1, 1), (1, 8, 32768, 1, 1, 1), (1, 8, 8, 0, 1, 1), (1, 8, 8, 17, 1, 1),
                 (1, 8, 8, 1, 9, 1), (1, 8, 8, 1, 1, 0), (1, 100, 100, 1, 65, 1)):
        assert q(*args) == 0, args


def test_shift_peak_and_apply_argument_checks():
    #       table n_b R ny nx min_ncc report field stream
    good = [P, 3, 4, 2, 3, 0.0, P, P, None]
    for i in (0, 6, 7):
        _bad('bdn_shift_peak', good, i, None, 'null pointer')
    for i, v, msg in ((1, 0, 'bands'), (1, 65, 'bands'), (2, 0, 'search radius'), (2, 17, 'search radius'), (3, 0, 'bad grid'), (4, 65, 'bad grid'),
                      (5, float('nan'), 'min_ncc'), (0, P + 4, 'aligned'), (6, P + 4, 'aligned'), (7, P + 2, 'aligned')):
        _bad('bdn_shift_peak', good, i, v, msg)
    #       src field ny nx out oob C  H   W  stream
    good = [P, P, 2, 3, 2 * P, None, 3, 33, 65, None]
    for i in (0, 1, 4):
        _bad('bdn_shift_apply', good, i, None, 'null pointer')
    for i, v, msg in ((4, P, 'out == src'), (2, 0, 'bad grid'), (3, 65, 'bad grid'), (2, 34, 'bad grid'), (3, 66, 'bad grid'), (6, 0, 'channels'),
                      (7, 0, 'bad grid'), (8, 32768, 'bad grid'), (0, P + 2, 'aligned'), (4, 2 * P + 1, 'aligned'), (1, P + 2, 'aligned')):
        _bad('bdn_shift_apply', good, i, v, msg)


# ---------------------------------------------------------------- the Python surface without a device
def test_check_estimate_and_apply_args_on_meta_tensors():
    a = torch.empty(3, 33, 65, device='meta')
    assert RG.check_estimate_args(a, a) == (3, 33, 65, 8, [0, 1, 2], 1, 1)
    ex = torch.empty(33, 65, dtype=torch.uint8, device='meta')
    assert RG.check_estimate_args(a, a, 16, [2, 0], (2, 3), ex, 255, 0.5) == (3, 33, 65, 16, [2, 0], 2, 3)
    for kw, msg in ((dict(max_shift=0), 'max_shift'), (dict(max_shift=17), 'max_shift'), (dict(max_shift=2.0), 'max_shift'), (dict(bands=[]), 'bands'),
                    (dict(bands=[3]), 'bands'), (dict(bands=[-1]), 'bands'), (dict(bands='0'), 'bands'), (dict(cells=(0, 1)), 'cells'),
                    (dict(cells=(34, 1)), 'cells'), (dict(cells=(1, 65)), 'cells'), (dict(cells=3), 'cells'), (dict(exclude=ex), 'exclude_value'),
                    (dict(exclude=ex, exclude_value=256), 'exclude_value'), (dict(exclude=ex.float(), exclude_value=0), 'exclude'),
                    (dict(exclude=torch.empty(33, 64, dtype=torch.uint8, device='meta'), exclude_value=0), 'exclude'),
                    (dict(min_ncc=2.0), 'min_ncc'), (dict(min_ncc=float('nan')), 'min_ncc')):
        with pytest.raises(ValueError, match=msg):
            RG.check_estimate_args(a, a, **kw)
    for bad in (a.double(), a[0], a.permute(0, 2, 1), torch.empty(0, 3, 3, device='meta'), np.zeros((3, 33, 65), np.float32)):
        with pytest.raises(ValueError, match='d1'):
            RG.check_estimate_args(bad, a)
    with pytest.raises(ValueError, match='d2'):
        RG.check_estimate_args(a, torch.empty(3, 33, 64, device='meta'))
    with pytest.raises(ValueError, match='d2 is on'):
        RG.check_estimate_args(a, torch.zeros(3, 33, 65))
    with pytest.raises(ValueError, match='name a subset'):
        RG.check_estimate_args(torch.empty(65, 4, 4, device='meta'), torch.empty(65, 4, 4, device='meta'))
    f = torch.empty(2, 3, 2, device='meta')
    assert RG.check_apply_args(a, f) == (3, 33, 65, 2, 3)
    assert RG.check_apply_args(a, f, torch.empty(3, 33, 65, device='meta'), ex) == (3, 33, 65, 2, 3)
    for args, msg in (((a, f.double()), 'field'), ((a, torch.empty(2, 3, device='meta')), 'field'), ((a, torch.empty(34, 1, 2, device='meta')), 'cells'),
                      ((a, f, torch.empty(3, 33, 64, device='meta')), 'out'), ((a, f, None, ex.float()), 'oob'), ((a.double(), f), 'd2')):
        with pytest.raises(ValueError, match=msg):
            RG.check_apply_args(*args)
    c = torch.zeros(3, 33, 65)
    with pytest.raises(ValueError, match='out must not be d2'):
        RG.check_apply_args(c, torch.zeros(1, 1, 2), c)
    with pytest.raises(RuntimeError, match='no CPU path'):
        RG.estimate_shift(c, c)
    with pytest.raises(RuntimeError, match='no CPU path'):
        RG.apply_shift(c, torch.zeros(1, 1, 2))
    with pytest.raises(ValueError, match='ignore_label'):
        RG.coregister_cities({}, ignore_label=256)
    import fabric_amd.utils as U
    for name in ('estimate_shift', 'apply_shift', 'coregister', 'coregister_cities', 'check_estimate_args', 'check_apply_args'):
        assert getattr(U, name) is getattr(RG, name)


def test_cli_coregister_flag_checks():
    from fabric_amd.train import check_coregister_flags as chk
    assert chk(0, [1, 1], None, 0.0) is None
    assert chk(4, [1, 1], None, 0.0) == dict(max_shift=4, cells=(1, 1), bands=None, min_ncc=0.0)
    ids = ['B02', 'B03', 'B04', 'B08']
    assert chk(8, [2, 3], ['B04', '0', 'B08'], 0.5, ids) == dict(max_shift=8, cells=(2, 3), bands=[2, 0, 3], min_ncc=0.5)
    assert chk(0, [1, 1], None, 0.0, None, 13, [2, -1], True) is None
    for args, msg in (((-1, [1, 1], None, 0.0), '--coregister -1'), ((17, [1, 1], None, 0.0), '--coregister 17'), ((0, [2, 2], None, 0.0), 'add --coregister R'),
                      ((0, [1, 1], ['0'], 0.0), 'add --coregister R'), ((0, [1, 1], None, 0.5), 'add --coregister R'), ((4, [0, 1], None, 0.0), 'coregister_cells'),
                      ((4, [1, 65], None, 0.0), 'coregister_cells'), ((4, [1, 1], None, 1.5), 'coregister_min_ncc'), ((4, [1, 1], ['13'], 0.0), 'coregister_bands 13'),
                      ((4, [1, 1], ['B05'], 0.0, ids), 'coregister_bands B05'), ((4, [1, 1], ['4'], 0.0, ids), 'coregister_bands 4'),
                      ((4, [1, 1], None, 0.0, None, 65), 'name a subset'), ((0, [1, 1], None, 0.0, None, 13, [1, 0], False), 'add --synthetic')):
        with pytest.raises(ValueError, match=msg):
            chk(*args)
    for flags, msg in ((['--coregister', '17'], '--coregister 17'), (['--coregister_cells', '2', '2'], 'add --coregister R')):
        r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1'] + flags,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and msg in r.stderr, r.stderr[-500:]


def test_synthetic_misreg():
    kw = dict(n_cities=2, bands=3, size=(40, 50), seed=3)
    base, same = synthetic_onera(**kw), synthetic_onera(misreg=(0, 0), **kw)
    for c in base:
        for k in ('images', 'labels'):
            assert base[c][k].dtype == same[c][k].dtype and np.array_equal(base[c][k].view(np.uint8), same[c][k].view(np.uint8))
    moved = synthetic_onera(misreg=(2, -1), **kw)
    for c in base:
        assert np.array_equal(moved[c]['labels'], base[c]['labels']) and np.array_equal(moved[c]['images'][0], base[c]['images'][0])
        want = base[c]['images'][1][:, np.clip(np.arange(40) + 2, 0, 39)][:, :, np.clip(np.arange(50) - 1, 0, 49)]
        assert np.array_equal(moved[c]['images'][1], want) and moved[c]['images'].flags['C_CONTIGUOUS']
        rep, _ = RR.estimate_ref(moved[c]['images'][0], moved[c]['images'][1], 3)
        assert (round(rep[-1, 0]), round(rep[-1, 1])) == (-2, 1)
    with pytest.raises(ValueError, match='misreg'):
        synthetic_onera(misreg=(0.5, 0), **kw)
