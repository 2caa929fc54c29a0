"""CPU tests of the mask clean-up feature: the host restatement tests/morph_ref.py is pinned to scipy.ndimage (binary_propagation,
binary_fill_holes with both structures, binary_dilation / binary_erosion(border_value=1) with the disc) and to brute force (the hole-area
bound by flood fill, the separable distance by looking at every site); then the parts that need no device: the declarations of the new
entries against _lib.SIGNATURES, every argument check of every new C entry (fake non-null pointers: each returns BDN_E_ARG before
anything touches a device), the check_* functions on meta tensors, check_cleanup_flags and the training CLI's defaults."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ndi = pytest.importorskip('scipy.ndimage')

from fabric_amd import _lib  # noqa: E402
from fabric_amd.utils import morphology as M  # noqa: E402
from tests import cc_ref, edt_ref  # noqa: E402
from tests import morph_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (0, 1, 2, 4, 5, 9, 10, 25)
BDN_E_ARG = -1


def _structure(conn):
    return ndi.generate_binary_structure(2, 1 if conn == 4 else 2)


def _rasters():
    """(name, uint8 [H,W]): random rasters of 1..40 pixels a side at three densities, and the pattern sets of cc_ref and edt_ref."""
    r = np.random.default_rng(7)
    out = []
    for k in range(36):
        h, w = (int(v) for v in r.integers(1, 41, 2))
        d = (0.1, 0.5, 0.8)[k % 3]
        out.append((f'random {h}x{w} {d}', (r.random((h, w)) < d).astype(np.uint8)))
    for h, w in ((1, 1), (1, 9), (9, 1), (23, 31)):
        out += [(f'cc {k} {h}x{w}', m) for k, m in cc_ref.patterns(h, w, tile=8).items()]
        out += [(f'edt {k} {h}x{w}', edt_ref.pattern(k, h, w)) for k in edt_ref.PATTERNS]
    return out


RASTERS = _rasters()


# ---------------------------------------------------------------- the restatement against scipy / brute force
@pytest.mark.parametrize('conn', [4, 8])
def test_reconstruct_is_binary_propagation(conn):
    r = np.random.default_rng(3)
    for name, m in RASTERS:
        seed = (r.random(m.shape) < 0.05).astype(np.uint8)           # seeds outside the mask too: they must not count
        want = ndi.binary_propagation((seed == 1) & (m == 1), structure=_structure(conn), mask=m == 1)
        assert np.array_equal(R.reconstruct(m, seed, conn), want.astype(np.uint8)), name
        assert not R.reconstruct(m, np.zeros_like(m), conn).any(), name
        assert np.array_equal(R.reconstruct(m, np.ones_like(m), conn), m), name


def test_hysteresis_definition():
    r = np.random.default_rng(4)
    p1 = r.random((17, 23)).astype(np.float32)
    p1[3, 4], p1[5, 6], p1[7, 7], p1[0, 0], p1[1, 1] = np.nan, np.inf, -np.inf, 0.25, 0.75
    proba = np.stack([1 - p1, p1])
    for conn in (4, 8):
        got = R.hysteresis_mask(proba, 0.25, 0.75, 1, conn)
        with np.errstate(invalid='ignore'):
            weak, strong = p1 >= np.float32(0.25), p1 >= np.float32(0.75)
        assert weak[0, 0] and strong[1, 1] and not weak[3, 4]
        assert np.array_equal(got, ndi.binary_propagation(strong, structure=_structure(conn), mask=weak).astype(np.uint8))
        assert np.array_equal(R.hysteresis_mask(proba, 0.5, 0.5, 1, conn), (p1 >= np.float32(0.5)).astype(np.uint8))


@pytest.mark.parametrize('conn', [4, 8])
def test_fill_holes_is_binary_fill_holes(conn):
    for name, m in RASTERS:
        want = ndi.binary_fill_holes(m == 1, structure=None if conn == 8 else np.ones((3, 3)))
        assert np.array_equal(R.fill_holes(m, None, conn), want.astype(np.uint8)), name


def _holes_by_flood_fill(m, bg_conn):
    """[(pixels of one background component, touches the edge)] by a stack-based flood fill."""
    h, w = m.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if bg_conn == 8 else [])
    seen = m == 1
    out = []
    for y0 in range(h):
        for x0 in range(w):
            if seen[y0, x0]:
                continue
            seen[y0, x0] = True
            stack, px, edge = [(y0, x0)], [], False
            while stack:
                y, x = stack.pop()
                px.append((y, x))
                edge |= y in (0, h - 1) or x in (0, w - 1)
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx]:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
            out.append((px, edge))
    return out


@pytest.mark.parametrize('conn', [4, 8])
def test_fill_holes_max_area_is_a_flood_fill(conn):
    for name, m in RASTERS[::3]:
        holes = _holes_by_flood_fill(m, 4 if conn == 8 else 8)
        for max_area in (1, 2, 5, 1 << 20):
            want = (m == 1).astype(np.uint8)
            for px, edge in holes:
                if not edge and len(px) <= max_area:
                    for y, x in px:
                        want[y, x] = 1
            assert np.array_equal(R.fill_holes(m, max_area, conn), want), (name, max_area)


@pytest.mark.parametrize('conn', [4, 8])
def test_clear_border_by_labels(conn):
    for name, m in RASTERS[::2]:
        lab, _ = ndi.label(m == 1, _structure(conn))
        edge = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
        want = ((lab > 0) & ~np.isin(lab, edge)).astype(np.uint8)
        assert np.array_equal(R.clear_border(m, conn), want), name


def test_separable_distance_is_brute_force():
    for name, m in RASTERS[::4]:
        for limit in (R.INT_MAX, 26, 1):
            assert np.array_equal(R.d2_sep(m == 1, limit), edt_ref.d2_brute(m == 1, limit)), (name, limit)


@pytest.mark.parametrize('radius2', RADII)
def test_disc_morphology_is_scipys(radius2):
    disc = R.disc(radius2)
    assert disc.sum() == sum(dy * dy + dx * dx <= radius2 for dy in range(-6, 7) for dx in range(-6, 7))
    for name, m in RASTERS:
        b = m == 1
        assert np.array_equal(R.binary_dilation(m, radius2), ndi.binary_dilation(b, disc).astype(np.uint8)), name
        assert np.array_equal(R.binary_erosion(m, radius2), ndi.binary_erosion(b, disc, border_value=1).astype(np.uint8)), name
        op, cl = R.binary_opening(m, radius2), R.binary_closing(m, radius2)
        assert np.array_equal(op, ndi.binary_dilation(ndi.binary_erosion(b, disc, border_value=1), disc).astype(np.uint8)), name
        assert np.array_equal(cl, ndi.binary_erosion(ndi.binary_dilation(b, disc), disc, border_value=1).astype(np.uint8)), name
        assert (op <= m).all() and (m <= cl).all(), name
        if radius2 == 0:
            assert np.array_equal(op, m) and np.array_equal(cl, m)


def test_mark_and_select_contract():
    m = np.array([[1, 1, 0, 0, 0], [0, 0, 0, 1, 0], [0, 1, 0, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]], np.uint8)
    lab = cc_ref.label(m == 1, 4)
    seed = np.zeros_like(m)
    seed[2, 3] = seed[3, 3] = 1                                      # one on the component rooted at 8, one on background
    mk = R.mark(lab, seed, 1, False)
    assert np.flatnonzero(mk).tolist() == [8]
    assert np.flatnonzero(R.mark(lab, None, 1, True)).tolist() == [0, 24]
    assert np.flatnonzero(R.mark(lab, seed, 1, True)).tolist() == [0, 8, 24]
    area = cc_ref.areas(lab)
    assert R.select(lab, mk, True).sum() == 2 and R.select(lab, mk, False).sum() == 4
    assert R.select(lab, None, True, area, 2, 2).sum() == 4 and R.select(lab, None, True, area, 1, 1).sum() == 2
    base = np.full_like(m, 7)
    base[3, 0] = 1
    assert R.select(lab, mk, True, base=base).sum() == 3


# ---------------------------------------------------------------- argument checks without a device
def _meta(*shape, dtype=torch.uint8):
    return torch.empty(*shape, dtype=dtype, device='meta')


def test_check_functions_on_meta_tensors():
    m = _meta(5, 7)
    assert M.check_reconstruct_args(m, m, 4, m) == (5, 7)
    assert M.check_fill_holes_args(m, 3, 8) == (5, 7) and M.check_fill_holes_args(m, None, 4, m) == (5, 7)
    assert M.check_morph_args(m, 0) == (5, 7) and M.check_morph_args(m, (1 << 31) - 2, m) == (5, 7)
    assert M.check_hysteresis_args(_meta(2, 5, 7, dtype=torch.float32), 0.25, 0.5, 1, 8, m) == (2, 5, 7, 0.25, 0.5)
    for bad in (_meta(5, 7, dtype=torch.int32), _meta(2, 5, 7), _meta(0, 7), _meta(5, 7).t(), 'x'):
        for fn in (M.check_reconstruct_args, M.check_fill_holes_args):
            with pytest.raises(ValueError, match='mask'):
                fn(bad)
        with pytest.raises(ValueError, match='mask'):
            M.check_morph_args(bad, 1)
    for conn in (0, 6, 8.0, True):
        with pytest.raises(ValueError, match='connectivity'):
            M.check_reconstruct_args(m, None, conn)
    for bad in (_meta(5, 6), _meta(5, 7, dtype=torch.int32), torch.zeros(5, 7, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='seed'):
            M.check_reconstruct_args(m, bad)
        with pytest.raises(ValueError, match='out'):
            M.check_reconstruct_args(m, None, 8, bad)
        with pytest.raises(ValueError, match='out'):
            M.check_morph_args(m, 1, bad)
    for bad in (0, -1, 2.0, True, 1 << 31):
        with pytest.raises(ValueError, match='max_area'):
            M.check_fill_holes_args(m, bad)
    for bad in (-1, 1.0, True, None, (1 << 31) - 1):
        with pytest.raises(ValueError, match='radius2'):
            M.check_morph_args(m, bad)
    with pytest.raises(ValueError, match='32767'):
        M.check_morph_args(_meta(1, 40000), 1)
    p = _meta(2, 5, 7, dtype=torch.float32)
    for low, high in ((0.6, 0.5), (-0.1, 0.5), (0.2, 1.5), (float('nan'), 0.5), (0.1, float('nan')), ('a', 0.5), (True, 1)):
        with pytest.raises(ValueError, match='low|high'):
            M.check_hysteresis_args(p, low, high)
    for bad in (_meta(5, 7, dtype=torch.float32), _meta(2, 5, 7, dtype=torch.float64), _meta(1, 5, 7, dtype=torch.float32)):
        with pytest.raises(ValueError, match='proba'):
            M.check_hysteresis_args(bad, 0.1, 0.5)
    for pc in (-1, 2, 1.0, True):
        with pytest.raises(ValueError, match='pos_class'):
            M.check_hysteresis_args(p, 0.1, 0.5, pc)
    with pytest.raises(ValueError, match='out'):
        M.check_hysteresis_args(p, 0.1, 0.5, 1, 8, _meta(5, 6))


def test_public_functions_validate_then_refuse_host_tensors():
    m = torch.zeros(5, 7, dtype=torch.uint8)
    p = torch.zeros(2, 5, 7)
    calls = ((M.reconstruct, (m, m)), (M.hysteresis_mask, (p, 0.2, 0.5)), (M.clear_border, (m,)), (M.fill_holes, (m,)),
             (M.binary_dilation, (m, 2)), (M.binary_erosion, (m, 2)), (M.binary_opening, (m, 2)), (M.binary_closing, (m, 2)))
    for fn, args in calls:
        with pytest.raises(RuntimeError, match='no CPU path'):
            fn(*args)
    with pytest.raises(ValueError, match='connectivity'):
        M.reconstruct(m, m, 5)
    with pytest.raises(ValueError, match='seed'):
        M.reconstruct(m, None)
    with pytest.raises(ValueError, match='low'):
        M.hysteresis_mask(p, 0.7, 0.5)
    with pytest.raises(ValueError, match='radius2'):
        M.binary_opening(m, -1)
    import fabric_amd.utils as U
    for fn, _ in calls:
        assert getattr(U, fn.__name__) is fn


def test_predict_scene_blended_arguments():
    from fabric_amd.utils.inference import predict_scene_blended
    sig = inspect.signature(predict_scene_blended).parameters
    names = list(sig)
    assert names[-4:] == ['hysteresis_low', 'close_radius2', 'fill_holes', 'open_radius2'] and names[-5] == 'connectivity'
    assert all(sig[k].default is None for k in names[-4:])
    assert M.check_cleanup_args() is None and M.check_cleanup_args(0.5, 0.2, 2, True, 25, 4) is None
    assert M.check_cleanup_args(None, None, None, 30) == 30 and M.check_cleanup_args(fill_holes=False) is None
    with pytest.raises(ValueError, match='needs a threshold'):
        M.check_cleanup_args(None, 0.2)
    for low in (0.6, -0.1, float('nan'), 'x', True):
        with pytest.raises(ValueError, match='hysteresis_low'):
            M.check_cleanup_args(0.5, low)
    with pytest.raises(ValueError, match='radius2'):
        M.check_cleanup_args(close_radius2=-1)
    with pytest.raises(ValueError, match='radius2'):
        M.check_cleanup_args(open_radius2=1.5)
    with pytest.raises(ValueError, match='max_area'):
        M.check_cleanup_args(fill_holes=0)
    with pytest.raises(ValueError, match='connectivity'):
        M.check_cleanup_args(connectivity=6)


def test_cli_cleanup_flag_checks():
    from fabric_amd.train import check_cleanup_flags, cleaned_scores
    assert check_cleanup_flags(None, None, 0, None, 'argmax', 8, 0) is None
    assert check_cleanup_flags(0.2, 2, -1, 25, 0.5, 4, 64) == {'hysteresis_low': 0.2, 'close_radius2': 2, 'fill_holes': True, 'open_radius2': 25}
    assert check_cleanup_flags(None, None, 40, None, 'argmax', 8, 32) == {'hysteresis_low': None, 'close_radius2': None, 'fill_holes': 40,
                                                                          'open_radius2': None}
    assert check_cleanup_flags(0.3, None, 0, None, 'val', 8, 32)['hysteresis_low'] == 0.3
    for args in ((0.2, None, 0, None, 0.5, 8, 0), (None, 2, 0, None, 'argmax', 8, 0), (None, None, -1, None, 'argmax', 8, -1),
                 (None, None, 0, 4, 'argmax', 8, 0)):
        with pytest.raises(ValueError, match='--scene_stride N > 0'):
            check_cleanup_flags(*args)
    with pytest.raises(ValueError, match='--scene_threshold val|FLOAT'):
        check_cleanup_flags(0.2, None, 0, None, 'argmax', 8, 32)
    with pytest.raises(ValueError, match='hysteresis_low'):
        check_cleanup_flags(0.7, None, 0, None, 0.5, 8, 32)
    with pytest.raises(ValueError, match='scene_fill_holes'):
        check_cleanup_flags(None, None, -2, None, 'argmax', 8, 32)
    with pytest.raises(ValueError, match='radius2'):
        check_cleanup_flags(None, -1, 0, None, 'argmax', 8, 32)
    mask = np.array([[1, 1, 0], [0, 1, 0]], np.uint8)
    lab = np.array([[1, 0, 1], [255, 255, 0]], np.uint8)
    assert {k: cleaned_scores(mask, lab, 255)[k] for k in ('tp', 'fp', 'fn')} == {'tp': 1, 'fp': 1, 'fn': 1}
    assert {k: cleaned_scores(mask, lab)[k] for k in ('tp', 'fp', 'fn')} == {'tp': 2, 'fp': 1, 'fn': 2}


def test_cli_defaults_are_off():
    src = open(os.path.join(ROOT, 'fabric_amd', 'train.py')).read()
    for flag, default in (('--scene_hysteresis', 'None'), ('--scene_close', 'None'), ('--scene_fill_holes', '0'), ('--scene_open', 'None')):
        m = re.search(r"add_argument\('" + flag + r"', type=(\w+), default=(\w+)", src)
        assert m and m.group(2) == default, flag


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


@pytest.mark.parametrize('name,n_args', [('bdn_cc_mark', 8), ('bdn_cc_select', 11), ('bdn_d2_mask', 6), ('bdn_threshold_pair', 9),
                                         ('bdn_mask_not', 4)])
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
    sec = hdr[hdr.index('cleaning a scene mask'):hdr.index('int bdn_cc_mark(')]
    for cite in ('scipy.ndimage', 'device-to-host copy', 'train.py:199', name):
        assert cite in sec
    assert getattr(_lib.load(), name)
    assert 'morph.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()


_MARK = dict(labels=64, seed=128, seed_value=1, border=0, mark=256, H=4, W=4, stream=None)
_SELECT = dict(labels=64, mark=128, keep_marked=1, area=256, min_area=1, max_area=5, base=None, out=512, H=4, W=4, stream=None)
_D2 = dict(d2=64, r2=2, greater=0, out=128, n=16, stream=None)
_PAIR = dict(proba=64, pos_class=1, low=0.25, high=0.5, mask_low=128, mask_high=256, ncls=2, HW=16, stream=None)
_NOT = dict(src=64, out=128, n=16, stream=None)
_BAD_SHAPES = (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(H=1, W=(1 << 31) - 1), dict(H=46341, W=46341))
_NAN = float('nan')


@pytest.mark.parametrize('name,defaults,bad', [
    ('bdn_cc_mark', _MARK, _BAD_SHAPES + (dict(labels=None), dict(mark=None), dict(labels=66), dict(mark=258), dict(mark=64), dict(seed_value=256),
                                          dict(seed_value=-1))),
    ('bdn_cc_select', _SELECT, _BAD_SHAPES + (dict(labels=None), dict(out=None), dict(labels=66), dict(mark=130), dict(area=258), dict(keep_marked=2),
                                              dict(min_area=0), dict(min_area=6), dict(area=None), dict(area=None, min_area=2, max_area=(1 << 31) - 1))),
    ('bdn_d2_mask', _D2, (dict(d2=None), dict(out=None), dict(d2=66), dict(r2=-1), dict(greater=2), dict(n=0), dict(n=-4), dict(n=1 << 31))),
    ('bdn_threshold_pair', _PAIR, (dict(proba=None), dict(mask_low=None), dict(mask_high=None), dict(mask_high=128), dict(proba=66), dict(low=-0.1),
                                   dict(high=1.5), dict(low=0.6), dict(low=_NAN), dict(high=_NAN), dict(ncls=1), dict(ncls=257), dict(HW=0),
                                   dict(HW=(1 << 31) - 1), dict(pos_class=2), dict(pos_class=-1))),
    ('bdn_mask_not', _NOT, (dict(src=None), dict(out=None), dict(out=64), dict(n=0), dict(n=1 << 31))),
])
def test_c_entries_refuse_bad_arguments_before_any_launch(name, defaults, bad):
    lib = _lib.load()
    for over in bad:
        a = dict(defaults)
        a.update(over)
        rc = getattr(lib, name)(*a.values())
        assert rc == BDN_E_ARG, (name, over, rc, lib.bdn_last_error().decode())
