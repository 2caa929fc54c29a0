"""-m "not gpu": what the distance transform, the boundary loss and the boundary scores pin without a device -- the reference of the GPU
tests (tests/edt_ref.py) against scipy and a brute force, the boundary definition, the declarations of the new entries against
_lib.SIGNATURES, every argument check of every new C entry (fake non-null pointers: BDN_E_ARG before anything touches a device), the
Criterion's validation / repr / parse, the argument checks of fabric_amd.utils.distance and the CLI flag checks."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd import criterion as CR
from fabric_amd.criterion import Criterion
from fabric_amd.utils import distance as D
from tests import edt_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 5), (5, 1), (7, 13), (33, 65)]
E_ARG = -1
P = 0x1000                                                  # a fake non-null, 16-byte aligned pointer: never dereferenced


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_is_scipy_and_brute_force(shape):
    from scipy import ndimage
    h, w = shape
    for name in ER.PATTERNS:
        site = ER.pattern(name, h, w) == 1
        brute = ER.d2_brute(site)
        assert np.array_equal(ER.d2_ref(site), brute), name
        if site.any():
            assert np.array_equal(brute, np.rint(ndimage.distance_transform_edt(~site) ** 2).astype(np.int64)), name
            assert (brute[site] == 0).all()
        else:
            assert (brute == ER.LIMIT).all()
        for limit in (1, 5, 26):
            assert np.array_equal(ER.d2_ref(site, limit), np.minimum(brute, limit))
    src = ER.pattern('rand50', h, w)
    valid = np.where(np.random.default_rng(1).random((h, w)) < 0.3, 7, 0).astype(np.uint8)
    s = ER.sites(src, 1, False, valid, 7)
    assert np.array_equal(s, (src != 1) & (valid != 7))


def test_float32_sqrt_of_the_integers_is_the_rounded_float64_sqrt():
    n = np.arange(0, 2 * 128 * 128 + 1, dtype=np.int64)
    assert np.array_equal(np.sqrt(n.astype(np.float32)), np.sqrt(n.astype(np.float64)).astype(np.float32))


def test_phi_is_kervadecs_one_hot2dist():
    from scipy import ndimage
    r = np.random.default_rng(0)
    lab = (r.random((33, 65)) < 0.5).astype(np.uint8)
    lab = np.repeat(np.repeat(lab[:9, :17], 4, axis=0), 4, axis=1)[:33, :65]
    pos = lab == 1
    # one_hot2dist: distance(negmask) * negmask - (distance(posmask) - 1) * posmask, the distances rounded to float32 first as the kernel has them
    d_neg, d_pos = (ndimage.distance_transform_edt(m).astype(np.float32) for m in (~pos, pos))
    want = d_neg * ~pos - (d_pos - np.float32(1)) * pos
    assert want.dtype == np.float32 and np.array_equal(ER.phi_ref(lab, 1), want)
    assert np.array_equal(ER.phi_ref(lab, 1, max_dist=3), np.clip(want, -3, 3))
    assert not ER.phi_ref(np.zeros((5, 7), np.uint8), 1).any() and not ER.phi_ref(np.ones((5, 7), np.uint8), 1).any()
    ign = lab.copy()
    ign[:, 30:40] = 255
    phi = ER.phi_ref(ign, 1, ignore=255)
    assert not phi[:, 30:40].any() and phi[:, :30].any()
    # the float64 term: gradient against a central difference
    lg = r.standard_normal((1, 2, 33, 65))
    t, g, _ = ER.boundary_loss_ref(lg, ign[None], 255, True, None)
    d = r.standard_normal(lg.shape) * (ign != 255)
    num = (ER.boundary_loss_ref(lg + 1e-6 * d, ign[None], 255, True)[0] - ER.boundary_loss_ref(lg - 1e-6 * d, ign[None], 255, True)[0]) / 2e-6
    assert abs(num - (g * d).sum()) <= 1e-7 * max(1.0, abs(num))


def test_boundary_definition():
    sq = np.zeros((9, 11), bool)
    sq[2:7, 3:9] = True
    valid = np.ones_like(sq)
    ring = sq.copy()
    ring[3:6, 4:8] = False
    assert np.array_equal(ER.boundary_ref(sq, valid), ring)
    assert not ER.boundary_ref(np.ones((5, 7), bool), np.ones((5, 7), bool)).any()          # the image edge makes no contour
    half = np.zeros((6, 8), bool)
    half[:, :4] = True
    v = np.ones_like(half)
    v[:, 4:] = False                                         # everything that is not foreground is ignored: no contour
    assert not ER.boundary_ref(half, v).any()
    v[:, 4:] = True
    assert np.array_equal(np.nonzero(ER.boundary_ref(half, v).any(axis=0))[0], [3])
    s = ER.boundary_scores_ref(sq.astype(np.uint8), sq.astype(np.uint8), 0)
    assert s['boundary_f1'] == 1.0 and s['hausdorff'] == 0.0 and s['n_pred'] == int(ring.sum())
    e = ER.boundary_scores_ref(np.zeros((9, 11), np.uint8), sq.astype(np.uint8), 2)
    assert e['boundary_f1'] == 0.0 and e['hausdorff'] is None and e['hd2_pred_to_true'] == -1
    assert D.scores_from_counts([s[k] for k in ('n_pred', 'n_true', 'pred_hit', 'true_hit', 'hd2_pred_to_true', 'hd2_true_to_pred')], 0) == s


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


ENTRIES = [('bdn_edt_workspace_bytes', 'size_t', 3), ('bdn_edt', 'int', 12), ('bdn_boundary_workspace_bytes', 'size_t', 4),
           ('bdn_boundary_loss', 'int', 17), ('bdn_signed_distance_workspace_bytes', 'size_t', 3), ('bdn_signed_distance', 'int', 10),
           ('bdn_boundary_mask', 'int', 8), ('bdn_boundary_score', 'int', 7)]


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
    assert 'edt.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()
    sec = hdr[hdr.index('exact squared Euclidean distance transform'):hdr.index('size_t bdn_edt_workspace_bytes(')]
    for cite in ('Kervadec', 'Meijster', 'binary_erosion', 'no float atomics', 'BDN_E_ARG before anything touches a device'):
        assert cite in sec


def _rc(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.bdn_last_error().decode()


def test_edt_argument_checks():
    lib = _lib.load()
    good = [P, 1, 1, None, 0, 5, P, P, 1, 8, 8, None]

    def bad(i, v, msg):
        a = list(good)
        a[i] = v
        rc, err = _rc('bdn_edt', *a)
        assert rc == E_ARG and msg in err, (i, v, rc, err)
    for i in (0, 6, 7):
        bad(i, None, 'null pointer')
    bad(5, 0, 'limit'); bad(5, -3, 'limit')
    bad(1, -1, 'site_value'); bad(1, 256, 'site_value'); bad(2, 2, 'site_equal')
    bad(8, 0, 'bad shape'); bad(9, -1, 'bad shape'); bad(10, 0, 'bad shape'); bad(9, 32768, 'bad shape'); bad(10, 32768, 'bad shape')
    a = list(good); a[8], a[9] = 70000, 32767                # N * H * W beyond 2^31
    assert _rc('bdn_edt', *a)[0] == E_ARG
    bad(7, P + 4, 'aligned'); bad(6, P + 2, 'aligned')
    a = list(good); a[3], a[4] = P, 256
    assert _rc('bdn_edt', *a)[0] == E_ARG and 'invalid_value' in lib.bdn_last_error().decode()
    assert lib.bdn_edt_workspace_bytes(1, 8, 8) == 128 and lib.bdn_edt_workspace_bytes(3, 130, 257) >= 6 * 3 * 130 * 257
    assert lib.bdn_edt_workspace_bytes(2, 64, 128) == 2 * 2 * 64 * 128              # up to 128 wide: no stack in the workspace
    for shape in ((0, 8, 8), (1, 32768, 8), (1, 8, 32768), (1, -1, 8), (3, 32767, 32767)):
        assert lib.bdn_edt_workspace_bytes(*shape) == 0


def test_boundary_loss_argument_checks():
    lib = _lib.load()
    good = [P, P, -1, 0, 0.0, 1.0, 0, P, P, None, None, None, 2, 2, 8, 8, None]

    def bad(i, v, msg):
        a = list(good)
        a[i] = v
        rc, err = _rc('bdn_boundary_loss', *a)
        assert rc == E_ARG and msg in err, (i, v, rc, err)
    for i in (0, 1, 7, 8):
        bad(i, None, 'null pointer')
    bad(2, -2, 'ignore_label'); bad(2, 256, 'ignore_label')
    bad(5, -0.5, 'negative weight'); bad(5, float('nan'), 'negative weight')
    bad(4, -1.0, 'negative max_dist'); bad(4, float('nan'), 'negative max_dist')
    bad(13, 1, 'ncls'); bad(13, 9, 'ncls')
    bad(12, 0, 'bad shape'); bad(14, -8, 'bad shape'); bad(15, 0, 'bad shape'); bad(14, 32768, 'bad shape'); bad(12, 1 << 24, 'bad shape')
    bad(7, P + 8, 'aligned')
    assert lib.bdn_boundary_workspace_bytes(2, 2, 8, 8) > 0 and lib.bdn_boundary_workspace_bytes(2, 2, 8, 8) % 16 == 0
    for shape in ((2, 1, 8, 8), (2, 9, 8, 8), (0, 2, 8, 8), (2, 2, 32768, 8), (1 << 24, 2, 8, 8)):
        assert lib.bdn_boundary_workspace_bytes(*shape) == 0


def test_signed_distance_and_score_argument_checks():
    lib = _lib.load()
    good = [P, 1, -1, 0.0, P, P, 1, 8, 8, None]

    def bad(name, good, i, v, msg):
        a = list(good)
        a[i] = v
        rc, err = _rc(name, *a)
        assert rc == E_ARG and msg in err, (name, i, v, rc, err)
    for i in (0, 4, 5):
        bad('bdn_signed_distance', good, i, None, 'null pointer')
    for i, v, msg in ((1, -1, 'cls'), (1, 256, 'cls'), (2, 300, 'ignore_label'), (3, -1.0, 'max_dist'), (6, 0, 'bad shape'), (7, 32768, 'bad shape'),
                      (8, -1, 'bad shape'), (4, P + 4, 'aligned')):
        bad('bdn_signed_distance', good, i, v, msg)
    assert lib.bdn_signed_distance_workspace_bytes(1, 8, 8) > 0 and lib.bdn_signed_distance_workspace_bytes(1, 8, 40000) == 0
    gm = [P, 1, None, 0, P, 8, 8, None]
    for i in (0, 4):
        bad('bdn_boundary_mask', gm, i, None, 'null pointer')
    for i, v, msg in ((1, 256, 'fg_value'), (5, 0, 'bad shape'), (6, 32768, 'bad shape')):
        bad('bdn_boundary_mask', gm, i, v, msg)
    a = list(gm); a[2], a[3] = P, -1
    assert _rc('bdn_boundary_mask', *a)[0] == E_ARG
    gs = [P, P, 4, P, 8, 8, None]
    for i in (0, 1, 3):
        bad('bdn_boundary_score', gs, i, None, 'null pointer')
    for i, v, msg in ((2, -1, 'tolerance'), (4, 0, 'bad shape'), (5, 32768, 'bad shape'), (3, P + 4, 'aligned')):
        bad('bdn_boundary_score', gs, i, v, msg)


# ---------------------------------------------------------------- the Python surface without a device
def test_check_edt_args():
    m = torch.zeros(5, 7, dtype=torch.uint8)
    assert D.check_edt_args(m) == (1, 5, 7, D.LIMIT_NONE) and D.check_edt_args(m[None].contiguous(), max_dist=3) == (1, 5, 7, 10)
    assert D.check_edt_args(m, max_dist=0)[3] == 1
    for kw, msg in ((dict(site_value=256), 'site_value'), (dict(equal=1), 'equal'), (dict(max_dist=-1), 'max_dist'), (dict(max_dist=2.5), 'max_dist'),
                    (dict(max_dist=46340), 'max_dist'), (dict(valid=m), 'invalid_value'), (dict(valid=m.float(), invalid_value=0), 'valid'),
                    (dict(valid=m[:4].contiguous(), invalid_value=0), 'valid'), (dict(out=m), 'out'),
                    (dict(out=torch.zeros(5, 8, dtype=torch.int32)), 'out')):
        with pytest.raises(ValueError, match=msg):
            D.check_edt_args(m, **kw)
    for bad in (m.float(), m[0], m.t(), torch.zeros(0, 3, dtype=torch.uint8), np.zeros((5, 7), np.uint8)):
        with pytest.raises(ValueError, match='mask'):
            D.check_edt_args(bad)
    with pytest.raises(RuntimeError, match='no CPU path'):
        D.distance_transform_sq(m)
    with pytest.raises(RuntimeError, match='no CPU path'):
        D.signed_distance(m, 1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        D.boundary_scores(m, m)
    for kw, msg in ((dict(cls=256), 'cls'), (dict(cls=1, ignore_index=-1), 'ignore_index'), (dict(cls=1, max_dist=0), 'max_dist')):
        with pytest.raises(ValueError, match=msg):
            D.check_signed_distance_args(m, **kw)
    assert D.check_boundary_args(m, m, 2, 1, 255) == (5, 7)
    for args, msg in (((m, m, -1), 'tolerance'), ((m, m, 1.5), 'tolerance'), ((m, m[:4].contiguous()), 'truth'), ((m, m, 2, 300), 'pos_class'),
                      ((m, m, 2, 1, 256), 'ignore_index'), ((m.int(), m), 'pred_mask')):
        with pytest.raises(ValueError, match=msg):
            D.check_boundary_args(*args)
    import fabric_amd.utils as U
    for name in ('distance_transform_sq', 'signed_distance', 'boundary_scores', 'check_edt_args'):
        assert getattr(U, name) is getattr(D, name)


def test_criterion_validation_repr_and_parse():
    assert CR.NAMES == ('tversky', 'dice', 'jaccard', 'focal', 'focal+tversky', 'focal+dice', 'focal+jaccard')
    assert CR.COMPOUND == ('focal+tversky', 'focal+dice', 'focal+jaccard') and CR.LOVASZ_NAMES == ('lovasz', 'focal+lovasz')
    assert CR.BOUNDARY_CLASSES == {'foreground': 0, 'all': 1}
    c = Criterion()
    assert c.w_boundary == 0.0 and c.boundary_classes == 'foreground' and c.boundary_max_dist is None and 'boundary' not in repr(c)
    assert repr(Criterion(w_boundary=0.0)) == repr(c) and not Criterion(w_boundary=0.0)._addon_only
    c = Criterion(w_focal=1.0, w_boundary=0.01, boundary_classes='all', boundary_max_dist=20)
    assert "w_boundary=0.01, boundary_classes='all', boundary_max_dist=20.0" in repr(c) and not c._addon_only and not c._lovasz_only
    c.w_boundary = 0.5
    assert c.w_boundary == 0.5 and 'w_boundary=0.5' in repr(c)
    c.w_boundary = 0.0                                       # the pass stays (weight 0): the buffers were sized for it
    assert c.has_boundary and 'w_boundary=0.0' in repr(c)
    with pytest.raises(ValueError, match='w_boundary'):
        c.w_boundary = -1.0
    with pytest.raises(ValueError, match='built with w_boundary > 0'):
        Criterion().w_boundary = 0.1
    for kw, msg in ((dict(w_boundary=-0.1), 'w_boundary'), (dict(w_boundary=float('nan')), 'w_boundary'),
                    (dict(w_boundary=1.0, boundary_classes='present'), 'boundary_classes'), (dict(w_boundary=1.0, boundary_max_dist=0), 'boundary_max_dist'),
                    (dict(w_boundary=1.0, boundary_max_dist=-2.0), 'boundary_max_dist'), (dict(w_boundary=1.0, boundary_max_dist=True), 'boundary_max_dist'),
                    (dict(w_overlap=0.0), 'zero')):
        with pytest.raises(ValueError, match=msg):
            Criterion(**kw)
    only = Criterion(w_overlap=0.0, w_boundary=1.0)
    assert only._addon_only and not only._lovasz_only
    both = Criterion(w_overlap=0.0, w_lovasz=1.0, w_boundary=1.0)
    assert both._addon_only and not both._lovasz_only and Criterion(w_overlap=0.0, w_lovasz=1.0)._lovasz_only
    p = Criterion.parse('focal+dice', focal_gamma=2.0, w_boundary=0.01, boundary_classes='all', boundary_max_dist=20)
    assert (p.w_focal, p.w_overlap, p.w_boundary, p.boundary_classes, p.boundary_max_dist) == (1.0, 1.0, 0.01, 'all', 20.0)
    p = Criterion.parse('focal+lovasz', w_boundary=0.1)
    assert p.w_lovasz == 1.0 and p.w_boundary == 0.1 and p.boundary_classes == 'foreground'
    assert repr(Criterion.parse('jaccard')) == repr(Criterion.parse('jaccard', w_boundary=0.0, boundary_classes='all'))
    assert not Criterion.parse('jaccard').has_boundary and Criterion.parse('jaccard', w_boundary=0.1).has_boundary
    for name in ('jaccard', 'focal+lovasz'):                 # parse validates the boundary options at any weight, as the constructor does
        for kw, msg in ((dict(boundary_classes='bogus'), 'boundary_classes'), (dict(boundary_max_dist=-1), 'boundary_max_dist')):
            with pytest.raises(ValueError, match=msg):
                Criterion.parse(name, w_boundary=0, **kw)
    from types import SimpleNamespace
    from fabric_amd.utils.helpers import criterion_from_opt
    o = SimpleNamespace(loss_function='focal+dice', focal_gamma=2.0, boundary_weight=0.01, boundary_classes='all', boundary_max_dist=20.0)
    assert criterion_from_opt(o).w_boundary == 0.01 and criterion_from_opt(o).boundary_max_dist == 20.0
    assert repr(criterion_from_opt(SimpleNamespace(loss_function='dice'))) == repr(Criterion.parse('dice'))
    import inspect
    assert inspect.signature(Criterion.evaluate).parameters['phi'].default is None


def test_cli_boundary_flag_checks():
    from fabric_amd.train import check_boundary_flags as chk
    assert chk(None, 'foreground', None, False, None, 0) is None and chk(0.01, 'all', 20.0, True, None, 0) is None
    assert chk(None, 'foreground', None, False, 2, 64) == 2 and chk(0.01, 'foreground', None, True, 0, 16) == 0
    for args, msg in (((0.01, 'foreground', None, False, None, 0), '--fused_step true'), ((0.0, 'foreground', None, True, None, 0), 'weight > 0'),
                      ((-1.0, 'foreground', None, True, None, 0), 'weight > 0'), ((None, 'all', None, True, None, 0), 'add --boundary_weight'),
                      ((None, 'foreground', 5.0, True, None, 0), 'add --boundary_weight'), ((0.1, 'foreground', 0.0, True, None, 0), 'boundary_max_dist'),
                      ((0.1, 'some', None, True, None, 0), 'boundary_classes'), ((None, 'foreground', None, False, 2, 0), '--scene_stride N > 0'),
                      ((None, 'foreground', None, False, -1, 16), 'scene_boundary_tol'), ((None, 'foreground', None, False, 40000, 16), 'scene_boundary_tol')):
        with pytest.raises(ValueError, match=msg):
            chk(*args)
    for flags, msg in ((['--boundary_weight', '0.01'], '--fused_step true'), (['--scene_boundary_tol', '2'], '--scene_stride N > 0')):
        r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1'] + flags,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and msg in r.stderr, r.stderr[-500:]
