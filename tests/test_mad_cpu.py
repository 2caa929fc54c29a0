"""-m "not gpu": what IR-MAD pins without a device -- the declarations of the new entries against _lib.SIGNATURES, every argument check of
every new C entry (fake non-null pointers: BDN_E_ARG before anything touches a device), the workspace bound, the argument checks of
fabric_amd.utils.mad and of the new normalize_cities / CLI arguments, and the numpy twin the GPU tests compare with (tests/mad_ref.py):
against independent routes (scipy's generalised eigenproblem, scipy's regularised incomplete gamma function) and on the properties of the
method (convergence, identical dates, swapped dates, permuted and rescaled bands, what the centre is for)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg
import scipy.special
import torch

from fabric_amd import _lib
from fabric_amd.utils import mad as MAD
from fabric_amd.utils import radiometry as RM
from fabric_amd.utils.dataloaders import synthetic_onera
from tests import curve_ref as CR
from tests import mad_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
P = 0x1000                                                  # a fake non-null, 16-byte aligned pointer: never dereferenced


# ---------------------------------------------------------------- the C ABI without a device
def _ctype(p):
    if '*' in p:
        return ctypes.c_void_p
    return {'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'int': ctypes.c_int}[p.rsplit(' ', 1)[0].strip()]


ENTRIES = [('bdn_mad_workspace_bytes', 'size_t', 3), ('bdn_mad_centre', 'int', 13), ('bdn_mad_moments', 'int', 15), ('bdn_mad_solve', 'int', 9),
           ('bdn_mad_chi2', 'int', 14), ('bdn_mad_mask', 'int', 14)]


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
    assert 'mad.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()
    sec = hdr[hdr.index('IR-MAD, the iteratively reweighted'):hdr.index('size_t bdn_mad_workspace_bytes(')]
    for cite in ('no float atomics', 'n 2^-53 sum |term|', 'BDN_E_ARG before anything touches a device', '1e-12 times its original diagonal entry',
                 'no launch reads a flag that the same launch writes', 'changes no byte anywhere', 'bounded whatever the scene size'):
        assert cite in sec, cite
    for n in (1, 13, 32):
        assert MAD.state_doubles(n) == MR.state_doubles(n) == 7 + 6 * n + 2 * n * n
        assert MAD.moment_doubles(n) == MR.moment_doubles(n) == 1 + 2 * n + n * (2 * n + 1)
    assert '#define BDN_MAD_STATE_DOUBLES(n_b) (7 + 6 * (n_b) + 2 * (n_b) * (n_b))' in hdr and '#define BDN_MAD_STATE_RHO 7' in hdr
    assert (MAD.ST_ITER, MAD.ST_OK, MAD.ST_CONVERGED, MAD.ST_SKIP, MAD.ST_DELTA, MAD.ST_S0, MAD.ST_NVALID, MAD.ST_RHO) == tuple(range(8))


def _rc(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.bdn_last_error().decode()


def _bad(name, good, i, v, msg):
    a = list(good)
    a[i] = v
    rc, err = _rc(name, *a)
    assert rc == E_ARG and msg in err, (name, i, v, rc, err)


SCENE_BAD = ((3, 0, 'band indices'), (3, 33, 'band indices'), (0, P + 2, 'aligned'), (1, P + 1, 'aligned'), (2, P + 2, 'aligned'))


def _scene_checks(name, good, c_at):
    for i in (0, 1, 2):
        _bad(name, good, i, None, 'null pointer')
    for i, v, msg in SCENE_BAD + ((c_at, 0, 'bad scene'), (c_at, 65536, 'bad scene'), (c_at + 1, 0, 'bad scene'), (c_at + 1, 32768, 'bad scene'),
                                  (c_at + 2, -5, 'bad scene'), (c_at + 2, 32768, 'bad scene')):
        _bad(name, good, i, v, msg)
    for exv in (256, -1):
        a = list(good); a[4], a[5] = P, exv
        rc, err = _rc(name, *a)
        assert rc == E_ARG and 'exclude_value' in err


def test_argument_checks_of_every_entry():
    #       d1 d2 bands n_b excl exv centre n_valid ws C  H   W   stream
    good = [P, P, P, 3, None, 0, P, P, P, 3, 33, 65, None]
    _scene_checks('bdn_mad_centre', good, 9)
    for i in (6, 7, 8):
        _bad('bdn_mad_centre', good, i, None, 'null pointer')
    for i, v in ((6, P + 4), (7, P + 4), (8, P + 8)):
        _bad('bdn_mad_centre', good, i, v, 'aligned')
    #       d1 d2 bands n_b excl exv weight centre state moments ws C  H   W   stream
    good = [P, P, P, 3, None, 0, None, P, None, P, P, 3, 33, 65, None]
    _scene_checks('bdn_mad_moments', good, 11)
    for i in (7, 9, 10):
        _bad('bdn_mad_moments', good, i, None, 'null pointer')
    for i, v in ((6, P + 2), (7, P + 4), (8, P + 4), (9, P + 4), (10, P + 8)):
        _bad('bdn_mad_moments', good, i, v, 'aligned')
    #       moments centre n_valid n_b first tol min_var state stream
    good = [P, P, P, 3, 1, 1e-3, 1e-9, P, None]
    for i in (0, 1, 2, 7):
        _bad('bdn_mad_solve', good, i, None, 'null pointer')
        _bad('bdn_mad_solve', good, i, P + 4, 'aligned')
    for i, v, msg in ((3, 0, 'band indices'), (3, 33, 'band indices'), (4, 2, 'first'), (4, -1, 'first'), (5, -1e-3, 'tol'), (5, float('nan'), 'tol'),
                      (5, float('inf'), 'tol'), (6, 0.0, 'min_var'), (6, -1.0, 'min_var'), (6, float('nan'), 'min_var')):
        _bad('bdn_mad_solve', good, i, v, msg)
    #       d1 d2 bands n_b excl exv state chi2 proba variates C  H   W   stream
    good = [P, P, P, 3, None, 0, P, P, P, None, 3, 33, 65, None]
    _scene_checks('bdn_mad_chi2', good, 10)
    for i in (6, 7, 8):
        _bad('bdn_mad_chi2', good, i, None, 'null pointer')
    for i, v in ((6, P + 4), (7, P + 2), (8, P + 1), (9, P + 2)):
        _bad('bdn_mad_chi2', good, i, v, 'aligned')
    #       proba d1 d2 bands n_b excl exv thr out mask C  H   W   stream
    good = [P, P, P, P, 3, None, 0, 0.5, 0, P, 3, 33, 65, None]
    for i in (0, 1, 2, 3, 9):
        _bad('bdn_mad_mask', good, i, None, 'null pointer')
    for i, v, msg in ((4, 0, 'band indices'), (4, 33, 'band indices'), (7, -0.1, 'threshold'), (7, 1.5, 'threshold'), (7, float('nan'), 'threshold'),
                      (8, 256, 'excluded_out'), (8, -1, 'excluded_out'), (0, P + 2, 'aligned'), (10, 0, 'bad scene'), (12, 32768, 'bad scene')):
        _bad('bdn_mad_mask', good, i, v, msg)


def test_workspace_is_bounded_whatever_the_scene_size():
    q = _lib.load().bdn_mad_workspace_bytes
    per_block = lambda nb: 128 * ((2 * nb + 4) // 4) * ((2 * nb + 4) // 4 + 1) // 2      # 16 doubles per 4 x 4 tile on or above the diagonal
    assert per_block(13) == 28 * 128 and per_block(32) == 153 * 128
    for nb in (1, 2, 3, 13, 32):
        assert q(nb, 1, 1) == per_block(nb) and q(nb, 37, 53) == -(-37 * 53 // 64) * per_block(nb)
        assert q(nb, 10000, 10000) == q(nb, 32767, 32767) == q(nb, 256, 256) == 768 * per_block(nb) and q(nb, 97, 131) % 16 == 0
    assert q(13, 10000, 10000) == 2752512 and q(32, 32767, 32767) <= 15 << 20
    for args in ((0, 8, 8), (33, 8, 8), (1, 0, 8), (1, 8, 32768), (1, 32768, 8), (1, 8, -1)):
        assert q(*args) == 0, args


# ---------------------------------------------------------------- the Python surface without a device
def test_check_mad_args_on_meta_tensors():
    a = torch.empty(3, 33, 65, device='meta')
    ex = torch.empty(33, 65, dtype=torch.uint8, device='meta')
    assert MAD.check_mad_args(a, a) == (3, 33, 65, [0, 1, 2])
    assert MAD.check_mad_args(a, a, [2, 0], ex, 255, 5, 0, 1e-6, True) == (3, 33, 65, [2, 0])
    for kw, msg in ((dict(bands=[]), 'bands'), (dict(bands=[3]), 'bands'), (dict(bands=[1, 1]), 'twice'), (dict(bands='0'), 'bands'),
                    (dict(exclude=ex), 'exclude_value'), (dict(exclude=ex, exclude_value=256), 'exclude_value'),
                    (dict(exclude=ex.float(), exclude_value=0), 'exclude'), (dict(iters=0), 'iters'), (dict(iters=1001), 'iters'),
                    (dict(iters=2.0), 'iters'), (dict(iters=True), 'iters'), (dict(tol=-1e-3), 'tol'), (dict(tol=float('nan')), 'tol'),
                    (dict(tol='1e-3'), 'tol'), (dict(min_var=0), 'min_var'), (dict(min_var=-1.0), 'min_var'), (dict(min_var=float('inf')), 'min_var'),
                    (dict(variates=1), 'variates')):
        with pytest.raises(ValueError, match=msg):
            MAD.check_mad_args(a, a, **kw)
    for bad in (a.double(), a[0], a.permute(0, 2, 1), np.zeros((3, 33, 65), np.float32)):
        with pytest.raises(ValueError, match='d1'):
            MAD.check_mad_args(bad, a)
    with pytest.raises(ValueError, match='d2'):
        MAD.check_mad_args(a, torch.empty(3, 33, 64, device='meta'))
    with pytest.raises(ValueError, match='d2 is on'):
        MAD.check_mad_args(a, torch.zeros(3, 33, 65))
    with pytest.raises(ValueError, match='name a subset'):
        MAD.check_mad_args(torch.empty(33, 4, 4, device='meta'), torch.empty(33, 4, 4, device='meta'))
    with pytest.raises(ValueError, match='name a subset'):
        MAD.check_mad_args(torch.empty(40, 4, 4, device='meta'), torch.empty(40, 4, 4, device='meta'), bands=list(range(33)))
    assert MAD.check_mad_args(torch.empty(40, 4, 4, device='meta'), torch.empty(40, 4, 4, device='meta'), bands=[39, 0])[3] == [39, 0]
    c = torch.zeros(3, 33, 65)
    with pytest.raises(RuntimeError, match='no CPU path'):
        MAD.irmad(c, c)
    res = MAD.MadResult(torch.zeros(4, 5), torch.zeros(2, 4, 5), None, torch.zeros(MAD.state_doubles(1), dtype=torch.float64), c, c, None, [0], None, 0)
    for kw, msg in ((dict(threshold=1.5), 'threshold'), (dict(threshold=float('nan')), 'threshold'), (dict(excluded_out=256), 'excluded_out'),
                    (dict(out=torch.zeros(4, 5)), 'out'), (dict(out=torch.zeros(4, 6, dtype=torch.uint8)), 'out')):
        with pytest.raises(ValueError, match=msg):
            MAD.change_mask(res, **kw)
    with pytest.raises(ValueError, match='MadResult'):
        MAD.change_mask((c, c))
    with pytest.raises(RuntimeError, match='no CPU path'):
        MAD.change_mask(res)
    import fabric_amd.utils as U
    for name in ('irmad', 'change_mask', 'check_mad_args', 'MadResult'):
        assert getattr(U, name) is getattr(MAD, name)
    v = MR.pack_state(MR.solve_ref(*MR.moments_ref(*MR.scene(1, 2, 9, 11)[:2], [0, 1], np.zeros(4)), np.zeros(4), 99, 2), 2)
    rd = MAD.read_state(v, 2)
    st = MR.unpack_state(v, 2)
    assert set(rd) == {'rho', 'var', 'iters', 'converged', 'ok', 'delta', 'n_valid', 'a', 'b', 'mean'} and rd['iters'] == 1 and rd['ok'] is True
    assert all(np.array_equal(rd[k], st[k]) for k in ('rho', 'var', 'a', 'b', 'mean')) and rd['n_valid'] == 99 and rd['delta'] == np.inf


def test_normalize_cities_and_cli_flag_checks():
    for kw, msg in ((dict(invariant='labels'), 'invariant'), (dict(invariant='mad', invariant_min=0.0), 'invariant_min'),
                    (dict(invariant='mad', invariant_min=1.5), 'invariant_min'), (dict(invariant='mad', mad_iters=0), 'mad_iters'),
                    (dict(invariant='mad', mad_tol=-1.0), 'mad_tol')):
        with pytest.raises(ValueError, match=msg):
            RM.normalize_cities({}, **kw)
    assert RM.normalize_cities({}, invariant='mad') == {} and RM.normalize_cities({}) == {}
    assert RM.mad_line('x', {'mad': {'ok': True, 'iters': 3}}) == {'city': 'x', 'ok': True, 'iters': 3}
    from fabric_amd.train import check_mad_flags as chk
    radiom = dict(method='range', knots=256, lower=0.02, upper=0.98, bands=None)
    assert chk() == {} and chk(radiom=radiom, explicit=True) == {}
    on = dict(invariant='mad', invariant_min=0.95, mad_iters=30, mad_tol=1e-3)
    assert chk('mad', radiom=radiom, explicit=True) == on
    assert chk('mad', 5, 0.0, 0.5, radiom, explicit=True) == dict(invariant='mad', invariant_min=0.5, mad_iters=5, mad_tol=0.0)
    kept = dict(radiom, **dict(on, mad_iters=7))
    assert chk(radiom=radiom, checkpoint=kept) == dict(on, mad_iters=7) and chk(radiom=radiom, checkpoint=radiom) == {}
    assert chk(radiom=radiom, checkpoint=kept, explicit=True) == {}          # --radiometric given again: its own settings
    for args, kw, msg in ((('mad',), {}, 'add --radiometric'), ((None, 5), dict(radiom=radiom, explicit=True), 'add --radiometric_invariant mad'),
                          ((None, None, 1e-3), {}, 'add --radiometric_invariant mad'), ((None, None, None, 0.9), {}, 'add --radiometric_invariant mad'),
                          (('cva',), dict(radiom=radiom, explicit=True), '--radiometric_invariant cva'),
                          (('mad', 0), dict(radiom=radiom, explicit=True), '--mad_iters 0'), (('mad', 1001), dict(radiom=radiom, explicit=True), '--mad_iters'),
                          (('mad', None, -1.0), dict(radiom=radiom, explicit=True), '--mad_tol'), (('mad', None, float('nan')), dict(radiom=radiom, explicit=True), '--mad_tol'),
                          (('mad', None, None, 0.0), dict(radiom=radiom, explicit=True), '--mad_invariant_min'),
                          (('mad', None, None, 1.5), dict(radiom=radiom, explicit=True), '--mad_invariant_min'),
                          (('mad',), dict(radiom=dict(radiom, bands=list(range(33))), explicit=True), 'name a subset'),
                          (('mad',), dict(radiom=radiom, checkpoint=kept), 'add --radiometric'),
                          ((), dict(radiom=radiom, checkpoint=dict(kept, invariant='cva')), 'unknown')):
        with pytest.raises(ValueError, match=msg):
            chk(*args, **kw)
    for flags, msg in ((['--radiometric_invariant', 'mad'], 'add --radiometric'), (['--mad_iters', '5'], 'add --radiometric_invariant mad'),
                       (['--radiometric', 'none', '--radiometric_invariant', 'mad'], 'add --radiometric')):
        r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1'] + flags,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and msg in r.stderr, r.stderr[-500:]


# ---------------------------------------------------------------- the twin against independent routes
@pytest.mark.parametrize('nb,weighted', [(1, False), (3, False), (3, True), (13, True)])
def test_rho_against_the_generalised_eigenproblem(nb, weighted):
    d1, d2, _ = MR.scene(20 + nb, nb, 37, 53)
    bands = list(range(nb))
    cen, n = MR.centre_ref(d1, d2, bands)
    w = np.random.default_rng(nb).random((37, 53)).astype(np.float32) if weighted else None
    s0, s1, s2 = MR.moments_ref(d1, d2, bands, cen, w)
    st = MR.solve_ref(s0, s1, s2, cen, n, nb)
    # an independent route: the weighted covariance by numpy, and Sxy Syy^-1 Syx a = rho^2 Sxx a by LAPACK's generalised symmetric solver
    v = MR.pixels(d1, d2, bands, np.ones((37, 53), bool))
    cov = np.cov(v.T, aweights=None if w is None else w.reshape(-1).astype(np.float64), bias=True).reshape(2 * nb, 2 * nb)
    sxx, sxy, syy = cov[:nb, :nb], cov[:nb, nb:], cov[nb:, nb:]
    lam = scipy.linalg.eigh(sxy @ np.linalg.solve(syy, sxy.T), sxx, eigvals_only=True)[::-1]
    err = np.abs(st['rho'] - np.sqrt(lam)).max()
    print(f'n_b = {nb}: largest |rho - sqrt(lambda)| = {err:.3g}')
    assert st['ok'] == 1 and err <= 1e-10 and (np.diff(st['rho']) <= 0).all()
    a, b = st['a'], st['b']
    assert np.abs(a @ sxx @ a.T - np.eye(nb)).max() < 1e-9 and np.abs(b @ syy @ b.T - np.eye(nb)).max() < 1e-9
    assert np.abs(a @ sxy @ b.T - np.diag(st['rho'])).max() < 1e-9
    assert (((sxx @ a.T) / np.sqrt(np.diag(sxx))[:, None]).sum(0) >= 0).all()             # the sign rule
    assert np.allclose(st['mean'], np.average(v, axis=0, weights=None if w is None else w.reshape(-1)), rtol=0, atol=1e-12)


@pytest.mark.parametrize('nb', [1, 2, 3, 13, 32])
def test_q_against_gammaincc(nb):
    """1e-12 relative wherever the tail is a normal double (>= 1e-300); below that both underflow and the absolute difference is checked."""
    r = np.random.default_rng(nb)
    chi2 = np.concatenate([[0.0, 1e8], np.logspace(-12, 8, 2001), r.uniform(0, 200, 2000), r.uniform(0, 4000, 2000)])
    q, want = MR.q_ref(nb, chi2), scipy.special.gammaincc(nb / 2.0, chi2 / 2.0)
    normal = want >= 1e-300
    err = np.abs(q[normal] - want[normal]) / want[normal]
    print(f'n_b = {nb}: largest relative error {err.max():.3g} over {int(normal.sum())} points; below 1e-300: {np.abs(q[~normal] - want[~normal]).max():.3g}')
    assert err.max() <= 1e-12 and np.abs(q[~normal] - want[~normal]).max() <= 1e-300
    assert q[0] == 1.0 and q[1] == 0.0 and (q <= 1).all() and (q >= 0).all() and (~normal).sum() > 100
    assert np.isnan(MR.q_ref(nb, np.nan)) and MR.q_ref(nb, np.inf) == 0.0


# ---------------------------------------------------------------- the properties of the method, on the twin
def test_convergence_and_the_flag_protocol():
    d1, d2, changed = MR.scene(3, 3, 37, 53)
    r = MR.irmad_ref(d1, d2, [0, 1, 2], iters=30, tol=1e-3)
    st = r['state']
    print(f'deltas {["%.3g" % d for d in r["deltas"]]}')
    assert st['ok'] == 1 and st['converged'] == 1 and st['skip'] == 1 and st['iter'] == len(r['deltas']) < 30 and r['deltas'][-1] < 1e-3
    assert r['deltas'][0] == np.inf and all(d >= 1e-3 for d in r['deltas'][:-1])
    again = MR.irmad_ref(d1, d2, [0, 1, 2], iters=st['iter'], tol=1e-3)             # the launches after the stop changed nothing
    assert all(np.array_equal(r[k], again[k], equal_nan=True) for k in ('chi2', 'proba', 'variates')) and again['state']['skip'] == 0
    assert r['proba'][1][changed].mean() > 0.99 and r['proba'].dtype == np.float32 and np.array_equal(r['proba'][0] + r['proba'][1] > 0.999, np.ones((37, 53), bool))
    free = MR.irmad_ref(d1, d2, [0, 1, 2], iters=8, tol=0.0)
    assert free['state']['iter'] == 8 and free['state']['converged'] == 0


def test_identical_dates():
    d1, _, _ = MR.scene(13, 13, 37, 53)
    r = MR.irmad_ref(d1, d1.copy(), list(range(13)), iters=3, tol=0.0)
    assert r['state']['ok'] == 1 and np.abs(1 - r['state']['rho']).max() <= 1e-10 and r['chi2_64'].max() <= 1e-12 and (r['proba'][0] == 1).all()
    assert not MR.mask_ref(r['proba'][0], r['valid'], 0.01).any()


def test_swapped_dates_permuted_bands_and_gains_of_two():
    d1, d2, _ = MR.scene(3, 3, 37, 53)
    base = MR.irmad_ref(d1, d2, [0, 1, 2], iters=6, tol=0.0)
    gains = np.array([2.0, 0.5, 8.0], np.float32)[:, None, None]
    for name, other in (('swapped', MR.irmad_ref(d2, d1, [0, 1, 2], iters=6, tol=0.0)),
                        ('permuted, scaled', MR.irmad_ref(d1, d2 * gains, [2, 0, 1], iters=6, tol=0.0))):
        rel = np.abs(other['chi2_64'] - base['chi2_64']) / base['chi2_64']
        print(f'{name}: chi2 moves by {rel.max():.3g} relative, rho by {np.abs(other["state"]["rho"] - base["state"]["rho"]).max():.3g}')
        assert rel.max() <= 1e-10 and np.abs(other['state']['rho'] - base['state']['rho']).max() <= 1e-10


def test_failures_and_invalid_pixels():
    d1, d2, _ = MR.scene(3, 3, 37, 53)
    const = d2.copy()
    const[1] = 4.25
    for a, b, ex in ((d1, const, None), (d1, d2, np.full((37, 53), 9, np.uint8)), (d1[:, :1, :1], d2[:, :1, :1], None)):
        r = MR.irmad_ref(a, b, [0, 1, 2], ex, 9, iters=3, tol=0.0)
        assert (r['state']['ok'], r['state']['converged'], r['state']['iter'], r['state']['skip']) == (0, 1, 1, 1)
        assert np.isnan(r['chi2']).all() and np.isnan(r['proba']).all() and not MR.mask_ref(r['proba'][0], np.ones(r['chi2'].shape, bool), 0.5).any()
    assert MR.centre_ref(d1, d2, [0, 3])[1] == 0
    bad = d2.copy()
    bad[1, 0, :3] = [np.nan, np.inf, -np.inf]
    r = MR.irmad_ref(d1, bad, [0, 1, 2], iters=2, tol=0.0)
    assert (~r['valid']).sum() == 3 and (r['chi2'][0, :3] == 0).all() and (r['proba'][0][0, :3] == 1).all() and (r['proba'][1][0, :3] == 0).all()
    assert MR.mask_ref(r['proba'][0], r['valid'], 0.95, 7)[0, :3].tolist() == [7, 7, 7]


def test_what_the_centre_is_for():
    """Raw second moments of data with an offset of 1000 and unit spread lose about 1e6 * 2^-53 of the covariance; centred ones do not."""
    d1, d2, _ = MR.scene(10, 3, 37, 53, offset=1000.0)
    bands = [0, 1, 2]
    cen, n = MR.centre_ref(d1, d2, bands)
    v = MR.pixels(d1, d2, bands, np.ones((37, 53), bool))
    exact = np.cov(v.T, bias=True)
    err = {}
    for name, c in (('raw', np.zeros(6)), ('centred', cen)):
        s0, s1, s2 = MR.moments_ref(d1, d2, bands, c)
        mz = s1 / s0
        err[name] = np.abs((s2 / s0 - np.outer(mz, mz)) - exact).max() / np.abs(exact).max()
    print(f'covariance error: raw moments {err["raw"]:.3g}, centred {err["centred"]:.3g}')
    assert err['raw'] > 100 * err['centred'] and err['centred'] < 1e-13


def test_the_twin_separates_a_synthetic_city_with_a_planted_gain_and_bias():
    """The unsupervised baseline: on a synthetic city whose date 2 carries a gain and a bias, the twin's change probability alone reaches an
    average precision of 0.95 against the labels (the score curve of tests/curve_ref.py, 1024 bins) -- the city and the run
    tests/test_gpu_mad_api.py feeds to ScoreCurve (mad_ref.AP_CITY).  That run is iters = 1, the MAD transform without reweighting.  What
    the reweighting does to this figure is measured here as well: it sharpens the ORDER of chi2 until the labels
    are separated perfectly, but the weights, uniform on unchanged pixels, shrink the weighted variances, chi2 of unchanged pixels grows
    (median 2.8 -> 9.8 at 4 degrees of freedom) and a sixth of them reach the last of the 1024 bins of 1 - Q, where the changed ones sit:
    the average precision of the BINNED probability falls although the statistic improved."""
    city = synthetic_onera(**MR.AP_CITY)['city0']
    lab = city['labels']

    def ap_by_rank(score):                                   # the average precision of the exact order, no bins
        hit = lab.reshape(-1)[np.argsort(-score.reshape(-1), kind='stable')] == 1
        return float((np.cumsum(hit) / np.arange(1, hit.size + 1) * hit).sum() / hit.sum())

    r = MR.irmad_ref(city['images'][0], city['images'][1], [0, 1, 2, 3], **MR.AP_RUN)
    ap = CR.summary(CR.histogram(r['proba'][1], lab, 1024))['AP']
    full = MR.irmad_ref(city['images'][0], city['images'][1], [0, 1, 2, 3], iters=30, tol=1e-3)
    ap_full = CR.summary(CR.histogram(full['proba'][1], lab, 1024))['AP']
    print(f'AP of the twin: {ap:.4f} at iters = 1 (by rank {ap_by_rank(r["chi2_64"]):.4f}); converged after {full["state"]["iter"]} iterations: '
          f'{ap_full:.4f} binned, {ap_by_rank(full["chi2_64"]):.4f} by rank')
    assert r['state']['ok'] == 1 and ap >= 0.95
    assert full['state']['converged'] == 1 and ap_by_rank(full['chi2_64']) >= 0.999 > ap_by_rank(r['chi2_64'])
