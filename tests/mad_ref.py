"""The float64 numpy twin of the IR-MAD entries (include/bidate_hip.h: bdn_mad_centre / _moments / _solve / _chi2 / _mask), written as the
header specifies them.  Sums are numpy's (pairwise) float64 sums, the SVD is LAPACK's: the device's reduction tree and Jacobi sweeps
legitimately differ, so the GPU tests compare within bounds, not bit for bit.  What is rounded to float32 on the device (chi2, proba,
variates, and with proba the weights between iterations) is rounded here in the same place."""
import math

import numpy as np

try:
    from scipy.special import erfc as _erfc
except ImportError:                                          # pragma: no cover
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])

ITER, OK, CONVERGED, SKIP, DELTA, S0, NVALID, RHO = range(8)
# the synthetic_onera city (a planted gain and bias on date 2) and the run on which the twin alone reaches AP >= 0.95 (tests/test_mad_cpu.py)
AP_CITY = dict(n_cities=1, bands=4, size=(97, 131), seed=1, radiometry=(1.3, 0.2))
AP_RUN = dict(iters=1, tol=1e-3)
FLT_MAX = float(np.finfo(np.float32).max)


def state_doubles(nb):
    return 7 + 6 * nb + 2 * nb * nb


def moment_doubles(nb):
    return 1 + 2 * nb + nb * (2 * nb + 1)


def valid_mask(d1, d2, bands, exclude=None, exclude_value=None):
    """bool [H,W]: all 2 n_b selected values finite and exclude != exclude_value; a band index outside the stack: nothing is valid."""
    c, h, w = d1.shape
    if any(not 0 <= b < c for b in bands):
        return np.zeros((h, w), bool)
    v = np.isfinite(d1[bands]).all(0) & np.isfinite(d2[bands]).all(0)
    if exclude is not None:
        v &= exclude != exclude_value
    return v


def pixels(d1, d2, bands, valid):
    """float64 [n, 2 n_b]: the vectors (x, y) of the valid pixels, in raster order."""
    if not valid.any():
        return np.zeros((0, 2 * len(bands)))
    return np.concatenate([d1[bands][:, valid], d2[bands][:, valid]]).astype(np.float64).T


def centre_ref(d1, d2, bands, exclude=None, exclude_value=None, with_abs=False):
    """(centre float64 [2 n_b], n_valid[, sum |value| per column])."""
    valid = valid_mask(d1, d2, bands, exclude, exclude_value)
    v = pixels(d1, d2, bands, valid)
    n = v.shape[0]
    cen = v.sum(0) / n if n else np.zeros(2 * len(bands))
    return (cen, n, np.abs(v).sum(0)) if with_abs else (cen, n)


def clean_weight(weight, shape):
    if weight is None:
        return np.ones(shape, np.float64)
    w = np.asarray(weight, np.float32)
    return np.where((w >= 0) & (w <= np.float32(FLT_MAX)), w, np.float32(0)).astype(np.float64)


def moments_ref(d1, d2, bands, centre, weight=None, exclude=None, exclude_value=None, with_abs=False):
    """(S0, S1 [D], S2 [D,D] full symmetric[, (A0, A1, A2) = the sums of the absolute terms, n]) over the valid pixels; the terms are
    fl(w z_k) z_l as on the device."""
    valid = valid_mask(d1, d2, bands, exclude, exclude_value)
    z = pixels(d1, d2, bands, valid) - np.asarray(centre, np.float64)[None, :]
    w = clean_weight(weight, valid.shape)[valid]
    wz = w[:, None] * z
    s0, s1, s2 = w.sum(), wz.sum(0), wz.T @ z
    s2 = np.triu(s2) + np.triu(s2, 1).T                     # entry (k, l), k <= l, is the one the device forms
    if not with_abs:
        return s0, s1, s2
    a2 = np.abs(wz).T @ np.abs(z)
    return s0, s1, s2, (np.abs(w).sum(), np.abs(wz).sum(0), np.triu(a2) + np.triu(a2, 1).T), int(valid.sum())


def pack_moments(s0, s1, s2):
    d = len(s1)
    return np.concatenate([[s0], s1, s2[np.triu_indices(d)]])


def unpack_moments(m, nb):
    d = 2 * nb
    s2 = np.zeros((d, d))
    s2[np.triu_indices(d)] = m[1 + d:]
    return m[0], m[1:1 + d].copy(), np.triu(s2) + np.triu(s2, 1).T


def cholesky_ref(a):
    """Lower Cholesky factor, or None at a pivot <= 1e-12 times its original diagonal entry."""
    a = np.array(a, np.float64)
    n = a.shape[0]
    dg = np.diag(a).copy()
    for j in range(n):
        d = a[j, j]
        if not d > 1e-12 * dg[j]:
            return None
        a[j, j] = math.sqrt(d)
        a[j + 1:, j] /= a[j, j]
        for i in range(j + 1, n):
            a[i, j + 1:i + 1] -= a[i, j] * a[j + 1:i + 1, j]
    return np.tril(a)


def solve_ref(s0, s1, s2, centre, n_valid, nb, prev=None, tol=1e-3, min_var=1e-9):
    """One bdn_mad_solve: `prev` is the state dict of the previous solve (None: first = 1).  Returns the state as a dict with the header's
    field names (iter, ok, converged, skip, delta, S0, n_valid, rho, var, mean, centre, a, b)."""
    d = 2 * nb
    centre = np.asarray(centre, np.float64)
    if prev is not None and prev['converged']:
        out = dict(prev)
        out['skip'] = 1
        return out
    st = {'iter': (prev['iter'] if prev is not None else 0) + 1, 'skip': 0, 'S0': float(s0), 'n_valid': int(n_valid), 'centre': centre.copy()}
    nan_n, nan_nn = np.full(nb, np.nan), np.full((nb, nb), np.nan)
    fail = dict(ok=0, converged=1, delta=np.nan, rho=nan_n, var=nan_n.copy(), a=nan_nn, b=nan_nn.copy())
    if not (s0 > 0 and np.isfinite(s0) and n_valid >= d + 1):
        st.update(fail, mean=np.full(d, np.nan))
        return st
    mz = s1 / s0
    cov = s2 / s0 - np.outer(mz, mz)
    st['mean'] = centre + mz
    sxx, sxy, syy = cov[:nb, :nb], cov[:nb, nb:], cov[nb:, nb:]
    lx, ly = cholesky_ref(sxx), cholesky_ref(syy)
    if lx is None or ly is None:
        st.update(fail)
        return st
    k = np.linalg.solve(lx, sxy)
    k = np.linalg.solve(ly, k.T).T
    u, sig, vt = np.linalg.svd(k)
    order = np.argsort(-sig, kind='stable')
    u, sig, v = u[:, order], sig[order], vt.T[:, order]
    a = np.linalg.solve(lx.T, u).T                           # a[i] = Lx^-T u_i
    b = np.linalg.solve(ly.T, v).T
    sign = np.where(((sxx @ a.T) / np.sqrt(np.diag(sxx))[:, None]).sum(0) < 0, -1.0, 1.0)
    a, b = a * sign[:, None], b * sign[:, None]
    rho = np.minimum(sig, 1.0)
    delta = float(np.abs(rho - prev['rho']).max()) if prev is not None else np.inf
    st.update(ok=1, converged=int(delta < tol), delta=delta, rho=rho, var=np.maximum(2.0 * (1.0 - rho), min_var), a=a, b=b)
    return st


def pack_state(st, nb):
    return np.concatenate([[st['iter'], st['ok'], st['converged'], st['skip'], st['delta'], st['S0'], st['n_valid']], st['rho'], st['var'],
                           st['mean'], st['centre'], np.ravel(st['a']), np.ravel(st['b'])]).astype(np.float64)


def unpack_state(v, nb):
    v = np.asarray(v, np.float64)
    d, o = 2 * nb, RHO
    st = {'iter': int(v[ITER]), 'ok': int(v[OK]), 'converged': int(v[CONVERGED]), 'skip': int(v[SKIP]), 'delta': float(v[DELTA]),
          'S0': float(v[S0]), 'n_valid': int(v[NVALID])}
    for name, size, shape in (('rho', nb, (nb,)), ('var', nb, (nb,)), ('mean', d, (d,)), ('centre', d, (d,)), ('a', nb * nb, (nb, nb)),
                              ('b', nb * nb, (nb, nb))):
        st[name] = v[o:o + size].reshape(shape).copy()
        o += size
    assert o == state_doubles(nb) == v.size
    return st


def q_ref(nb, chi2):
    """Q(n_b / 2, chi2 / 2) by the header's closed form, float64, elementwise."""
    chi2 = np.asarray(chi2, np.float64)
    t = 0.5 * chi2
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        tt = np.where(np.isfinite(t) & (t > 0), t, 1.0)
        h = np.exp(-0.5 * tt)
        m = nb // 2
        s = np.zeros_like(tt)
        if nb & 1:
            r = np.sqrt(tt)
            term = h * r * 1.1283791670955126
            for k in range(1, m + 1):
                s = s + term
                term = term * (tt / (k + 0.5))
            q = _erfc(r) + s * h
        else:
            term = h
            for k in range(1, m + 1):
                s = s + term
                term = term * (tt / float(k))
            q = s * h
        q = np.minimum(q, 1.0)
        q = np.where(t > 0, q, 1.0)
        q = np.where(np.isfinite(t), q, np.where(t > 0, 0.0, np.nan))
    return q


def chi2_ref(d1, d2, bands, st, exclude=None, exclude_value=None):
    """(chi2 float32 [H,W], proba float32 [2,H,W], variates float32 [n_b,H,W], chi2 float64 before the rounding) from a state dict."""
    nb = len(bands)
    _, h, w = d1.shape
    if not st['ok']:
        return (np.full((h, w), np.nan, np.float32), np.full((2, h, w), np.nan, np.float32), np.full((nb, h, w), np.nan, np.float32),
                np.full((h, w), np.nan))
    valid = valid_mask(d1, d2, bands, exclude, exclude_value)
    v = pixels(d1, d2, bands, valid)
    m = (v[:, :nb] - st['mean'][:nb]) @ st['a'].T - (v[:, nb:] - st['mean'][nb:]) @ st['b'].T
    c = (m * m / st['var'][None, :]).sum(1)
    q = q_ref(nb, c)
    chi2 = np.zeros((h, w), np.float32)
    c64 = np.zeros((h, w))
    proba = np.zeros((2, h, w), np.float32)
    proba[0] = 1
    var = np.zeros((nb, h, w), np.float32)
    chi2[valid], c64[valid] = c.astype(np.float32), c
    proba[0][valid], proba[1][valid] = q.astype(np.float32), (1.0 - q).astype(np.float32)
    var[:, valid] = m.T.astype(np.float32)
    return chi2, proba, var, c64


def mask_ref(proba0, valid, threshold, excluded_out=0):
    """uint8 [H,W]: 1 where proba0 < float32(threshold), 0 elsewhere (NaN: 0), excluded_out where invalid."""
    with np.errstate(invalid='ignore'):
        m = (np.asarray(proba0, np.float32) < np.float32(threshold)).astype(np.uint8)
    m[~valid] = excluded_out
    return m


def irmad_ref(d1, d2, bands, exclude=None, exclude_value=None, iters=30, tol=1e-3, min_var=1e-9):
    """The driver's launch sequence with the flag protocol: centre, then `iters` times (moments, solve, chi2).  Returns a dict: chi2, proba,
    variates, state (dict), deltas (of the solves that worked), valid."""
    nb = len(bands)
    cen, n = centre_ref(d1, d2, bands, exclude, exclude_value)
    st, mom, out, deltas = None, None, None, []
    for it in range(iters):
        if st is None or not st['converged']:
            mom = moments_ref(d1, d2, bands, cen, None if it == 0 else out[1][0], exclude, exclude_value)
        st = solve_ref(*mom, cen, n, nb, st, tol, min_var)
        if not st['skip']:
            deltas.append(st['delta'])
            out = chi2_ref(d1, d2, bands, st, exclude, exclude_value)
    return {'chi2': out[0], 'proba': out[1], 'variates': out[2], 'chi2_64': out[3], 'state': st, 'deltas': deltas,
            'valid': valid_mask(d1, d2, bands, exclude, exclude_value)}


def scene(seed, nb, h, w, c=None, change=0.08, gain=None, bias=None, offset=0.0, noise=0.05):
    """A synthetic pair: date 1 = correlated bands, date 2 = an affine function of date 1 per band plus noise, with a changed blob of
    `change` of the pixels that takes other values.  Returns (d1, d2 float32 [C,H,W], changed bool [H,W])."""
    c = c or nb
    r = np.random.default_rng(seed)
    base = r.standard_normal((c, h, w))
    mix = np.eye(c) + 0.4 * r.standard_normal((c, c))
    d1 = np.tensordot(mix, base, 1)
    g = np.asarray(gain if gain is not None else r.uniform(0.7, 1.4, c))
    b = np.asarray(bias if bias is not None else r.uniform(-0.5, 0.5, c))
    level = noise * 12.0 ** (np.arange(c) / max(c - 1, 1))   # the noise grows from band to band: the canonical correlations spread out
    d2 = g[:, None, None] * d1 + b[:, None, None] + level[:, None, None] * r.standard_normal((c, h, w))
    yy, xx = np.mgrid[:h, :w]
    changed = ((yy - 0.3 * h) ** 2 + (xx - 0.6 * w) ** 2) < change * h * w / math.pi
    d2[:, changed] = (1.5 * r.standard_normal((c, h, w)) + 1.0)[:, changed]
    return (d1 + offset).astype(np.float32), (d2 + offset).astype(np.float32), changed
