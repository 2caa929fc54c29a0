"""The numpy restatement of bdn_raster_hist, bdn_hist_threshold and bdn_raster_mask (include/bidate_hip.h) and of
fabric_amd.utils.thresholds.bin_edges.  Counts are integers; every float64 sum is formed in the order the single-block kernel forms it
(256 chunks of ceil(n_bins / 256) consecutive bins, each summed ascending from 0; the 256 partials summed in order from 0; a prefix sum
continues the sum of the earlier partials), product by product with no fused multiply-add, so that the kernel and this file perform the
same roundings everywhere except inside log and exp."""
import math

import numpy as np

OTSU, KITTLER, ROSIN, EM = 1, 2, 4, 8
METHODS = ('otsu', 'kittler', 'rosin', 'em')
COLS = ('OK', 'BIN', 'VALUE', 'CRIT', 'N0', 'N1', 'MEAN0', 'MEAN1', 'SD0', 'SD1', 'W1', 'ITERS', 'LOGLIK', 'N', 'BELOW', 'ABOVE')
COL = {k: i for i, k in enumerate(COLS)}
THREADS = 256
TWO_PI = 6.283185307179586


# ---------------------------------------------------------------- bin_edges
def bin_edges(lo, hi, n_bins=1024, spacing='linear'):
    """(edges float32 [n_bins + 1], coord float64 [n_bins]).  With f = identity / sqrt / log: u_i = f(lo) + (f(hi) - f(lo)) i / n_bins in
    float64, edge_i = float32(f^-1(u_i)) clamped to [float32(lo), float32(hi)] with the two ends exactly those, coord_i = (u_i + u_{i+1}) / 2: the bin
    centres in the coordinate the bins are uniform in."""
    lo, hi = float(lo), float(hi)
    f, inv = {'linear': (lambda v: v, lambda u: u), 'sqrt': (math.sqrt, lambda u: u * u), 'log': (math.log, np.exp)}[spacing]
    a, b = f(lo), f(hi)
    u = a + (b - a) * (np.arange(n_bins + 1, dtype=np.float64) / n_bins)
    edges = np.clip(inv(u).astype(np.float32), np.float32(lo), np.float32(hi))
    edges[0], edges[-1] = np.float32(lo), np.float32(hi)
    return edges, (u[:-1] + u[1:]) * 0.5


def mixture_hist(parts, edges, n=1e7):
    """uint64 [n_bins + 3]: rint(n (F(edge[i+1]) - F(edge[i]))) of a mixture [(weight, mean)] of unit-variance Gaussians -- an analytic
    histogram, no sampling; nothing below, above or skipped."""
    e = np.asarray(edges, np.float64)
    cdf = np.vectorize(lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0))))
    F = sum(w * cdf(e - m) for w, m in parts)
    return np.concatenate([np.rint(n * np.diff(F)).astype(np.uint64), np.zeros(3, np.uint64)])


# ---------------------------------------------------------------- raster_hist / raster_mask
def raster_hist(raster, edges, exclude=None, exclude_value=0, hist=None):
    """uint64 [n_bins + 3] = hist + the counts of `raster`: bins, below, above, skipped."""
    v = np.asarray(raster, np.float32).ravel()
    edges = np.asarray(edges, np.float32)
    n = edges.size - 1
    skip = ~np.isfinite(v)
    if exclude is not None:
        skip |= np.asarray(exclude).ravel() == exclude_value
    out = np.zeros(n + 3, np.uint64) if hist is None else np.array(hist, np.uint64)
    w = v[~skip]
    below, above = w < edges[0], w > edges[n]
    inside = w[~below & ~above]
    b = np.searchsorted(edges[:n], inside, side='right') - 1
    out[:n] += np.bincount(b, minlength=n).astype(np.uint64)
    out[n] += np.uint64(below.sum())
    out[n + 1] += np.uint64(above.sum())
    out[n + 2] += np.uint64(skip.sum())
    return out


def raster_mask(raster, thr, below=False, exclude=None, exclude_value=0, excluded_out=0):
    v = np.asarray(raster, np.float32)
    with np.errstate(invalid='ignore'):
        m = (np.isfinite(v) & ((v < np.float32(thr)) if below else (v >= np.float32(thr)))).astype(np.uint8)
    if exclude is not None:
        m[np.asarray(exclude).reshape(v.shape) == exclude_value] = excluded_out
    return m


# ---------------------------------------------------------------- the kernel's summation order
def _serial(terms, start=0.0):
    """start + t0 + t1 + ... left to right."""
    return float(np.cumsum(np.concatenate(([start], np.asarray(terms, np.float64))))[-1])


class _Order:
    def __init__(self, n_bins):
        self.n, self.per = n_bins, -(-n_bins // THREADS)

    def _rows(self, terms):
        """[256][per]: the terms by owner, zeros past n_bins (adding 0.0 changes no sum)."""
        m = np.zeros(THREADS * self.per)
        m[:self.n] = terms
        return m.reshape(THREADS, self.per)

    def partials(self, terms):
        return np.cumsum(self._rows(terms), axis=1)[:, -1]           # np.cumsum adds strictly left to right

    def total(self, terms):
        return _serial(self.partials(terms))

    def prefix(self, terms):
        """[n_bins]: the sum of the terms of the bins below b, as bin b's owner holds it."""
        rows = self._rows(terms)
        before = np.cumsum(np.concatenate(([0.0], np.cumsum(rows, axis=1)[:, -1])))[:THREADS]
        return np.cumsum(np.hstack((before[:, None], rows)), axis=1)[:, :self.per].reshape(-1)[:self.n]


def _first(values, valid, maximise):
    """The first index of the extreme of values[valid], or -1."""
    idx = np.flatnonzero(valid)
    if idx.size == 0:
        return -1
    v = values[idx]
    return int(idx[np.argmax(v) if maximise else np.argmin(v)])


def _classes(o, c, y, s):
    """Per class (bins < s, bins >= s): count, sum c y, sum c y^2, each summed for itself."""
    cd = c.astype(np.float64)
    cy = cd * y
    cyy = cy * y
    k = np.arange(c.size) >= s
    n = [int(c[~k].sum()), int(c[k].sum())]
    a = [o.total(np.where(k, 0.0, cy)), o.total(np.where(k, cy, 0.0))]
    q = [o.total(np.where(k, 0.0, cyy)), o.total(np.where(k, cyy, 0.0))]
    return n, a, q


def _mean(n, a, i):
    return a[i] / n[i] if n[i] else 0.0


def _var(n, a, q, i):
    if not n[i]:
        return 0.0
    m = a[i] / n[i]
    return q[i] / n[i] - m * m


def criteria(hist, coord):
    """(otsu [n_bins], kittler [n_bins]) of every split t, NaN where the split is not valid: what the walk of the kernel evaluates."""
    n_bins = len(coord)
    o = _Order(n_bins)
    c = np.array([int(v) for v in hist[:n_bins]], dtype=object)
    cd = np.array([float(v) for v in c])
    N = int(sum(c))
    M = o.total(cd * coord) / N
    y = coord - M
    cy = cd * y
    cyy = cy * y
    a_t, q_t = o.total(cy), o.total(cyy)
    a0, q0 = o.prefix(cy), o.prefix(cyy)
    n0 = np.concatenate(([0], np.cumsum(c)[:-1])).astype(object)
    otsu, kit = np.full(n_bins, np.nan), np.full(n_bins, np.nan)
    dN = float(N)
    for b in range(1, n_bins):
        k0, k1 = int(n0[b]), N - int(n0[b])
        if not k0 or not k1:
            continue
        d0, d1 = float(k0), float(k1)
        a1, q1 = a_t - a0[b], q_t - q0[b]
        m0, m1 = a0[b] / d0, a1 / d1
        dm = m0 - m1
        v = (d0 * d1) * (dm * dm)
        if math.isfinite(v):
            otsu[b] = v
        v0, v1 = q0[b] / d0 - m0 * m0, q1 / d1 - m1 * m1
        if v0 > 0.0 and v1 > 0.0:
            P0, P1 = d0 / dN, d1 / dN
            J = (1.0 + (P0 * math.log(v0) + P1 * math.log(v1))) - 2.0 * (P0 * math.log(P0) + P1 * math.log(P1))
            if math.isfinite(J):
                kit[b] = J
    return otsu, kit


def hist_threshold(hist, coord, edges, methods=OTSU | KITTLER | ROSIN | EM, em_iters=100, em_tol=1e-9):
    """(table float64 [4][16], thr float32 [4]) of bdn_hist_threshold."""
    coord = np.asarray(coord, np.float64)
    edges = np.asarray(edges, np.float32)
    n_bins = coord.size
    table, thr = np.zeros((4, 16)), np.full(4, np.nan, np.float32)
    c = np.array([int(v) for v in hist[:n_bins]], dtype=np.int64)
    N = int(c.sum())
    if np.count_nonzero(c) < 2:
        return table, thr
    o = _Order(n_bins)
    cd = c.astype(np.float64)
    M = o.total(cd * coord) / N
    y = coord - M
    dN = float(N)

    def write(row, b, crit, n, mean0, mean1, sd0, sd1, w1, iters, loglik):
        table[row] = [1.0, b, float(edges[b]), crit, n[0], n[1], mean0, mean1, sd0, sd1, w1, iters, loglik, N, float(hist[n_bins]),
                      float(hist[n_bins + 1])]
        thr[row] = edges[b]

    def split_row(row, b, crit):
        n, a, q = _classes(o, c, y, b)
        write(row, b, crit, n, _mean(n, a, 0) + M, _mean(n, a, 1) + M, math.sqrt(max(_var(n, a, q, 0), 0.0)),
              math.sqrt(max(_var(n, a, q, 1), 0.0)), n[1] / dN, 0.0, 0.0)

    otsu_bin = kit_bin = -1
    if methods & (OTSU | KITTLER | EM):
        otsu, kit = criteria(hist, coord)
        otsu_bin = _first(otsu, ~np.isnan(otsu), True)
        kit_bin = _first(kit, ~np.isnan(kit), False)
        if methods & OTSU and otsu_bin >= 0:
            split_row(0, otsu_bin, otsu[otsu_bin])
        if methods & KITTLER and kit_bin >= 0:
            split_row(1, kit_bin, kit[kit_bin])

    if methods & ROSIN and N < 1 << 49:
        p = int(np.argmax(c))
        e = int(np.flatnonzero(c)[-1])
        if e >= p + 2:
            i = np.arange(p + 1, e)
            d = (int(c[e]) - int(c[p])) * (i - p) - (e - p) * (c[i] - int(c[p]))
            b = int(i[np.argmax(d)])
            split_row(2, b, float(d[b - p - 1]))

    if not methods & EM:
        return table, thr
    start = kit_bin if kit_bin >= 0 else otsu_bin
    if start < 0:
        return table, thr
    sp = coord[1:] - coord[:-1]
    if not (sp > 0).any():
        return table, thr
    smin = sp[sp > 0].min()
    vfloor = (smin * smin) / 12.0
    n, a, q = _classes(o, c, y, start)
    w = [n[0] / dN, n[1] / dN]
    mu = [_mean(n, a, 0), _mean(n, a, 1)]
    var = [max(_var(n, a, q, 0), vfloor), max(_var(n, a, q, 1), vfloor)]
    occ = c > 0
    loglik = prev = 0.0
    iters = 0

    def logpost():
        k0 = math.log(w[0]) - 0.5 * math.log(TWO_PI * var[0])
        k1 = math.log(w[1]) - 0.5 * math.log(TWO_PI * var[1])
        e0, e1 = y - mu[0], y - mu[1]
        return k0 - (e0 * e0) / (2.0 * var[0]), k1 - (e1 * e1) / (2.0 * var[1])

    for it in range(1, em_iters + 1):
        l0, l1 = logpost()
        mx = np.maximum(l0, l1)
        x0, x1 = np.exp(l0 - mx), np.exp(l1 - mx)
        s = x0 + x1
        g0, g1 = cd * (x0 / s), cd * (x1 / s)
        terms = [cd * (mx + np.log(s)), g0, g0 * y, (g0 * y) * y, g1, g1 * y, (g1 * y) * y]
        tot = [o.total(np.where(occ, t, 0.0)) for t in terms]
        loglik, iters = tot[0], it
        if not math.isfinite(loglik) or not tot[1] > 0.0 or not tot[4] > 0.0:
            return table, thr
        if it > 1 and abs(loglik - prev) <= em_tol * abs(loglik):
            break
        prev = loglik
        for i in range(2):
            R = tot[1 + 3 * i]
            w[i] = R / dN
            mu[i] = tot[2 + 3 * i] / R
            var[i] = max(tot[3 + 3 * i] / R - mu[i] * mu[i], vfloor)
    if not mu[1] > mu[0] or not math.isfinite(mu[0]) or not math.isfinite(mu[1]):
        return table, thr
    le0, le1 = np.flatnonzero(y <= mu[0]), np.flatnonzero(y <= mu[1])
    b0 = int(le0[-1]) if le0.size else 0
    b1 = int(le1[-1]) if le1.size else -1
    l0, l1 = logpost()
    idx = np.arange(n_bins)
    hit = np.flatnonzero((idx > b0) & (idx <= b1) & (l1 >= l0))
    if hit.size == 0:
        return table, thr
    b = int(hit[0])
    n, _, _ = _classes(o, c, y, b)
    write(3, b, loglik, n, mu[0] + M, mu[1] + M, math.sqrt(var[0]), math.sqrt(var[1]), w[1], float(iters), loglik)
    return table, thr


def read_table(table, thr):
    """{method: {column lower-case: value, 'thr': float}}: the shape of ThresholdTable.read()."""
    out = {}
    for r, name in enumerate(METHODS):
        d = {k.lower(): float(table[r][i]) for i, k in enumerate(COLS)}
        d['ok'] = bool(d['ok'])
        for k in ('bin', 'n0', 'n1', 'iters', 'n', 'below', 'above'):
            d[k] = int(d[k])
        d['thr'] = float(thr[r])
        out[name] = d
    return out
