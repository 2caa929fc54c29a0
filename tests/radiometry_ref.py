"""The numpy twin of fabric_amd/csrc/radiometry.hip (include/bidate_hip.h, "radiometric matching"): the order statistics from np.sort of
the valid values in the key order with the header's rank formula, the piecewise-linear transfer with explicit float32 roundings (numpy
float32 arithmetic rounds once per operation and never fuses), and stretch_8bit's arithmetic in float64.  The GPU tests compare bits."""
import numpy as np

OFFSET, SLOPE = 0, 1


def keys(v):
    """The monotone uint32 key of float32 values (csrc/common.hpp topk_key): ascending keys are ascending floats, -0.0 below +0.0."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def valid_sorted(band, exclude=None, exclude_value=None, positive_only=False):
    """The valid values of a band, sorted in the key order."""
    band = np.asarray(band, np.float32)
    m = np.isfinite(band)
    if exclude is not None:
        m &= np.asarray(exclude) != exclude_value
    if positive_only:
        m &= band > 0
    return unkeys(np.sort(keys(band[m])))


def quantiles_sorted(v, probs):
    """(value float64 [n_q], order float32 [n_q, 2]) of the sorted valid values v."""
    probs = np.asarray(probs, np.float64)
    n = v.size
    value, order = np.full(probs.size, np.nan), np.full((probs.size, 2), np.nan, np.float32)
    for q, p in enumerate(probs):
        if n == 0 or not 0.0 <= p <= 1.0:
            continue
        h = np.float64(p) * np.float64(n - 1)
        lo = int(np.floor(h))
        hi = min(lo + 1, n - 1)
        t = h - np.float64(lo)
        a, b = np.float64(v[lo]), np.float64(v[hi])
        order[q] = v[lo], v[hi]
        value[q] = a + (b - a) * t
    return value, order


def quantiles_ref(scene, probs, bands=None, exclude=None, exclude_value=None, positive_only=False):
    """(value float64 [n_b, n_q], order float32 [n_b, n_q, 2], count int64 [n_b]); a band index outside the stack has no pixel."""
    scene = np.asarray(scene, np.float32)
    bands = list(range(scene.shape[0])) if bands is None else list(bands)
    out = []
    for b in bands:
        v = valid_sorted(scene[b], exclude, exclude_value, positive_only) if 0 <= b < scene.shape[0] else np.zeros(0, np.float32)
        out.append(quantiles_sorted(v, probs) + (v.size,))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)


def default_probs(K):
    return np.arange(K, dtype=np.float64) / np.float64(K - 1)


def fit_ref(d2, d1, probs=None, knots=256, bands=None, exclude=None, exclude_value=None):
    """(src float32 [n_b, K], dst float32 [n_b, K], count int64 [2, n_b]): the quantiles of date 2 and of date 1, each rounded once."""
    probs = default_probs(knots) if probs is None else np.asarray(probs, np.float64)
    v2, _, n2 = quantiles_ref(d2, probs, bands, exclude, exclude_value)
    v1, _, n1 = quantiles_ref(d1, probs, bands, exclude, exclude_value)
    return v2.astype(np.float32), v1.astype(np.float32), np.stack([n2, n1])


def transfer_band(x, s, t, mode=OFFSET, exact=False):
    """One band through its knot tables s, t (float32 [K]); x of any shape; float32 arithmetic, one rounding per operation."""
    x = np.asarray(x, np.float32)
    s, t = np.asarray(s, np.float32), np.asarray(t, np.float32)
    K = s.size
    out = x.copy()
    if exact or np.isnan(s).any() or np.isnan(t).any():
        return out
    fin = np.isfinite(x)
    xf = x[fin]

    def seg(v, k):
        s0, s1, t0, t1 = s[k], s[k + 1], t[k], t[k + 1]
        with np.errstate(all='ignore'):
            y = t0 + (v - s0) * ((t1 - t0) / (s1 - s0))
        return np.where((s0 == t0) & (s1 == t1), v, y).astype(np.float32)

    def off(v, e):
        d = t[e] - s[e]
        return v if d == 0 else (v + d).astype(np.float32)

    k = np.clip(np.searchsorted(s, xf, side='right') - 1, 0, K - 2)           # the last index with s_k <= x
    y = seg(xf, k)
    below, above = xf < s[0], xf >= s[K - 1]
    lo_seg, hi_seg = mode == SLOPE and s[1] > s[0], mode == SLOPE and s[K - 1] > s[K - 2]
    y[below] = seg(xf[below], np.zeros(int(below.sum()), np.int64)) if lo_seg else off(xf[below], 0)
    y[above] = seg(xf[above], np.full(int(above.sum()), K - 2, np.int64)) if hi_seg else off(xf[above], K - 1)
    out[fin] = y
    return out


def apply_ref(src, bands, S, T, mode=OFFSET, exact=None):
    """The transfer over a [C,H,W] stack: the named bands through their rows (the first row that names a band counts), the others copied."""
    src = np.asarray(src, np.float32)
    out = src.copy()
    done = set()
    for i, b in enumerate(bands):
        if b in done or not 0 <= b < src.shape[0]:
            continue
        done.add(b)
        out[b] = transfer_band(src[b], S[i], T[i], mode, bool(exact[i]) if exact is not None else False)
    return out


def match_ref(d2, d1, method='histogram', knots=256, lower=0.02, upper=0.98, bands=None, exclude=None, exclude_value=None):
    """(date 2 matched to date 1, src, dst, count): 'histogram' = K knots at k / (K - 1) with OFFSET, 'range' = two knots with SLOPE."""
    bands = list(range(np.asarray(d2).shape[0])) if bands is None else list(bands)
    if method == 'histogram':
        s, t, n = fit_ref(d2, d1, None, knots, bands, exclude, exclude_value)
        return apply_ref(d2, bands, s, t, OFFSET), s, t, n
    s, t, n = fit_ref(d2, d1, [lower, upper], 2, bands, exclude, exclude_value)
    return apply_ref(d2, bands, s, t, SLOPE), s, t, n


def stretch_ref(x, c, d):
    """stretch_8bit's arithmetic for one band: float64, clamp to [0, 255], truncate; a NaN gives 0."""
    with np.errstate(all='ignore'):
        v = (np.asarray(x).astype(np.float64) - np.float64(c)) * (np.float64(255.0) / (np.float64(d) - np.float64(c)))
    out = np.zeros(v.shape, np.uint8)
    pos = v > 0
    out[pos] = np.minimum(v[pos], 255.0).astype(np.uint8)
    return out


def stretch_8bit_ref(x, lower_percent=2, higher_percent=98):
    """The device stretch_8bit of one band or of a [C,H,W] stack, band by band: the percentiles over the values > 0."""
    x = np.asarray(x)
    if x.ndim == 2:
        return stretch_8bit_ref(x[None], lower_percent, higher_percent)[0]
    out = np.empty(x.shape, np.uint8)
    for b in range(x.shape[0]):
        v = valid_sorted(x[b].astype(np.float32), positive_only=True)
        (c, d), _ = quantiles_sorted(v, [lower_percent / 100, higher_percent / 100])
        out[b] = stretch_ref(x[b], c, d)
    return out
