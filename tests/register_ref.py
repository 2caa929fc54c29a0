"""numpy restatement of the co-registration entries (include/bidate_hip.h: bdn_shift_corr, bdn_shift_peak, bdn_shift_apply), for the CPU
and the GPU tests:
  the table   every entry the correctly rounded sum (math.fsum) of its exact terms -- products of float32 values are exact in float64;
  the score   and the peak in float64, one rounding per operation, in the kernel's operation order;
  the field   interpolation between cell centres in float32;
  the taps    and the blend of the resampling in float32.
Nothing here is fast: the shapes of the tests are small.
"""
import math

import numpy as np

F1, F0, HALF = np.float32(1), np.float32(0), np.float32(0.5)


def cell_bounds(n, extent):
    """[(lo, hi)] of the n cells along an axis of `extent` pixels."""
    return [(i * extent // n, (i + 1) * extent // n) for i in range(n)]


def valid_mask(d, exclude=None, exclude_value=None):
    """bool [C,H,W]: finite and not excluded."""
    v = np.isfinite(d)
    if exclude is not None:
        v &= (exclude != exclude_value)[None]
    return v


def _shifted(a, dy, dx, fill):
    """s[y, x] = a[y + dy, x + dx], `fill` where that lies outside."""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def terms(d1, d2, band, dy, dx, exclude=None, exclude_value=None):
    """(mask, a, b) over the scene for one band and shift: float64 a, b (0 where the mask is off)."""
    va, vb = valid_mask(d1[band:band + 1], exclude, exclude_value)[0], valid_mask(d2[band:band + 1], exclude, exclude_value)[0]
    m = va & _shifted(vb, dy, dx, False)
    a = np.where(m, d1[band], 0).astype(np.float64)
    b = np.where(m, _shifted(d2[band], dy, dx, 0), 0).astype(np.float64)
    return m, a, b


def table_ref(d1, d2, bands, R, ny, nx, exclude=None, exclude_value=None, exact=True):
    """(table, sum_abs): float64 [n_b,ny,nx,S,S,6] = {n, Sa, Sb, Saa, Sbb, Sab} and the sums of the |terms| (the error bound's scale).
    exact=True: math.fsum per entry; False: numpy's sum (the vectorised host route, for timing and the sub-pixel tests)."""
    S = 2 * R + 1
    _, h, w = d1.shape
    table = np.zeros((len(bands), ny, nx, S, S, 6))
    sabs = np.zeros_like(table)
    rows, cols = cell_bounds(ny, h), cell_bounds(nx, w)
    tot = (lambda v: math.fsum(v.ravel().tolist())) if exact else (lambda v: float(v.sum()))
    for bi, band in enumerate(bands):
        for iy, dy in enumerate(range(-R, R + 1)):
            for ix, dx in enumerate(range(-R, R + 1)):
                m, a, b = terms(d1, d2, band, dy, dx, exclude, exclude_value)
                prods = (a, b, a * a, b * b, a * b)          # exact: 24-bit significands
                for i, (r0, r1) in enumerate(rows):
                    for j, (c0, c1) in enumerate(cols):
                        e, ea = table[bi, i, j, iy, ix], sabs[bi, i, j, iy, ix]
                        e[0] = ea[0] = m[r0:r1, c0:c1].sum()
                        for k, t in enumerate(prods):
                            e[1 + k] = tot(t[r0:r1, c0:c1])
                            ea[1 + k] = float(np.abs(t[r0:r1, c0:c1]).sum())
    return table, sabs


def table_brute(d1, d2, bands, R, ny, nx, exclude=None, exclude_value=None):
    """The same table by a double loop over the pixels, from the definition (tiny shapes only)."""
    S = 2 * R + 1
    _, h, w = d1.shape
    out = np.zeros((len(bands), ny, nx, S, S, 6))
    lists = {}
    rows, cols = cell_bounds(ny, h), cell_bounds(nx, w)
    row_of = [next(i for i, (lo, hi) in enumerate(rows) if lo <= y < hi) for y in range(h)]
    col_of = [next(j for j, (lo, hi) in enumerate(cols) if lo <= x < hi) for x in range(w)]
    bad = (lambda y, x: False) if exclude is None else (lambda y, x: exclude[y, x] == exclude_value)
    for bi, band in enumerate(bands):
        for y in range(h):
            for x in range(w):
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        yy, xx = y + dy, x + dx
                        if not (0 <= yy < h and 0 <= xx < w) or bad(y, x) or bad(yy, xx):
                            continue
                        a, b = float(d1[band, y, x]), float(d2[band, yy, xx])
                        if not (math.isfinite(a) and math.isfinite(b)):
                            continue
                        lists.setdefault((bi, row_of[y], col_of[x], dy + R, dx + R), []).append((1.0, a, b, a * a, b * b, a * b))
    for key, ts in lists.items():
        out[key] = [math.fsum(t[k] for t in ts) for k in range(6)]
    return out


def whole_table(table):
    """[n_b,S,S,6]: the cells' tables added in (i, j) order, one float64 addition each."""
    nb, ny, nx = table.shape[:3]
    tot = np.zeros(table.shape[:1] + table.shape[3:])
    for i in range(ny):
        for j in range(nx):
            tot = tot + table[:, i, j]
    return tot


def score_ref(t):
    """float64 [S,S] from [n_b,S,S,6]: the mean over the defined bands of the NCC, -2 where no band is defined."""
    acc = np.zeros(t.shape[1:3])
    cnt = np.zeros(t.shape[1:3])
    with np.errstate(all='ignore'):
        for b in range(t.shape[0]):
            n, sa, sb, saa, sbb, sab = (t[b, ..., k] for k in range(6))
            va = (n * saa) - (sa * sa)
            vb = (n * sbb) - (sb * sb)
            cov = (n * sab) - (sa * sb)
            ok = (n >= 2.0) & (va > 0.0) & (vb > 0.0)
            ncc = cov / np.sqrt(va * vb)
            acc = acc + np.where(ok, ncc, 0.0)               # adding 0.0 changes nothing
            cnt = cnt + ok
        return np.where(cnt > 0, acc / np.maximum(cnt, 1), -2.0)


def _parabola(cm, c0, cp, border):
    if border or cm == -2.0 or cp == -2.0:
        return 0.0
    den = (cm - (2.0 * c0)) + cp
    if not den < 0.0:
        return 0.0
    return float(min(max((0.5 * (cm - cp)) / den, -0.5), 0.5))


def peak_ref(score, R):
    """(dy, dx, ncc, ok, (py, px)) of one score window."""
    S = 2 * R + 1
    sc = np.asarray(score, np.float64)
    best = 0
    flat = sc.ravel()
    for s in range(1, S * S):
        if flat[s] > flat[best]:
            best = s
    py, px = divmod(best, S)
    ncc = float(flat[best])
    if not ncc > -2.0:
        return 0.0, 0.0, ncc, 0, (py, px)
    by, bx = py in (0, S - 1), px in (0, S - 1)
    dy = float(py - R) + _parabola(0.0 if by else sc[py - 1, px], sc[py, px], 0.0 if by else sc[py + 1, px], by)
    dx = float(px - R) + _parabola(0.0 if bx else sc[py, px - 1], sc[py, px], 0.0 if bx else sc[py, px + 1], bx)
    return dy, dx, ncc, 1, (py, px)


def peak_margins(score, R):
    """(best - second best score, the smaller |c- - 2 c0 + c+| of the two axes, None where no parabola is formed): how far a case
    is from a tie and from a flat parabola."""
    S = 2 * R + 1
    sc = np.asarray(score, np.float64)
    flat = np.sort(sc.ravel())
    gap = float(flat[-1] - flat[-2]) if flat.size > 1 else math.inf
    _, _, _, ok, (py, px) = peak_ref(sc, R)
    curv = []
    if ok:
        if py not in (0, S - 1) and sc[py - 1, px] != -2.0 and sc[py + 1, px] != -2.0:
            curv.append(abs(sc[py - 1, px] - 2 * sc[py, px] + sc[py + 1, px]))
        if px not in (0, S - 1) and sc[py, px - 1] != -2.0 and sc[py, px + 1] != -2.0:
            curv.append(abs(sc[py, px - 1] - 2 * sc[py, px] + sc[py, px + 1]))
    return gap, (min(curv) if curv else None)


def report_ref(table, R, min_ncc=0.0):
    """(report float64 [ny nx + 1, 4], field float32 [ny,nx,2], scores [ny nx + 1,S,S]) from a table."""
    nb, ny, nx = table.shape[:3]
    scores = [score_ref(table[:, i, j]) for i in range(ny) for j in range(nx)] + [score_ref(whole_table(table))]
    rep = np.array([peak_ref(s, R)[:4] for s in scores], np.float64)
    g = rep[-1]
    field = np.zeros((ny, nx, 2), np.float32)
    for c in range(ny * nx):
        dy, dx, ncc, ok = rep[c]
        if not ok or ncc < min_ncc:
            dy, dx = (g[0], g[1]) if g[3] else (0.0, 0.0)
        field[c // nx, c % nx] = (np.float32(dy), np.float32(dx))
    return rep, field, np.array(scores)


def _axis(extent, n):
    """(i0, i1, t) per pixel along one axis: the cells whose centres bracket the pixel and the float32 weight of the second."""
    q = np.arange(extent, dtype=np.float32)
    if n == 1:
        z = np.zeros(extent, np.int64)
        return z, z, np.zeros(extent, np.float32)
    centres = np.array([HALF * np.float32(lo + hi - 1) for lo, hi in cell_bounds(n, extent)], np.float32)
    i0 = np.clip(np.searchsorted(centres, q, side='right') - 1, 0, n - 2)       # the last centre <= q
    i1 = i0 + 1
    t = (q - centres[i0]) / (centres[i1] - centres[i0])
    return i0, i1, np.clip(t, F0, F1).astype(np.float32)


def _lerp2(tx, ty, v00, v01, v10, v11):
    gx, gy = F1 - tx, F1 - ty
    top = (gx * v00) + (tx * v01)
    bot = (gx * v10) + (tx * v11)
    return (gy * top) + (ty * bot)


def field_ref(field, h, w):
    """float32 [2,H,W]: (s_y, s_x) at every pixel."""
    field = np.asarray(field, np.float32)
    ny, nx = field.shape[:2]
    i0, i1, ty = _axis(h, ny)
    j0, j1, tx = _axis(w, nx)
    ty, tx = ty[:, None], tx[None, :]
    with np.errstate(all='ignore'):
        return np.stack([_lerp2(tx, ty, field[i0][:, j0, k], field[i0][:, j1, k], field[i1][:, j0, k], field[i1][:, j1, k]) for k in range(2)])


def apply_ref(src, field):
    """(out float32 [C,H,W], oob uint8 [H,W]) of bdn_shift_apply."""
    src = np.asarray(src, np.float32)
    _, h, w = src.shape
    s = field_ref(field, h, w)
    assert s.dtype == np.float32
    with np.errstate(all='ignore'):
        yy = np.arange(h, dtype=np.float32)[:, None] + s[0]
        xx = np.arange(w, dtype=np.float32)[None, :] + s[1]
        yf, xf = np.floor(yy), np.floor(xx)
        fy, fx = yy - yf, xx - xf
        iy = np.clip(yf, -2.0 ** 30, 2.0 ** 30).astype(np.int64)
        ix = np.clip(xf, -2.0 ** 30, 2.0 ** 30).astype(np.int64)
        ya, yb = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
        xa, xb = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
        out = _lerp2(fx[None], fy[None], src[:, ya, xa], src[:, ya, xb], src[:, yb, xa], src[:, yb, xb])
    in_y = (iy >= 0) & (np.where(fy > 0, iy + 1, iy) <= h - 1)
    in_x = (ix >= 0) & (np.where(fx > 0, ix + 1, ix) <= w - 1)
    assert out.dtype == np.float32
    return out, (~(in_y & in_x)).astype(np.uint8)


def estimate_ref(d1, d2, R, bands=None, cells=(1, 1), exclude=None, exclude_value=None, min_ncc=0.0, exact=False):
    """The whole estimate on the host: (report, field)."""
    bands = list(range(d1.shape[0])) if bands is None else bands
    table, _ = table_ref(d1, d2, bands, R, cells[0], cells[1], exclude, exclude_value, exact=exact)
    rep, field, _ = report_ref(table, R, min_ncc)
    return rep, field


def shift_bilinear(img, ty, tx):
    """img [C,H,W] sampled at (y + ty, x + tx) with a replicate border, float64 arithmetic (test inputs, not a kernel's reference)."""
    _, h, w = img.shape
    yy, xx = np.arange(h)[:, None] + float(ty), np.arange(w)[None, :] + float(tx)
    y0, x0 = np.floor(yy).astype(int), np.floor(xx).astype(int)
    fy, fx = yy - y0, xx - x0
    ya, yb, xa, xb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1), np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    a = img.astype(np.float64)
    out = (1 - fy) * ((1 - fx) * a[:, ya, xa] + fx * a[:, ya, xb]) + fy * ((1 - fx) * a[:, yb, xa] + fx * a[:, yb, xb])
    return out.astype(np.float32)
