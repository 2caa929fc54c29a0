"""numpy twin of bdn_sample_patches_warp: the warp record of a sample from its draws, the affine map with bilinear taps from a given
record, and the output patches, composed with the value stages of tests/augment_ref.py.

This file restates the specification (include/bidate_hip.h) and shares no code with the kernel.  Two halves:
  record64   the record from the Philox words in float64.  The kernel forms it with its float32 cosf / sinf / exp2f, which numpy cannot
             reproduce bit for bit: the rotation and zoom entries are compared under a tolerance (tests/test_gpu_warp.py); the two
             translations are one float32 product each and are exact (record_shift32).
  gather     everything downstream of a float32 record, bit for bit: numpy float32 elementwise operations, one per rounding, in the
             order of the specification.  Nothing here may be fused or reassociated.
A warp policy is a fabric_amd.augment.PatchWarp, an augment policy a PatchAugment (their fields only).
"""
import math

import numpy as np

from tests import augment_ref as R

WARP = 0x57415250
F32 = np.float32
ONE, HALF = F32(1), F32(0.5)
IDENTITY = np.array([[1, 0, 0, 0, 1, 0]] * 2, np.float32)


def policy_f32(warp):
    """(rotate_rad, log2_lo, log2_hi, misreg) as the entry receives them: Python doubles rounded to float32."""
    return tuple(F32(v) for v in warp.abi_args()[:4])


def sgn(w):
    """2 u(w) - 1 in [-1, 1): exact in float32."""
    return F32(2) * R.u(w) - ONE


def record64(warp, seed, key):
    """float64 [2][6]: per date (a_ii, a_ij, t_i, a_ji, a_jj, t_j) of the sample with this key, from the float32 policy scalars."""
    rad, lo, hi, m = (float(v) for v in policy_f32(warp))
    w = R.draw(seed, key, WARP, 0)
    theta = float(sgn(w[0])) * rad
    s = 2.0 ** (lo + float(R.u(w[1])) * (hi - lo))
    c, sn = math.cos(theta) / s, math.sin(theta) / s
    ti, tj = m * float(sgn(w[2])), m * float(sgn(w[3]))
    return np.array([[c, -sn, 0.0, sn, c, 0.0], [c, -sn, ti, sn, c, tj]], np.float64)


def record_shift32(warp, seed, key):
    """float32 (t_i, t_j) of date 2: misreg * sgn(w), one rounding -- bit-exact."""
    m = policy_f32(warp)[3]
    w = R.draw(seed, key, WARP, 0)
    return m * sgn(w[2]), m * sgn(w[3])


def drawn(warp, seed, key):
    """dict(theta, s, t_i, t_j) in float64: what test coverage is stated on."""
    rad, lo, hi, m = (float(v) for v in policy_f32(warp))
    w = R.draw(seed, key, WARP, 0)
    return dict(theta=float(sgn(w[0])) * rad, s=2.0 ** (lo + float(R.u(w[1])) * (hi - lo)), t_i=m * float(sgn(w[2])), t_j=m * float(sgn(w[3])))


def rotation_record(quarter_turns, t2=(0.0, 0.0)):
    """float32 [2][6]: the exact record of a rotation by quarter_turns * 90 degrees (cos, sin in {0, 1, -1}); date 2 shifted by t2."""
    c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[quarter_turns % 4]
    return np.array([[c, -s, 0, s, c, 0], [c, -s, t2[0], s, c, t2[1]]], np.float32)


def coords(rec, S, sym):
    """float32 [S][S] y, x of every output pixel, relative to the window origin.  rec: float32 [6] of one date."""
    a_ii, a_ij, t_i, a_ji, a_jj, t_j = (F32(v) for v in np.asarray(rec, np.float32))
    i, j = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    ri = S - 1 - i if sym & 2 else i
    cj = S - 1 - j if sym & 1 else j
    ip, jp = (cj, ri) if sym & 4 else (ri, cj)              # the window coordinate the symmetry gives output pixel (i, j)
    h = F32((S - 1) / 2)
    di, dj = ip.astype(np.float32) - h, jp.astype(np.float32) - h
    y = ((a_ii * di) + (a_ij * dj)) + (h + t_i)
    x = ((a_ji * di) + (a_jj * dj)) + (h + t_j)
    assert y.dtype == np.float32 and x.dtype == np.float32
    return y, x


def taps(rec, S, sym, row, col, H, W):
    """The unclamped integer taps and the weights of the bilinear gather: (iy, ix, fy, fx); tap rows are row + iy and + 1."""
    y, x = coords(rec, S, sym)
    y0, x0 = np.floor(y), np.floor(x)
    return row + y0.astype(np.int64), col + x0.astype(np.int64), y - y0, x - x0


def gather_plane(plane, rec, S, sym, row, col):
    """float32 [S][S]: one plane [H][W] through one date's record."""
    H, W = plane.shape
    iy, ix, fy, fx = taps(rec, S, sym, row, col, H, W)
    r0, r1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    c0, c1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    gx, gy = ONE - fx, ONE - fy
    with np.errstate(all='ignore'):
        top = (gx * plane[r0, c0]) + (fx * plane[r0, c1])
        bot = (gx * plane[r1, c0]) + (fx * plane[r1, c1])
        out = (gy * top) + (fy * bot)
    assert out.dtype == np.float32
    return out


def label_taps(rec, S, sym, row, col):
    """The unclamped nearest-neighbour label indices (rows, columns) of date 1's record."""
    y, x = coords(rec, S, sym)
    return row + np.floor(y + HALF).astype(np.int64), col + np.floor(x + HALF).astype(np.int64)


def gather_labels(lab, rec, S, sym, row, col, oob_label):
    """(uint8 [S][S] labels, bool [S][S] outside): nearest neighbour, clamped; outside pixels become oob_label when it is not None."""
    H, W = lab.shape
    iy, ix = label_taps(rec, S, sym, row, col)
    outside = (iy < 0) | (iy > H - 1) | (ix < 0) | (ix > W - 1)
    out = lab[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)]
    if oob_label is not None:
        out = np.where(outside, np.uint8(oob_label), out)
    return out.astype(np.uint8), outside


def reference_sample(pol, warp, records, key, desc, cities, S):
    """One sample through a GIVEN float32 record [2][6].  desc = (city, row, col, sym); cities[k] = {'images': float32 [2,C,H,W],
    'labels': uint8 [H,W]}.  Returns what augment_ref.reference_sample returns, plus outside = bool [S,S] (labels beyond the city)."""
    city, row, col, sym = (int(v) for v in desc)
    im, lb = cities[city]['images'], cities[city]['labels']
    C, (H, W) = im.shape[1], lb.shape
    g = R.geometry(pol, key, row, col, sym, H, W, S)
    records = np.asarray(records, np.float32)
    x = np.stack([np.stack([gather_plane(im[d, c], records[d], S, g['sym'], g['row'], g['col']) for c in range(C)]) for d in range(2)])
    labels, outside = gather_labels(lb, records[0], S, g['sym'], g['row'], g['col'], warp.oob_label)
    radio = R.radiometry(pol, key, C)
    if pol.gain != 0.0 or pol.bias != 0.0:
        with np.errstate(all='ignore'):
            x = radio[:, :, 0, None, None] * x + radio[:, :, 1, None, None]          # float32: the product rounds, then the sum
    x64 = None
    if pol.noise_std > 0.0:
        z = np.stack([R.noise_z64(pol.seed, key, p, S) for p in range(2 * C)]).reshape(2, C, S, S)
        x64 = x.astype(np.float64) + float(np.float32(pol.noise_std)) * z
    mask = np.zeros((S, S), bool)
    if g['erased']:
        mask[g['top']:g['top'] + g['eh'], g['left']:g['left'] + g['ew']] = True
        x = x.copy()
        x[:, :, mask] = np.float32(pol.erase_fill)
        if x64 is not None:
            x64[:, :, mask] = float(np.float32(pol.erase_fill))
        if pol.erase_label is not None:
            labels = labels.copy()
            labels[mask] = pol.erase_label
    assert x.dtype == np.float32
    return dict(geom=R.geom_row(g), raw=g, radio=radio, x=x, x64=x64, mask=mask, labels=labels, outside=outside)


def reference_batch(pol, warp, records, keys, desc, cities, S):
    """The batch through given records float32 [n][2][6] (the kernel's exported ones, or an override)."""
    return [reference_sample(pol, warp, r, int(k), d, cities, S) for r, k, d in zip(records, keys, desc)]
