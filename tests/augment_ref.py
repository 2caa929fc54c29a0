"""numpy twin of bdn_sample_patches_aug: Philox4x32-10, the draws of one sample and the output patches cut from host stacks.

This file restates the specification (include/bidate_hip.h, DESIGN.md "Augmenting device-cut patches") and shares no code with the
kernel or with csrc/philox_core.hpp.  Integers are exact by construction; float32 stages use numpy float32 arithmetic, one rounding per
operation, which is what the kernel does; the noise is formed in float64 from the same words (the kernel's float32 transcendentals are
compared against it under a bar, tests/test_gpu_augment.py).  A policy is a fabric_amd.augment.PatchAugment (its fields only).
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = 0xFFFFFFFF
_MASK, _32 = np.uint64(MASK), np.uint64(32)
GEOMETRY, RADIOMETRY, NOISE = 0, 1, 2
F24 = np.float32(2.0 ** -24)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
    counter, key = np.asarray(counter, np.uint64), np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + W0) & _MASK, (k1 + W1) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def draw(seed, sample_key, stream, slot):
    """The four words of (seed, sample key, stream, slot); `slot` may be an array (-> [..., 4])."""
    slot = np.asarray(slot, np.uint64)
    ctr = np.stack(np.broadcast_arrays(np.uint64(sample_key & MASK), np.uint64(sample_key >> 32), slot, np.uint64(stream)), -1)
    return philox4x32_10(ctr, np.array([seed & MASK, seed >> 32], np.uint64))


def u(w):
    """float32(w >> 8) * 2^-24 in [0, 1): exact."""
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float32) * F24


def rng(w, n):
    """(uint64(w) * n) >> 32 in [0, n)."""
    return (np.asarray(w, np.uint64) * np.uint64(n)) >> np.uint64(32)


def sample_key(epoch, index):
    return (int(epoch) << 32) | int(index)


def geometry(pol, key, row, col, sym, H, W, S):
    """(row', col', sym, erased, top, left, eh, ew) and the raw (dy, dx) of one sample."""
    J = pol.jitter
    erase_on = pol.erase_p > 0.0
    if J == 0 and not pol.symmetry and not erase_on:
        return dict(row=row, col=col, sym=sym, erased=0, top=0, left=0, eh=0, ew=0, dy=0, dx=0)
    w = draw(pol.seed, key, GEOMETRY, 0)
    dy, dx = int(rng(w[0], 2 * J + 1)) - J, int(rng(w[1], 2 * J + 1)) - J
    out = dict(row=min(max(row + dy, 0), H - S), col=min(max(col + dx, 0), W - S), sym=int(w[2] >> np.uint32(29)) if pol.symmetry else sym,
               erased=int(erase_on and bool(u(w[3]) < np.float32(pol.erase_p))), top=0, left=0, eh=0, ew=0, dy=dy, dx=dx)
    if erase_on:
        lo, hi = pol.erase_size
        v = draw(pol.seed, key, GEOMETRY, 1)
        out['eh'], out['ew'] = lo + int(rng(v[0], hi - lo + 1)), lo + int(rng(v[1], hi - lo + 1))
        out['top'], out['left'] = int(rng(v[2], S - out['eh'] + 1)), int(rng(v[3], S - out['ew'] + 1))
    return out


def geom_row(g):
    return [g[k] for k in ('row', 'col', 'sym', 'erased', 'top', 'left', 'eh', 'ew')]


def radiometry(pol, key, C):
    """float32 [2][C][2] = (g, b); (1, 0) when the stage is off."""
    out = np.empty((2, C, 2), np.float32)
    if pol.gain == 0.0 and pol.bias == 0.0:
        out[..., 0], out[..., 1] = 1.0, 0.0
        return out
    one, two = np.float32(1), np.float32(2)
    for date in range(2):
        w = draw(pol.seed, key, RADIOMETRY, (date * C if pol.per_date else 0) + np.arange(C))
        t, t2 = two * u(w[:, 0]) - one, two * u(w[:, 1]) - one
        out[date, :, 0] = one + np.float32(pol.gain) * t
        out[date, :, 1] = np.float32(pol.bias) * t2
    return out


def noise_z64(seed, key, plane, S):
    """float64 [S][S]: the Box-Muller deviates of output plane `plane` = date * C + c, from the same words as the kernel's."""
    i, j = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    w = draw(seed, key, NOISE + plane, i * ((S + 3) // 4) + (j >> 2))
    k = (j >> 1) & 1
    a = np.take_along_axis(w, (2 * k)[..., None], -1)[..., 0]
    b = np.take_along_axis(w, (2 * k + 1)[..., None], -1)[..., 0]
    u1 = (((a >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * F24).astype(np.float64)
    u2 = u(b).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    return np.where(j & 1, r * np.sin(2.0 * np.pi * u2), r * np.cos(2.0 * np.pi * u2))


def symmetry(win, sym):
    """Transpose the last two axes if sym & 4, then reverse the rows if sym & 2, then the columns if sym & 1."""
    if sym & 4:
        win = np.swapaxes(win, -1, -2)
    if sym & 2:
        win = win[..., ::-1, :]
    if sym & 1:
        win = win[..., ::-1]
    return np.ascontiguousarray(win)


def reference_sample(pol, key, desc, cities, S):
    """One sample.  desc = (city, row, col, sym); cities[k] = {'images': float32 [2,C,H,W], 'labels': uint8 [H,W]}.
    Returns dict(geom=[8 ints], raw=geometry dict, radio=float32 [2,C,2], x=float32 [2,C,S,S] (every stage but the noise; erased),
    x64=float64 [2,C,S,S] or None (with float64 noise, when noise_std > 0; erased), mask=bool [S,S] erased pixels, labels=uint8 [S,S])."""
    city, row, col, sym = (int(v) for v in desc)
    im, lb = cities[city]['images'], cities[city]['labels']
    C, (H, W) = im.shape[1], lb.shape
    g = geometry(pol, key, row, col, sym, H, W, S)
    x = symmetry(im[:, :, g['row']:g['row'] + S, g['col']:g['col'] + S], g['sym'])
    labels = symmetry(lb[g['row']:g['row'] + S, g['col']:g['col'] + S], g['sym'])
    radio = radiometry(pol, key, C)
    if pol.gain != 0.0 or pol.bias != 0.0:
        with np.errstate(all='ignore'):
            x = radio[:, :, 0, None, None] * x + radio[:, :, 1, None, None]          # float32: the product rounds, then the sum
    x64 = None
    if pol.noise_std > 0.0:
        z = np.stack([noise_z64(pol.seed, key, p, S) for p in range(2 * C)]).reshape(2, C, S, S)
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
    return dict(geom=geom_row(g), raw=g, radio=radio, x=x, x64=x64, mask=mask, labels=labels)


def reference_batch(pol, keys, desc, cities, S):
    return [reference_sample(pol, int(k), d, cities, S) for k, d in zip(keys, desc)]
