"""Host restatement of fabric_amd.utils.morphology and of the bdn_cc_mark / bdn_cc_select / bdn_d2_mask / bdn_threshold_pair contract of
include/bidate_hip.h, in numpy: per-root flags on the labels of tests/cc_ref.py, the selection, an exact separable squared distance and
the functions built on them.  Written from the contract, not from the kernels; no scipy here (the GPU tests must not need it):
tests/test_morph_cpu.py pins every function to scipy.ndimage and to brute force."""
import numpy as np

from tests import cc_ref

INT_MAX = (1 << 31) - 1


def fg(mask):
    """A pixel is foreground iff it equals 1."""
    return np.asarray(mask) == 1


def mark(labels, seed=None, seed_value=1, border=False):
    """int32 [H,W]: 1 at index r if the component rooted at r has a pixel with seed == seed_value or (border) a pixel on the image edge."""
    lab = np.asarray(labels)
    hit = np.zeros(lab.shape, bool)
    if seed is not None:
        hit |= np.asarray(seed) == seed_value
    if border:
        hit[0, :] = hit[-1, :] = True
        hit[:, 0] = hit[:, -1] = True
    out = np.zeros(lab.size, np.int32)
    out[lab[hit & (lab > 0)] - 1] = 1
    return out.reshape(lab.shape)


def select(labels, mark_=None, keep_marked=True, area=None, min_area=1, max_area=INT_MAX, base=None):
    """uint8 [H,W]: (base == 1) | sel, sel as bdn_cc_select defines it."""
    lab = np.asarray(labels)
    sel = lab > 0
    root = np.where(sel, lab - 1, 0)
    if mark_ is not None:
        sel &= (np.asarray(mark_).ravel()[root] != 0) == bool(keep_marked)
    if area is not None:
        a = np.asarray(area).ravel()[root]
        sel &= (a >= min_area) & (a <= max_area)
    if base is not None:
        sel = sel | (np.asarray(base) == 1)
    return sel.astype(np.uint8)


def reconstruct(mask, seed, connectivity=8):
    lab = cc_ref.label(fg(mask), connectivity)
    return select(lab, mark(lab, seed, 1, False), True)


def threshold_pair(proba, low, high, pos_class=1):
    """(proba[pos] >= low, proba[pos] >= high) in float32, NaN giving 0."""
    p = np.asarray(proba, np.float32)[pos_class]
    with np.errstate(invalid='ignore'):
        return (p >= np.float32(low)).astype(np.uint8), (p >= np.float32(high)).astype(np.uint8)


def hysteresis_mask(proba, low, high, pos_class=1, connectivity=8):
    weak, strong = threshold_pair(proba, low, high, pos_class)
    return reconstruct(weak, strong, connectivity)


def clear_border(mask, connectivity=8):
    lab = cc_ref.label(fg(mask), connectivity)
    return select(lab, mark(lab, None, 1, True), False)


def fill_holes(mask, max_area=None, connectivity=8):
    lab = cc_ref.label(~fg(mask), 4 if connectivity == 8 else 8)
    area = None if max_area is None else cc_ref.areas(lab)
    return select(lab, mark(lab, None, 1, True), False, area, 1, INT_MAX if max_area is None else max_area, base=mask)


def d2_sep(site, limit=INT_MAX):
    """int64 [H,W]: min(limit, the squared distance to the nearest True pixel): the distance along the column first, then per row the
    minimum over the row's columns of (x - x')^2 + g(x')^2, every candidate looked at."""
    site = np.asarray(site, bool)
    h, w = site.shape
    big = 1 << 20                                        # farther than any pixel of a test raster
    ys = np.arange(h)
    g = np.full((h, w), big, np.int64)
    for x in range(w):
        rows = np.flatnonzero(site[:, x])
        if rows.size:
            g[:, x] = np.abs(ys[:, None] - rows[None, :]).min(axis=1)
    xs = np.arange(w)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                # [x, x']
    d = (dx2[None, :, :] + (g * g)[:, None, :]).min(axis=2)
    return np.minimum(d, limit)


def binary_dilation(mask, radius2):
    return (d2_sep(fg(mask), radius2 + 1) <= radius2).astype(np.uint8)


def binary_erosion(mask, radius2):
    return (d2_sep(~fg(mask), radius2 + 1) > radius2).astype(np.uint8)


def binary_opening(mask, radius2):
    return binary_dilation(binary_erosion(mask, radius2), radius2)


def binary_closing(mask, radius2):
    return binary_erosion(binary_dilation(mask, radius2), radius2)


def cleanup(mask, close_radius2=None, fill=None, open_radius2=None, connectivity=8):
    """The fixed order of predict_scene_blended behind the threshold: closing, hole filling, opening."""
    m = np.asarray(mask)
    if close_radius2 is not None:
        m = binary_closing(m, close_radius2)
    if fill is not None and fill is not False:
        m = fill_holes(m, None if fill is True else fill, connectivity)
    if open_radius2 is not None:
        m = binary_opening(m, open_radius2)
    return m


def disc(radius2):
    """bool [2k+1, 2k+1]: the structuring element {dy^2 + dx^2 <= radius2}."""
    k = int(np.floor(np.sqrt(radius2)))
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return yy * yy + xx * xx <= radius2
