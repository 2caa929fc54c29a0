"""The definitions behind bdn_edt, bdn_boundary_loss and the boundary scores, restated on the host: a brute-force integer squared distance,
the scipy-derived one (rint(distance_transform_edt(~site)^2): tests/test_edt_cpu.py pins the two to each other), the signed distance phi,
the boundary sets through scipy's binary_erosion, the boundary scores, and the float64 term and gradient of the boundary loss."""
import math

import numpy as np

LIMIT = (1 << 31) - 1


def sites(src, site_value=1, equal=True, valid=None, invalid_value=None):
    s = (src == site_value) if equal else (src != site_value)
    if valid is not None:
        s = s & (valid != invalid_value)
    return s


def d2_brute(site, limit=LIMIT):
    """int64 [H,W]: min(limit, min over the sites of dy^2 + dx^2), by looking at every site from every pixel."""
    site = np.asarray(site, dtype=bool)
    h, w = site.shape
    ys, xs = np.nonzero(site)
    out = np.full((h, w), limit, dtype=np.int64)
    if ys.size:
        yy, xx = np.mgrid[0:h, 0:w]
        d = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
        out = np.minimum(out, d.min(axis=-1))
    return out


def d2_ref(site, limit=LIMIT):
    """The same through scipy: exact because the float64 distances are square roots of integers far below 2^52."""
    from scipy import ndimage
    site = np.asarray(site, dtype=bool)
    if not site.any():
        return np.full(site.shape, limit, dtype=np.int64)
    d = ndimage.distance_transform_edt(~site)
    return np.minimum(np.rint(d * d).astype(np.int64), limit)


def phi_ref(labels, cls, ignore=None, max_dist=None):
    """float32 [H,W] of one image: the signed distance of class cls (include/bidate_hip.h, bdn_boundary_loss)."""
    labels = np.asarray(labels)
    valid = np.ones(labels.shape, bool) if ignore is None else labels != ignore
    fg, bg = valid & (labels == cls), valid & (labels != cls)
    phi = np.zeros(labels.shape, np.float32)
    if fg.any() and bg.any():
        to_fg = np.sqrt(d2_ref(fg).astype(np.float64)).astype(np.float32)          # float32(sqrt64(n)) == sqrtf(n) for these integers
        to_bg = np.sqrt(d2_ref(bg).astype(np.float64)).astype(np.float32)
        phi = np.where(bg, to_fg, np.where(fg, -(to_bg - np.float32(1)), np.float32(0))).astype(np.float32)
    if max_dist:
        phi = np.clip(phi, -np.float32(max_dist), np.float32(max_dist))
    return phi


def included(ncls, classes_all):
    return list(range(0 if classes_all else 1, ncls))


def boundary_loss_ref(logits, labels, ignore=None, classes_all=False, max_dist=None):
    """(term, dterm/dlogits float64 [B,C,H,W], phi float32 [C,B,H,W]) of float [B,C,H,W] logits and uint8 [B,H,W] labels.  The logits of
    ignored pixels are not looked at."""
    logits = np.asarray(logits, dtype=np.float64)
    b, c, h, w = logits.shape
    valid = np.ones(labels.shape, bool) if ignore is None else labels != ignore
    phi = np.zeros((c, b, h, w), np.float32)
    for k in included(c, classes_all):
        for i in range(b):
            phi[k, i] = phi_ref(labels[i], k, ignore, max_dist)
    z = np.where(valid[:, None], logits, 0.0)
    z = z - z.max(axis=1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(axis=1, keepdims=True)
    n = int(valid.sum())
    q = phi.transpose(1, 0, 2, 3).astype(np.float64)                                # [B,C,H,W]; 0 for a class that is not included
    if n == 0:
        return 0.0, np.zeros_like(logits), phi
    s = (p * q).sum(axis=1, keepdims=True)
    term = float((s[:, 0] * valid).sum() / n)
    grad = p * (q - s) / n * valid[:, None]
    return term, grad, phi


def boundary_ref(fg, valid):
    """valid & fg & ~binary_erosion(fg | ~valid, 4-neighbour cross, border_value=1)."""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    return valid & fg & ~ndimage.binary_erosion(fg | ~valid, structure=cross, border_value=1)


def boundary_scores_ref(pred_mask, truth, tolerance=2, pos_class=1, ignore=None):
    valid = np.ones(truth.shape, bool) if ignore is None else truth != ignore
    bp, bt = boundary_ref(pred_mask == 1, valid), boundary_ref(truth == pos_class, valid)
    n_pred, n_true = int(bp.sum()), int(bt.sum())
    d_to_p, d_to_t = d2_ref(bp), d2_ref(bt)
    pred_hit, true_hit = int((d_to_t[bp] <= tolerance ** 2).sum()), int((d_to_p[bt] <= tolerance ** 2).sum())
    both = n_pred > 0 and n_true > 0
    hd_pt = int(d_to_t[bp].max()) if both else -1
    hd_tp = int(d_to_p[bt].max()) if both else -1
    p = pred_hit / n_pred if n_pred else 0.0
    r = true_hit / n_true if n_true else 0.0
    f = 2 * p * r / (p + r) if p + r else 0.0
    hd2 = max(hd_pt, hd_tp)
    return {'n_pred': n_pred, 'n_true': n_true, 'pred_hit': pred_hit, 'true_hit': true_hit, 'hd2_pred_to_true': hd_pt, 'hd2_true_to_pred': hd_tp,
            'boundary_precision': p, 'boundary_recall': r, 'boundary_f1': f, 'hausdorff': math.sqrt(hd2) if hd2 >= 0 else None,
            'boundary_tol': tolerance}


PATTERNS = ('empty', 'full', 'corner00', 'corner01', 'corner10', 'corner11', 'row', 'column', 'checker', 'rand2', 'rand50', 'rand98')


def pattern(name, h, w, seed=0):
    """uint8 [H,W] of 0 / 1."""
    m = np.zeros((h, w), np.uint8)
    if name == 'full':
        m[:] = 1
    elif name.startswith('corner'):
        m[(h - 1) * int(name[6]), (w - 1) * int(name[7])] = 1
    elif name == 'row':
        m[h // 2] = 1
    elif name == 'column':
        m[:, w // 2] = 1
    elif name == 'checker':
        m[(np.add.outer(np.arange(h), np.arange(w)) & 1) == 1] = 1
    elif name.startswith('rand'):
        m = (np.random.default_rng(seed + h * 131 + w).random((h, w)) < int(name[4:]) / 100).astype(np.uint8)
    elif name != 'empty':
        raise ValueError(name)
    return m
