"""Distances on the device: the exact squared Euclidean distance transform of a raster, the signed distance of the boundary loss and the
boundary scores of a predicted change mask (boundary F1 at a pixel tolerance, Csurka et al., BMVC 2013, and the Hausdorff distance) --
what scipy.ndimage.distance_transform_edt gives on the host after copying the scene mask down.  All of it runs through bdn_edt /
bdn_signed_distance / bdn_boundary_mask / bdn_boundary_score (include/bidate_hip.h) on the current stream: integer kernels, the same bits
on every run.  Allocation sizes come from the library's size queries; nothing is cached across calls.
"""
import math

import torch

from .. import _lib

MAX_DIM = 32767
MAX_PIXELS = (1 << 31) - 1
LIMIT_NONE = (1 << 31) - 1


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _byte(v, what):
    if not _is_int(v) or not 0 <= v <= 255:
        raise ValueError(f'{what} must be a byte 0..255, got {v!r}')
    return v


def check_edt_args(mask, site_value=1, equal=True, valid=None, invalid_value=None, max_dist=None, out=None, name='mask'):
    """Validate the arguments of distance_transform_sq without touching a device (any tensor with .dtype / .shape / .is_contiguous() will
    do, on any device).  Returns (N, H, W, limit)."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() not in (2, 3):
        raise ValueError(f'{name} must be a uint8 [H,W] or [N,H,W] tensor, got {getattr(mask, "dtype", type(mask))} {tuple(getattr(mask, "shape", ()))}')
    if not mask.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    n, h, w = (1,) + tuple(mask.shape) if mask.dim() == 2 else tuple(mask.shape)
    if n < 1 or h < 1 or w < 1 or h > MAX_DIM or w > MAX_DIM or n * h * w > MAX_PIXELS:
        raise ValueError(f'{name}: need 1 <= N, 1 <= H, W <= {MAX_DIM} and N * H * W < 2^31, got {n} x {h} x {w}')
    _byte(site_value, 'site_value')
    if not isinstance(equal, bool):
        raise ValueError(f'equal must be True or False, got {equal!r}')
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or tuple(valid.shape) != tuple(mask.shape) or not valid.is_contiguous():
            raise ValueError(f'valid must be a contiguous uint8 tensor shaped like {name}')
        if valid.device != mask.device:
            raise ValueError(f'valid is on {valid.device}, {name} on {mask.device}')
        _byte(invalid_value, 'invalid_value (when valid is given)')
    limit = LIMIT_NONE
    if max_dist is not None:
        if not _is_int(max_dist) or not 0 <= max_dist <= 46339:
            raise ValueError(f'max_dist must be None or an integer 0..46339 (limit = max_dist^2 + 1 fits an int32), got {max_dist!r}')
        limit = max_dist * max_dist + 1
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != tuple(mask.shape) or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous int32 tensor shaped like {name}')
        if out.device != mask.device:
            raise ValueError(f'out is on {out.device}, {name} on {mask.device}')
    return n, h, w, limit


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what}: the tensors must be on the device: there is no CPU path')


def _workspace(nbytes, device):
    return torch.empty((int(nbytes) + 15) // 16 * 16, dtype=torch.uint8, device=device)


def distance_transform_sq(mask, site_value=1, equal=True, valid=None, invalid_value=None, max_dist=None, out=None):
    """int32 tensor shaped like mask (uint8 [H,W] or [N,H,W], the images independent): the squared Euclidean distance of every pixel to the
    nearest site of its image.  A pixel is a site if mask == site_value there (equal=False: mask != site_value) and, with `valid` given,
    valid != invalid_value.  max_dist=d caps the result at d*d + 1 (every pixel farther than d reads d*d + 1); without it an image with no
    site reads 2^31 - 1 everywhere.  Exact, integers only; two launches, no host read."""
    n, h, w, limit = check_edt_args(mask, site_value, equal, valid, invalid_value, max_dist, out)
    _need_device(mask, 'distance_transform_sq')
    if out is None:
        out = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    ws = _workspace(_lib.load().bdn_edt_workspace_bytes(n, h, w), mask.device)
    _lib.call('bdn_edt', _lib.ptr(mask), site_value, int(equal), _lib.ptr(valid), 0 if valid is None else invalid_value, limit, _lib.ptr(out),
              _lib.ptr(ws), n, h, w, _lib.stream_ptr())
    return out


def check_signed_distance_args(labels, cls, ignore_index=None, max_dist=None):
    """Validate the arguments of signed_distance without touching a device.  Returns (N, H, W)."""
    n, h, w, _ = check_edt_args(labels, name='labels')
    if 2 * n * h * w > MAX_PIXELS:
        raise ValueError(f'labels: 2 * N * H * W must stay below 2^31, got {n} x {h} x {w}')
    _byte(cls, 'cls')
    if ignore_index is not None:
        _byte(ignore_index, 'ignore_index')
    if max_dist is not None and not (isinstance(max_dist, (int, float)) and not isinstance(max_dist, bool) and max_dist > 0 and math.isfinite(max_dist)):
        raise ValueError(f'max_dist must be None or a positive number, got {max_dist!r}')
    return n, h, w


def signed_distance(labels, cls, ignore_index=None, max_dist=None):
    """float32 tensor shaped like labels (uint8 [H,W] or [N,H,W]): the signed distance phi of class cls that the boundary loss uses (the
    Criterion's w_boundary; bdn_boundary_loss in include/bidate_hip.h): +distance to the nearest pixel of the class outside it,
    -(distance to the nearest other pixel - 1) inside, 0 at pixels with label ignore_index and over an image where the class is absent
    or fills every valid pixel.  max_dist clamps to [-max_dist, max_dist]."""
    n, h, w = check_signed_distance_args(labels, cls, ignore_index, max_dist)
    _need_device(labels, 'signed_distance')
    phi = torch.empty(labels.shape, dtype=torch.float32, device=labels.device)
    ws = _workspace(_lib.load().bdn_signed_distance_workspace_bytes(n, h, w), labels.device)
    _lib.call('bdn_signed_distance', _lib.ptr(labels), cls, -1 if ignore_index is None else ignore_index, float(max_dist or 0.0), _lib.ptr(ws),
              _lib.ptr(phi), n, h, w, _lib.stream_ptr())
    return phi


def check_boundary_args(pred_mask, truth, tolerance=2, pos_class=1, ignore_index=None):
    """Validate the arguments of boundary_scores without touching a device.  Returns (H, W)."""
    for t, name in ((pred_mask, 'pred_mask'), (truth, 'truth')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous uint8 [H,W] tensor')
    if tuple(truth.shape) != tuple(pred_mask.shape) or truth.device != pred_mask.device:
        raise ValueError(f'truth must be shaped like pred_mask and on its device, got {tuple(truth.shape)} on {truth.device}')
    h, w = pred_mask.shape
    if h < 1 or w < 1 or h > MAX_DIM or w > MAX_DIM or 2 * h * w > MAX_PIXELS:
        raise ValueError(f'pred_mask: need 1 <= H, W <= {MAX_DIM} and 2 * H * W < 2^31, got {h} x {w}')
    check_boundary_tolerance(tolerance)
    _byte(pos_class, 'pos_class')
    if ignore_index is not None:
        _byte(ignore_index, 'ignore_index')
    return h, w


def check_boundary_tolerance(tolerance):
    """The pixel tolerance of boundary F1: a whole number of pixels 0..32767."""
    if not _is_int(tolerance) or not 0 <= tolerance <= MAX_DIM:
        raise ValueError(f'tolerance must be an integer 0..{MAX_DIM} (pixels), got {tolerance!r}')
    return tolerance


def boundary_counts(pred_mask, truth, tolerance=2, pos_class=1, ignore_index=None):
    """int64[6] device tensor {n_pred, n_true, pred_hit, true_hit, hd2_pred_to_true, hd2_true_to_pred} of boundary_scores; no host read."""
    h, w = check_boundary_args(pred_mask, truth, tolerance, pos_class, ignore_index)
    _need_device(pred_mask, 'boundary_scores')
    dev, st = pred_mask.device, _lib.stream_ptr()
    valid, inv = (truth, ignore_index) if ignore_index is not None else (None, 0)
    bnd = torch.empty(2, h, w, dtype=torch.uint8, device=dev)
    _lib.call('bdn_boundary_mask', _lib.ptr(pred_mask), 1, _lib.ptr(valid), inv, bnd[0].data_ptr(), h, w, st)
    _lib.call('bdn_boundary_mask', _lib.ptr(truth), pos_class, _lib.ptr(valid), inv, bnd[1].data_ptr(), h, w, st)
    d2 = distance_transform_sq(bnd)
    out = torch.empty(6, dtype=torch.int64, device=dev)
    _lib.call('bdn_boundary_score', _lib.ptr(bnd), _lib.ptr(d2), tolerance * tolerance, _lib.ptr(out), h, w, st)
    return out


def scores_from_counts(counts, tolerance):
    """The host values of boundary_scores from the six integers."""
    n_pred, n_true, pred_hit, true_hit, hd_pt, hd_tp = (int(v) for v in counts)
    p = pred_hit / n_pred if n_pred else 0.0
    r = true_hit / n_true if n_true else 0.0
    f = 2 * p * r / (p + r) if p + r else 0.0
    hd2 = max(hd_pt, hd_tp)
    return {'n_pred': n_pred, 'n_true': n_true, 'pred_hit': pred_hit, 'true_hit': true_hit, 'hd2_pred_to_true': hd_pt, 'hd2_true_to_pred': hd_tp,
            'boundary_precision': p, 'boundary_recall': r, 'boundary_f1': f, 'hausdorff': math.sqrt(hd2) if hd2 >= 0 else None,
            'boundary_tol': tolerance}


def boundary_scores(pred_mask, truth, tolerance=2, pos_class=1, ignore_index=None):
    """Contour quality of a predicted change mask (uint8, 1 = change) against a truth raster (uint8 class indices), both [H,W] on the device.
    Foreground is pred_mask == 1, or truth == pos_class; valid is truth != ignore_index.  A foreground pixel is on the boundary if it is
    valid and one of its 4-neighbours inside the image is valid and not foreground: the image edge and the ignore region make no contour.
    pred_hit / true_hit count the boundary pixels within `tolerance` pixels (Euclidean) of the other boundary; boundary_precision =
    pred_hit / n_pred, boundary_recall = true_hit / n_true, boundary_f1 their harmonic mean (0 where a ratio has no denominator, the rule
    of object_scores); hausdorff = the largest distance from a boundary pixel to the other boundary, None (hd2_* = -1) if either boundary
    is empty.  One host read, at the end."""
    return scores_from_counts(boundary_counts(pred_mask, truth, tolerance, pos_class, ignore_index).tolist(), tolerance)
