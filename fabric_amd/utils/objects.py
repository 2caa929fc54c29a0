"""Objects of a change mask on the device: connected-component labels, removal of small components, a per-object table and object-level
precision / recall / F1 -- what scipy.ndimage.label + np.bincount give on the host after copying the scene mask down (the mask of
train.py:199).  All of it runs through bdn_cc_label / bdn_cc_compact / bdn_cc_filter / bdn_cc_stats (include/bidate_hip.h) on the current
stream: integer kernels, the same bits on every run.  Allocation sizes come from bdn_cc_workspace_bytes; nothing is cached across calls.
"""
import torch

from .. import _lib

MAX_PIXELS = (1 << 31) - 2


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_cc_args(mask, connectivity=8, fg_value=1, exclude=None, exclude_value=None, min_area=1, name='mask'):
    """Validate the arguments of the functions below without touching a device (any tensor with .dtype / .shape / .is_contiguous() will
    do, on any device).  Returns (H, W)."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() != 2:
        raise ValueError(f'{name} must be a uint8 [H,W] tensor, got {getattr(mask, "dtype", type(mask))} {tuple(getattr(mask, "shape", ()))}')
    if not mask.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    h, w = mask.shape
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError(f'{name}: need 1 <= H, W and H * W <= 2^31 - 2, got {h} x {w}')
    if not _is_int(connectivity) or connectivity not in (4, 8):
        raise ValueError(f'connectivity must be 4 or 8, got {connectivity!r}')
    if not _is_int(fg_value) or not 0 <= fg_value <= 255:
        raise ValueError(f'fg_value must be a byte 0..255, got {fg_value!r}')
    if not _is_int(min_area) or min_area < 1:
        raise ValueError(f'min_area must be an integer >= 1, got {min_area!r}')
    if exclude is not None:
        if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.uint8 or tuple(exclude.shape) != (h, w) or not exclude.is_contiguous():
            raise ValueError(f'exclude must be a contiguous uint8 [{h},{w}] tensor like {name}')
        if exclude.device != mask.device:
            raise ValueError(f'exclude is on {exclude.device}, {name} on {mask.device}')
        if not _is_int(exclude_value) or not 0 <= exclude_value <= 255:
            raise ValueError(f'exclude_value must be a byte 0..255 when exclude is given, got {exclude_value!r}')
    return h, w


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what}: the tensors must be on the device: there is no CPU path')


def _label(mask, connectivity, fg_value, exclude, exclude_value, want_area):
    """(labels, area or None, counts, workspace): the three launches of bdn_cc_label, no host read."""
    h, w = mask.shape
    dev = mask.device
    labels = torch.empty(h, w, dtype=torch.int32, device=dev)
    area = torch.empty(h, w, dtype=torch.int32, device=dev) if want_area else None
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().bdn_cc_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
    _lib.call('bdn_cc_label', _lib.ptr(mask), fg_value, _lib.ptr(exclude), 0 if exclude is None else exclude_value, connectivity, h, w,
              _lib.ptr(labels), _lib.ptr(area), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr())
    return labels, area, counts, ws


def _read_counts(counts):
    c = counts.tolist()                                   # the one host read
    if c[2] != 0:
        raise RuntimeError('bdn_cc_label hit an iteration cap (counts[2] != 0): the labels are not valid')
    return c


def label_components(mask, connectivity=8, fg_value=1, exclude=None, exclude_value=None, compact=True):
    """Connected components of the pixels mask == fg_value (a pixel with exclude == exclude_value is background).  Returns (labels int32
    [H,W], n): compact=True: 0 on background and 1..n elsewhere, numbered by each component's first pixel in raster order
    (scipy.ndimage.label's numbering); compact=False: 1 + the smallest linear index y * W + x of the pixel's component.  n is one host read;
    RuntimeError if the kernels report an iteration cap."""
    h, w = check_cc_args(mask, connectivity, fg_value, exclude, exclude_value)
    _need_device(mask, 'label_components')
    labels, _, counts, ws = _label(mask, connectivity, fg_value, exclude, exclude_value, False)
    if compact:
        out = torch.empty_like(labels)
        _lib.call('bdn_cc_compact', _lib.ptr(labels), h, w, _lib.ptr(out), None, _lib.ptr(ws), _lib.stream_ptr())
        labels = out
    return labels, _read_counts(counts)[0]


def remove_small_objects(mask, min_area, connectivity=8, out=None):
    """uint8 [H,W]: 1 where mask == 1 and the pixel's component has at least min_area pixels, else 0.  No host read.  out: the tensor to
    write (it may be mask itself)."""
    h, w = check_cc_args(mask, connectivity, min_area=min_area)
    _need_device(mask, 'remove_small_objects')
    if out is None:
        out = torch.empty_like(mask)
    else:
        check_cc_args(out, name='out')
        if tuple(out.shape) != (h, w) or out.device != mask.device:
            raise ValueError(f'out must be a uint8 [{h},{w}] tensor on {mask.device}')
    labels, area, _, _ = _label(mask, connectivity, 1, None, None, True)
    _lib.call('bdn_cc_filter', _lib.ptr(mask), _lib.ptr(labels), _lib.ptr(area), min_area, _lib.ptr(out), h, w, _lib.stream_ptr())
    return out


def component_table(labels, n, other=None, other_value=1):
    """int32 [n, 8] device tensor = {area, ymin, xmin, ymax, xmax, overlap, 0, 0} of the compact labels 1..n (label_components); overlap =
    the component's pixels with other == other_value (other: uint8 [H,W]; None: 0)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.dim() != 2 or not labels.is_contiguous():
        raise ValueError('labels must be a contiguous int32 [H,W] tensor')
    h, w = labels.shape
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError(f'labels: need 1 <= H, W and H * W <= 2^31 - 2, got {h} x {w}')
    if not _is_int(n) or n < 0:
        raise ValueError(f'n must be a non-negative integer, got {n!r}')
    if other is not None:
        if not isinstance(other, torch.Tensor) or other.dtype != torch.uint8 or tuple(other.shape) != (h, w) or not other.is_contiguous():
            raise ValueError(f'other must be a contiguous uint8 [{h},{w}] tensor')
        if not _is_int(other_value) or not 0 <= other_value <= 255:
            raise ValueError(f'other_value must be a byte 0..255, got {other_value!r}')
    _need_device(labels, 'component_table')
    table = torch.empty(n, 8, dtype=torch.int32, device=labels.device)
    if n:
        _lib.call('bdn_cc_stats', _lib.ptr(labels), n, _lib.ptr(other), other_value if other is not None else 0, -1, h, w, _lib.ptr(table),
                  _lib.stream_ptr())
    return table


def object_scores(pred_mask, truth, pos_class=1, ignore_index=None, connectivity=8, min_area=1, min_overlap=1):
    """Object-level scores of a predicted change mask (uint8, 1 = change) against a truth raster (uint8 class indices).  Predicted objects:
    the components of pred_mask == 1 outside truth == ignore_index, those below min_area pixels dropped; true objects: the components of
    truth == pos_class.  A predicted object is hit when at least min_overlap of its pixels are truth == pos_class, a true object when at
    least min_overlap of its pixels lie on a kept predicted object.  Returns {objects_pred, objects_true, pred_hit, true_hit,
    object_precision = pred_hit / objects_pred, object_recall = true_hit / objects_true, object_f1} (0 where a ratio has no denominator,
    the rule of batch_prf_from_counts).  One host read, at the end.
    Memory: the object counts stay on the device until that read, so each of the two tables is sized by the most components the raster can
    hold -- 32 bytes x ceil(H / 2) ceil(W / 2) rows under 8-connectivity (0.8 GB for a 10 000^2 scene), 32 bytes x ceil(H W / 2) under
    4-connectivity (1.6 GB) -- one table at a time, beside about 12 bytes per pixel of labels, areas and workspace per labelling."""
    h, w = check_cc_args(pred_mask, connectivity, 1, truth, 0 if ignore_index is None else ignore_index, min_area, name='pred_mask')
    if not _is_int(pos_class) or not 0 <= pos_class <= 255:
        raise ValueError(f'pos_class must be a byte 0..255, got {pos_class!r}')
    if not _is_int(min_overlap) or min_overlap < 1:
        raise ValueError(f'min_overlap must be an integer >= 1, got {min_overlap!r}')
    _need_device(pred_mask, 'object_scores')
    st = _lib.stream_ptr()
    excl = truth if ignore_index is not None else None
    labels, area, c_all, ws = _label(pred_mask, connectivity, 1, excl, ignore_index, True)
    kept = torch.empty_like(pred_mask)
    _lib.call('bdn_cc_filter', _lib.ptr(pred_mask), _lib.ptr(labels), _lib.ptr(area), min_area, _lib.ptr(kept), h, w, st)
    if min_area > 1:                                      # the kept objects, numbered afresh
        labels, _, c_pred, ws = _label(kept, connectivity, 1, None, None, False)
    else:
        c_pred = c_all
    comp_p = torch.empty_like(labels)
    _lib.call('bdn_cc_compact', _lib.ptr(labels), h, w, _lib.ptr(comp_p), None, _lib.ptr(ws), st)
    lab_t, _, c_true, ws_t = _label(truth, connectivity, pos_class, None, None, False)
    comp_t = torch.empty_like(lab_t)
    _lib.call('bdn_cc_compact', _lib.ptr(lab_t), h, w, _lib.ptr(comp_t), None, _lib.ptr(ws_t), st)
    # The object counts are on the device and the host reads once, at the end, so the tables are sized by the most components a raster
    # can hold (every other pixel under 4-connectivity, every other pixel of every other row under 8); rows past the last object hold
    # overlap 0 and never count as hit.  32 bytes per row: 0.8 GB for a 10 000^2 scene under 8-connectivity, freed before the next one.
    n_bound = (h * w + 1) // 2 if connectivity == 4 else ((h + 1) // 2) * ((w + 1) // 2)
    if n_bound > (1 << 28) - 1:
        raise ValueError(f'object_scores: a {h} x {w} raster can hold more than 2^28 - 1 objects; score it in parts')
    pred_hit = (component_table(comp_p, n_bound, truth, pos_class)[:, 5] >= min_overlap).sum(dtype=torch.int32)
    true_hit = (component_table(comp_t, n_bound, kept, 1)[:, 5] >= min_overlap).sum(dtype=torch.int32)
    c_all, c_pred, c_true, hits = torch.cat([c_all, c_pred, c_true, torch.stack([pred_hit, true_hit, pred_hit * 0, pred_hit * 0])]).view(4, 4).tolist()
    if c_all[2] or c_pred[2] or c_true[2]:
        raise RuntimeError('bdn_cc_label hit an iteration cap (counts[2] != 0): the labels are not valid')
    n_pred, n_true, pred_hit, true_hit = c_pred[0], c_true[0], hits[0], hits[1]
    p = pred_hit / n_pred if n_pred else 0.0
    r = true_hit / n_true if n_true else 0.0
    f = 2 * p * r / (p + r) if p + r else 0.0
    return {'objects_pred': n_pred, 'objects_true': n_true, 'pred_hit': pred_hit, 'true_hit': true_hit,
            'object_precision': p, 'object_recall': r, 'object_f1': f}
