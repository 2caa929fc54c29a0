"""Cleaning a change mask on the device: hysteresis thresholding, binary reconstruction, border clearing, hole filling and opening / closing
with a disc -- what scipy.ndimage.binary_propagation / binary_fill_holes / binary_dilation / binary_erosion give on the host after copying
the scene mask down (the mask of train.py:199).  Reconstruction runs on the canonical labels of bdn_cc_label through bdn_cc_mark /
bdn_cc_select, disc morphology is a threshold (bdn_d2_mask) on the exact squared distances of bdn_edt (include/bidate_hip.h): integer
kernels on the current stream, no host read, the same bits on every run.  Every function returns a uint8 [H,W] raster of 0 / 1, treats a
pixel as foreground iff it equals 1 and takes out= (which may be the input).  Nothing is cached across calls.
"""
import math

import torch

from .. import _lib
from .distance import MAX_DIM
from .objects import MAX_PIXELS, check_cc_args

INT_MAX = (1 << 31) - 1
MAX_RADIUS2 = INT_MAX - 1                               # bdn_edt's limit = radius2 + 1 is an int32


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what}: the tensors must be on the device: there is no CPU path')


def _check_like(t, mask, name):
    h, w = mask.shape
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != (h, w) or not t.is_contiguous():
        raise ValueError(f'{name} must be a contiguous uint8 [{h},{w}] tensor')
    if t.device != mask.device:
        raise ValueError(f'{name} is on {t.device}, mask on {mask.device}')


def check_reconstruct_args(mask, seed=None, connectivity=8, out=None):
    """Validate the arguments of reconstruct / clear_border without touching a device (tensors on any device).  Returns (H, W)."""
    h, w = check_cc_args(mask, connectivity)
    if seed is not None:
        _check_like(seed, mask, 'seed')
    if out is not None:
        _check_like(out, mask, 'out')
    return h, w


def check_fill_holes_args(mask, max_area=None, connectivity=8, out=None):
    """Validate the arguments of fill_holes without touching a device.  Returns (H, W)."""
    h, w = check_reconstruct_args(mask, None, connectivity, out)
    if max_area is not None and (not _is_int(max_area) or not 1 <= max_area <= INT_MAX):
        raise ValueError(f'max_area must be None or an integer 1..2^31 - 1, got {max_area!r}')
    return h, w


def check_hysteresis_args(proba, low, high, pos_class=1, connectivity=8, out=None):
    """Validate the arguments of hysteresis_mask without touching a device.  Returns (C, H, W, low, high) with the thresholds as floats."""
    if not isinstance(proba, torch.Tensor) or proba.dtype != torch.float32 or proba.dim() != 3 or not proba.is_contiguous():
        raise ValueError(f'proba must be a contiguous float32 [C,H,W] tensor, got {getattr(proba, "dtype", type(proba))} {tuple(getattr(proba, "shape", ()))}')
    c, h, w = proba.shape
    if not 2 <= c <= 256:
        raise ValueError(f'proba: need 2 <= C <= 256 classes, got {c}')
    check_cc_args(torch.empty(h, w, dtype=torch.uint8, device='meta'), connectivity, name='proba[pos_class]')
    if not _is_int(pos_class) or not 0 <= pos_class < c:
        raise ValueError(f'pos_class must be an integer 0..{c - 1}, got {pos_class!r}')
    for v, name in ((low, 'low'), (high, 'high')):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ValueError(f'{name} must be a number in [0, 1], got {v!r}')
    if not 0 <= low <= high <= 1:
        raise ValueError(f'need 0 <= low <= high <= 1, got low={low!r}, high={high!r}')
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (h, w) or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous uint8 [{h},{w}] tensor')
        if out.device != proba.device:
            raise ValueError(f'out is on {out.device}, proba on {proba.device}')
    return c, h, w, float(low), float(high)


def check_morph_args(mask, radius2, out=None):
    """Validate the arguments of binary_dilation / binary_erosion / binary_opening / binary_closing without touching a device.  Returns
    (H, W)."""
    h, w = check_cc_args(mask)
    if h > MAX_DIM or w > MAX_DIM:
        raise ValueError(f'mask: need H, W <= {MAX_DIM} (bdn_edt), got {h} x {w}')
    if not _is_int(radius2) or not 0 <= radius2 <= MAX_RADIUS2:
        raise ValueError(f'radius2 must be an integer 0..2^31 - 2 (the squared radius of the disc), got {radius2!r}')
    if out is not None:
        _check_like(out, mask, 'out')
    return h, w


def _out(mask, out):
    return torch.empty_like(mask) if out is None else out


def _labels(mask, connectivity, want_area):
    h, w = mask.shape
    dev = mask.device
    labels = torch.empty(h, w, dtype=torch.int32, device=dev)
    area = torch.empty(h, w, dtype=torch.int32, device=dev) if want_area else None
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().bdn_cc_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
    _lib.call('bdn_cc_label', _lib.ptr(mask), 1, None, 0, connectivity, h, w, _lib.ptr(labels), _lib.ptr(area), _lib.ptr(counts), _lib.ptr(ws),
              _lib.stream_ptr())
    return labels, area


def _select(mask, connectivity, seed, border, keep_marked, max_area, base, out):
    """Label mask == 1, flag the components that hold a seed pixel (seed == 1) or touch the image edge, write base | the chosen ones."""
    h, w = mask.shape
    labels, area = _labels(mask, connectivity, max_area is not None)
    mark = torch.empty(h, w, dtype=torch.int32, device=mask.device)
    st = _lib.stream_ptr()
    _lib.call('bdn_cc_mark', _lib.ptr(labels), _lib.ptr(seed), 1, int(border), _lib.ptr(mark), h, w, st)
    _lib.call('bdn_cc_select', _lib.ptr(labels), _lib.ptr(mark), int(keep_marked), _lib.ptr(area), 1, INT_MAX if max_area is None else max_area,
              _lib.ptr(base), _lib.ptr(out), h, w, st)
    return out


def reconstruct(mask, seed, connectivity=8, out=None):
    """uint8 [H,W]: the pixels of mask == 1 whose component (`connectivity` 4 or 8) contains a pixel with seed == 1 and mask == 1 --
    scipy.ndimage.binary_propagation(seed & mask, structure, mask=mask).  Six launches (three of bdn_cc_label, two of bdn_cc_mark, one of
    bdn_cc_select), no host read.  out may be mask or seed."""
    check_reconstruct_args(mask, seed, connectivity, out)
    if seed is None:
        raise ValueError('seed must be a contiguous uint8 tensor shaped like mask')
    _need_device(mask, 'reconstruct')
    return _select(mask, connectivity, seed, False, True, None, None, _out(mask, out))


def hysteresis_mask(proba, low, high, pos_class=1, connectivity=8, out=None):
    """uint8 [H,W] of a float32 [C,H,W] probability map: reconstruct(proba[pos_class] >= low, proba[pos_class] >= high) -- weak change kept
    only where it hangs on strong change.  0 <= low <= high <= 1; low == high gives the bits of bdn_threshold_mask at that threshold; a
    NaN probability is background.  Seven launches (bdn_threshold_pair, then reconstruct's six), no host read."""
    c, h, w, low, high = check_hysteresis_args(proba, low, high, pos_class, connectivity, out)
    _need_device(proba, 'hysteresis_mask')
    weak = torch.empty(h, w, dtype=torch.uint8, device=proba.device)
    strong = torch.empty_like(weak)
    _lib.call('bdn_threshold_pair', _lib.ptr(proba), pos_class, low, high, _lib.ptr(weak), _lib.ptr(strong), c, h * w, _lib.stream_ptr())
    return _select(weak, connectivity, strong, False, True, None, None, strong if out is None else out)


def clear_border(mask, connectivity=8, out=None):
    """uint8 [H,W]: mask == 1 without the components that have a pixel in the first or last row or column.  Six launches, no host read."""
    check_reconstruct_args(mask, None, connectivity, out)
    _need_device(mask, 'clear_border')
    return _select(mask, connectivity, None, True, False, None, None, _out(mask, out))


def fill_holes(mask, max_area=None, connectivity=8, out=None):
    """uint8 [H,W]: mask == 1 with its holes filled.  `connectivity` is the foreground's; the background (mask != 1) is labelled with the
    other one (8 <-> 4), and a hole is a background component with no pixel on the image edge and, with max_area given, at most max_area
    pixels.  max_area=None: scipy.ndimage.binary_fill_holes(mask) for connectivity=8, binary_fill_holes(mask, structure=np.ones((3, 3)))
    for connectivity=4.  Seven launches (the complement, bdn_cc_label's three, bdn_cc_mark's two, bdn_cc_select), no host read."""
    h, w = check_fill_holes_args(mask, max_area, connectivity, out)
    _need_device(mask, 'fill_holes')
    back = torch.empty_like(mask)
    _lib.call('bdn_mask_not', _lib.ptr(mask), _lib.ptr(back), h * w, _lib.stream_ptr())
    return _select(back, 4 if connectivity == 8 else 8, None, True, False, max_area, mask, _out(mask, out))


def _disc(mask, radius2, erode, out):
    """One threshold of one transform: dilation = d2(to the foreground) <= radius2, erosion = d2(to the background) > radius2."""
    h, w = mask.shape
    dev = mask.device
    d2 = torch.empty(h, w, dtype=torch.int32, device=dev)
    ws = torch.empty((_lib.load().bdn_edt_workspace_bytes(1, h, w) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()
    _lib.call('bdn_edt', _lib.ptr(mask), 1, 0 if erode else 1, None, 0, radius2 + 1, _lib.ptr(d2), _lib.ptr(ws), 1, h, w, st)
    _lib.call('bdn_d2_mask', _lib.ptr(d2), radius2, 1 if erode else 0, _lib.ptr(out), h * w, st)
    return out


def binary_dilation(mask, radius2, out=None):
    """uint8 [H,W]: the pixels within squared distance radius2 of a pixel with mask == 1 -- scipy.ndimage.binary_dilation with the disc
    {dy^2 + dx^2 <= radius2}; outside the image is background.  radius2 = 0 gives the 0 / 1 image of mask.  Three launches, no host read."""
    check_morph_args(mask, radius2, out)
    _need_device(mask, 'binary_dilation')
    return _disc(mask, radius2, False, _out(mask, out))


def binary_erosion(mask, radius2, out=None):
    """uint8 [H,W]: the pixels farther than squared distance radius2 from every pixel with mask != 1 -- scipy.ndimage.binary_erosion with
    the disc and border_value=1: outside the image is foreground, so the image edge does not erode and a mask without background stays
    whole.  Three launches, no host read."""
    check_morph_args(mask, radius2, out)
    _need_device(mask, 'binary_erosion')
    return _disc(mask, radius2, True, _out(mask, out))


def binary_opening(mask, radius2, out=None):
    """uint8 [H,W]: the dilation of the erosion, both with the disc of squared radius radius2: cuts spurs and specks narrower than the disc.
    Six launches, no host read."""
    check_morph_args(mask, radius2, out)
    _need_device(mask, 'binary_opening')
    out = _out(mask, out)
    return _disc(_disc(mask, radius2, True, out), radius2, False, out)


def binary_closing(mask, radius2, out=None):
    """uint8 [H,W]: the erosion of the dilation, both with the disc of squared radius radius2: bridges gaps narrower than the disc.  Six
    launches, no host read."""
    check_morph_args(mask, radius2, out)
    _need_device(mask, 'binary_closing')
    out = _out(mask, out)
    return _disc(_disc(mask, radius2, False, out), radius2, True, out)


def check_cleanup_args(threshold=None, hysteresis_low=None, close_radius2=None, fill_holes=None, open_radius2=None, connectivity=8):
    """Validate the clean-up arguments of predict_scene_blended without touching a device; returns the hole-area bound (None: off or
    every hole) -- fill_holes is None / False (off), True (every hole) or a maximum hole area >= 1."""
    meta = torch.empty(1, 1, dtype=torch.uint8, device='meta')
    check_cc_args(meta, connectivity)
    if hysteresis_low is not None:
        if threshold is None:
            raise ValueError('hysteresis_low needs a threshold (the high one)')
        if isinstance(hysteresis_low, bool) or not isinstance(hysteresis_low, (int, float)) or not 0 <= hysteresis_low <= threshold:
            raise ValueError(f'hysteresis_low must be a number in [0, threshold = {threshold!r}], got {hysteresis_low!r}')
    for v in (close_radius2, open_radius2):
        if v is not None:
            check_morph_args(meta, v)
    if fill_holes is None or isinstance(fill_holes, bool):
        return None
    check_fill_holes_args(meta, fill_holes, connectivity)
    return fill_holes


def cleanup_mask(mask, close_radius2=None, fill=None, open_radius2=None, connectivity=8):
    """The fixed clean-up order behind the threshold, in place on mask: closing, hole filling (fill: None / False off, True every hole, an
    integer the largest hole filled), opening."""
    if close_radius2 is not None:
        binary_closing(mask, close_radius2, out=mask)
    if fill is not None and fill is not False:
        fill_holes(mask, None if fill is True else fill, connectivity, out=mask)
    if open_radius2 is not None:
        binary_opening(mask, open_radius2, out=mask)
    return mask
