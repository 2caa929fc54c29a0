"""Co-registration of the two dates of a scene on the device: the shift of date 2 against date 1 is estimated by normalised
cross-correlation over the integer shifts of a search window, per cell of a grid and for the whole scene, refined to a fraction of a pixel by
a parabola through the peak, and date 2 is resampled through the shift field -- what a search loop in numpy and
scipy.ndimage.map_coordinates give on the host after copying both stacks down.  All of it runs through bdn_shift_corr / bdn_shift_peak /
bdn_shift_apply (include/bidate_hip.h) on the current stream: double sums in a fixed order, the same bits on every run.  Sign convention:
d2(y + dy, x + dx) ~ d1(y, x), so apply_shift(d2, field) lies on date 1's grid; labels stay in date 1's frame.  Allocation sizes come from
the library's size query; nothing is cached across calls.
"""
import numpy as np
import torch

from .. import _lib

MAX_SHIFT = 16
MAX_CELLS = 64
MAX_BANDS = 64
MAX_DIM = 32767
MAX_CHANNELS = 65535


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _check_scene(t, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3:
        raise ValueError(f'{name} must be a float32 [C,H,W] tensor, got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    c, h, w = t.shape
    if not (1 <= c <= MAX_CHANNELS and 1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f'{name}: need 1 <= C <= {MAX_CHANNELS} and 1 <= H, W <= {MAX_DIM}, got {c} x {h} x {w}')
    return c, h, w


def check_cells(cells, h, w):
    """The cell grid (ny, nx): 1..64 each, no more cells than pixels along an axis."""
    if not (isinstance(cells, (tuple, list)) and len(cells) == 2 and all(_is_int(v) for v in cells)):
        raise ValueError(f'cells must be a pair of integers (ny, nx), got {cells!r}')
    ny, nx = cells
    if not (1 <= ny <= MAX_CELLS and 1 <= nx <= MAX_CELLS and ny <= h and nx <= w):
        raise ValueError(f'cells: need 1 <= ny <= min({MAX_CELLS}, H) and 1 <= nx <= min({MAX_CELLS}, W), got {ny} x {nx} on a {h} x {w} scene')
    return ny, nx


def check_estimate_args(d1, d2, max_shift=8, bands=None, cells=(1, 1), exclude=None, exclude_value=None, min_ncc=0.0):
    """Validate the arguments of estimate_shift without touching a device (any tensor with .dtype / .shape / .is_contiguous() will do, on
    any device).  Returns (C, H, W, R, band list, ny, nx)."""
    c, h, w = _check_scene(d1, 'd1')
    if _check_scene(d2, 'd2') != (c, h, w):
        raise ValueError(f'd2 must be shaped like d1, got {tuple(d2.shape)} against {tuple(d1.shape)}')
    if d2.device != d1.device:
        raise ValueError(f'd2 is on {d2.device}, d1 on {d1.device}')
    if not _is_int(max_shift) or not 1 <= max_shift <= MAX_SHIFT:
        raise ValueError(f'max_shift must be an integer 1..{MAX_SHIFT} (pixels), got {max_shift!r}')
    if bands is None:
        bands = list(range(c))
    if not isinstance(bands, (tuple, list)) or not all(_is_int(b) for b in bands):
        raise ValueError(f'bands must be None or a list of band indices, got {bands!r}')
    if not 1 <= len(bands) <= MAX_BANDS:
        raise ValueError(f'bands: 1..{MAX_BANDS} indices, got {len(bands)}' + (' (name a subset with bands=)' if len(bands) > MAX_BANDS else ''))
    if any(not 0 <= b < c for b in bands):
        raise ValueError(f'bands: indices must lie in [0, {c}), got {list(bands)}')
    ny, nx = check_cells(cells, h, w)
    if exclude is not None:
        if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.uint8 or tuple(exclude.shape) != (h, w) or not exclude.is_contiguous():
            raise ValueError(f'exclude must be a contiguous uint8 [H,W] tensor shaped like the scene ({h} x {w})')
        if exclude.device != d1.device:
            raise ValueError(f'exclude is on {exclude.device}, d1 on {d1.device}')
        if not _is_int(exclude_value) or not 0 <= exclude_value <= 255:
            raise ValueError(f'exclude_value (when exclude is given) must be a byte 0..255, got {exclude_value!r}')
    if isinstance(min_ncc, bool) or not isinstance(min_ncc, (int, float)) or not -1.0 <= min_ncc <= 1.0:
        raise ValueError(f'min_ncc must be a number in [-1, 1], got {min_ncc!r}')
    return c, h, w, max_shift, list(bands), ny, nx


def check_apply_args(d2, field, out=None, oob=None):
    """Validate the arguments of apply_shift without touching a device.  Returns (C, H, W, ny, nx)."""
    c, h, w = _check_scene(d2, 'd2')
    if not isinstance(field, torch.Tensor) or field.dtype != torch.float32 or field.dim() != 3 or field.shape[2] != 2 or not field.is_contiguous():
        raise ValueError('field must be a contiguous float32 [ny,nx,2] tensor')
    if field.device != d2.device:
        raise ValueError(f'field is on {field.device}, d2 on {d2.device}')
    ny, nx = check_cells((int(field.shape[0]), int(field.shape[1])), h, w)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (c, h, w) or not out.is_contiguous():
            raise ValueError('out must be a contiguous float32 tensor shaped like d2')
        if out.device != d2.device:
            raise ValueError(f'out is on {out.device}, d2 on {d2.device}')
        if out is d2 or (out.device.type != 'meta' and out.data_ptr() == d2.data_ptr()):
            raise ValueError('out must not be d2: every output pixel reads four source pixels')
    if oob is not None:
        if not isinstance(oob, torch.Tensor) or oob.dtype != torch.uint8 or tuple(oob.shape) != (h, w) or not oob.is_contiguous():
            raise ValueError(f'oob must be a contiguous uint8 [H,W] tensor shaped like the scene ({h} x {w})')
        if oob.device != d2.device:
            raise ValueError(f'oob is on {oob.device}, d2 on {d2.device}')
    return c, h, w, ny, nx


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what}: the tensors must be on the device: there is no CPU path')


class ShiftEstimate:
    """What estimate_shift leaves on the device: .field float32 [ny,nx,2] = (dy, dx) per cell (a cell that is not ok or below min_ncc holds
    the whole-scene shift), .report float64 [ny*nx + 1, 4] = {dy, dx, ncc, ok}, the last row the whole scene, and .table, the float64
    [n_b,ny,nx,2R+1,2R+1,6] sums.  .read() is the one host read."""

    def __init__(self, field, report, table, max_shift, bands, cells, min_ncc):
        self.field, self.report, self.table = field, report, table
        self.max_shift, self.bands, self.cells, self.min_ncc = max_shift, list(bands), tuple(cells), float(min_ncc)

    def read(self):
        """{'dy', 'dx', 'ncc', 'ok'}: the whole scene; 'cells': float64 numpy [ny,nx,4] of the same per cell; 'field': float32 numpy
        [ny,nx,2]; 'cells_ok': how many cells kept their own shift (ok and ncc >= min_ncc)."""
        ny, nx = self.cells
        both = torch.cat([self.report.flatten(), self.field.flatten().double()]).cpu().numpy()      # float32 -> float64 is exact
        rep = both[:4 * (ny * nx + 1)].reshape(-1, 4)
        field = both[rep.size:].astype(np.float32).reshape(ny, nx, 2)
        cells = rep[:-1].reshape(ny, nx, 4)
        own = (cells[..., 3] != 0) & ~(cells[..., 2] < self.min_ncc)
        return {'dy': float(rep[-1, 0]), 'dx': float(rep[-1, 1]), 'ncc': float(rep[-1, 2]), 'ok': bool(rep[-1, 3]), 'cells': cells,
                'field': field, 'cells_ok': int(own.sum())}


def _workspace(nbytes, device):
    return torch.empty((int(nbytes) + 15) // 16 * 16, dtype=torch.uint8, device=device)


def estimate_shift(d1, d2, max_shift=8, bands=None, cells=(1, 1), exclude=None, exclude_value=None, min_ncc=0.0):
    """The shift of d2 against d1 (float32 [C,H,W] device tensors, one scene each): d2(y + dy, x + dx) ~ d1(y, x), searched over
    |dy|, |dx| <= max_shift (1..16) on the bands named (indices; default all, at most 64), per cell of the grid `cells` = (ny, nx) and
    for the whole scene.  Pixels where `exclude` (uint8 [H,W]) equals exclude_value, and NaN / infinite pixels, take no part.  Returns a
    ShiftEstimate; three launches, no host read."""
    c, h, w, r, bands, ny, nx = check_estimate_args(d1, d2, max_shift, bands, cells, exclude, exclude_value, min_ncc)
    _need_device(d1, 'estimate_shift')
    dev, st, s = d1.device, _lib.stream_ptr(), 2 * r + 1
    nb = len(bands)
    band_t = torch.tensor(bands, dtype=torch.int32).to(dev)
    table = torch.empty(nb, ny, nx, s, s, 6, dtype=torch.float64, device=dev)
    report = torch.empty(ny * nx + 1, 4, dtype=torch.float64, device=dev)
    field = torch.empty(ny, nx, 2, dtype=torch.float32, device=dev)
    ws = _workspace(_lib.load().bdn_shift_corr_workspace_bytes(nb, h, w, r, ny, nx), dev)
    _lib.call('bdn_shift_corr', _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(band_t), nb, _lib.ptr(exclude), 0 if exclude is None else exclude_value,
              r, ny, nx, _lib.ptr(table), _lib.ptr(ws), c, h, w, st)
    _lib.call('bdn_shift_peak', _lib.ptr(table), nb, r, ny, nx, float(min_ncc), _lib.ptr(report), _lib.ptr(field), st)
    return ShiftEstimate(field, report, table, r, bands, (ny, nx), min_ncc)


def apply_shift(d2, field, out=None, oob=None):
    """d2 (float32 [C,H,W]) resampled bilinearly at (y + s_y, x + s_x), s the float32 [ny,nx,2] field interpolated between cell centres,
    with a replicate border; `oob` (uint8 [H,W]) is set to 1 where a tap of non-zero weight lies outside the scene.  A zero field returns
    finite inputs bit for bit, an integer shift moves bits.  One launch; returns out (a new tensor unless given; never d2)."""
    c, h, w, ny, nx = check_apply_args(d2, field, out, oob)
    _need_device(d2, 'apply_shift')
    if out is None:
        out = torch.empty_like(d2)
    _lib.call('bdn_shift_apply', _lib.ptr(d2), _lib.ptr(field), ny, nx, _lib.ptr(out), _lib.ptr(oob), c, h, w, _lib.stream_ptr())
    return out


def coregister(d1, d2, max_shift=8, bands=None, cells=(1, 1), exclude=None, exclude_value=None, min_ncc=0.0, out=None, oob=None):
    """(d2 on date 1's grid, the ShiftEstimate): estimate_shift then apply_shift with the estimated field, enqueued back to back -- the
    host reads nothing in between."""
    est = estimate_shift(d1, d2, max_shift, bands, cells, exclude, exclude_value, min_ncc)
    return apply_shift(d2, est.field, out, oob), est


def coregister_cities(full_load, max_shift=8, bands=None, cells=(1, 1), min_ncc=0.0, ignore_label=None, device='cuda'):
    """Align date 2 of every city of a `full_load` dict ({city: {'images': float32 [2,C,H,W], 'labels': uint8 [H,W]}}) to its date 1, in
    place: device stacks are rewritten on the device, numpy stacks are uploaded, aligned and written back into the same arrays (numpy in,
    numpy out).  Date 1 is never written; labels stay in date 1's frame and are untouched unless ignore_label (a byte) is given: label
    pixels whose date-2 taps lie outside the scene (apply_shift's oob) then become ignore_label, and pixels that already hold it are
    excluded from the estimate.  Returns {city: ShiftEstimate.read()}; one host read per city, after its launches."""
    if ignore_label is not None and (not _is_int(ignore_label) or not 0 <= ignore_label <= 255):
        raise ValueError(f'ignore_label must be None or a byte 0..255, got {ignore_label!r}')
    reports = {}
    for city, d in full_load.items():
        images, labels = d['images'], d['labels']
        host = not torch.is_tensor(images)
        stack = torch.from_numpy(images).to(device) if host else images
        if stack.dim() != 4 or stack.shape[0] != 2:
            raise ValueError(f'city {city!r}: images must be [2,C,H,W], got {tuple(stack.shape)}')
        exclude = oob = None
        if ignore_label is not None:
            lab_host = not torch.is_tensor(labels)
            lab = torch.from_numpy(np.ascontiguousarray(labels)).to(stack.device) if lab_host else labels.to(stack.device)
            exclude = lab.contiguous()
            oob = torch.empty(stack.shape[2:], dtype=torch.uint8, device=stack.device)
        aligned, est = coregister(stack[0], stack[1], max_shift, bands, cells, exclude, ignore_label, min_ncc, oob=oob)
        stack[1].copy_(aligned)
        if oob is not None:
            if lab_host:
                labels[oob.cpu().numpy() != 0] = ignore_label
            else:
                labels[oob.to(labels.device) != 0] = ignore_label
        if host:
            images[1] = stack[1].cpu().numpy()
        reports[city] = est.read()
    return reports


def report_line(city, rep):
    """The fields of train.py's `coreg` log line for one city."""
    return {'city': city, 'dy': rep['dy'], 'dx': rep['dx'], 'ncc': rep['ncc'], 'cells_ok': rep['cells_ok']}
