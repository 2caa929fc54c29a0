"""Thresholds without labels: a change statistic (IR-MAD's chi2, a scene's change probability) becomes a mask at a number selected from
the histogram of the statistic itself -- Otsu's between-class variance, Kittler and Illingworth's minimum error, Rosin's unimodal corner
(Rosin and Ioannidis 2003 evaluate it for change images) and the two-Gaussian EM of Bruzzone and Prieto (2000).  bdn_raster_hist counts a
float raster of any size into given bin edges (integers: exact, order-independent, the same bits on every run), bdn_hist_threshold applies
the rules in one single-block launch, bdn_raster_mask thresholds the raster at a number that stays in device memory
(include/bidate_hip.h).  Everything runs on the current stream, nothing is read back until ThresholdTable.read(); every argument check
runs before a device is touched (meta tensors will do).  CPU tensors raise: there is no CPU path.
"""
import math

import torch

from .. import _lib
from .registration import _is_int, _need_device

METHODS = ('otsu', 'kittler', 'rosin', 'em')                      # row order of the table; bit k of bdn_hist_threshold's `methods`
COLUMNS = ('ok', 'bin', 'value', 'crit', 'n0', 'n1', 'mean0', 'mean1', 'sd0', 'sd1', 'w1', 'iters', 'loglik', 'n', 'below', 'above')
SPACINGS = ('linear', 'sqrt', 'log')
MAX_BINS = 4096
_INT_COLUMNS = ('bin', 'n0', 'n1', 'iters', 'n', 'below', 'above')


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _is_scalar_tensor(v):
    return isinstance(v, torch.Tensor) and v.dim() == 0


def _check_bins(n_bins, spacing):
    if not _is_int(n_bins) or not 2 <= n_bins <= MAX_BINS:
        raise ValueError(f'n_bins must be an integer in 2..{MAX_BINS}, got {n_bins!r}')
    if spacing not in SPACINGS:
        raise ValueError(f'spacing must be one of {SPACINGS}, got {spacing!r}')


def check_method(method):
    if method not in METHODS:
        raise ValueError(f'method must be one of {METHODS}, got {method!r}')
    return METHODS.index(method)


def check_methods(methods):
    """The bit mask of a method name or a sequence of names."""
    if isinstance(methods, str):
        methods = (methods,)
    if not isinstance(methods, (tuple, list)) or not methods:
        raise ValueError(f'methods must be a name or a non-empty sequence of names out of {METHODS}, got {methods!r}')
    bits = 0
    for m in methods:
        bits |= 1 << check_method(m)
    return bits


def check_em_args(em_iters=100, em_tol=1e-9):
    if not _is_int(em_iters) or not 1 <= em_iters <= 1000:
        raise ValueError(f'em_iters must be an integer in 1..1000, got {em_iters!r}')
    if not _is_number(em_tol) or not 0.0 <= em_tol < math.inf:          # NaN fails the comparison
        raise ValueError(f'em_tol must be a finite number >= 0, got {em_tol!r}')


def check_raster_args(raster, exclude=None, exclude_value=None, out=None, excluded_out=0):
    """Validate a raster, its exclude raster and a mask output without touching a device.  Returns the number of pixels."""
    if not isinstance(raster, torch.Tensor) or raster.dtype != torch.float32 or raster.numel() < 1 or not raster.is_contiguous():
        raise ValueError('raster must be a contiguous float32 tensor with at least one element')
    if exclude is None:
        if exclude_value is not None:
            raise ValueError('exclude_value needs an exclude raster')
    else:
        if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.uint8 or exclude.shape != raster.shape or not exclude.is_contiguous():
            raise ValueError(f'exclude must be a contiguous uint8 tensor shaped like the raster {tuple(raster.shape)}')
        if exclude.device != raster.device:
            raise ValueError(f'exclude is on {exclude.device}, the raster on {raster.device}')
        if not _is_int(exclude_value) or not 0 <= exclude_value <= 255:
            raise ValueError(f'exclude_value must be a byte 0..255, got {exclude_value!r}')
    if not _is_int(excluded_out) or not 0 <= excluded_out <= 255:
        raise ValueError(f'excluded_out must be a byte 0..255, got {excluded_out!r}')
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != raster.shape or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous uint8 tensor shaped like the raster {tuple(raster.shape)}')
        if out.device != raster.device:
            raise ValueError(f'out is on {out.device}, the raster on {raster.device}')
        if out.device.type != 'meta':
            for other, name in ((raster, 'the raster'), (exclude, 'exclude')):
                if other is not None and out.untyped_storage().data_ptr() == other.untyped_storage().data_ptr():
                    raise ValueError(f'out must not share memory with {name}')
    return raster.numel()


def bin_edges(lo, hi, n_bins=1024, spacing='linear'):
    """(edges float32 [n_bins + 1], coord float64 [n_bins]) of n_bins bins over [lo, hi], uniform in v ('linear'), sqrt v ('sqrt': narrow
    bins near 0 and wide ones in the tail, for a chi-square statistic) or ln v ('log').  With u_i = f(lo) + (f(hi) - f(lo)) i / n_bins in
    float64: edges_i = float32(f^-1(u_i)) clamped to [float32(lo), float32(hi)], the two ends exactly those; coord_i = (u_i + u_{i+1}) / 2,
    the bin centres in the coordinate the bins are uniform in, which is the coordinate the selection rules work in.
    Python numbers: built on the host (CPU tensors), ValueError on lo >= hi, a non-finite end, lo <= 0 with 'log', lo < 0 with 'sqrt'.
    0-d device tensors: built with torch ops on their device, nothing is read -- ends that the host would refuse give a table on which
    no rule finds a split (a NaN threshold)."""
    _check_bins(n_bins, spacing)
    on_device = _is_scalar_tensor(lo) and _is_scalar_tensor(hi)
    if on_device:
        if lo.device != hi.device:
            raise ValueError(f'lo is on {lo.device}, hi on {hi.device}')
        dev = lo.device
        a, b = lo.to(torch.float64), hi.to(torch.float64)
    elif _is_number(lo) and _is_number(hi):
        if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
            raise ValueError(f'bin_edges needs finite lo < hi, got {lo!r}, {hi!r}')
        if spacing == 'log' and lo <= 0:
            raise ValueError(f"spacing 'log' needs lo > 0, got {lo!r}")
        if spacing == 'sqrt' and lo < 0:
            raise ValueError(f"spacing 'sqrt' needs lo >= 0, got {lo!r}")
        dev = torch.device('cpu')
        a, b = torch.tensor(float(lo), dtype=torch.float64), torch.tensor(float(hi), dtype=torch.float64)
    else:
        raise ValueError('lo and hi must both be Python numbers or both be 0-d tensors')
    lo32, hi32 = a.to(torch.float32), b.to(torch.float32)
    if spacing == 'sqrt':
        a, b = a.sqrt(), b.sqrt()
    elif spacing == 'log':
        a, b = a.log(), b.log()
    u = a + (b - a) * (torch.arange(n_bins + 1, dtype=torch.float64, device=dev) / n_bins)
    v = u * u if spacing == 'sqrt' else u.exp() if spacing == 'log' else u
    edges = torch.minimum(torch.maximum(v.to(torch.float32), lo32), hi32)
    edges[0], edges[-1] = lo32, hi32
    return edges, (u[:-1] + u[1:]) * 0.5


class ThresholdTable:
    """What RasterHistogram.select leaves on the device: .thr float32 [4] (edges[bin] per method, NaN where the method found no split
    or was not asked for), .table float64 [4, 16] (rows METHODS, columns COLUMNS), and the .edges / .coord they were selected on."""

    def __init__(self, thr, table, edges, coord):
        self.thr, self.table, self.edges, self.coord = thr, table, edges, coord

    def read(self):
        """The one host read: {method: {column: value, 'thr': float}} with ok a bool and the counts Python ints."""
        flat = torch.cat([self.table.reshape(-1), self.thr.to(torch.float64)]).tolist()
        out = {}
        for r, name in enumerate(METHODS):
            d = dict(zip(COLUMNS, flat[16 * r:16 * r + 16]))
            d['ok'] = bool(d['ok'])
            for k in _INT_COLUMNS:
                d[k] = int(d[k])
            d['thr'] = flat[64 + r]
            out[name] = d
        return out

    def mask(self, raster, method, below=False, exclude=None, exclude_value=None, excluded_out=0, out=None):
        """uint8 mask shaped like `raster`: 1 where raster >= the method's threshold (below=True: <), 0 elsewhere and at a non-finite
        value, excluded_out where exclude == exclude_value; all 0 (but for excluded pixels) when the method found no split.  The threshold
        is read by the kernel from .thr: one launch (bdn_raster_mask), no host read.  Returns out (a new tensor unless given)."""
        row = check_method(method)
        if not isinstance(below, bool):
            raise ValueError(f'below must be a bool, got {below!r}')
        n = check_raster_args(raster, exclude, exclude_value, out, excluded_out)
        if raster.device != self.thr.device:
            raise ValueError(f'the raster is on {raster.device}, the table on {self.thr.device}')
        _need_device(raster, 'ThresholdTable.mask')
        if out is None:
            out = torch.empty(raster.shape, dtype=torch.uint8, device=raster.device)
        _lib.call('bdn_raster_mask', _lib.ptr(raster), _lib.ptr(exclude), 0 if exclude is None else exclude_value,
                  self.thr.data_ptr() + 4 * row, int(below), excluded_out, _lib.ptr(out), n, _lib.stream_ptr())
        return out


class RasterHistogram:
    """The histogram of float rasters over given bin edges, accumulated on the device over any number of rasters or tiles.

    edges: float32 [n_bins + 1], non-decreasing; coord: float64 [n_bins], the bins' coordinates for the selection rules (bin_edges gives
    both); 2 <= n_bins <= 4096.  counts: int64 [n_bins + 3] = the bins, then the values below edges[0], above edges[-1], and the skipped
    pixels (excluded or not finite).  A value v lies in bin max{i : edges[i] <= v}; v == edges[-1] lies in the last bin."""

    def __init__(self, edges, coord):
        if not isinstance(edges, torch.Tensor) or edges.dtype != torch.float32 or edges.dim() != 1 or not edges.is_contiguous():
            raise ValueError('edges must be a contiguous float32 [n_bins + 1] tensor')
        n_bins = edges.numel() - 1
        if not 2 <= n_bins <= MAX_BINS:
            raise ValueError(f'edges must hold 3..{MAX_BINS + 1} values (2..{MAX_BINS} bins), got {edges.numel()}')
        if not isinstance(coord, torch.Tensor) or coord.dtype != torch.float64 or tuple(coord.shape) != (n_bins,) or not coord.is_contiguous():
            raise ValueError(f'coord must be a contiguous float64 [{n_bins}] tensor')
        if coord.device != edges.device:
            raise ValueError(f'coord is on {coord.device}, edges on {edges.device}')
        self.edges, self.coord, self.n_bins = edges, coord, n_bins
        self.counts = torch.zeros(n_bins + 3, dtype=torch.int64, device=edges.device)

    def update(self, raster, exclude=None, exclude_value=None):
        """Add a raster (float32, any shape); pixels where `exclude` (uint8, same shape) equals exclude_value, and values that are not
        finite, are skipped (and counted as such).  One launch."""
        n = check_raster_args(raster, exclude, exclude_value)
        if raster.device != self.edges.device:
            raise ValueError(f'the raster is on {raster.device}, the histogram on {self.edges.device}')
        _need_device(raster, 'RasterHistogram.update')
        _lib.call('bdn_raster_hist', _lib.ptr(raster), _lib.ptr(exclude), 0 if exclude is None else exclude_value, _lib.ptr(self.edges),
                  self.n_bins, _lib.ptr(self.counts), n, _lib.stream_ptr())

    def reset(self):
        self.counts.zero_()

    def merge(self, other):
        """Add another instance's counts (the same edges: the caller's responsibility beyond their number)."""
        if not isinstance(other, RasterHistogram) or other.n_bins != self.n_bins:
            raise ValueError('RasterHistogram.merge: the two histograms differ in n_bins')
        self.counts.add_(other.counts.to(self.counts.device))

    def all_reduce(self, group=None):
        """One SUM of the int64 counts over the process group: exact whatever the world size."""
        import torch.distributed as dist
        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)

    def select(self, methods=METHODS, em_iters=100, em_tol=1e-9):
        """Apply the rules named (a name or a sequence out of METHODS) to the counts: one launch, no host read.  Returns a ThresholdTable."""
        bits = check_methods(methods)
        check_em_args(em_iters, em_tol)
        _need_device(self.counts, 'RasterHistogram.select')
        dev = self.counts.device
        table = torch.empty(4, 16, dtype=torch.float64, device=dev)
        thr = torch.empty(4, dtype=torch.float32, device=dev)
        _lib.call('bdn_hist_threshold', _lib.ptr(self.counts), _lib.ptr(self.coord), _lib.ptr(self.edges), self.n_bins, bits, em_iters,
                  float(em_tol), _lib.ptr(table), _lib.ptr(thr), _lib.stream_ptr())
        return ThresholdTable(thr, table, self.edges, self.coord)


def finite_range(raster, exclude=None, exclude_value=None):
    """(min, max) of the finite, not excluded values of a device raster as 0-d float32 tensors; (+inf, -inf) without one.  No host read."""
    keep = torch.isfinite(raster)
    if exclude is not None:
        keep &= exclude != exclude_value
    inf = torch.tensor(math.inf, dtype=torch.float32, device=raster.device)
    return torch.where(keep, raster, inf).min(), torch.where(keep, raster, -inf).max()


def auto_threshold(raster, method='rosin', n_bins=1024, spacing='linear', lo=None, hi=None, below=False, exclude=None, exclude_value=None,
                   excluded_out=0, em_iters=100, em_tol=1e-9, out=None):
    """Histogram `raster` (float32, on the device), select a threshold by `method` and apply it: returns (mask uint8 like the raster,
    ThresholdTable).  lo / hi: the ends of the bins, Python numbers or 0-d device tensors; None: the smallest / largest finite, not excluded
    value of the raster, found on the device.  Three launches behind the min / max; no host read."""
    check_method(method)
    _check_bins(n_bins, spacing)
    check_em_args(em_iters, em_tol)
    if not isinstance(below, bool):
        raise ValueError(f'below must be a bool, got {below!r}')
    check_raster_args(raster, exclude, exclude_value, out, excluded_out)
    for v, name in ((lo, 'lo'), (hi, 'hi')):
        if v is not None and not _is_number(v) and not _is_scalar_tensor(v):
            raise ValueError(f'{name} must be None, a number or a 0-d tensor, got {v!r}')
    if _is_number(lo) and _is_number(hi):
        edges, coord = bin_edges(lo, hi, n_bins, spacing)              # refuses bad ends before the device is touched
    _need_device(raster, 'auto_threshold')
    if _is_number(lo) and _is_number(hi):
        edges, coord = edges.to(raster.device), coord.to(raster.device)
    else:
        rlo, rhi = finite_range(raster, exclude, exclude_value) if lo is None or hi is None else (None, None)
        ends = [torch.tensor(float(v), dtype=torch.float32, device=raster.device) if _is_number(v) else r if v is None else v.to(raster.device)
                for v, r in ((lo, rlo), (hi, rhi))]
        edges, coord = bin_edges(ends[0], ends[1], n_bins, spacing)
    hist = RasterHistogram(edges, coord)
    hist.update(raster, exclude, exclude_value)
    table = hist.select(method, em_iters, em_tol)
    return table.mask(raster, method, below, exclude, exclude_value, excluded_out, out), table
