"""IR-MAD on the device: the iteratively reweighted multivariate alteration detection of Nielsen (2007) between the two dates of a scene --
a canonical correlation analysis of date 1 against date 2 in which every pixel is weighted by its probability of no change, iterated to a
fixed point.  It gives an unsupervised change baseline (a per-pixel chi-square statistic and a change probability in the layout of
predict_scene_blended's `proba`, invariant to any affine radiometric difference between the dates) and an invariant-pixel mask that needs
no labels (Canty and Nielsen 2008), which radiometry.fit_transfer takes as its `exclude`.  Everything runs through bdn_mad_centre /
_moments / _solve / _chi2 / _mask (include/bidate_hip.h) on the current stream; the iteration is enqueued whole, convergence is carried by
flags on the device, results stay on the device and .read() is the one host read.  Allocation sizes come from the library's size query;
nothing is cached across calls.
"""
import numpy as np
import torch

from .. import _lib
from .radiometry import _check_bands, _check_exclude
from .registration import _check_scene, _is_int, _need_device, _workspace

MAX_BANDS = 32
MAX_ITERS = 1000
ST_ITER, ST_OK, ST_CONVERGED, ST_SKIP, ST_DELTA, ST_S0, ST_NVALID, ST_RHO = range(8)


def state_doubles(nb):
    """BDN_MAD_STATE_DOUBLES of include/bidate_hip.h."""
    return 7 + 6 * nb + 2 * nb * nb


def moment_doubles(nb):
    """BDN_MAD_MOMENT_DOUBLES of include/bidate_hip.h."""
    return 1 + 2 * nb + nb * (2 * nb + 1)


def _number(v, name, lo=None, hi=None, lo_open=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float('inf'), float('-inf')):
        raise ValueError(f'{name} must be a finite number, got {v!r}')
    if lo is not None and (v <= lo if lo_open else v < lo):
        raise ValueError(f'{name} must be {">" if lo_open else ">="} {lo}, got {v!r}')
    if hi is not None and v > hi:
        raise ValueError(f'{name} must be <= {hi}, got {v!r}')
    return float(v)


def check_mad_args(d1, d2, bands=None, exclude=None, exclude_value=None, iters=30, tol=1e-3, min_var=1e-9, variates=False):
    """Validate the arguments of irmad without touching a device (meta tensors will do).  Returns (C, H, W, band list)."""
    c, h, w = _check_scene(d1, 'd1')
    if _check_scene(d2, 'd2') != (c, h, w):
        raise ValueError(f'd2 must be shaped like d1, got {tuple(d2.shape)} against {tuple(d1.shape)}')
    if d2.device != d1.device:
        raise ValueError(f'd2 is on {d2.device}, d1 on {d1.device}')
    if bands is None and c > MAX_BANDS:
        raise ValueError(f'bands: 1..{MAX_BANDS} indices, the scene has {c} bands (name a subset with bands=)')
    bands = _check_bands(bands, c)
    if len(bands) > MAX_BANDS:
        raise ValueError(f'bands: 1..{MAX_BANDS} indices, got {len(bands)} (name a subset with bands=)')
    _check_exclude(exclude, exclude_value, d1, h, w)
    if not _is_int(iters) or not 1 <= iters <= MAX_ITERS:
        raise ValueError(f'iters must be an integer 1..{MAX_ITERS}, got {iters!r}')
    _number(tol, 'tol', lo=0.0)
    _number(min_var, 'min_var', lo=0.0, lo_open=True)
    if not isinstance(variates, bool):
        raise ValueError(f'variates must be a bool, got {variates!r}')
    return c, h, w, bands


class MadResult:
    """What irmad leaves on the device: .chi2 float32 [H,W], .proba float32 [2,H,W] = {no change, change}, .variates float32 [n_b,H,W] or
    None, .state float64 [BDN_MAD_STATE_DOUBLES(n_b)]; and what change_mask needs again: the two dates, .band_t, .bands, .exclude,
    .exclude_value.  .read() is the one host read."""

    def __init__(self, chi2, proba, variates, state, d1, d2, band_t, bands, exclude, exclude_value):
        self.chi2, self.proba, self.variates, self.state = chi2, proba, variates, state
        self.d1, self.d2, self.band_t, self.bands, self.exclude, self.exclude_value = d1, d2, band_t, list(bands), exclude, exclude_value

    def read(self):
        """{'rho', 'var': float64 [n_b], 'iters', 'converged', 'ok', 'delta', 'n_valid', 'a', 'b': float64 [n_b,n_b], 'mean': float64 [2 n_b]}."""
        return read_state(self.state.cpu().numpy(), len(self.bands))


def read_state(v, nb):
    """The fields of a state block (a host float64 vector) as .read() returns them."""
    o = ST_RHO
    rho, var, mean = v[o:o + nb].copy(), v[o + nb:o + 2 * nb].copy(), v[o + 2 * nb:o + 4 * nb].copy()
    a = v[o + 6 * nb:o + 6 * nb + nb * nb].reshape(nb, nb).copy()
    b = v[o + 6 * nb + nb * nb:o + 6 * nb + 2 * nb * nb].reshape(nb, nb).copy()
    return {'rho': rho, 'var': var, 'iters': int(v[ST_ITER]), 'converged': bool(v[ST_CONVERGED]), 'ok': bool(v[ST_OK]), 'delta': float(v[ST_DELTA]),
            'n_valid': int(v[ST_NVALID]), 'a': a, 'b': b, 'mean': mean}


def irmad(d1, d2, bands=None, exclude=None, exclude_value=None, iters=30, tol=1e-3, min_var=1e-9, variates=False):
    """IR-MAD between d1 and d2 (float32 [C,H,W] device scenes of one shape) on the bands named (indices; default all, at most 32).  Pixels
    where `exclude` (uint8 [H,W]) equals exclude_value, and pixels with a non-finite value in a named band of either date, take no part and
    get chi2 = 0, proba = {1, 0}.  At most `iters` iterations; the iteration stops on the device once the canonical correlations move by
    less than `tol` (0: never), and the launches after that change nothing.  var_i = max(2 (1 - rho_i), min_var).  A rank-deficient date,
    or fewer than 2 n_b + 1 valid pixels, gives ok = 0 and NaN rasters.  Returns a MadResult; 2 + 4 iters launches, no host read."""
    c, h, w, bands = check_mad_args(d1, d2, bands, exclude, exclude_value, iters, tol, min_var, variates)
    _need_device(d1, 'irmad')
    dev, st, nb = d1.device, _lib.stream_ptr(), len(bands)
    exv = 0 if exclude is None else exclude_value
    band_t = torch.tensor(bands, dtype=torch.int32).to(dev)
    centre = torch.empty(2 * nb, dtype=torch.float64, device=dev)
    n_valid = torch.empty(1, dtype=torch.int64, device=dev)
    moments = torch.empty(moment_doubles(nb), dtype=torch.float64, device=dev)
    state = torch.empty(state_doubles(nb), dtype=torch.float64, device=dev)
    chi2 = torch.empty(h, w, dtype=torch.float32, device=dev)
    proba = torch.empty(2, h, w, dtype=torch.float32, device=dev)
    var_t = torch.empty(nb, h, w, dtype=torch.float32, device=dev) if variates else None
    ws = _workspace(_lib.load().bdn_mad_workspace_bytes(nb, h, w), dev)
    scene = (_lib.ptr(d1), _lib.ptr(d2), _lib.ptr(band_t), nb, _lib.ptr(exclude), exv)
    _lib.call('bdn_mad_centre', *scene, _lib.ptr(centre), _lib.ptr(n_valid), _lib.ptr(ws), c, h, w, st)
    for it in range(iters):
        first = it == 0
        _lib.call('bdn_mad_moments', *scene, None if first else _lib.ptr(proba), _lib.ptr(centre), None if first else _lib.ptr(state),
                  _lib.ptr(moments), _lib.ptr(ws), c, h, w, st)
        _lib.call('bdn_mad_solve', _lib.ptr(moments), _lib.ptr(centre), _lib.ptr(n_valid), nb, 1 if first else 0, float(tol), float(min_var),
                  _lib.ptr(state), st)
        _lib.call('bdn_mad_chi2', *scene, _lib.ptr(state), _lib.ptr(chi2), _lib.ptr(proba), _lib.ptr(var_t), c, h, w, st)
    return MadResult(chi2, proba, var_t, state, d1, d2, band_t, bands, exclude, exv)


def change_mask(result, threshold=0.01, excluded_out=0, out=None):
    """uint8 [H,W]: 1 where the no-change probability of `result` (a MadResult) lies below `threshold` (in [0, 1]), 0 elsewhere (a failed
    solve's NaN included), `excluded_out` (a byte) where the pixel took no part.  With a small threshold the ones are the changed pixels;
    with threshold = p, excluded_out = 1 the zeros are the pixels invariant with probability >= p: the `exclude` raster (value 1) of
    radiometry.fit_transfer.  One launch; returns out (a new tensor unless given)."""
    if not isinstance(result, MadResult):
        raise ValueError(f'result must be a MadResult (irmad), got {type(result).__name__}')
    _number(threshold, 'threshold', lo=0.0, hi=1.0)
    if not _is_int(excluded_out) or not 0 <= excluded_out <= 255:
        raise ValueError(f'excluded_out must be a byte 0..255, got {excluded_out!r}')
    _, h, w = result.proba.shape
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (h, w) or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous uint8 [H,W] tensor ({h} x {w})')
        if out.device != result.proba.device:
            raise ValueError(f'out is on {out.device}, the result on {result.proba.device}')
    _need_device(result.proba, 'change_mask')
    if out is None:
        out = torch.empty(h, w, dtype=torch.uint8, device=result.proba.device)
    _lib.call('bdn_mad_mask', _lib.ptr(result.proba), _lib.ptr(result.d1), _lib.ptr(result.d2), _lib.ptr(result.band_t), len(result.bands),
              _lib.ptr(result.exclude), result.exclude_value, float(threshold), excluded_out, _lib.ptr(out), int(result.d1.shape[0]), h, w,
              _lib.stream_ptr())
    return out


def check_auto_mask_args(result, method='rosin', on='chi2', n_bins=1024, spacing='sqrt', chi2_max=None, excluded_out=0, out=None):
    """Validate the arguments of auto_change_mask without touching a device.  Returns the raster the threshold is selected on."""
    from . import thresholds as T
    if not isinstance(result, MadResult):
        raise ValueError(f'result must be a MadResult (irmad), got {type(result).__name__}')
    T.check_method(method)
    if on not in ('chi2', 'proba'):
        raise ValueError(f"on must be 'chi2' or 'proba', got {on!r}")
    T._check_bins(n_bins, spacing)
    if spacing == 'log':
        raise ValueError("spacing 'log' cannot start at 0, where chi2 and the change probability start; use 'linear' or 'sqrt'")
    if chi2_max is not None:
        if on != 'chi2':
            raise ValueError("chi2_max goes with on='chi2'")
        _number(chi2_max, 'chi2_max', lo=0.0, lo_open=True)
    raster = result.chi2 if on == 'chi2' else result.proba[1]
    T.check_raster_args(raster, None, None, out, excluded_out)
    return raster


def auto_change_mask(result, method='rosin', on='chi2', n_bins=1024, spacing='sqrt', chi2_max=None, excluded_out=0, out=None):
    """The change mask of `result` (a MadResult) at a threshold selected from the histogram of its own statistic
    (fabric_amd.utils.thresholds): `on` = 'chi2', binned over [0, chi2_max] (None: the largest chi2 of a valid pixel, found on the device),
    or 'proba', the change probability, over [0, 1]; `method` one of 'otsu', 'kittler', 'rosin', 'em'.  The pixels that took no part
    (bdn_mad_mask's invalid pixels) are left out of the histogram and get `excluded_out`.  Returns (mask uint8 [H,W]: 1 where the
    statistic >= the threshold, ThresholdTable); a rule without a split (a failed solve's NaN raster) gives an all-zero mask.  Five
    launches behind the maximum, no host read.  change_mask is the fixed-probability route."""
    from . import thresholds as T
    raster = check_auto_mask_args(result, method, on, n_bins, spacing, chi2_max, excluded_out, out)
    _need_device(raster, 'auto_change_mask')
    invalid = change_mask(result, threshold=0.0, excluded_out=1)           # no probability lies below 0: 1 exactly at the invalid pixels
    return T.auto_threshold(raster, method, n_bins, spacing, 0.0, chi2_max if on == 'chi2' else 1.0, False, invalid, 1, excluded_out, out=out)
