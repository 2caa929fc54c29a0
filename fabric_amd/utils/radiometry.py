"""Radiometric matching of the two dates of a scene on the device: date 2 is mapped through a piecewise-linear transfer whose knots are
the quantiles of date 2 (source) and of date 1 (destination), per band -- quantile transfer, what np.quantile plus np.interp per band give
on the host after copying both stacks down and sorting them.  The quantiles are exact order statistics (bdn_band_quantiles: a radix
select over integer histograms, the same bits on every run), the transfer is pointwise (bdn_transfer_apply), and stretch_8bit is the
reference's percentile stretch to bytes (bdn_stretch_u8); include/bidate_hip.h states the arithmetic.  Everything runs on the current
stream, results stay on the device and .read() is the one host read; allocation sizes come from the library's size query; nothing is
cached across calls.  Alignment comes first (utils/registration.py): a correlation does not see an affine radiometric change, and
resampling moves the histogram slightly.
"""
import numpy as np
import torch

from .. import _lib
from .registration import MAX_BANDS, MAX_DIM, _check_scene, _is_int, _need_device, _workspace

MAX_PROBS = 1024
MAX_KNOTS = 1024
EXTRAPOLATE = {'offset': 0, 'slope': 1}
REPORT_PROBS = (0.02, 0.5, 0.98)


def _check_bands(bands, c):
    if bands is None:
        bands = list(range(c))
    if not isinstance(bands, (tuple, list)) or not all(_is_int(b) for b in bands):
        raise ValueError(f'bands must be None or a list of band indices, got {bands!r}')
    if not 1 <= len(bands) <= MAX_BANDS:
        raise ValueError(f'bands: 1..{MAX_BANDS} indices, got {len(bands)}' + (' (name a subset with bands=)' if len(bands) > MAX_BANDS else ''))
    if any(not 0 <= b < c for b in bands):
        raise ValueError(f'bands: indices must lie in [0, {c}), got {list(bands)}')
    if len(set(bands)) != len(bands):
        raise ValueError(f'bands: an index is named twice in {list(bands)}')
    return list(bands)


def _check_exclude(exclude, exclude_value, scene, h, w):
    if exclude is None:
        return
    if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.uint8 or tuple(exclude.shape) != (h, w) or not exclude.is_contiguous():
        raise ValueError(f'exclude must be a contiguous uint8 [H,W] tensor shaped like the scene ({h} x {w})')
    if exclude.device != scene.device:
        raise ValueError(f'exclude is on {exclude.device}, the scene on {scene.device}')
    if not _is_int(exclude_value) or not 0 <= exclude_value <= 255:
        raise ValueError(f'exclude_value (when exclude is given) must be a byte 0..255, got {exclude_value!r}')


def _check_probs(probs, device, what='probs', sorted_=False):
    """The probabilities as (host float64 array or None, count): a device tensor is taken as it is (the kernel answers NaN for a value
    outside [0, 1]); a host sequence is checked here."""
    if isinstance(probs, torch.Tensor):
        if probs.dtype != torch.float64 or probs.dim() != 1 or not probs.is_contiguous():
            raise ValueError(f'{what} as a tensor must be a contiguous float64 vector')
        if probs.device != device:
            raise ValueError(f'{what} is on {probs.device}, the scene on {device}')
        n = int(probs.shape[0])
        host = None
    else:
        try:
            host = None if isinstance(probs, str) else np.asarray(probs, np.float64)
        except (TypeError, ValueError):
            host = None
        if host is None or host.ndim != 1:
            raise ValueError(f'{what} must be a sequence of probabilities or a float64 device vector, got {probs!r}')
        if not ((host >= 0.0) & (host <= 1.0)).all():
            raise ValueError(f'{what} must lie in [0, 1]')
        if sorted_ and (np.diff(host) < 0).any():
            raise ValueError(f'{what} must be nondecreasing: the knots of a transfer are')
        n = host.size
    if not 1 <= n <= MAX_PROBS:
        raise ValueError(f'{what}: 1..{MAX_PROBS} probabilities, got {n}')
    return host, n


def check_quantile_args(scene, probs, bands=None, exclude=None, exclude_value=None, positive_only=False):
    """Validate the arguments of band_quantiles without touching a device (meta tensors will do).  Returns (C, H, W, band list, n_q)."""
    c, h, w = _check_scene(scene, 'scene')
    bands = _check_bands(bands, c)
    _check_exclude(exclude, exclude_value, scene, h, w)
    if not isinstance(positive_only, bool):
        raise ValueError(f'positive_only must be a bool, got {positive_only!r}')
    _, nq = _check_probs(probs, scene.device)
    return c, h, w, bands, nq


def check_fit_args(d2, d1, probs=None, knots=256, bands=None, exclude=None, exclude_value=None, extrapolate='offset'):
    """Validate the arguments of fit_transfer without touching a device.  Returns (C, H, W, band list, K, extrapolate code)."""
    c, h, w = _check_scene(d2, 'd2')
    if _check_scene(d1, 'd1') != (c, h, w):
        raise ValueError(f'd1 must be shaped like d2, got {tuple(d1.shape)} against {tuple(d2.shape)}')
    if d1.device != d2.device:
        raise ValueError(f'd1 is on {d1.device}, d2 on {d2.device}')
    bands = _check_bands(bands, c)
    _check_exclude(exclude, exclude_value, d2, h, w)
    if extrapolate not in EXTRAPOLATE:
        raise ValueError(f"extrapolate must be 'offset' or 'slope', got {extrapolate!r}")
    if probs is None:
        if not _is_int(knots) or not 2 <= knots <= MAX_KNOTS:
            raise ValueError(f'knots must be an integer 2..{MAX_KNOTS}, got {knots!r}')
        k = knots
    else:
        _, k = _check_probs(probs, d2.device, sorted_=True)
        if k < 2:
            raise ValueError(f'probs: a transfer needs 2..{MAX_KNOTS} knots, got {k}')
    return c, h, w, bands, k, EXTRAPOLATE[extrapolate]


def check_transfer_args(d2, transfer, out=None):
    """Validate the arguments of apply_transfer without touching a device.  Returns (C, H, W, n_b, K)."""
    c, h, w = _check_scene(d2, 'd2')
    if not isinstance(transfer, BandTransfer):
        raise ValueError(f'transfer must be a BandTransfer (fit_transfer), got {type(transfer).__name__}')
    nb, k = len(transfer.bands), int(transfer.src.shape[-1])
    for name in ('src', 'dst'):
        t = getattr(transfer, name)
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (nb, k) or not t.is_contiguous():
            raise ValueError(f'transfer.{name} must be a contiguous float32 [n_b,K] tensor ({nb} x {k})')
        if t.device != d2.device:
            raise ValueError(f'transfer.{name} is on {t.device}, d2 on {d2.device}')
    if not 2 <= k <= MAX_KNOTS:
        raise ValueError(f'transfer: 2..{MAX_KNOTS} knots, got {k}')
    _check_bands(transfer.bands, c)
    if transfer.extrapolate not in EXTRAPOLATE:
        raise ValueError(f"transfer.extrapolate must be 'offset' or 'slope', got {transfer.extrapolate!r}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (c, h, w) or not out.is_contiguous():
            raise ValueError('out must be a contiguous float32 tensor shaped like d2')
        if out.device != d2.device:
            raise ValueError(f'out is on {out.device}, d2 on {d2.device}')
    return c, h, w, nb, k


class BandQuantiles:
    """What band_quantiles leaves on the device: .value float64 [n_b,n_q], .order float32 [n_b,n_q,2] = the two order statistics each
    value lies between, .count int64 [n_b] = the valid pixels.  .read() is the one host read."""

    def __init__(self, value, order, count, bands, probs):
        self.value, self.order, self.count, self.bands, self.probs = value, order, count, list(bands), probs

    def read(self):
        """{'value': float64 numpy [n_b,n_q], 'order': float32 numpy [n_b,n_q,2], 'count': int64 numpy [n_b], 'bands'}."""
        nb, nq = self.value.shape
        both = torch.cat([self.value.flatten(), self.order.flatten().double(), self.count.double()]).cpu().numpy()   # exact: counts < 2^53
        return {'value': both[:nb * nq].reshape(nb, nq), 'order': both[nb * nq:3 * nb * nq].astype(np.float32).reshape(nb, nq, 2),
                'count': both[3 * nb * nq:].astype(np.int64), 'bands': list(self.bands)}


class BandTransfer:
    """What fit_transfer leaves on the device: .src, .dst float32 [n_b,K] = the knots of date 2 and of date 1 (the float64 quantiles
    rounded once), .count int64 [2,n_b] = the valid pixels of date 2 (row 0) and date 1 (row 1), .bands, .extrapolate ('offset' or
    'slope') and .probs (float64 [K] on the device).  A band without a valid pixel in either date has NaN knots and passes through."""

    def __init__(self, src, dst, count, bands, extrapolate, probs=None):
        self.src, self.dst, self.count, self.bands, self.extrapolate, self.probs = src, dst, count, list(bands), extrapolate, probs

    def read(self):
        """{'src', 'dst': float32 numpy [n_b,K], 'count': int64 numpy [2,n_b], 'bands', 'extrapolate'}."""
        nb, k = self.src.shape
        both = torch.cat([self.src.flatten().double(), self.dst.flatten().double(), self.count.flatten().double()]).cpu().numpy()
        return {'src': both[:nb * k].astype(np.float32).reshape(nb, k), 'dst': both[nb * k:2 * nb * k].astype(np.float32).reshape(nb, k),
                'count': both[2 * nb * k:].astype(np.int64).reshape(2, nb), 'bands': list(self.bands), 'extrapolate': self.extrapolate}


def _probs_on(probs, host, device):
    return probs if host is None else torch.from_numpy(np.ascontiguousarray(host)).to(device)


def _quantiles(scene, probs_t, band_t, bands, exclude, exclude_value, positive_only):
    c, h, w = scene.shape
    nb, nq, dev = len(bands), int(probs_t.shape[0]), scene.device
    value = torch.empty(nb, nq, dtype=torch.float64, device=dev)
    order = torch.empty(nb, nq, 2, dtype=torch.float32, device=dev)
    count = torch.empty(nb, dtype=torch.int64, device=dev)
    ws = _workspace(_lib.load().bdn_band_quantiles_workspace_bytes(nb, nq, h, w), dev)
    _lib.call('bdn_band_quantiles', _lib.ptr(scene), _lib.ptr(band_t), nb, _lib.ptr(exclude), 0 if exclude is None else exclude_value,
              1 if positive_only else 0, _lib.ptr(probs_t), nq, _lib.ptr(value), _lib.ptr(order), _lib.ptr(count), _lib.ptr(ws), c, h, w,
              _lib.stream_ptr())
    return BandQuantiles(value, order, count, bands, probs_t)


def band_quantiles(scene, probs, bands=None, exclude=None, exclude_value=None, positive_only=False):
    """The quantiles of the bands named (indices; default all, at most 64) of a float32 [C,H,W] device scene at the probabilities `probs`
    (a sequence in [0, 1] or a float64 device vector, at most 1024): numpy's 'linear' rule, value = a + (b - a) t between the order
    statistics a = v_(floor(h)) and b, h = p (n - 1), over the valid pixels -- finite, not where `exclude` (uint8 [H,W]) equals
    exclude_value, and > 0 with positive_only.  Returns a BandQuantiles; seven launches per group of bands, no host read."""
    c, h, w, bands, nq = check_quantile_args(scene, probs, bands, exclude, exclude_value, positive_only)
    _need_device(scene, 'band_quantiles')
    host, _ = _check_probs(probs, scene.device)
    band_t = torch.tensor(bands, dtype=torch.int32).to(scene.device)
    return _quantiles(scene, _probs_on(probs, host, scene.device), band_t, bands, exclude, exclude_value, positive_only)


def _fit(d2, d1, probs, knots, bands, exclude, exclude_value, extrapolate, extra=()):
    """fit_transfer with `extra` probabilities appended to the same two quantile calls: (BandTransfer, extra values float64
    [2,n_b,len(extra)] or None)."""
    c, h, w, bands, k, _ = check_fit_args(d2, d1, probs, knots, bands, exclude, exclude_value, extrapolate)
    _need_device(d2, 'fit_transfer')
    dev = d2.device
    if probs is None:
        probs_t = torch.arange(k, dtype=torch.float64, device=dev) / float(k - 1)
    else:
        host, _ = _check_probs(probs, dev, sorted_=True)
        probs_t = _probs_on(probs, host, dev)
    all_t = probs_t
    if extra:
        all_t = torch.cat([probs_t, torch.tensor(list(extra), dtype=torch.float64).to(dev)])
    band_t = torch.tensor(bands, dtype=torch.int32).to(dev)
    if all_t.shape[0] <= MAX_PROBS:
        q2 = _quantiles(d2, all_t, band_t, bands, exclude, exclude_value, False)
        q1 = _quantiles(d1, all_t, band_t, bands, exclude, exclude_value, False)
        v2, v1 = q2.value[:, :k], q1.value[:, :k]
        ex = torch.stack([q2.value[:, k:], q1.value[:, k:]]) if extra else None
    else:                                                    # the knots fill the limit: the extra probabilities in calls of their own
        q2 = _quantiles(d2, probs_t, band_t, bands, exclude, exclude_value, False)
        q1 = _quantiles(d1, probs_t, band_t, bands, exclude, exclude_value, False)
        v2, v1 = q2.value, q1.value
        extra_t = all_t[k:].contiguous()
        ex = torch.stack([_quantiles(d, extra_t, band_t, bands, exclude, exclude_value, False).value for d in (d2, d1)])
    tr = BandTransfer(v2.float().contiguous(), v1.float().contiguous(), torch.stack([q2.count, q1.count]), bands, extrapolate, probs_t)
    return tr, ex


def fit_transfer(d2, d1, probs=None, knots=256, bands=None, exclude=None, exclude_value=None, extrapolate='offset'):
    """The transfer that carries the quantiles of d2 onto those of d1 (float32 [C,H,W] device scenes of one shape), per band named: the
    knots are the quantiles at `probs` (nondecreasing, 2..1024 of them; default k / (K - 1), K = knots), rounded once to float32.  Pixels
    where `exclude` equals exclude_value and non-finite pixels take no part.  Returns a BandTransfer; both fits are enqueued back to
    back, no host read."""
    return _fit(d2, d1, probs, knots, bands, exclude, exclude_value, extrapolate)[0]


def apply_transfer(d2, transfer, out=None):
    """d2 through the transfer: inside the knots the line through the two knots around a pixel, outside them transfer.extrapolate
    ('offset': the end knot's shift; 'slope': the end segment continued); un-named bands are copied, non-finite pixels keep their bits,
    a transfer whose tables are equal returns d2 bit for bit.  One launch; returns out (a new tensor unless given; out may be d2)."""
    c, h, w, nb, k = check_transfer_args(d2, transfer, out)
    _need_device(d2, 'apply_transfer')
    if out is None:
        out = torch.empty_like(d2)
    band_t = torch.tensor(transfer.bands, dtype=torch.int32).to(d2.device)
    _lib.call('bdn_transfer_apply', _lib.ptr(d2), _lib.ptr(out), _lib.ptr(band_t), nb, _lib.ptr(transfer.src), _lib.ptr(transfer.dst), k,
              EXTRAPOLATE[transfer.extrapolate], None, c, h, w, _lib.stream_ptr())
    return out


def match_histograms(d2, d1, knots=256, bands=None, exclude=None, exclude_value=None, out=None):
    """(d2 with the histogram of d1, the BandTransfer): `knots` quantiles at k / (K - 1) of each date, 'offset' beyond the extremes."""
    tr = fit_transfer(d2, d1, None, knots, bands, exclude, exclude_value, 'offset')
    return apply_transfer(d2, tr, out), tr


def _check_range(lower, upper):
    for v in (lower, upper):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f'lower / upper must be numbers, got {lower!r}, {upper!r}')
    if not 0.0 <= lower < upper <= 1.0:
        raise ValueError(f'need 0 <= lower < upper <= 1, got {lower!r}, {upper!r}')
    return float(lower), float(upper)


def match_range(d2, d1, lower=0.02, upper=0.98, bands=None, exclude=None, exclude_value=None, out=None):
    """(d2 mapped linearly so that its `lower` and `upper` quantiles land on d1's, the BandTransfer): two knots, the line continued."""
    tr = fit_transfer(d2, d1, list(_check_range(lower, upper)), 2, bands, exclude, exclude_value, 'slope')
    return apply_transfer(d2, tr, out), tr


def normalize_cities(full_load, method='histogram', knots=256, lower=0.02, upper=0.98, bands=None, ignore_label=None, device='cuda',
                     invariant=None, invariant_min=0.95, mad_iters=30, mad_tol=1e-3):
    """Match date 2 of every city of a `full_load` dict ({city: {'images': float32 [2,C,H,W], 'labels': uint8 [H,W]}}) to its date 1, in
    place: device stacks are rewritten on the device, numpy stacks are uploaded, matched and written back into the same arrays (numpy in,
    numpy out).  method 'histogram' is match_histograms (knots), 'range' is match_range (lower, upper).  Date 1 and the labels are never
    written; label pixels equal to ignore_label (a byte) are left out of the fit.  Returns {city: report}, report = {'method', 'bands',
    'count': [2][n_b] (date 2, date 1), 'p': (0.02, 0.5, 0.98), 'src', 'dst': [n_b][3] = the quantiles of date 2 before matching and of
    date 1 at p}; one host read per city, after its launches.
    invariant='mad': the transfer is fitted on invariant pixels only.  Per city, utils.mad.irmad runs on the same bands (ignore_label left
    out, at most mad_iters iterations, stopping at mad_tol), change_mask(threshold=invariant_min, excluded_out=1) marks the pixels whose
    no-change probability lies below invariant_min and the ignored ones, and that raster (value 1) is the `exclude` of the fit.  A failed
    solve (a rank-deficient date, too few pixels) falls back to the exclude above, with one difference: a pixel that is not finite in
    any named band of either date is left out of the fit of every band (IR-MAD's rule of validity), where the plain path drops
    non-finite values band by band; on finite data the two are the same raster.  The report gains 'mad': {'ok', 'iters', 'converged',
    'rho', 'invariant_frac' (of the scene's pixels), 'fallback'}, read with the same single host read.  None (default): the calls above."""
    if method not in ('histogram', 'range'):
        raise ValueError(f"method must be 'histogram' or 'range', got {method!r}")
    if ignore_label is not None and (not _is_int(ignore_label) or not 0 <= ignore_label <= 255):
        raise ValueError(f'ignore_label must be None or a byte 0..255, got {ignore_label!r}')
    if invariant not in (None, 'mad'):
        raise ValueError(f"invariant must be None or 'mad', got {invariant!r}")
    if invariant is not None:
        from . import mad as MAD
        if isinstance(invariant_min, bool) or not isinstance(invariant_min, (int, float)) or not 0.0 < invariant_min <= 1.0:
            raise ValueError(f'invariant_min must be a probability in (0, 1], got {invariant_min!r}')
        if not _is_int(mad_iters) or not 1 <= mad_iters <= MAD.MAX_ITERS:
            raise ValueError(f'mad_iters must be an integer 1..{MAD.MAX_ITERS}, got {mad_iters!r}')
        MAD._number(mad_tol, 'mad_tol', lo=0.0)
    if method == 'range':
        probs, k, mode = list(_check_range(lower, upper)), 2, 'slope'
    else:
        if not _is_int(knots) or not 2 <= knots <= MAX_KNOTS:
            raise ValueError(f'knots must be an integer 2..{MAX_KNOTS}, got {knots!r}')
        probs, k, mode = None, knots, 'offset'
    reports = {}
    for city, d in full_load.items():
        images, labels = d['images'], d['labels']
        host = not torch.is_tensor(images)
        stack = torch.from_numpy(images).to(device) if host else images
        if stack.dim() != 4 or stack.shape[0] != 2:
            raise ValueError(f'city {city!r}: images must be [2,C,H,W], got {tuple(stack.shape)}')
        exclude = None
        if ignore_label is not None:
            lab = torch.from_numpy(np.ascontiguousarray(labels)) if not torch.is_tensor(labels) else labels
            exclude = lab.to(stack.device).contiguous()
        res = inv = None
        if invariant == 'mad':
            res = MAD.irmad(stack[0], stack[1], bands, exclude, ignore_label, mad_iters, mad_tol)
            # after a failed solve every no-change probability is NaN, which the mask turns into 0: the raster then holds 1 at the ignored
            # pixels (the exclude above) and at the pixels that are not finite in some named band of either date, which the plain path
            # drops band by band only -- the fallback needs no host read before the fit
            inv = MAD.change_mask(res, invariant_min, 1)
            tr, ex = _fit(stack[1], stack[0], probs, k, bands, inv, 1, mode, extra=REPORT_PROBS)
        else:
            tr, ex = _fit(stack[1], stack[0], probs, k, bands, exclude, ignore_label, mode, extra=REPORT_PROBS)
        apply_transfer(stack[1], tr, out=stack[1])
        if host:
            images[1] = stack[1].cpu().numpy()
        nb = len(tr.bands)
        parts = [ex.flatten(), tr.count.flatten().double()]
        if res is not None:
            parts += [res.state, (inv == 0).sum().double().reshape(1)]
        both = torch.cat(parts).cpu().numpy()
        ex_h = both[:2 * nb * 3].reshape(2, nb, 3)
        reports[city] = {'method': method, 'bands': list(tr.bands), 'count': both[2 * nb * 3:2 * nb * 4].astype(np.int64).reshape(2, nb).tolist(),
                         'p': list(REPORT_PROBS), 'src': ex_h[0].tolist(), 'dst': ex_h[1].tolist()}
        if res is not None:
            m = MAD.read_state(both[2 * nb * 4:-1], nb)
            reports[city]['mad'] = {'ok': m['ok'], 'iters': m['iters'], 'converged': m['converged'], 'rho': m['rho'].tolist(),
                                    'invariant_frac': float(both[-1]) / float(inv.numel()), 'fallback': not m['ok']}
    return reports


def report_line(city, rep):
    """The fields of train.py's `radiom` log line for one city."""
    return {'city': city, 'method': rep['method'], 'bands': rep['bands'], 'count': rep['count'], 'p': rep['p'], 'src': rep['src'],
            'dst': rep['dst']}


def mad_line(city, rep):
    """The fields of train.py's `mad` log line for one city (normalize_cities(invariant='mad'))."""
    return dict({'city': city}, **rep['mad'])


def _as_stack(band):
    """(device tensor [C,H,W], was numpy, was [H,W]) of a band or stack of float32 / uint16 values."""
    host = not torch.is_tensor(band)
    t = band
    if host:
        a = np.ascontiguousarray(band)
        if a.dtype not in (np.float32, np.uint16):
            raise ValueError(f'stretch_8bit takes float32 or uint16 values, got {a.dtype}')
        t = torch.from_numpy(a)
    if t.dtype not in (torch.float32, torch.uint16) or t.dim() not in (2, 3) or not t.is_contiguous():
        raise ValueError(f'stretch_8bit takes a contiguous float32 or uint16 [H,W] or [C,H,W] array, got {t.dtype} {tuple(t.shape)}')
    flat = t.dim() == 2
    return (t[None] if flat else t), host, flat


def stretch_8bit(band, lower_percent=2, higher_percent=98, device='cuda'):
    """The reference's stretch_8bit (utils/dataloaders.py:38-48) on the device: c, d = the lower and higher percentile of the values > 0 of
    the band, out = uint8((band - c) * (255 / (d - c)) clamped to [0, 255]) in float64.  `band`: a float32 or uint16 [H,W] band, or a
    [C,H,W] stack that is stretched band by band (at most 64); a device tensor gives a uint8 device tensor, a numpy array goes through the
    device and comes back as numpy.  With d == c (a constant band) values above c give 255, the others 0; a band without a value > 0
    gives 0 everywhere.  Two launches of the quantile select's seven, then one; no host read."""
    for v in (lower_percent, higher_percent):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 100:
            raise ValueError(f'percentiles must be numbers in [0, 100], got {lower_percent!r}, {higher_percent!r}')
    t, host, flat = _as_stack(band)
    if host:
        t = t.to(device)
    _need_device(t, 'stretch_8bit')
    c, h, w = t.shape
    if not (1 <= c <= MAX_BANDS and 1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f'stretch_8bit: need 1 <= C <= {MAX_BANDS} and 1 <= H, W <= {MAX_DIM}, got {c} x {h} x {w}')
    scene = t if t.dtype == torch.float32 else t.to(torch.float32)             # uint16 -> float32 is exact
    q = band_quantiles(scene, [lower_percent / 100, higher_percent / 100], positive_only=True)
    out = torch.empty(c, h, w, dtype=torch.uint8, device=t.device)
    _lib.call('bdn_stretch_u8', _lib.ptr(t), 1 if t.dtype == torch.uint16 else 0, _lib.ptr(q.value), _lib.ptr(out), c, h, w, _lib.stream_ptr())
    out = out[0] if flat else out
    return out.cpu().numpy() if host else out
