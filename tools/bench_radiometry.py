"""Times the radiometric matching (fabric_amd/utils/radiometry.py) on a 500 x 500 city and on a 10 000 x 10 000 pair of 13 bands: the fit at
K = 2 and K = 256 (two bdn_band_quantiles calls each: date 2 and date 1), the apply, stretch_8bit on the stack, bdn_shift_apply on the same
scene as a bandwidth yardstick (it reads and writes every band once, as the apply does), the same fits on a tie-heavy variant (the scene
quantised to 16 values), and the host route (copy down, np.quantile, np.interp per band) on a stride-decimated scene when the full one
would take minutes.  Device times are the median of event-timed repetitions after one warm-up; one JSON line per measurement.

    python tools/bench_radiometry.py [--sizes 500 10000] [--bands 13] [--reps 5] > profiles/radiometry_bench.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fabric_amd.utils import radiometry as RM               # noqa: E402
from fabric_amd.utils import registration as RG             # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def line(**kw):
    print(json.dumps(kw), flush=True)


def host_route(d2, d1, knots, stride):
    """The host route on every stride-th pixel: copy down, np.quantile of both dates, np.interp per band.  Seconds (copy, fit, apply)."""
    t0 = time.perf_counter()
    a, b = d1[:, ::stride, ::stride].contiguous().cpu().numpy(), d2[:, ::stride, ::stride].contiguous().cpu().numpy()
    t1 = time.perf_counter()
    p = np.arange(knots) / (knots - 1)
    src = [np.quantile(b[c], p) for c in range(b.shape[0])]
    dst = [np.quantile(a[c], p) for c in range(a.shape[0])]
    t2 = time.perf_counter()
    out = np.stack([np.interp(b[c], src[c], dst[c]) for c in range(b.shape[0])])
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, out.shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[500, 10000])
    ap.add_argument('--bands', type=int, default=13)
    ap.add_argument('--reps', type=int, default=5)
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    line(device=torch.cuda.get_device_name(dev), torch=torch.__version__, bands=opt.bands, reps=opt.reps,
         note='ms = median of event-timed repetitions after one warm-up; GB/s counts the bytes of the scene read (fits, per pass) or read + written')
    for n in opt.sizes:
        g = torch.Generator(device=dev).manual_seed(n)
        d1 = torch.randn(opt.bands, n, n, device=dev, generator=g)
        d2 = torch.empty_like(d1)
        for c in range(opt.bands):                           # band by band: no second scene-sized temporary
            d2[c] = 1.3 * d1[c] + 0.2 + 0.3 * torch.randn(n, n, device=dev, generator=g)
        out = torch.empty_like(d2)
        gb = d1.numel() * 4 / 1e9
        scene = f'{opt.bands}x{n}x{n}'
        def fits_and_applies(variant):
            trs = {}
            for k in (2, 256):
                def fit(k=k):
                    trs[k] = RM.fit_transfer(d2, d1, [0.02, 0.98] if k == 2 else None, k, extrapolate='slope' if k == 2 else 'offset')
                med, lo, hi = timed(fit, opt.reps)
                # a fit reads each of the two scenes three times (one histogram pass per level)
                line(scene=scene, data=variant, what=f'fit K={k}', ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                     gbps_read=round(6 * gb / (med * 1e-3), 1))
            for k in (2, 256):
                med, lo, hi = timed(lambda k=k: RM.apply_transfer(d2, trs[k], out=out), opt.reps)
                line(scene=scene, data=variant, what=f'apply K={k}', ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                     gbps_read_write=round(2 * gb / (med * 1e-3), 1))

        fits_and_applies('continuous')
        med, lo, hi = timed(lambda: RM.stretch_8bit(d2), opt.reps)
        line(scene=scene, data='continuous', what=f'stretch_8bit ({opt.bands} bands: the quantiles of the values > 0, then the bytes)', ms=round(med, 3),
             ms_min=round(lo, 3), ms_max=round(hi, 3))
        field = torch.zeros(1, 1, 2, device=dev)
        med, lo, hi = timed(lambda: RG.apply_shift(d2, field, out=out), opt.reps)
        line(scene=scene, what='bdn_shift_apply (yardstick: reads and writes every band once)', ms=round(med, 3), ms_min=round(lo, 3),
             ms_max=round(hi, 3), gbps_read_write=round(2 * gb / (med * 1e-3), 1))
        stride = 1 if n <= 2000 else 10
        for k in (2, 256):
            copy_s, fit_s, apply_s, shape = host_route(d2, d1, k, stride)
            line(scene=scene, what=f'host route K={k}', stride=stride, host_pixels_per_band=int(shape[1] * shape[2]), copy_ms=round(copy_s * 1e3, 1),
                 quantile_ms=round(fit_s * 1e3, 1), interp_ms=round(apply_s * 1e3, 1),
                 note='one run, wall clock' + ('' if stride == 1 else f'; on every {stride}th pixel of each axis: 1 / {stride * stride} of the scene'))
        for d in (d1, d2):                                   # every pixel of a band in 16 bins: the tie-heavy case
            d.mul_(2).round_().clamp_(-8, 7)
        fits_and_applies('16 values')
        del d1, d2, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
