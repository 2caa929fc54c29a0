"""Times the label-free thresholds (fabric_amd/utils/thresholds.py) on a 10 000 x 10 000 raster: bdn_raster_hist at 1024 and 4096 bins
(linear and sqrt spacing, with and without an exclude raster), bdn_hist_threshold (all four rules; EM at its default budget) and
bdn_raster_mask, beside the yardsticks on the same raster in the same run: bdn_score_hist (the power-of-two score histogram, which needs a
label raster), bdn_threshold_mask and bdn_mad_mask.  The raster is a chi-square-like statistic: 4 degrees of freedom, with 3 % of the
pixels in a far tail.  Device times are the median of event-timed repetitions after one warm-up; one JSON line per measurement.

    python tools/bench_thresholds.py [--size 10000] [--reps 3] [--hbm_tbps 8.0] > profiles/thresholds_bench.txt
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fabric_amd import _lib                                  # noqa: E402
from fabric_amd.utils import thresholds as T                # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--hbm_tbps', type=float, default=8.0, help='the HBM rate the byte counts are divided by (MI355X: 8 TB/s peak)')
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    n = opt.size
    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, raster=f'{n}x{n}', reps=opt.reps, hbm_tbps=opt.hbm_tbps,
                          note='us = median of event-timed repetitions after one warm-up; hbm_us = the bytes the entry must move / the HBM rate')),
          flush=True)
    g = torch.Generator(device=dev).manual_seed(n)
    chi2 = torch.randn(4, n, n, device=dev, generator=g).square_().sum(0)
    tail = torch.rand(n, n, device=dev, generator=g) < 0.03
    chi2 += tail * (20.0 + 30.0 * torch.rand(n, n, device=dev, generator=g))
    exclude = (torch.rand(n, n, device=dev, generator=g) < 0.05).to(torch.uint8)
    labels = tail.to(torch.uint8)
    proba = torch.empty(2, n, n, device=dev)
    proba[1] = (chi2 / 64.0).clamp_(0.0, 1.0)
    proba[0] = 1.0 - proba[1]
    del tail
    plane_gb, st = n * n * 4 / 1e9, _lib.stream_ptr()

    def report(what, t, gb, **kw):
        med, lo, hi = t
        print(json.dumps(dict(what=what, us=round(med * 1e3, 1), us_min=round(lo * 1e3, 1), us_max=round(hi * 1e3, 1), gb=round(gb, 3),
                              hbm_us=round(gb / opt.hbm_tbps * 1e3, 1), gbps=round(gb / (med * 1e-3), 1) if gb else None, **kw)), flush=True)

    tables = {}
    for n_bins in (1024, 4096):
        for spacing in ('linear', 'sqrt'):
            edges, coord = (t.to(dev) for t in T.bin_edges(0.0, 64.0, n_bins, spacing))
            h = T.RasterHistogram(edges, coord)
            report(f'bdn_raster_hist {n_bins} bins {spacing}', timed(lambda: h.update(chi2), opt.reps), plane_gb)
            report(f'bdn_raster_hist {n_bins} bins {spacing}, exclude raster', timed(lambda: h.update(chi2, exclude, 1), opt.reps), 1.25 * plane_gb)
            h.reset()
            h.update(chi2, exclude, 1)
            for methods in (('otsu', 'kittler', 'rosin'), T.METHODS):
                tab = {}
                t = timed(lambda: tab.update(t=h.select(methods)), opt.reps)
                rd = tab['t'].read()
                report(f'bdn_hist_threshold {n_bins} bins {spacing} {"+".join(methods)}', t, 0.0,
                       thresholds={m: rd[m]['value'] if rd[m]['ok'] else None for m in methods}, em_iters=rd['em']['iters'])
            tables[(n_bins, spacing)] = tab['t']
    table = tables[(1024, 'sqrt')]
    mask = torch.empty(n, n, dtype=torch.uint8, device=dev)
    report('bdn_raster_mask', timed(lambda: table.mask(chi2, 'rosin', out=mask), opt.reps), 1.25 * plane_gb)
    report('bdn_raster_mask, exclude raster', timed(lambda: table.mask(chi2, 'rosin', exclude=exclude, exclude_value=1, out=mask), opt.reps), 1.5 * plane_gb)
    hist = torch.zeros(2, 1024, dtype=torch.int64, device=dev)
    report('bdn_score_hist 1024 bins (yardstick: one probability plane and a label raster)',
           timed(lambda: _lib.call('bdn_score_hist', proba.data_ptr(), 0, labels.data_ptr(), -1, 1, 1, 2, n * n, 1024, hist.data_ptr(), None, st), opt.reps),
           1.25 * plane_gb)
    report('bdn_threshold_mask (yardstick: the threshold by value)',
           timed(lambda: _lib.call('bdn_threshold_mask', proba.data_ptr(), 1, 0.3, mask.data_ptr(), 2, n * n, st), opt.reps), 1.25 * plane_gb)
    band = torch.zeros(1, dtype=torch.int32, device=dev)
    d = chi2.reshape(1, n, n)
    report('bdn_mad_mask (yardstick: one band per date read for validity)',
           timed(lambda: _lib.call('bdn_mad_mask', proba.data_ptr(), d.data_ptr(), d.data_ptr(), band.data_ptr(), 1, None, 0, 0.01, 0, mask.data_ptr(),
                                   1, n, n, st), opt.reps), 3.25 * plane_gb)


if __name__ == '__main__':
    main()
