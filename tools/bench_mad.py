"""Times IR-MAD (fabric_amd/utils/mad.py) on a 10 000 x 10 000 pair of 13 bands: bdn_mad_centre, bdn_mad_moments (unweighted and weighted),
bdn_mad_solve, bdn_mad_chi2 and bdn_mad_mask each on its own, a whole irmad at tol = 1e-3 with a budget of 30 iterations (every launch of
the budget is enqueued; those after the stop return at once) and one at the iteration count it converged at; beside them one
bdn_shift_apply and one K = 2 fit_transfer on the same scene, and the time that moving each entry's bytes at the HBM rate alone would take.
Device times are the median of event-timed repetitions after one warm-up; one JSON line per measurement.

    python tools/bench_mad.py [--sizes 10000] [--bands 13] [--reps 5] [--hbm_tbps 8.0] > profiles/mad_bench.txt
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fabric_amd import _lib                                  # noqa: E402
from fabric_amd.utils import mad as MAD                      # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[10000])
    ap.add_argument('--bands', type=int, default=13)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hbm_tbps', type=float, default=8.0, help='the HBM rate the byte counts are divided by (MI355X: 8 TB/s peak)')
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    nb = opt.bands
    line(device=torch.cuda.get_device_name(dev), torch=torch.__version__, bands=nb, reps=opt.reps, hbm_tbps=opt.hbm_tbps,
         note='ms = median of event-timed repetitions after one warm-up; hbm_ms = the bytes the entry must move / the HBM rate; gbps = those bytes / ms')
    for n in opt.sizes:
        g = torch.Generator(device=dev).manual_seed(n)
        d1 = torch.randn(nb, n, n, device=dev, generator=g)
        d2 = torch.empty_like(d1)
        for c in range(nb):                                  # band by band: no second scene-sized temporary
            d2[c] = 1.3 * d1[c] + 0.2 + 0.3 * torch.randn(n, n, device=dev, generator=g)
        d2[:, n // 4:n // 4 + n // 10, n // 2:n // 2 + n // 10] += 1.5          # a changed block: 1 % of the scene
        scene_gb, plane_gb = 2 * d1.numel() * 4 / 1e9, n * n * 4 / 1e9
        scene = f'{nb}x{n}x{n}'

        def report(what, t, gb, **kw):
            med, lo, hi = t
            line(scene=scene, what=what, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), gb=round(gb, 3),
                 hbm_ms=round(gb / opt.hbm_tbps, 3), gbps=round(gb / (med * 1e-3), 1), **kw)

        st, lib = _lib.stream_ptr(), _lib.load()
        band_t = torch.arange(nb, dtype=torch.int32, device=dev)
        f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)
        cen, mom, state, nv = f64(2 * nb), f64(MAD.moment_doubles(nb)), f64(MAD.state_doubles(nb)), torch.empty(1, dtype=torch.int64, device=dev)
        chi2, proba, mask = torch.empty(n, n, device=dev), torch.empty(2, n, n, device=dev), torch.empty(n, n, dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.bdn_mad_workspace_bytes(nb, n, n), dtype=torch.uint8, device=dev)
        sc = (d1.data_ptr(), d2.data_ptr(), band_t.data_ptr(), nb, None, 0)
        centre = lambda: _lib.call('bdn_mad_centre', *sc, cen.data_ptr(), nv.data_ptr(), ws.data_ptr(), nb, n, n, st)
        moments = lambda w: _lib.call('bdn_mad_moments', *sc, w, cen.data_ptr(), None, mom.data_ptr(), ws.data_ptr(), nb, n, n, st)
        solve = lambda: _lib.call('bdn_mad_solve', mom.data_ptr(), cen.data_ptr(), nv.data_ptr(), nb, 1, 0.0, 1e-9, state.data_ptr(), st)
        chi = lambda: _lib.call('bdn_mad_chi2', *sc, state.data_ptr(), chi2.data_ptr(), proba.data_ptr(), None, nb, n, n, st)
        report('bdn_mad_centre', timed(centre, opt.reps), scene_gb)
        report('bdn_mad_moments, unweighted', timed(lambda: moments(None), opt.reps), scene_gb)
        report('bdn_mad_solve', timed(solve, opt.reps), 0.0)
        report('bdn_mad_chi2', timed(chi, opt.reps), scene_gb + 3 * plane_gb)
        report('bdn_mad_moments, weighted', timed(lambda: moments(proba.data_ptr()), opt.reps), scene_gb + plane_gb)
        report('bdn_mad_mask', timed(lambda: _lib.call('bdn_mad_mask', proba.data_ptr(), *sc, 0.01, 0, mask.data_ptr(), nb, n, n, st), opt.reps),
               scene_gb + 1.25 * plane_gb)
        res = {}
        t = timed(lambda: res.update(r=MAD.irmad(d1, d2, iters=30, tol=1e-3)), opt.reps)
        rd = res['r'].read()
        per_iter = 2 * scene_gb + 4 * plane_gb
        report('irmad(iters=30, tol=1e-3)', t, scene_gb + rd['iters'] * per_iter - plane_gb, iters=rd['iters'], converged=rd['converged'],
               rho_min=round(float(rd['rho'].min()), 6), rho_max=round(float(rd['rho'].max()), 6))
        report(f'irmad(iters={rd["iters"]}, tol=1e-3): the count it converged at', timed(lambda: MAD.irmad(d1, d2, iters=rd['iters'], tol=1e-3), opt.reps),
               scene_gb + rd['iters'] * per_iter - plane_gb, iters=rd['iters'])
        del chi2, proba, res
        out = torch.empty_like(d2)
        field = torch.zeros(1, 1, 2, device=dev)
        report('bdn_shift_apply (yardstick: reads and writes every band once)', timed(lambda: RG.apply_shift(d2, field, out=out), opt.reps), scene_gb)
        del out
        report('fit_transfer K=2 (yardstick: reads each date three times)', timed(lambda: RM.fit_transfer(d2, d1, [0.02, 0.98], 2, extrapolate='slope'), opt.reps),
               3 * scene_gb)
        del d1, d2
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
