"""Micro-benchmark (test infrastructure): co-registration on the device, in one process:

    (a) estimate_shift (bdn_shift_corr + bdn_shift_peak) at R = 8 with 13 and 3 bands, cells 1 x 1 and 8 x 8, and apply_shift
        (bdn_shift_apply, 13 bands) on an OSCD-sized city (500 x 500) and on a SCENE x SCENE pair (default 10 000)
    (b) the entry points of one estimate, each with its own event pair
    (c) the host route: the vectorised numpy table of tests/register_ref.py (exact=False) on ONE band of a CROP x CROP crop (default
        2 000), SCALED to the scene and band count by pair products (HOST=0 skips it: it takes about a minute)

timed with one event pair per call, medians over REPS calls after a warm-up.  A pair product is one (pixel, shift, band) term: five double
additions / fused multiply-adds (sum a, sum b, sum a^2, sum b^2, sum a b) and a count.  The rate is set against the device's peak
double-precision vector rate (PEAK_FP64_TFLOPS, 78.6 for the MI355X data sheet; an FMA counts two).  The recorded run:
profiles/register_bench.txt.
python tools/bench_register.py   (BIDATE_LIB selects a library variant; SCENE=N the large scene's edge)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from fabric_amd import _lib
from fabric_amd.utils import registration as RG

REPS = int(os.environ.get('REPS', 5))
SCENE = int(os.environ.get('SCENE', 10000))
CROP = int(os.environ.get('CROP', 2000))
HOST = int(os.environ.get('HOST', 1))
PEAK = float(os.environ.get('PEAK_FP64_TFLOPS', 78.6))
R = 8
dev = 'cuda'
torch.manual_seed(0)
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def median_ms(f, reps=REPS, warm=1):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        f()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def pair(c, n):
    """date 2 = date 1 moved by (2, -1) plus noise; made band by band to keep the peak allocation at two stacks."""
    d1 = torch.empty(c, n, n, device=dev)
    d2 = torch.empty(c, n, n, device=dev)
    for k in range(c):
        d1[k].normal_()
        d2[k] = torch.roll(d1[k], (-2, 1), (0, 1))
        d2[k] += 0.3 * torch.randn(n, n, device=dev)
    return d1, d2


say(f'(a) estimate_shift at R = {R} ({(2 * R + 1) ** 2} shifts) and apply_shift; medians of {REPS} calls (fastest, slowest)')
for n in (500, SCENE):
    d1, d2 = pair(13, n)
    out = torch.empty_like(d2)
    for bands in (list(range(13)), [1, 2, 3]):
        for cells in ((1, 1), (8, 8)):
            est = RG.estimate_shift(d1, d2, R, bands, cells)
            rep = est.read()
            assert (round(rep['dy']), round(rep['dx'])) == (-2, 1), rep
            med, lo, hi = median_ms(lambda: RG.estimate_shift(d1, d2, R, bands, cells), reps=REPS if n > 2000 else 10 * REPS)
            pairs = len(bands) * n * n * (2 * R + 1) ** 2
            ws = _lib.load().bdn_shift_corr_workspace_bytes(len(bands), n, n, R, *cells)
            say(f'    {n:5d}^2  {len(bands):2d} bands  cells {cells[0]} x {cells[1]}   median {med:10.3f} ms ({lo:10.3f}, {hi:10.3f})   '
                f'{pairs / med / 1e6:8.1f} G pair products/s   {100 * pairs * 7 / (med * 1e-3) / (PEAK * 1e12):5.1f} % of the FP64 vector peak '
                f'(7 flop per pair product)   workspace {ws / 2 ** 20:6.1f} MiB   ncc {rep["ncc"]:.4f}')
    field = RG.estimate_shift(d1, d2, R, [1, 2, 3], (8, 8)).field
    med, lo, hi = median_ms(lambda: RG.apply_shift(d2, field, out), reps=REPS if n > 2000 else 10 * REPS)
    say(f'    {n:5d}^2  13 bands  apply_shift (8 x 8 field)   median {med:10.3f} ms ({lo:10.3f}, {hi:10.3f})   '
        f'{2 * 13 * n * n * 4 / (med * 1e-3) / 1e12:6.3f} TB/s of planes read once and written once')
    for cells in ((1, 1), (8, 8)):
        say(f'(b) the entry points of one estimate, {n}^2, 13 bands, cells {cells[0]} x {cells[1]}')
        _lib.PROFILE = []
        for _ in range(5):
            RG.estimate_shift(d1, d2, R, None, cells)
        torch.cuda.synchronize()
        per = {}
        for name, _, _, e0, e1 in _lib.PROFILE:
            per.setdefault(name, []).append(e0.elapsed_time(e1))
        _lib.PROFILE = None
        for name, t in per.items():
            t.sort()
            say(f'    entry point  {name:18s} median {t[len(t) // 2]:10.3f} ms')
    if n == SCENE and HOST:
        from tests import register_ref as RR
        crop = min(CROP, n)
        h1, h2 = d1[:1, :crop, :crop].cpu().numpy(), d2[:1, :crop, :crop].cpu().numpy()
        t0 = time.perf_counter()
        rep_h, _ = RR.estimate_ref(h1, h2, R, exact=False)
        t1 = time.perf_counter()
        assert (round(rep_h[-1, 0]), round(rep_h[-1, 1])) == (-2, 1)
        scale = 13 * n * n / (crop * crop)
        say(f'(c) host route: numpy table + peak on 1 band of a {crop}^2 crop {t1 - t0:8.2f} s; SCALED by pair products (x{scale:.0f}) to 13 bands '
            f'of {n}^2: {scale * (t1 - t0):9.1f} s (not run at that size)')
    del d1, d2, out

out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'register_bench.txt')
with open(out_path, 'w') as fh:
    fh.write('python tools/bench_register.py\n' + '\n'.join(LINES) + '\n')
