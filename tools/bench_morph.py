"""Micro-benchmark (test infrastructure): the mask clean-up functions of fabric_amd.utils.morphology on a 10 000 x 10 000 raster at 2 % and
30 % density (the blob masks of tools/bench_cc.py: a smoothed random field cut at a quantile, its field as the probability map):
hysteresis_mask, fill_holes, binary_opening and binary_closing at radius2 2 and 25, and the full chain (hysteresis, closing, hole filling,
opening, area filter) -- beside remove_small_objects, bdn_threshold_mask and distance_transform_sq on the same raster in the same run, as
yardsticks for one labelling, one streaming pass and one distance transform.  The functions are timed through their Python surface
(allocations included: that is what a caller pays), in turn, one event pair per call; medians over REPS calls.
The output is also written to OUT (default profiles/morph_bench.txt).
python tools/bench_morph.py   (SIDE, REPS, OUT, BIDATE_LIB from the environment)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fabric_amd import _lib
from fabric_amd.utils import morphology as M
from fabric_amd.utils.distance import distance_transform_sq
from fabric_amd.utils.objects import remove_small_objects

SIDE = int(os.environ.get('SIDE', 10000))
REPS = int(os.environ.get('REPS', 20))
OUT = os.environ.get('OUT', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'morph_bench.txt'))
lib = _lib.load()
dev = 'cuda'
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def median_us(fns, reps=REPS):
    """Medians (and the 10 % / 90 % points) of the per-call times of the callables, run in turn (a, b, c, a, b, c, ...) after a warm-up of each."""
    for f in fns:
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for k, f in enumerate(fns):
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    out = []
    for k in range(len(fns)):
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[k])
        out.append((t[len(t) // 2], t[len(t) // 10], t[9 * len(t) // 10]))
    return out


def blob_field(h, w, gen):
    x = torch.rand(1, 1, h, w, device=dev, generator=gen)
    return torch.nn.functional.avg_pool2d(x, 5, stride=1, padding=2)[0, 0].contiguous()


def run(density, conn=8, min_area=16):
    h = w = SIDE
    n = h * w
    gen = torch.Generator(device=dev).manual_seed(0)
    field = blob_field(h, w, gen)
    sample = field.flatten()[:: max(1, n // 1000000)]
    high = float(torch.quantile(sample, 1 - density))
    low = float(torch.quantile(sample, 1 - min(1.5 * density, 0.9)))          # half as much weak change again
    proba = torch.stack([1 - field, field]).contiguous()
    del field, sample
    mask = torch.empty(h, w, dtype=torch.uint8, device=dev)
    _lib.call('bdn_threshold_mask', proba.data_ptr(), 1, high, mask.data_ptr(), 2, n, _lib.stream_ptr())
    out = torch.empty_like(mask)

    def chain():
        M.hysteresis_mask(proba, low, high, 1, conn, out=out)
        M.cleanup_mask(out, 2, True, 2, conn)
        remove_small_objects(out, min_area, conn, out=out)

    fns = [('hysteresis_mask', lambda: M.hysteresis_mask(proba, low, high, 1, conn, out=out)),
           ('fill_holes', lambda: M.fill_holes(mask, None, conn, out=out)),
           ('binary_opening r2=2', lambda: M.binary_opening(mask, 2, out=out)),
           ('binary_opening r2=25', lambda: M.binary_opening(mask, 25, out=out)),
           ('binary_closing r2=2', lambda: M.binary_closing(mask, 2, out=out)),
           ('binary_closing r2=25', lambda: M.binary_closing(mask, 25, out=out)),
           ('chain (hyst, close 2, fill, open 2, min_area)', chain),
           ('remove_small_objects', lambda: remove_small_objects(mask, min_area, conn, out=out)),
           ('bdn_threshold_mask', lambda: _lib.call('bdn_threshold_mask', proba.data_ptr(), 1, high, out.data_ptr(), 2, n, _lib.stream_ptr())),
           ('distance_transform_sq', lambda: distance_transform_sq(mask)),
           ('distance_transform_sq max_dist=5', lambda: distance_transform_sq(mask, max_dist=5))]
    res = median_us([f for _, f in fns])
    t = {name: r[0] for (name, _), r in zip(fns, res)}
    say(f'density {density:.2f} ({float(mask.float().mean()):.4f} foreground at the high threshold {high:.4f}, low threshold {low:.4f}), '
        f'connectivity {conn}, min_area {min_area}')
    for (name, _), (med, lo, hi) in zip(fns, res):
        say(f'  {name:46s} median {med:10.1f} us (10 % {lo:10.1f}, 90 % {hi:10.1f})   x{med / t["remove_small_objects"]:5.2f} of remove_small_objects   '
            f'x{med / t["distance_transform_sq"]:5.2f} of distance_transform_sq')
    say(f'  hysteresis_mask / remove_small_objects = {t["hysteresis_mask"] / t["remove_small_objects"]:.2f} (expected <= 2);   '
        f'binary_opening r2=2 / distance_transform_sq = {t["binary_opening r2=2"] / t["distance_transform_sq"]:.2f}, r2=25: '
        f'{t["binary_opening r2=25"] / t["distance_transform_sq"]:.2f} (expected <= 2.5)')
    torch.cuda.synchronize()


say(f'{SIDE} x {SIDE}, REPS = {REPS}, {torch.cuda.get_device_name(0)}')
for d in (0.02, 0.30):
    run(d)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(_lines) + '\n')
