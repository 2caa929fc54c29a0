"""Micro-benchmark (test infrastructure): bdn_cc_label + bdn_cc_filter through the C ABI on a 10 000 x 10 000 mask at 2 % and 30 % density
(blobs of a few pixels, as a thresholded change map has them, not white noise), beside bdn_threshold_mask on a probability map of the same
scene -- the existing one-pass kernel, as a yardstick for what one pass over the scene costs.  The entry points are timed alternately, one
event pair per call, and the medians over REPS calls are printed with the bytes each call has to move; bdn_cc_label is timed with and
without its area output (the difference is the flatten kernel's atomics and the tile kernel's zeroing).  The host alternative -- scipy.ndimage.label + np.bincount plus the
device-to-host copy of the mask and the host-to-device copy of the filtered one -- is timed in the same script where scipy is importable.
The output is also written to OUT (default profiles/cc_bench.txt).
python tools/bench_cc.py   (SIDE, REPS, OUT, HOST=0 to skip the host part, BIDATE_LIB from the environment)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fabric_amd import _lib

SIDE = int(os.environ.get('SIDE', 10000))
REPS = int(os.environ.get('REPS', 20))
OUT = os.environ.get('OUT', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'cc_bench.txt'))
lib = _lib.load()
st = _lib.stream_ptr()
dev = 'cuda'
P = lambda t: None if t is None else t.data_ptr()
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def median_us(fns, reps=REPS):
    """Medians (and the 10 % / 90 % points) of the per-call times of the callables, run in turn (a, b, c, a, b, c, ...) after a warm-up of each."""
    for f in fns:
        for _ in range(3):
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


def blob_mask(h, w, density, gen):
    """uint8 [h,w]: a smoothed random field thresholded at the quantile that leaves `density` foreground -- blobs, not white noise."""
    x = torch.rand(1, 1, h, w, device=dev, generator=gen)
    x = torch.nn.functional.avg_pool2d(x, 5, stride=1, padding=2)
    thr = torch.quantile(x.flatten()[:: max(1, h * w // 1000000)], 1 - density)
    return (x[0, 0] > thr).to(torch.uint8).contiguous(), x[0, 0].contiguous()


def run(density, conn=8, min_area=16):
    h = w = SIDE
    n = h * w
    gen = torch.Generator(device=dev).manual_seed(0)
    mask, field = blob_mask(h, w, density, gen)
    proba = torch.stack([1 - field, field]).contiguous()
    del field
    labels = torch.empty(h, w, dtype=torch.int32, device=dev)
    area = torch.empty(h, w, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    out = torch.empty_like(mask)
    tmask = torch.empty_like(mask)
    ws = torch.empty(lib.bdn_cc_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
    lab = lambda a=area: _lib.call('bdn_cc_label', P(mask), 1, None, 0, conn, h, w, P(labels), P(a), P(counts), P(ws), st)
    flt = lambda: _lib.call('bdn_cc_filter', P(mask), P(labels), P(area), min_area, P(out), h, w, st)
    thr = lambda: _lib.call('bdn_threshold_mask', P(proba), 1, 0.5, P(tmask), 2, n, st)
    res = median_us([lab, lambda: lab(None), flt, thr])
    c = counts.tolist()
    fgd = c[1] / n
    # bytes each call must move: label = mask in, parents out and in (tile, flatten; the seams touch 1/32 of them), labels out, area
    # zeroed; filter = labels in, mask out, one area word per foreground pixel; threshold = one float plane in, mask out
    mb = [n * (1 + 4 + 4 + 4 + 4), n * (1 + 4 + 4 + 4), n * (4 + 1) + 4 * c[1], n * (4 + 1)]
    say(f'density {density:.2f} ({fgd:.4f} foreground, {c[0]} components, status {c[2]}), connectivity {conn}, min_area {min_area}')
    for name, (med, lo, hi), b in zip(('bdn_cc_label (with area)', 'bdn_cc_label (area NULL)', 'bdn_cc_filter', 'bdn_threshold_mask'), res, mb):
        say(f'  {name:26s} median {med:9.1f} us (10 % {lo:9.1f}, 90 % {hi:9.1f})  {b / 1e6:7.1f} MB  {b / med / 1e6:6.3f} TB/s   '
            f'x{med / res[3][0]:.1f} of threshold_mask')
    say(f'  label + filter             {res[0][0] + res[2][0]:9.1f} us')
    torch.cuda.synchronize()
    if os.environ.get('HOST', '1') == '0':
        return
    try:
        import numpy as np
        from scipy import ndimage
    except ImportError:
        say('  host alternative: scipy is not importable here')
        return
    t0 = time.perf_counter()
    m = mask.cpu().numpy()
    t1 = time.perf_counter()
    hl, hn = ndimage.label(m, ndimage.generate_binary_structure(2, 2 if conn == 8 else 1))
    t2 = time.perf_counter()
    keep = (np.bincount(hl.ravel()) >= min_area)
    keep[0] = False
    hm = keep[hl].astype(np.uint8)
    t3 = time.perf_counter()
    back = torch.from_numpy(hm).to(dev)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    same = bool(torch.equal(back, out)) and hn == c[0]
    say(f'  host alternative: copy down {t1 - t0:.3f} s, scipy.ndimage.label {t2 - t1:.3f} s, bincount + filter {t3 - t2:.3f} s, copy up '
        f'{t4 - t3:.3f} s = {t4 - t0:.3f} s (single thread, pageable copies); same mask and count as the device: {same}')


say(f'{SIDE} x {SIDE}, REPS = {REPS}, tile {lib.bdn_cc_tile()}, {torch.cuda.get_device_name(0)}')
for d in (0.02, 0.30):
    run(d)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(_lines) + '\n')
