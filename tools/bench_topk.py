"""Micro-benchmark (test infrastructure): bdn_criterion_topk against bdn_criterion_masked on the same build and the same inputs, through
the C ABI at B=64 2x128x128, focal(2)+dice, both reductions, with and without the gradient pass, at topk_ppm 1 000 000 / 250 000 /
100 000.  The entry points are timed alternately, one event pair per call, and the medians over REPS calls are printed (the recorded run:
profiles/topk_bench.txt).  python tools/bench_topk.py   (BIDATE_LIB selects a library variant)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fabric_amd import _lib

B, NC, H, W = int(os.environ.get('B', 64)), 2, 128, 128
REPS = int(os.environ.get('REPS', 300))
PPMS = (1_000_000, 250_000, 100_000)
lib = _lib.load()
st = _lib.stream_ptr()
dev = 'cuda'
torch.manual_seed(0)
logits = 3 * torch.randn(B, NC, H, W, device=dev)
labels = (torch.rand(B, H, W, device=dev) < 0.1).to(torch.uint8)
labels = torch.where(torch.rand(B, H, W, device=dev) < 0.1, torch.full_like(labels, 255), labels)        # 10 % unlabelled
dlogits = torch.empty_like(logits)
loss, terms = torch.empty(1, device=dev), torch.empty(3, device=dev)
counts = torch.empty(6, dtype=torch.int32, device=dev)
P = lambda t: None if t is None else t.data_ptr()


def median_us(fns, reps=REPS):
    """Medians of the per-call times of the callables, run in turn (a, b, c, a, b, c, ...) after a warm-up of each."""
    for f in fns:
        for _ in range(5):
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


for reduce_w in (0, 1):
    ws_m = torch.empty(lib.bdn_criterion_masked_workspace_bytes(B, NC, H, W, reduce_w) + 16, dtype=torch.uint8, device=dev)
    ws_t = torch.empty(lib.bdn_criterion_topk_workspace_bytes(B, NC, H, W, reduce_w) + 16, dtype=torch.uint8, device=dev)
    for grad in (True, False):
        dl = dlogits if grad else None
        masked = lambda: _lib.call('bdn_criterion_masked', P(logits), P(labels), 255, 1.0, 0.5, 0.5, 5e-8, reduce_w, 1.0, 2.0, None, 1,
                                   P(ws_m), P(loss), P(terms), P(counts), P(dl), B, NC, H, W, st)
        topk = lambda ppm: _lib.call('bdn_criterion_topk', P(logits), P(labels), 255, 1.0, 0.5, 0.5, 5e-8, reduce_w, 1.0, 2.0, None, 1, ppm,
                                     P(ws_t), P(loss), P(terms), P(counts), P(dl), None, None, B, NC, H, W, st)
        res = median_us([masked] + [lambda ppm=ppm: topk(ppm) for ppm in PPMS])
        names = ['bdn_criterion_masked'] + [f'bdn_criterion_topk ppm={ppm}' for ppm in PPMS]
        for name, (med, lo, hi) in zip(names, res):
            print(f"reduce={'image' if reduce_w else 'columns':7s} gradient={'yes' if grad else 'no ':3s} {name:36s} median {med:7.1f} us "
                  f'(10 % {lo:7.1f}, 90 % {hi:7.1f})   x{med / res[0][0]:.3f}', flush=True)
