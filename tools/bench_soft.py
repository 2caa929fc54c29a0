"""Micro-benchmark (test infrastructure): bdn_criterion_soft against bdn_criterion_masked -- existing code, the yardstick -- on the same
build and the same logits, through the C ABI at B=64 2x128x128 with the gradient pass, reduce='columns'.  Configurations: smoothing only,
smoothing + weights, float targets, float targets + weights; each for focal(2)+dice and for focal(2) alone, and for focal(0)+dice (cross-entropy + dice: no modulating factor, so no powf in
either pass).  The entry points are timed
alternately (masked, a, b, c, d, masked, ...), one event pair per call after a warm-up of each, and the median with the 10 % / 90 %
quantiles over REPS calls is printed beside the ratio to the masked median and the ratio of the bytes the passes move (computed from the
shapes: statistics pass reads, gradient pass reads and writes).  Before timing, the hard-label form at smoothing 0 is compared with the
masked entry point on the timed inputs.  Clocks are not touched.
    python tools/bench_soft.py [out.txt]   (BIDATE_LIB selects a library variant; B, REPS from the environment)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fabric_amd import _lib

B, NC, H, W = int(os.environ.get('B', 64)), 2, 128, 128
REPS = int(os.environ.get('REPS', 400))
assert torch.cuda.is_available(), 'bench_soft.py measures on a ROCm device: there is nothing to time without one'
lib = _lib.load()
st = _lib.stream_ptr()
dev = 'cuda'
torch.manual_seed(0)
logits = 3 * torch.randn(B, NC, H, W, device=dev)
labels = (torch.rand(B, H, W, device=dev) < 0.1).to(torch.uint8)
weights = torch.where(torch.rand(B, H, W, device=dev) < 0.3, torch.zeros((), device=dev), 2 * torch.rand(B, H, W, device=dev)).contiguous()
targets = torch.distributions.Dirichlet(torch.full((NC,), 0.5, device=dev)).sample((B, H, W)).permute(0, 3, 1, 2).contiguous()
dlogits = torch.empty_like(logits)
loss, terms = torch.empty(1, device=dev), torch.empty(2, device=dev)
counts = torch.empty(5, dtype=torch.int32, device=dev)
ws_m = torch.empty(lib.bdn_criterion_masked_workspace_bytes(B, NC, H, W, 0) + 16, dtype=torch.uint8, device=dev)
ws_s = torch.empty(lib.bdn_criterion_soft_workspace_bytes(B, NC, H, W, 0) + 16, dtype=torch.uint8, device=dev)
P = lambda t: None if t is None else t.data_ptr()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def masked(w_o, gamma):
    return lambda: _lib.call('bdn_criterion_masked', P(logits), P(labels), 255, w_o, 0.5, 0.5, 5e-8, 0, 1.0, gamma, None, 1, P(ws_m), P(loss),
                             P(terms), P(counts), P(dlogits), B, NC, H, W, st)


def soft(w_o, gamma, lab, tgt, wgt, e):
    return lambda: _lib.call('bdn_criterion_soft', P(logits), P(lab), P(tgt), P(wgt), 255 if lab is not None else -1, e, w_o, 0.5, 0.5, 5e-8,
                             0, 1.0, gamma, None, 1, P(ws_s), P(loss), P(terms), P(counts), P(dlogits), B, NC, H, W, st)


def bytes_moved(tgt, wgt):
    """Bytes per pixel of the statistics pass (reads) and the gradient pass (reads + the dlogits it writes)."""
    src = 4 * NC if tgt else 1
    return 2 * (4 * NC + src + (4 if wgt else 0)) + 4 * NC


def median_us(fns, reps=REPS):
    for f in fns:
        for _ in range(10):
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


say(f'bdn_criterion_soft vs bdn_criterion_masked, B={B} {NC}x{H}x{W}, reduce=columns, with the gradient pass, {torch.cuda.get_device_name(0)}, '
    f'{REPS} alternating calls each, event pair per call, median (10 % .. 90 %)')
for w_o, g, crit in ((1.0, 2.0, 'focal(2)+dice'), (0.0, 2.0, 'focal(2)'), (1.0, 0.0, 'focal(0)+dice')):
    masked(w_o, g)()
    want = (loss.clone(), dlogits.clone())
    soft(w_o, g, labels, None, None, 0.0)()
    torch.cuda.synchronize()
    say(f'{crit}: hard labels at smoothing 0 against the masked entry point on these inputs: |loss diff| {abs(loss.item() - want[0].item()):.2e}, '
        f'max|dlogits diff| {(dlogits - want[1]).abs().max().item():.2e} (max|dlogits| {want[1].abs().max().item():.2e})')
    cfgs = [('bdn_criterion_masked (yardstick)', masked(w_o, g), bytes_moved(False, False)),
            ('soft: smoothing 0.1', soft(w_o, g, labels, None, None, 0.1), bytes_moved(False, False)),
            ('soft: smoothing 0.1 + weights', soft(w_o, g, labels, None, weights, 0.1), bytes_moved(False, True)),
            ('soft: float targets', soft(w_o, g, None, targets, None, 0.0), bytes_moved(True, False)),
            ('soft: float targets + weights', soft(w_o, g, None, targets, weights, 0.0), bytes_moved(True, True))]
    res = median_us([c[1] for c in cfgs])
    for (name, _, nbytes), (med, lo, hi) in zip(cfgs, res):
        say(f'{crit:14s} {name:34s} median {med:7.1f} us ({lo:7.1f} .. {hi:7.1f})   x{med / res[0][0]:.3f} of masked   '
            f'{nbytes} B/pixel, x{nbytes / cfgs[0][2]:.3f} of masked')
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
