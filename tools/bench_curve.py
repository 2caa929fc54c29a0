"""Micro-benchmark (test infrastructure): bdn_score_hist alone, through the C ABI, beside bdn_argmax on the same bytes in the same process
(bdn_argmax is the existing HBM-bound kernel that reads the same tensor).  Two shapes -- the training shape, B=64 2x128x128 logits, and a
10 000^2 two-class probability map -- and three inputs each: uniform scores, a realistic skew (97 % of the pixels negative with a score
below 1 / n_bins) and all pixels in one (label, bin) cell.  The entry points are timed alternately, one event pair per call, and the
medians over REPS calls are printed with the bytes each call has to move (the recorded run: profiles/curve_bench.txt).
python tools/bench_curve.py   (N_BINS, REPS, BIDATE_LIB from the environment)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fabric_amd import _lib

N_BINS = int(os.environ.get('N_BINS', 1024))
REPS = int(os.environ.get('REPS', 200))
_lib.load()
st = _lib.stream_ptr()
dev = 'cuda'
P = lambda t: None if t is None else t.data_ptr()


def median_us(fns, reps=REPS):
    """Medians (and the 10 % / 90 % points) of the per-call times of the callables, run in turn (a, b, c, a, b, c, ...) after a warm-up of each."""
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


def scores_and_labels(kind, n, gen):
    """float32 scores [n] in (0, 1) and uint8 labels [n]."""
    if kind == 'uniform':
        s = torch.rand(n, device=dev, generator=gen).clamp_(1e-6, 1 - 1e-6)
        lab = (torch.rand(n, device=dev, generator=gen) < s).to(torch.uint8)
    elif kind == 'skew':                                  # 97 % negatives below the first bin edge; the rest spread, a third of them positives
        s = torch.rand(n, device=dev, generator=gen)
        low = torch.rand(n, device=dev, generator=gen) < 0.97
        s = torch.where(low, s * (0.9 / N_BINS) + 1e-7, s.clamp(1e-6, 1 - 1e-6))
        lab = (~low & (torch.rand(n, device=dev, generator=gen) < 0.34)).to(torch.uint8)
    else:                                                 # one cell
        s = torch.full((n,), 0.5, device=dev)
        lab = torch.zeros(n, dtype=torch.uint8, device=dev)
    return s, lab


def run(title, is_logits, B, H, W):
    n = B * H * W
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.zeros(2, N_BINS, dtype=torch.int64, device=dev)
    out = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    scores_out = torch.empty(B, H, W, device=dev)
    base = None
    for kind in ('uniform', 'skew', 'one cell'):
        s, lab = scores_and_labels(kind, n, gen)
        x = torch.empty(B, 2, H, W, device=dev)
        if is_logits:                                     # logits (0, z) whose softmax gives s for class 1
            x[:, 0] = 0
            x[:, 1] = torch.log(s / (1 - s)).reshape(B, H, W)
        else:
            x[:, 1] = s.reshape(B, H, W)
            x[:, 0] = 1 - x[:, 1]
        del s
        h = lambda so=None: _lib.call('bdn_score_hist', P(x), is_logits, P(lab), -1, 1, B, 2, H * W, N_BINS, P(hist), P(so), st)
        a = lambda: _lib.call('bdn_argmax', P(x), P(out), B, 2, H, W, st)
        res = median_us([h, lambda: h(scores_out), a])
        read = (8 if is_logits else 4) * n + n            # a probability map: only the plane of pos_class is read
        mb = [read, read + 4 * n, 8 * n + n]
        base = base or res[0][0]
        for name, (med, lo, hi), bts in zip(('bdn_score_hist', 'bdn_score_hist + scores_out', 'bdn_argmax'), res, mb):
            print(f'{title:26s} {kind:8s} {name:28s} median {med:8.1f} us (10 % {lo:8.1f}, 90 % {hi:8.1f})  {bts / 1e6:7.1f} MB  '
                  f'{bts / med / 1e6:6.2f} TB/s   x{med / res[2][0]:.2f} of argmax   x{med / base:.2f} of uniform', flush=True)
        del x, lab


print(f'n_bins = {N_BINS}, REPS = {REPS}', flush=True)
run('logits 64x2x128x128', 1, 64, 128, 128)
run('proba 1x2x10000x10000', 0, 1, 10000, 10000)
