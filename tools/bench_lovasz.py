"""Micro-benchmark (test infrastructure): the Lovasz-Softmax term at B=64 2x128x128, forward + gradient, in one process:

    bdn_criterion_masked           focal(2)+jaccard, the criterion users pair it with today
    focal+lovasz                   bdn_criterion_masked (focal alone) + bdn_lovasz_softmax(accumulate=1), what Criterion.evaluate launches
    torch on the device            the same term restated with softmax, torch.sort, cumsum and autograd backward (+ cross-entropy)

timed alternately, one event pair per call, medians over REPS calls; then the two entry points of focal+lovasz apart (the kernels of the
term apart: rocprofv3 --kernel-trace --stats over this script with STEP=0) and the whole bf16 TrainStep of BiDateNet(13, 2) at B=64 with the
default criterion, focal+jaccard and focal+lovasz, alternately.  The recorded run: profiles/lovasz_bench.txt.
python tools/bench_lovasz.py   (BIDATE_LIB selects a library variant; STEP=0 skips the train step)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fabric_amd import BiDateNet, _lib
from fabric_amd.criterion import Criterion
from fabric_amd.train_step import TrainStep

B, NC, H, W = int(os.environ.get('B', 64)), 2, 128, 128
REPS = int(os.environ.get('REPS', 200))
lib = _lib.load()
dev = 'cuda'
torch.manual_seed(0)
logits = 3 * torch.randn(B, NC, H, W, device=dev)
labels = (torch.rand(B, H, W, device=dev) < 0.1).to(torch.uint8)
labels = torch.where(torch.rand(B, H, W, device=dev) < 0.1, torch.full_like(labels, 255), labels)        # 10 % unlabelled


def median_us(fns, reps=REPS, warm=5):
    """Medians (and the 10 % / 90 % points) of the per-call times of the callables, run in turn (a, b, c, a, b, c, ...) after a warm-up."""
    for f in fns:
        for _ in range(warm):
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


def torch_route(lg, lb):
    """cross-entropy + batch-level Lovasz-Softmax ('present') with library calls only: what a user would write without the fused term."""
    x = lg.detach().requires_grad_(True)
    flat = x.permute(0, 2, 3, 1).reshape(-1, NC)
    t = lb.reshape(-1).long()
    keep = t != 255
    flat, t = flat[keep], t[keep]
    ce = torch.nn.functional.cross_entropy(flat, t)
    p = torch.softmax(flat, 1)
    losses = []
    for c in range(NC):
        fg = (t == c).float()
        es, perm = torch.sort((fg - p[:, c]).abs(), descending=True, stable=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1 - fs).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac))
    loss = ce + torch.stack(losses).mean()            # (both classes are present in these labels)
    loss.backward()
    return loss.detach(), x.grad


jac = Criterion.parse('focal+jaccard', focal_gamma=2.0, ignore_index=255)
lov = Criterion.parse('focal+lovasz', focal_gamma=2.0, ignore_index=255)
ce_lov = Criterion.parse('focal+lovasz', focal_gamma=0.0, ignore_index=255)
alone = Criterion.parse('lovasz', ignore_index=255)
bufs = {c: c.buffers(logits.shape, logits.device) for c in (jac, lov, ce_lov, alone)}

# the restatement computes what the fused term computes (float32 sort keys differ in ties and roundings only)
fused = ce_lov.evaluate(logits, labels, out=bufs[ce_lov])
ref_loss, ref_grad = torch_route(logits, labels)
torch.cuda.synchronize()
print(f'B={B} {NC}x{H}x{W}, 10 % unlabelled; CE + Lovasz: fused loss {fused[0].item():.7f}, torch restatement {ref_loss.item():.7f}, '
      f'max|dlogits diff| {(fused[3] - ref_grad).abs().max().item():.3e} of max|dlogits| {ref_grad.abs().max().item():.3e}', flush=True)

rows = [('bdn_criterion_masked focal(2)+jaccard', lambda: jac.evaluate(logits, labels, out=bufs[jac])),
        ('focal(2)+lovasz (masked + bdn_lovasz_softmax)', lambda: lov.evaluate(logits, labels, out=bufs[lov])),
        ('CE+lovasz, torch sort / cumsum / autograd', lambda: torch_route(logits, labels)),
        ('lovasz alone (counts + bdn_lovasz_softmax)', lambda: alone.evaluate(logits, labels, out=bufs[alone]))]
res = median_us([f for _, f in rows])
for (name, _), (med, lo, hi) in zip(rows, res):
    print(f'forward + gradient  {name:48s} median {med:8.1f} us (10 % {lo:8.1f}, 90 % {hi:8.1f})   x{med / res[0][0]:.2f} of focal+jaccard', flush=True)
print(f'fused focal+lovasz against the torch restatement: x{res[1][0] / res[2][0]:.3f} of its time', flush=True)

# the two entry points of focal+lovasz apart, by _lib's profiling hook (one event pair per entry point); the kernels of the term apart:
# rocprofv3 --kernel-trace --stats over this script with STEP=0
_lib.PROFILE = []
for _ in range(20):
    lov.evaluate(logits, labels, out=bufs[lov])
torch.cuda.synchronize()
per = {}
for name, _, _, e0, e1 in _lib.PROFILE:
    per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
_lib.PROFILE = None
for name, t in per.items():
    t.sort()
    print(f'entry point  {name:28s} median {t[len(t) // 2]:8.1f} us', flush=True)

if int(os.environ.get('STEP', 1)):
    C = 13
    g = torch.Generator().manual_seed(0)
    x1 = torch.randn(B, C, H, W, generator=g)
    x2 = (x1 + 0.3 * torch.randn(B, C, H, W, generator=g)).to(dev)
    x1 = x1.to(dev)
    sd = {k: v.clone() for k, v in BiDateNet(C, 2).state_dict().items()}
    steps = {}
    for name, crit in (('default (bdn_tversky)', None), ('focal(2)+jaccard', jac), ('focal(2)+lovasz', lov)):
        m = BiDateNet(C, 2, precision='bf16')
        m.load_state_dict(sd)
        steps[name] = TrainStep(m.to(dev).train(), lr=1e-3, criterion=crit)
    import statistics
    rounds, n_steps = int(os.environ.get('STEP_ROUNDS', 5)), int(os.environ.get('STEP_N', 10))
    ms = {name: [] for name in steps}
    with torch.cuda.stream(next(iter(steps.values())).stream()):        # every TrainStep shares the process's chain stream
        for _ in range(rounds):
            for name, ts in steps.items():
                for _ in range(3):
                    ts.step(x1, x2, labels)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_steps):
                    ts.step(x1, x2, labels)
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / n_steps)
    med = {name: statistics.median(v) for name, v in ms.items()}
    base, default = med['focal(2)+jaccard'], med['default (bdn_tversky)']
    for name in steps:
        print(f'bf16 TrainStep B={B} 13x{H}x{W}  {name:24s} median {med[name]:8.4f} ms  {(med[name] - base) * 1e3:+8.1f} us against focal+jaccard '
              f'({100 * (med[name] - base) / base:+.2f} %), {100 * (med[name] - default) / default:+.2f} % against the default step   '
              f'{[round(t, 4) for t in ms[name]]}', flush=True)
