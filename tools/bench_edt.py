"""Micro-benchmark (test infrastructure): the device distance transform and the boundary term, in one process:

    (a) bdn_edt on one SCENE x SCENE mask (default 10 000): 2 % and 30 % density, an empty mask and a single-pixel mask, against
        bdn_threshold_mask on the same raster (a streaming pass: the floor for anything that touches every pixel) and against the host
        route, the copy down + scipy.ndimage.distance_transform_edt (HOST=0 skips it: it takes seconds per case)
    (b) the fused criterion at B=64 2x128x128, forward + gradient: focal(2)+jaccard, the same + the boundary term (foreground and all
        classes), and the term restated with a copy down, scipy on the host, a copy up and torch autograd
    (c) the whole bf16 TrainStep of BiDateNet(13, 2) at B=64 with focal+jaccard and with focal+jaccard + the boundary term, alternately

timed with one event pair per call, medians over REPS calls after a warm-up (tools/bench_lovasz.py's arrangement).  The recorded run:
profiles/edt_bench.txt.
python tools/bench_edt.py   (BIDATE_LIB selects a library variant; STEP=0 skips the train step, SCENE=N the scene edge)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from fabric_amd import BiDateNet, _lib
from fabric_amd.criterion import Criterion
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.distance import distance_transform_sq

B, NC, H, W = int(os.environ.get('B', 64)), 2, 128, 128
REPS = int(os.environ.get('REPS', 100))
SCENE = int(os.environ.get('SCENE', 10000))
HOST = int(os.environ.get('HOST', 1))
lib = _lib.load()
dev = 'cuda'
torch.manual_seed(0)
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def median_us(fns, reps=REPS, warm=3):
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


# ---------------------------------------------------------------- (a) scenes
from scipy import ndimage
masks = {'2 % density': (torch.rand(SCENE, SCENE, device=dev) < 0.02).to(torch.uint8),
         '30 % density': (torch.rand(SCENE, SCENE, device=dev) < 0.30).to(torch.uint8),
         'empty': torch.zeros(SCENE, SCENE, dtype=torch.uint8, device=dev),
         'single pixel': torch.zeros(SCENE, SCENE, dtype=torch.uint8, device=dev)}
masks['single pixel'][SCENE // 3, SCENE // 5] = 1
out = torch.empty(SCENE, SCENE, dtype=torch.int32, device=dev)
ws = torch.empty(lib.bdn_edt_workspace_bytes(1, SCENE, SCENE), dtype=torch.uint8, device=dev)
proba = torch.rand(2, SCENE, SCENE, device=dev)
tmask = torch.empty(SCENE, SCENE, dtype=torch.uint8, device=dev)
say(f'(a) bdn_edt on {SCENE} x {SCENE}: workspace {ws.numel() / 2 ** 20:.0f} MiB')


def edt_call(m):
    return lambda: _lib.call('bdn_edt', m.data_ptr(), 1, 1, None, 0, (1 << 31) - 1, out.data_ptr(), ws.data_ptr(), 1, SCENE, SCENE,
                             _lib.stream_ptr())


thr = median_us([lambda: _lib.call('bdn_threshold_mask', proba.data_ptr(), 1, 0.5, tmask.data_ptr(), 2, SCENE * SCENE, _lib.stream_ptr())],
                reps=20)[0]
say(f'    bdn_threshold_mask on the same raster            median {thr[0]:10.1f} us')
for name, m in masks.items():
    med, lo, hi = median_us([edt_call(m)], reps=max(5, REPS // 10), warm=1)[0]
    line = f'    bdn_edt {name:14s}                          median {med:10.1f} us (10 % {lo:10.1f}, 90 % {hi:10.1f})  x{med / thr[0]:.1f} of the threshold pass'
    if HOST:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = m.cpu().numpy()
        d = ndimage.distance_transform_edt(host != 1) if host.any() else np.full(host.shape, np.inf)
        t1 = time.perf_counter()
        if host.any():                                      # the same numbers: exact integers against the rounded float64 distances
            assert np.array_equal(out.cpu().numpy(), np.rint(d * d).astype(np.int64)), name
        line += f'   host copy + scipy {1e3 * (t1 - t0):9.1f} ms (x{1e6 * (t1 - t0) / med:.0f})'
    say(line)
del masks, out, ws, proba, tmask

# ---------------------------------------------------------------- (b) the criterion
logits = 3 * torch.randn(B, NC, H, W, device=dev)
small = torch.rand(B, H // 8, W // 8, device=dev) < 0.1
labels = small.repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.uint8)                            # 8 x 8 blocks of change, 10 %
labels = torch.where(torch.rand(B, H, W, device=dev) < 0.1, torch.full_like(labels, 255), labels)        # 10 % unlabelled


def host_route(lg, lb):
    """The boundary term as a user would write it today: labels down, scipy per image, phi up, softmax and autograd on the device."""
    lab = lb.cpu().numpy()
    phi = np.zeros(lab.shape, np.float32)
    for i in range(lab.shape[0]):
        valid = lab[i] != 255
        fg, bg = valid & (lab[i] == 1), valid & (lab[i] != 1)
        if fg.any() and bg.any():
            phi[i] = np.where(bg, ndimage.distance_transform_edt(~fg), np.where(fg, -(ndimage.distance_transform_edt(~bg) - 1), 0))
    phi_d = torch.from_numpy(phi).to(lg.device)
    x = lg.detach().requires_grad_(True)
    keep = (lb != 255)
    loss = (torch.softmax(x, 1)[:, 1] * phi_d * keep).sum() / keep.sum()
    loss.backward()
    return loss.detach(), x.grad


jac = Criterion.parse('focal+jaccard', focal_gamma=2.0, ignore_index=255)
bnd = Criterion.parse('focal+jaccard', focal_gamma=2.0, ignore_index=255, w_boundary=0.01)
bnd_all = Criterion.parse('focal+jaccard', focal_gamma=2.0, ignore_index=255, w_boundary=0.01, boundary_classes='all')
alone = Criterion(w_overlap=0.0, ignore_index=255, w_boundary=1.0)
bufs = {c: c.buffers(logits.shape, logits.device) for c in (jac, bnd, bnd_all, alone)}
fused = alone.evaluate(logits, labels, out=bufs[alone])
ref_loss, ref_grad = host_route(logits, labels)
torch.cuda.synchronize()
say(f'(b) B={B} {NC}x{H}x{W}, 10 % unlabelled; boundary term: fused {fused[1][-1].item():.7f}, host restatement {ref_loss.item():.7f}, '
      f'max|dlogits diff| {(fused[3] - ref_grad).abs().max().item():.3e} of max|dlogits| {ref_grad.abs().max().item():.3e}')
rows = [('bdn_criterion_masked focal(2)+jaccard', lambda: jac.evaluate(logits, labels, out=bufs[jac])),
        ('focal(2)+jaccard + boundary (foreground)', lambda: bnd.evaluate(logits, labels, out=bufs[bnd])),
        ('focal(2)+jaccard + boundary (all classes)', lambda: bnd_all.evaluate(logits, labels, out=bufs[bnd_all])),
        ('boundary alone (counts + bdn_boundary_loss)', lambda: alone.evaluate(logits, labels, out=bufs[alone]))]
res = median_us([f for _, f in rows])
for (name, _), (med, lo, hi) in zip(rows, res):
    say(f'    forward + gradient  {name:46s} median {med:8.1f} us (10 % {lo:8.1f}, 90 % {hi:8.1f})   x{med / res[0][0]:.2f} of focal+jaccard')
host_t = median_us([lambda: host_route(logits, labels)], reps=5, warm=1)[0]
say(f'    forward + gradient  {"boundary term: copy down, scipy, copy up, autograd":46s} median {host_t[0]:8.1f} us   the fused term alone takes '
      f'x{res[3][0] / host_t[0]:.4f} of it')
_lib.PROFILE = []
for _ in range(20):
    bnd.evaluate(logits, labels, out=bufs[bnd])
torch.cuda.synchronize()
per = {}
for name, _, _, e0, e1 in _lib.PROFILE:
    per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
_lib.PROFILE = None
for name, t in per.items():
    t.sort()
    say(f'    entry point  {name:28s} median {t[len(t) // 2]:8.1f} us')

# ---------------------------------------------------------------- (c) the train step
if int(os.environ.get('STEP', 1)):
    C = 13
    g = torch.Generator().manual_seed(0)
    x1 = torch.randn(B, C, H, W, generator=g)
    x2 = (x1 + 0.3 * torch.randn(B, C, H, W, generator=g)).to(dev)
    x1 = x1.to(dev)
    sd = {k: v.clone() for k, v in BiDateNet(C, 2).state_dict().items()}
    steps = {}
    for name, crit in (('focal(2)+jaccard', jac), ('focal(2)+jaccard+boundary', bnd)):
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
    base = med['focal(2)+jaccard']
    for name in steps:
        say(f'(c) bf16 TrainStep B={B} 13x{H}x{W}  {name:26s} median {med[name]:8.4f} ms  {(med[name] - base) * 1e3:+8.1f} us against focal+jaccard '
              f'({100 * (med[name] - base) / base:+.2f} %)   {[round(t, 4) for t in ms[name]]}')

out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'edt_bench.txt')
with open(out_path, 'w') as fh:
    fh.write('python tools/bench_edt.py\n' + '\n'.join(LINES) + '\n')
