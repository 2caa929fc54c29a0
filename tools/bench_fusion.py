"""Micro-benchmark (test infrastructure) of the date-fusion modes, 'product' against 'absdiff', in ONE process:
  (a) the three training fusion kernels alone at the shapes of the B = 64, 13 x 128 x 128 step -- fusion + MaxPool2d(2) at encoder levels
      1-4 (and its bf16x3 split form at level 1), the plain fusion at level 5, the encoder-skip backward at all five levels (with dP below
      level 5, with bs_partial, as the engine calls it) -- HIP events over --reps back-to-back launches after a warm-up, the two modes
      alternating, the whole interleaving repeated --rounds times: median us per launch and TB/s of the bytes the kernel must move
      (computed from the shapes below; the same for both modes);
  (b) the bf16 B = 64 13 x 128 x 128 TrainStep step under both modes, interleaved like tools/bench_optim.py (--rounds rounds of 5 warm-up +
      --steps timed steps per mode): median ms and the difference.
    python tools/bench_fusion.py [--reps 100] [--rounds 5] [--steps 20] [--precision bf16] [--skip-step]
Prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd._lib import BDN_BF16, BDN_F32, FUSE_ABSDIFF, FUSE_PRODUCT
from fabric_amd.engine import ENC_CH
from fabric_amd.train_step import TrainStep

MODES = (('product', FUSE_PRODUCT), ('absdiff', FUSE_ABSDIFF))
HBM_PEAK = 8.0                     # TB/s, MI355X spec


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def kernels(reps, rounds, precision, B=64, S=128):
    dev = torch.device('cuda', 0)
    dt, td, es = (BDN_BF16, torch.bfloat16, 2) if precision == 'bf16' else (BDN_F32, torch.float32, 4)
    st = _lib.stream_ptr()
    g = torch.Generator(device='cpu').manual_seed(0)
    cases = []                     # (name, bytes, {mode: callable})
    keep = []
    for k in range(1, 6):
        H = W = S >> (k - 1)
        C = ENC_CH[k - 1]
        z = torch.randn(2 * B, H, W, C, generator=g).to(dev, td)
        bn = torch.empty(2, 4, C)
        bn[:, 0], bn[:, 1], bn[:, 2], bn[:, 3] = 0.0, 1.0, 1.0 + 0.1 * torch.randn(2, C, generator=g), 0.1 * torch.randn(2, C, generator=g)
        bn = bn.to(dev)
        f = torch.empty(B, H, W, C, dtype=td, device=dev)
        pool = torch.empty(2 * B, H // 2, W // 2, C, dtype=td, device=dev)
        dF = torch.randn(B, H, W, C, generator=g).to(dev, td)
        dP = torch.randn(2 * B, H // 2, W // 2, C, generator=g).to(dev, td) if k < 5 else None
        dA = torch.empty(2 * B, H, W, C, dtype=td, device=dev)
        rows = _lib.load().bdn_enc_skip_bwd_rows(dt, B, H, W, C)
        part = torch.empty(2, rows, 2, C, device=dev)
        keep += [z, bn, f, pool, dF, dP, dA, part]
        n = B * H * W * C * es
        if k < 5:
            cases.append((f'fuse_pool L{k} {H}x{W}x{C}', 2 * n + n + n // 2, {
                m: (lambda v=v, a=(z, bn, f, pool, B, H, W, C): _lib.call('bdn_fuse_dates_pool', dt, v, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                                                                          a[3].data_ptr(), *a[4:], st)) for m, v in MODES}))
        else:
            cases.append((f'fuse L{k} {H}x{W}x{C}', 3 * n, {
                m: (lambda v=v, a=(z, bn, f, B, H, W, C): _lib.call('bdn_fuse_dates', dt, v, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), *a[3:], st))
                for m, v in MODES}))
        cases.append((f'enc_skip_bwd L{k} {H}x{W}x{C}', 2 * n + n + (n // 2 if k < 5 else 0) + 2 * n, {
            m: (lambda v=v, a=(dF, z, bn, dP, dA, part, B, H, W, C): _lib.call('bdn_enc_skip_bwd_fusion', dt, v, a[0].data_ptr(), a[9], a[1].data_ptr(),
                                                                               a[2].data_ptr(), a[3].data_ptr() if a[3] is not None else None,
                                                                               a[4].data_ptr(), a[5].data_ptr(), *a[6:], st)) for m, v in MODES}))
        if k == 1:                 # bf16x3 form: float32 z, [hi | lo] bf16 outputs (skip inside the decoder's two-source operand)
            z32 = torch.randn(2 * B, H, W, C, generator=g).to(dev)
            Ct = C + 64
            fs = torch.empty(B, H, W, 2 * Ct, dtype=torch.bfloat16, device=dev)
            ps = torch.empty(2 * B, H // 2, W // 2, 2 * C, dtype=torch.bfloat16, device=dev)
            keep += [z32, fs, ps]
            n4 = B * H * W * C * 4
            cases.append((f'fuse_pool_split L1 {H}x{W}x{C}', 2 * n4 + n4 + n4 // 2, {
                m: (lambda v=v, a=(z32, bn, fs, ps, Ct, B, H, W, C): _lib.call('bdn_fuse_dates_pool_split', v, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                                                                               2 * a[4], a[4], a[3].data_ptr(), *a[5:], st)) for m, v in MODES}))
    out = {}
    for name, nbytes, fns in cases:
        t = {m: [] for m, _ in MODES}
        for m, _ in MODES:
            for _ in range(10):
                fns[m]()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for m, _ in MODES:
                t[m].append(_time(fns[m], reps))
        med = {m: statistics.median(t[m]) for m in t}
        out[name] = {'MB': round(nbytes / 1e6, 1),
                     **{m: {'us': round(med[m], 2), 'TB_s': round(nbytes / med[m] * 1e-6, 2), 'min_us': round(min(t[m]), 2), 'max_us': round(max(t[m]), 2)}
                        for m in med},
                     'absdiff_over_product': round(med['absdiff'] / med['product'], 4)}
        print(f'{name:34s} {nbytes / 1e6:7.1f} MB  ' + '  '.join(
            f'{m} {med[m]:8.1f} us {nbytes / med[m] * 1e-6:5.2f} TB/s [{min(t[m]):.1f}..{max(t[m]):.1f}]' for m in med) +
            f'  ratio {med["absdiff"] / med["product"]:.4f}', flush=True)
    return out


def steps(rounds, n_steps, precision, batch=64):
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    x1 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    x2 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    lbl = (torch.rand(batch, 128, 128, generator=g) < 0.1).to(torch.uint8).to(dev)
    ts = {}
    for m, _ in MODES:
        torch.manual_seed(0)
        ts[m] = TrainStep(BiDateNet(13, 2, precision=precision, fusion=m).to(dev).train(), lr=1e-4)
    res = {m: [] for m, _ in MODES}
    with torch.cuda.stream(ts['product'].stream()):            # every TrainStep shares the process's chain stream
        for _ in range(rounds):
            for m, _ in MODES:
                s = ts[m]
                for _ in range(5):
                    s.step(x1, x2, lbl)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_steps):
                    s.step(x1, x2, lbl)
                e1.record()
                torch.cuda.synchronize()
                res[m].append(e0.elapsed_time(e1) / n_steps)
    base = statistics.median(res['product'])
    out = {}
    for m, _ in MODES:
        med = statistics.median(res[m])
        out[m] = {'ms': round(med, 4), 'delta_us': round((med - base) * 1e3, 1), 'rounds_ms': [round(t, 4) for t in res[m]]}
        print(f'step {precision} B={batch} {m:8s} median {med:.4f} ms  ({(med - base) * 1e3:+7.1f} us vs product)  {out[m]["rounds_ms"]}', flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--skip-step', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fusion.py needs a ROCm device: there is no CPU path and no timing without one')
    out = {'device': torch.cuda.get_device_name(0), 'precision': a.precision, 'reps': a.reps, 'rounds': a.rounds,
           'kernels': kernels(a.reps, a.rounds, a.precision)}
    if not a.skip_step:
        out['step'] = steps(a.rounds, a.steps, a.precision)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
