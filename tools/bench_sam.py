"""Benchmark (test infrastructure) of sharpness-aware minimisation in the fused step, in one process on one card.

1. Kernels: bdn_sam_perturb (SAM and ASAM) and bdn_sam_restore on BiDateNet(13, 2)'s real per-tensor table (74 tensors, 13,401,156
   floats, one implicit group), beside bdn_grad_norm + bdn_sgd_step on the same n: --reps back-to-back calls between two HIP events after
   a warm-up, the arms interleaved and the whole interleaving repeated --rounds times (the spread between the rounds of one arm is the
   margin).  Per arm: us per call (median of the rounds), the bytes it moves per element, TB/s.
   Bytes per element (4-byte floats; the partial sums and the table are kilobytes):
     sam_perturb 20 (norm: g read; apply: p g read, saved p written)     asam_perturb 24 (the norm reads p too)
     sam_restore  8 (saved read, p written)                              grad_norm + sgd_step 16 (g read; p g read, p written)
2. The step: TrainStep on BiDateNet(13, 2, precision='bf16'), B = 64, 13x128x128 -- the flagship shapes -- plain, sam_rho=0.05 and
   sam_rho=0.5 with sam_adaptive, each its own model: --steps steps on the step's stream between two device synchronisations, the arms
   alternated, --rounds rounds.  The expectation is one more forward / backward, the two kernels and one more repack, so the table
   reports t_sam - 2 * t_plain per round, with its median and range.

    python tools/bench_sam.py [--reps 200] [--steps 30] [--rounds 5] [--out profiles/sam_bench.txt]
Prints the table and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd import optim as O
from fabric_amd.engine import param_order
from fabric_amd.parallel import FlatLayout
from fabric_amd.train_step import TrainStep


def bench_kernels(a, dev, lines):
    model = BiDateNet(13, 2)
    named = list(model.named_parameters())
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(13))
    n, n_ten = layout.total, len(layout.order)
    pg = O.ParamGroups(O.OptimConfig(), [k for k, _ in named], None, ())
    ends, lens, ids, _ = (t.to(dev) for t in O.tensor_table(layout, pg))
    g = torch.Generator(device='cpu').manual_seed(0)
    p = torch.randn(n, generator=g).to(dev)
    gr = (torch.randn(n, generator=g) * 1e-3).to(dev)
    saved = p.clone()
    lib = _lib.load()
    ws = torch.empty(lib.bdn_sam_workspace_bytes(n, n_ten) // 8, dtype=torch.float64, device=dev)
    nws = torch.empty(lib.bdn_grad_norm_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    out, nout = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    st = _lib.stream_ptr()

    def perturb(adaptive):
        _lib.call('bdn_sam_perturb', p.data_ptr(), saved.data_ptr(), gr.data_ptr(), ends.data_ptr(), lens.data_ptr(), ids.data_ptr(), n_ten,
                  0.05, adaptive, 1e-12, ws.data_ptr(), out.data_ptr(), n, st)

    def restore():
        _lib.call('bdn_sam_restore', p.data_ptr(), saved.data_ptr(), ends.data_ptr(), ids.data_ptr(), n_ten, n, st)

    def norm_sgd():
        _lib.call('bdn_grad_norm', gr.data_ptr(), None, None, 0, 1.0, float('inf'), nws.data_ptr(), nout.data_ptr(), n, st)
        _lib.call('bdn_sgd_step', p.data_ptr(), gr.data_ptr(), 1e-6, 1.0, n, st)

    cases = [('sam_perturb', 20, lambda: perturb(0)), ('asam_perturb', 24, lambda: perturb(1)), ('sam_restore', 8, restore),
             ('grad_norm+sgd_step', 16, norm_sgd)]
    res = {name: [] for name, _, _ in cases}
    for _ in range(a.rounds):
        for name, _, fn in cases:
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / a.reps * 1e3)
    rec = {}
    lines.append(f'SAM kernels on BiDateNet(13, 2): n = {n} floats, {n_ten} tensors; {a.reps} back-to-back calls, {a.rounds} rounds')
    for name, bpe, _ in cases:
        med = statistics.median(res[name])
        rec[name] = {'us': round(med, 2), 'bytes_per_element': bpe, 'TB_s': round(bpe * n / med * 1e-6, 2),
                     'rounds_us': [round(t, 2) for t in res[name]]}
        lines.append(f'{name:20s} median {med:8.2f} us  {bpe:2d} B/element  {bpe * n / med * 1e-6:5.2f} TB/s (effective)  {rec[name]["rounds_us"]}')
    both = rec['sam_perturb']['us'] + rec['sam_restore']['us']
    lines.append(f'sam_perturb + sam_restore: {both:.2f} us = x{both / rec["grad_norm+sgd_step"]["us"]:.2f} of grad_norm + sgd_step')
    return {'n': n, 'tensors': n_ten, 'kernels': rec}


def bench_step(a, dev, lines):
    B, C, S = 64, 13, 128
    g = torch.Generator(device='cpu').manual_seed(1)
    x1 = torch.randn(B, C, S, S, generator=g).to(dev)
    x2 = (x1.cpu() + 0.3 * torch.randn(B, C, S, S, generator=g)).to(dev)
    lbl = (torch.rand(B, S, S, generator=g) < 0.1).to(torch.uint8).to(dev)
    arms = {'plain': {}, 'sam': dict(sam_rho=0.05), 'asam': dict(sam_rho=0.5, sam_adaptive=True)}
    steps = {k: TrainStep(BiDateNet(C, 2, precision='bf16').to(dev).train(), lr=1e-3, tversky_alpha=0.1, tversky_beta=0.9, **kw)
             for k, kw in arms.items()}
    res = {k: [] for k in arms}

    def run(ts, n):
        with torch.cuda.stream(ts.stream()):
            for _ in range(n):
                ts.step(x1, x2, lbl)
        torch.cuda.synchronize()

    for ts in steps.values():
        run(ts, 5)                                             # every shape, code object and workspace the timed window uses
    for _ in range(a.rounds):
        for k, ts in steps.items():
            run(ts, 2)
            t0 = time.perf_counter()
            run(ts, a.steps)
            res[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    rec = {}
    lines.append(f'fused step, BiDateNet(13, 2) bf16, B = {B}, {C}x{S}x{S}: {a.steps} steps per window, {a.rounds} alternated rounds')
    for k in arms:
        rec[k] = {'ms': round(statistics.median(res[k]), 3), 'rounds_ms': [round(t, 3) for t in res[k]]}
        lines.append(f'{k:6s} median {rec[k]["ms"]:7.3f} ms / step  {rec[k]["rounds_ms"]}')
    for k in ('sam', 'asam'):
        d = [s - 2 * p for s, p in zip(res[k], res['plain'])]
        rec[f'{k}-2*plain'] = {'ms': round(statistics.median(d), 3), 'min_ms': round(min(d), 3), 'max_ms': round(max(d), 3),
                               'ratio': round(statistics.median(res[k]) / statistics.median(res['plain']), 3)}
        lines.append(f't_{k} - 2 * t_plain: median {statistics.median(d):+.3f} ms (range {min(d):+.3f} .. {max(d):+.3f} over the rounds); '
                     f't_{k} / t_plain = {rec[f"{k}-2*plain"]["ratio"]:.3f}')
    return {'step': rec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sam.py measures on the GPU: no device found')
    dev = torch.device('cuda', 0)
    lines = [torch.cuda.get_device_name(0)]
    out = bench_kernels(a, dev, lines)
    out.update(bench_step(a, dev, lines))
    print('\n'.join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
