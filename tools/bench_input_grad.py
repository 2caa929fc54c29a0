"""Input gradients and eval-mode backward, measured (input gradients).

    python tools/bench_input_grad.py kernel [--batch 64 --size 128 --channels 13]
        bdn_conv3x3_dgrad_first alone per storage form (bf16; float32 = fp32 / bf16x3 / bf16x3-fast), dz formed on load from dA and z:
        device-event time per launch and the TB/s of its HBM bytes (dA + z read, the two NCHW outputs written).  For the per-kernel
        time without events run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_input_grad.py kernel`.
    python tools/bench_input_grad.py step [--precision bf16]
        a training forward + backward through BiDateNet's autograd node with and without input gradients, interleaved, device events.
    python tools/bench_input_grad.py attr [--precision bf16]
        an eval-mode backward (recomputed forward + frozen-BatchNorm backward) on a frozen model with input gradients (attribution)
        against the same backward with every parameter gradient, interleaved, device events.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fabric_amd import BiDateNet, _lib                     # noqa: E402
from fabric_amd._lib import BDN_BF16, BDN_F32               # noqa: E402


def _time(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def kernel(a):
    B, H, W, cr, C = a.batch, a.size, a.size, a.channels, 64
    N = 2 * B
    for name, dt, td in (('bf16', BDN_BF16, torch.bfloat16), ('float32', BDN_F32, torch.float32)):
        dA = torch.randn(N, H, W, C, device='cuda').to(td)
        z = torch.randn(N, H, W, C, device='cuda').to(td)
        tab = torch.rand(2, 4, C, device='cuda') + 0.5
        sums = torch.randn(2, 2, C, device='cuda')
        w = torch.randn(C, cr, 3, 3, device='cuda') * 0.05
        dx1 = torch.empty(B, cr, H, W, device='cuda')
        dx2 = torch.empty_like(dx1)
        st = _lib.stream_ptr()

        def run():
            _lib.call('bdn_conv3x3_dgrad_first', dt, dA.data_ptr(), C, z.data_ptr(), tab.data_ptr(), sums.data_ptr(), B,
                      w.data_ptr(), cr, dx1.data_ptr(), dx2.data_ptr(), B, H, W, st)
        _time(run, a.warmup)
        ms = statistics.median(_time(run, a.iters))
        nbytes = 2 * dA.numel() * dA.element_size() + 2 * dx1.numel() * 4
        flops = 2.0 * N * H * W * C * 9 * 16
        print(json.dumps({'what': 'dgrad_first', 'storage': name, 'B': B, 'H': H, 'W': W, 'C_real': cr, 'us': round(ms * 1e3, 1),
                          'GB': round(nbytes / 1e9, 3), 'TB_per_s': round(nbytes / ms / 1e9, 2),
                          'TFLOP_per_s_padded': round(flops / ms / 1e9, 1)}), flush=True)
        del dA, z


def _setup(a, training):
    model = BiDateNet(a.channels, 2, precision=a.precision).cuda().train(training)
    g = torch.Generator(device='cuda').manual_seed(0)
    x1 = torch.randn(a.batch, a.channels, a.size, a.size, device='cuda', generator=g)
    x2 = torch.randn(a.batch, a.channels, a.size, a.size, device='cuda', generator=g)
    return model, x1, x2


def _interleaved(a, fns):
    out = {k: [] for k in fns}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    for _ in range(a.iters):
        for k, fn in fns.items():
            out[k] += _time(fn, 1)
    return {k: round(statistics.median(v), 3) for k, v in out.items()}


def step(a):
    model, x1, x2 = _setup(a, True)
    xg1, xg2 = x1.clone().requires_grad_(), x2.clone().requires_grad_()

    def plain():
        model(x1, x2).float().mean().backward()

    def with_dx():
        model(xg1, xg2).float().mean().backward()
    r = _interleaved(a, {'fwd_bwd_ms': plain, 'fwd_bwd_input_grad_ms': with_dx})
    print(json.dumps({'what': 'train_step_autograd', 'precision': a.precision, 'B': a.batch, 'size': a.size, **r,
                      'input_grad_cost_pct': round(100 * (r['fwd_bwd_input_grad_ms'] / r['fwd_bwd_ms'] - 1), 2)}), flush=True)


def attr(a):
    full, x1, x2 = _setup(a, False)
    frozen, _, _ = _setup(a, False)
    frozen.load_state_dict(full.state_dict())
    for p in frozen.parameters():
        p.requires_grad_(False)
    xg1 = x1.clone().requires_grad_()

    def frozen_bwd():
        frozen(xg1, x2).float().mean().backward()

    def full_bwd():
        full(xg1, x2).float().mean().backward()
    r = _interleaved(a, {'eval_attribution_frozen_ms': frozen_bwd, 'eval_backward_all_params_ms': full_bwd})
    print(json.dumps({'what': 'eval_backward', 'precision': a.precision, 'B': a.batch, 'size': a.size, **r}), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kernel', 'step', 'attr'])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--channels', type=int, default=13)
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'bf16x3', 'bf16x3-fast', 'fp32'])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    {'kernel': kernel, 'step': step, 'attr': attr}[a.what](a)
