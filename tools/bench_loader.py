"""Micro-benchmark (test infrastructure) of where training batches come from, at batch 64, 13 bands, 128 x 128, bf16, in one process:
  (1) resident: the fused TrainStep loop on one batch that already sits on the device (bench.py's headline loop);
  (2) host: make_loaders (numpy crop + augmentation, collate, pinning; --workers worker processes, default 2, at most 16) through
      DeviceFeeder into TrainStep;
  (3) device: make_device_loaders (bdn_sample_patches from HBM-resident cities) into TrainStep, timed between two resident runs as
      bench.py's host_fed_leg does;
  (4) sampler: bdn_sample_patches alone, back-to-back launches of planned batches between two HIP events, for random symmetries
      (augmentation on) and for the identity (off): us per batch, bytes moved and TB/s.
Every arm is warmed up first.  The synthetic cities (--cities x --size^2, stride 16) give several epochs of distinct origins.
    python tools/bench_loader.py [--steps 120] [--warmup 20] [--host-steps 40] [--workers 2] [--sampler-only]
Prints one JSON line at the end."""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.device_loader import plan_descriptors
from fabric_amd.input_pipeline import DeviceFeeder
from fabric_amd.train import make_device_loaders, make_loaders
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.dataloaders import synthetic_onera

B, C, S, STRIDE = 64, 13, 128, 16
COPY_RATE = 6.29                  # TB/s, the measured device copy rate of MI355X_MICROARCH.md


def resident(ts, x1, x2, lbl, n, warm=3):
    torch.cuda.synchronize()
    with torch.cuda.stream(ts.stream()):
        for _ in range(warm):
            ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def fed(ts, batches, n, warm):
    """ms per step of TrainStep over `warm` untimed + `n` timed batches of the iterable, on the step's stream."""
    torch.cuda.synchronize()
    with torch.cuda.stream(ts.stream()):
        it = iter(batches)
        for _ in range(warm):
            ts.step(*next(it))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ts.step(*next(it))
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def sampler_alone(loader, reps, batches=8):
    """us per bdn_sample_patches launch over `batches` planned batches of `loader`, launched `reps` times back to back."""
    dev = loader.device
    idx = list(loader.sampler)
    tables = [plan_descriptors(loader.dataset, idx[k * B:(k + 1) * B], loader.city_index) for k in range(batches)]
    pins = [torch.from_numpy(t).pin_memory() for t in tables]
    descs = [p.to(dev) for p in pins]
    o1 = torch.empty((B, C, S, S), device=dev)
    o2, ol = torch.empty_like(o1), torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()

    def launch(k):
        _lib.call('bdn_sample_patches', loader.city_table.data_ptr(), loader.city_hw.ctypes.data, len(loader.cities), C,
                  pins[k].data_ptr(), descs[k].data_ptr(), B, S, o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), st)

    for k in range(20):
        launch(k % batches)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        launch(k % batches)
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = 2 * (2 * B * C * S * S * 4 + B * S * S)            # images and labels, each read once and written once
    syms = np.concatenate(tables)[:, 3]
    return {'us_per_batch': us, 'bytes_per_batch': nbytes, 'TBps': nbytes / us / 1e6, 'syms_seen': sorted(set(syms.tolist())),
            'at_copy_rate_us': nbytes / COPY_RATE / 1e6, 'gate_4TBps': nbytes / us / 1e6 >= 4.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=120)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--host-steps', type=int, default=40)
    ap.add_argument('--workers', type=int, default=2)
    ap.add_argument('--cities', type=int, default=5)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--sampler-only', action='store_true', help='arm (4) alone (for a rocprofv3 --kernel-trace --stats run)')
    a = ap.parse_args()
    workers = max(0, min(16, a.workers))
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    data = synthetic_onera(n_cities=a.cities, bands=C, size=(a.size, a.size), seed=0)
    val = [f'city{a.cities - 1}']
    random.seed(0)
    d_tr, _ = make_device_loaders(data, val, S, STRIDE, B, True, seed=0, device=dev)
    d_id, _ = make_device_loaders(data, val, S, STRIDE, B, False, seed=0, device=dev)
    out = {'workload': f'BiDateNet(13,2) bf16, batch {B}, {S}x{S}, {a.cities - 1} training cities of {a.size}x{a.size}',
           'batches_per_epoch': len(d_tr), 'cpus': len(os.sched_getaffinity(0)), 'host_workers': workers}
    out['sampler_random_syms'] = sampler_alone(d_tr, a.reps)
    out['sampler_identity'] = sampler_alone(d_id, a.reps)
    if not a.sampler_only:
        torch.manual_seed(0)
        model = BiDateNet(C, 2, precision='bf16').to(dev)
        ts = TrainStep(model, lr=1e-3, tversky_alpha=0.1, tversky_beta=0.9)
        x1, x2, lbl = next(iter(d_tr))
        x1, x2, lbl = x1.clone(), x2.clone(), lbl.clone()
        torch.cuda.synchronize()
        res0 = resident(ts, x1, x2, lbl, a.steps, warm=a.warmup)
        h_tr, _ = make_loaders(data, val, S, STRIDE, B, True, num_workers=workers, seed=0)
        feeder = DeviceFeeder(dev)
        host_ms = fed(ts, feeder(h_tr), a.host_steps, min(a.warmup, 5))
        feeder.close()
        res_a = resident(ts, x1, x2, lbl, a.steps // 2)
        dev_ms = fed(ts, d_tr, a.steps, a.warmup)
        res_b = resident(ts, x1, x2, lbl, a.steps // 2)
        res = 0.5 * (res_a + res_b)
        out['resident'] = {'pairs_per_s': B / res * 1e3, 'ms_per_step': res, 'first_run_ms_per_step': res0}
        out['host_loader'] = {'pairs_per_s': B / host_ms * 1e3, 'ms_per_step': host_ms, 'steps': a.host_steps}
        out['device_loader'] = {'pairs_per_s': B / dev_ms * 1e3, 'ms_per_step': dev_ms, 'vs_resident': res / dev_ms}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
