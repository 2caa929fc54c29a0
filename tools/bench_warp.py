"""Micro-benchmark (test infrastructure) of bdn_sample_patches_warp beside bdn_sample_patches_aug with the same value stages and beside
bdn_sample_patches, at batch 64, 13 bands, 128 x 128: the same planned batches (make_device_loaders over synthetic cities, identity
symmetries in the descriptors), back-to-back launches between two HIP events, every arm warmed up, the arms interleaved over --rounds
rounds so that a drift of the clock hits all of them alike (tools/bench_augment.py's arrangement).
Arms:  plain            bdn_sample_patches
       aug geometry     bdn_sample_patches_aug: crop jitter 8 + drawn symmetry + erase (p = 0.5, 16..48 pixels)
       aug everything   ... and per-date per-band gain 0.1 / bias 0.05 and Gaussian noise, sigma 0.02
       warp identity    bdn_sample_patches_warp, geometry stages, an `off` warp policy (the gather at fx = fy = 0: its floor)
       warp rot+zoom    (a) geometry stages, rotation up to 30 degrees and a zoom in [0.8, 1.25]
       warp misreg      (b) geometry stages, misregistration up to 0.75 pixels only
       warp everything  (c) rotation, zoom, misregistration and every value stage including the noise
    python tools/bench_warp.py [--reps 200] [--rounds 3] [--out profiles/warp_bench.txt]
Prints a table (us per batch: median and range over the rounds, ratio to plain and to the aug arm with the same value stages) and one
JSON line; --out also writes both to a file."""
import argparse
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from fabric_amd import _lib
from fabric_amd.augment import PatchAugment, PatchWarp
from fabric_amd.device_loader import plan_descriptors, plan_keys
from fabric_amd.train import make_device_loaders
from fabric_amd.utils.dataloaders import synthetic_onera

B, C, S, STRIDE = 64, 13, 128, 16
GEO = dict(seed=1, jitter=8, symmetry=True, erase_p=0.5, erase_size=(16, 48), erase_label=255)
GEOMETRY, EVERYTHING = PatchAugment(**GEO), PatchAugment(gain=0.1, bias=0.05, noise_std=0.02, **GEO)
# (name, PatchAugment or None for the plain entry, PatchWarp or None for the aug entry, the aug arm it is compared with)
ARMS = [('plain', None, None, None),
        ('aug geometry', GEOMETRY, None, None),
        ('aug everything', EVERYTHING, None, None),
        ('warp identity', GEOMETRY, PatchWarp(), 'aug geometry'),
        ('warp rot+zoom', GEOMETRY, PatchWarp(rotate=30.0, scale=(0.8, 1.25), oob_label=255), 'aug geometry'),
        ('warp misreg', GEOMETRY, PatchWarp(misreg=0.75), 'aug geometry'),
        ('warp everything', EVERYTHING, PatchWarp(rotate=30.0, scale=(0.8, 1.25), misreg=0.75, oob_label=255), 'aug everything')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--cities', type=int, default=5)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    data = synthetic_onera(n_cities=a.cities, bands=C, size=(a.size, a.size), seed=0)
    random.seed(0)
    loader, _ = make_device_loaders(data, [f'city{a.cities - 1}'], S, STRIDE, B, False, seed=0, device=dev)
    idx = list(loader.sampler)
    tables = [plan_descriptors(loader.dataset, idx[k * B:(k + 1) * B], loader.city_index) for k in range(a.batches)]
    pins = [torch.from_numpy(t).pin_memory() for t in tables]
    descs = [p.to(dev) for p in pins]
    keys = [torch.from_numpy(plan_keys(idx[k * B:(k + 1) * B], 0).view(np.int64)).to(dev) for k in range(a.batches)]
    o1 = torch.empty((B, C, S, S), device=dev)
    o2, ol = torch.empty_like(o1), torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()
    hw = _lib.host_int32(loader.city_hw)

    def launch(pol, warp, k):
        if pol is None:
            _lib.call('bdn_sample_patches', loader.city_table.data_ptr(), loader.city_hw.ctypes.data, len(loader.cities), C,
                      pins[k].data_ptr(), descs[k].data_ptr(), B, S, o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), st)
            return
        args = (loader.city_table.data_ptr(), hw, len(loader.cities), C, _lib.host_int32(pins[k].data_ptr()), descs[k].data_ptr(), B, S,
                o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), keys[k].data_ptr(), *pol.abi_args(), None, None)
        if warp is None:
            _lib.call('bdn_sample_patches_aug', *args, st)
        else:
            _lib.call('bdn_sample_patches_warp', *args, *warp.abi_args(), None, None, None, st)

    def timed(pol, warp):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.reps):
            launch(pol, warp, k % a.batches)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    for _, pol, warp, _ in ARMS:                               # warm-up: code objects, clocks, the cities' first touch
        for k in range(20):
            launch(pol, warp, k % a.batches)
    torch.cuda.synchronize()
    us = {name: [] for name, _, _, _ in ARMS}
    for _ in range(a.rounds):
        for name, pol, warp, _ in ARMS:
            us[name].append(timed(pol, warp))
    out_bytes = 2 * B * C * S * S * 4 + B * S * S               # what every arm writes; the warp arms read four taps per element through the caches
    med = {name: statistics.median(v) for name, v in us.items()}
    lines = [f'bdn_sample_patches_warp vs bdn_sample_patches_aug vs bdn_sample_patches: B={B} C={C} S={S}, {a.reps} back-to-back launches x '
             f'{a.rounds} interleaved rounds, {out_bytes / 1e6:.1f} MB written per batch',
             f'{"arm":<17}{"us/batch (median)":>20}{"min":>10}{"max":>10}{"x plain":>10}{"x aug":>8}{"pairs/s":>12}']
    res = {}
    for name, _, _, ref in ARMS:
        m = med[name]
        res[name] = {'us_per_batch': m, 'min': min(us[name]), 'max': max(us[name]), 'ratio_to_plain': m / med['plain'],
                     'ratio_to_aug': m / med[ref] if ref else None, 'pairs_per_s': B / m * 1e6}
        lines.append(f'{name:<17}{m:>20.1f}{min(us[name]):>10.1f}{max(us[name]):>10.1f}{m / med["plain"]:>10.2f}'
                     f'{(f"{m / med[ref]:.2f}" if ref else "-"):>8}{B / m * 1e6:>12.0f}')
    text = '\n'.join(lines)
    print(text)
    js = json.dumps({'B': B, 'C': C, 'S': S, 'reps': a.reps, 'rounds': a.rounds, 'bytes_written_per_batch': out_bytes, 'arms': res})
    print(js, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n' + js + '\n')


if __name__ == '__main__':
    main()
