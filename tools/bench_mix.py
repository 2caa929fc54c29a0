"""Micro-benchmark (test infrastructure) of cross-sample mixing through DevicePatchLoader at batch 64, 13 bands, 128 x 128: the augmenting
loader without `mix` beside the same loader with PatchMix at p in {0.25, 0.5, 1}, in both modes (and at p = 1e-9, where nobody is
mixed: the floor of the extra calls), in one process over the same synthetic
cities (make_device_loaders; crop jitter 8 + drawn symmetry + per-date gain / bias + erase, tools/bench_augment.py's policy without the noise).
Per arm and round, two measurements:
  wall    one pass of --batches batches through the loader, host clock around a pass that ends in a device synchronise: what a training
          loop that only loads would pay, the host's planning (Python) included.
  device  the launches of the batch the pass ended with, replayed back to back between two HIP events (tools/bench_warp.py's method):
          the cut of its n recipients alone, the cut of its n + m rows (m donors), and bdn_mix_patches on them.
Arms are interleaved over --rounds rounds.  The expectation to confirm or refute: a mixed batch costs the cut of n + m samples plus one
pass that touches only masked pixels.
    python tools/bench_mix.py [--batches 100] [--reps 200] [--rounds 3] [--out profiles/mix_bench.txt]
Prints a table (us per batch, medians over the rounds) and one JSON line; --out also writes both to a file."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fabric_amd import _lib
from fabric_amd.augment import MIX_MODES, PatchAugment, PatchMix
from fabric_amd.device_loader import device_stacks
from fabric_amd.train import make_device_loaders
from fabric_amd.utils.dataloaders import synthetic_onera

B, C, S, STRIDE = 64, 13, 128, 16
POLICY = PatchAugment(seed=1, jitter=8, symmetry=True, gain=0.1, bias=0.05, erase_p=0.5, erase_size=(16, 48), erase_label=255)
PS = (0.25, 0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=100)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--cities', type=int, default=5)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    data = device_stacks(synthetic_onera(n_cities=a.cities, bands=C, size=(a.size, a.size), seed=0), dev)      # one upload for all the arms

    def loader(mix=None):
        random.seed(0)
        return make_device_loaders(data, [f'city{a.cities - 1}'], S, STRIDE, B, False, seed=0, device=dev, augment=POLICY, mix=mix)[0]

    plain = loader()
    assert len(plain) >= a.batches, f'{len(plain)} batches per pass, --batches {a.batches}'
    pool = PatchMix(p=1.0, mode='object').donors_from(plain.label_counts(1), 1).donors      # object arms: donors with change at their grid position
    arms = [('aug (no mix)', plain), ('box p=1e-9', loader(PatchMix(p=1e-9, mode='box', box_size=(32, 96))))]      # 1e-9: nobody is mixed, the floor
    arms += [(f'box p={p}', loader(PatchMix(p=p, mode='box', box_size=(32, 96)))) for p in PS]
    arms += [(f'object p={p}', loader(PatchMix(p=p, mode='object', margin=2, donors=pool))) for p in PS]
    st = _lib.stream_ptr()

    def one_pass(ld):
        for k, _ in enumerate(ld):
            if k + 1 == a.batches:
                break

    def wall(ld):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_pass(ld)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.batches

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(10):
            call()
        e0.record()
        for _ in range(a.reps):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    def device(ld):
        """(cut of n rows, cut of n + m rows, mix, n + m) of the batch the loader issued last: its slot still holds the tables."""
        slot = ld.slots[(ld._k - 1) % ld.depth]
        rows = B + (int(slot.plan_np[:B, 0].sum()) if ld.mix is not None else 0)

        def cut(r):
            _lib.call('bdn_sample_patches_aug', ld.city_table.data_ptr(), _lib.host_int32(ld.city_hw), len(ld.cities), C,
                      _lib.host_int32(slot.desc_pin.data_ptr()), slot.desc_dev.data_ptr(), r, S, slot.d1.data_ptr(), slot.d2.data_ptr(),
                      slot.labels.data_ptr(), slot.keys_dev.data_ptr(), *POLICY.abi_args(), None, None, st)

        def mix():
            _lib.call('bdn_mix_patches', _lib.host_int32(slot.plan_pin.data_ptr()), slot.plan_dev.data_ptr(), B, rows, C, S,
                      MIX_MODES[ld.mix.mode], ld.mix.paste_label, ld.mix.margin, slot.d1.data_ptr(), slot.d2.data_ptr(),
                      slot.labels.data_ptr(), None, st)

        torch.cuda.synchronize()
        return timed(lambda: cut(B)), timed(lambda: cut(rows)), timed(mix) if ld.mix is not None else 0.0, rows

    for _, ld in arms:                                         # warm-up: code objects, clocks, the cities' first touch
        ld.set_epoch(0)
        one_pass(ld)
    torch.cuda.synchronize()
    rec = {name: {'wall': [], 'cut_n': [], 'cut': [], 'mix': [], 'rows': []} for name, _ in arms}
    for rnd in range(a.rounds):
        for name, ld in arms:
            ld.set_epoch(rnd + 1)
            rec[name]['wall'].append(wall(ld))
            for k, v in zip(('cut_n', 'cut', 'mix', 'rows'), device(ld)):
                rec[name][k].append(v)
    med = {name: {k: statistics.median(v) for k, v in r.items()} for name, r in rec.items()}
    lines = [f'DevicePatchLoader with and without PatchMix: B={B} C={C} S={S}; wall: {a.batches} batches per pass; device: {a.reps} back-to-back '
             f'launches of the last batch; {a.rounds} interleaved rounds, medians; {len(pool)} of {len(plain.dataset)} items in the object pool',
             f'{"arm":<15}{"wall us":>9}{"x aug":>7}{"pairs/s":>10} |{"rows":>6}{"cut(n)":>8}{"cut(rows)":>11}{"us/row":>8}{"mix":>7}{"cut+mix":>9}{"x cut(n)":>10}']
    res = {}
    for name, _ in arms:
        m = med[name]
        total = m['cut'] + m['mix']
        res[name] = {'wall_us': m['wall'], 'wall_ratio': m['wall'] / med['aug (no mix)']['wall'], 'wall_range': [min(rec[name]['wall']), max(rec[name]['wall'])],
                     'rows': m['rows'], 'cut_n_us': m['cut_n'], 'cut_rows_us': m['cut'], 'mix_us': m['mix'], 'mix_range': [min(rec[name]['mix']), max(rec[name]['mix'])],
                     'device_ratio': total / m['cut_n']}
        lines.append(f'{name:<15}{m["wall"]:>9.1f}{m["wall"] / med["aug (no mix)"]["wall"]:>7.2f}{B / m["wall"] * 1e6:>10.0f} |{m["rows"]:>6.0f}{m["cut_n"]:>8.1f}'
                     f'{m["cut"]:>11.1f}{m["cut"] / m["rows"]:>8.2f}{m["mix"]:>7.1f}{total:>9.1f}{total / m["cut_n"]:>10.2f}')
    text = '\n'.join(lines)
    print(text)
    js = json.dumps({'B': B, 'C': C, 'S': S, 'batches': a.batches, 'reps': a.reps, 'rounds': a.rounds, 'pool': len(pool), 'arms': res})
    print(js, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n' + js + '\n')


if __name__ == '__main__':
    main()
