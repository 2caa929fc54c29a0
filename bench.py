#!/usr/bin/env python
"""Headline benchmark: patch-pairs/s of one BiDateNet(13, 2) training step (forward + Tversky +
backward + gradient all-reduce + SGD) on synthetic 13-band 128x128 patch pairs, batch 64 per GPU
(BASELINE.json configs[1]; configs[2] = the same per-GPU work on N GPUs, weak scaling).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (contract in the task description).  `value` is measured with the inputs resident in HBM.
A plain run does only what that line's headline needs: set-up, warm-up, the timed steps, --dump-outputs, the line; the roofline
rides on the timed steps themselves (below).  Everything else it can measure runs only with --full:

    python bench.py --gpus 1 --steps 20 --warmup 5 --full

Extra objects on the same line:
  roofline       the dominant MFMA kernel of the step: algorithmic FLOP per launch / launch time measured with HIP events on
                 the launch stream inside the timed region (one launch bracketed per step, every launch shape weighted
                 equally), against the dense bf16 MFMA peak (2.5 PFLOP/s, MI355X_MICROARCH.md); HBM bytes per launch and
                 per step from the committed PMC passes (profiles/);
With --full only (the legs from collectives on: N = 1 and bf16, unless --no-extras):
  step_classes   where the step's time goes, per launch class and per queue, from one instrumented untimed step;
  cpu_baseline   the oracle's stock-torch assembly of the reference graph timed on the host cores (rank 0, N=1 only): median of 5
                 steps at B=16 and at B=4, at the fastest thread count;
  collectives    the same step with its five gradient-bucket all-reduces forced through RCCL (one rank), timed beside the local step
                 (with N > 1 or --force-collectives, in every run: the set-up guard's report on the headline loop's own all-reduces);
  mfma_ceiling   a bare MFMA loop on zero and on random bf16 operands: the data-dependent (power-bound) ceiling of the matrix cores;
  host_fed       the same step fed from pinned HOST memory through fabric_amd.input_pipeline.DeviceFeeder (PCIe inclusive);
  parity_setting pairs/s of the two float32-class settings (bf16x3: logits within 1e-3; fp32: exact f32 MFMA);
  val_f1         the second half of BASELINE.json's metric: tail training F1 and held-out validation F1 of a 60-step synthetic change-blob
                 run in the fp32, bf16x3 and bf16 settings, and |dF1| against fp32;
  conv3d         BASELINE configs[3] shapes: DoubleConv3d (3x3x3) forward + backward at 2 x 5 x 13 x 128 x 128 (parity unpinned);
  scene          BASELINE configs[4]: full-scene sliding-window inference of a 13-band 10000 x 10000 scene pair, resident in HBM and
                 (scene.host_fed) streamed from pinned host memory under the compute.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_PAIR_FWD_BWD = 69.43e9
FLOP_PER_PAIR_FWD = 23.144e9
MFMA_BF16_PEAK = 2.5e15                  # dense, MI355X_MICROARCH.md
MFMA_F32_PEAK = 157.3e12
HBM_PEAK = 8.0e12


def _cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def cpu_baseline(search_budget=30.0, confirm_budget=75.0):
    """Reference CPU path (oracle port) on the host cores: fwd + Tversky + bwd + SGD, fp32 (B=16 and B=4, median of
    >= 5 timed steps after warm-up).  Phase 1 searches the thread count with short runs at B=16 -- "all cores" is tried, but so are
    smaller counts: stock torch/oneDNN gets SLOWER past one thread per physical core on the big two-socket hosts (256 logical CPUs:
    0.17 pairs/s against 4.7 with 64 threads), and a baseline should be the reference's best configuration.  Phase 2 times the best
    count properly: 5 steps at B=16 (`value`) and 5 steps at B=4 (`b4`).  Every count tried is listed in `sample`."""
    from oracle import bidate_oracle as O
    from oracle import filler
    try:
        ncores = len(os.sched_getaffinity(0))
    except AttributeError:
        ncores = os.cpu_count() or 1
    net = O.build_torch_baseline(13, 2).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)

    def make(B):
        x1, x2, lbl = filler.make_inputs(B, 13, 128, seed=0)
        return torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(lbl).long()

    def step(batch):
        opt.zero_grad()
        loss = O.tversky_loss(net(batch[0], batch[1]), batch[2], 0.1, 0.9)
        loss.backward()
        opt.step()

    def timed(batch, n, budget, warmups=2):
        t_begin = time.perf_counter()
        for _ in range(warmups):                      # warm-up (oneDNN primitive creation for this thread count / shape); BASELINE.md section 3: two
            t_w = time.perf_counter()
            step(batch)
            warm = time.perf_counter() - t_w
        times = []
        while len(times) < n and (not times or time.perf_counter() - t_begin + times[-1] < budget):
            t0 = time.perf_counter()
            step(batch)
            times.append(time.perf_counter() - t0)
        times.sort()
        return (times[len(times) // 2] if times else warm), len(times)

    b16, b4 = make(16), make(4)
    tried, t_start = [], time.perf_counter()
    cands = []
    for th in (min(ncores, 64), max(1, ncores // 2), ncores, min(ncores, 32)):     # 64 first: one thread per core of one socket
        if th not in cands:
            cands.append(th)
    for th in cands:
        left = search_budget - (time.perf_counter() - t_start)
        done_ = [t for t in tried if t[1] is not None]
        # skip a count that cannot finish warm-up + 2 steps in what is left of the budget, or once adding threads made it slower
        if done_ and (left < 3.5 * done_[-1][1] or done_[-1][1] > 1.3 * min(t[1] for t in done_)):
            tried.append((th, None, 0))
            continue
        torch.set_num_threads(th)
        t, n = timed(b16, 2, max(left, 1.0), warmups=1)     # the search only ranks thread counts; the confirm runs below warm up twice
        tried.append((th, t, n))
    best_th = min((t for t in tried if t[1] is not None), key=lambda t: t[1])[0]
    torch.set_num_threads(best_th)
    t16, n16 = timed(b16, 5, confirm_budget * 0.75)
    t4, n4 = timed(b4, 5, confirm_budget * 0.25)
    # BASELINE configs[0] (the reference's own CPU-runnable case): BiDateNet(3, 2), 32 x 32 patches, batch 4
    net, opt = O.build_torch_baseline(3, 2).train(), None
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    x1, x2, lbl = filler.make_inputs(4, 3, 32, seed=0)
    c1 = (torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(lbl).long())
    torch.set_num_threads(min(best_th, 8))              # a 1.4 GFLOP step: more threads only add synchronisation
    tc1, nc1 = timed(c1, 5, 10.0)
    torch.set_num_threads(best_th)
    listing = ', '.join(f'{th} threads: ' + (f'{16 / t:.2f} pairs/s ({n} steps)' if t is not None else 'skipped (budget / already slower with fewer threads)') for th, t, n in tried)
    return {'value': 16 / t16, 'unit': 'patch-pairs/s', 'cores': best_th, 'kind': 'port',
            'b4': {'value': 4 / t4, 'unit': 'patch-pairs/s', 'timed_steps': n4, 'ms_per_step': t4 * 1e3},
            'config1': {'workload': 'BiDateNet(3,2) 32x32 patch pairs, batch 4 (BASELINE configs[0])', 'value': 4 / tc1, 'unit': 'patch-pairs/s',
                        'timed_steps': nc1, 'ms_per_step': tc1 * 1e3, 'cores': min(best_th, 8)},
            'timed_steps': n16, 'ms_per_step': t16 * 1e3,
            'sample': f'13x128x128 fwd+Tversky+bwd+SGD steps, fp32 stock torch.nn assembly of the reference graph (oracle.build_torch_baseline, '
                      f'pinned to the golden logits by tests/test_oracle_cpu.py): median of {n16} timed steps at B=16 (value) and of {n4} at B=4 (b4) '
                      f'after two warm-up steps each (BASELINE.md section 3), at the fastest thread count of a short search (one warm-up + up to 2 steps per count); host has {ncores} usable CPUs '
                      f'({_cpu_model()}); search at B=16: {listing}'}


# ---------------------------------------------------------------------------------------------- committed profile artefacts
def _latest(pattern):
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', pattern)))
    return files[-1] if files else None


def _kkey(kernel):
    return kernel.replace('bf16', 'unsigned short').replace(',', ', ')


def pmc_tables(precision):
    """(per-kernel dict, path) of the newest committed PMC summary (tools/pmc_traffic.sh: FETCH_SIZE and WRITE_SIZE collected in
    separate rocprofv3 --pmc passes of this same bench, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950)."""
    path = _latest('r*_pmc_traffic.json')
    if precision != 'bf16' or not path:
        return None, None
    return json.load(open(path)), path


def pmc_traffic(kernel, precision):
    tab, path = pmc_tables(precision)
    if not tab:
        return None
    rec = tab.get(_kkey(kernel))
    if not rec:       # template spellings differ between rocprofv3 versions: match on the name up to the argument list
        cand = [v for k, v in tab.items() if k.startswith(_kkey(kernel).split('<')[0]) and _kkey(kernel).rstrip('>') in k]
        rec = cand[0] if cand else None
    if not rec:
        return None
    return {'unit': 'bytes/launch', 'hbm_read': rec['fetch_bytes_per_launch_corrected'],
            'hbm_write': rec['write_bytes_per_launch'], 'source': os.path.relpath(path, ROOT),
            'correction': 'FETCH_SIZE x2 (gfx950 counts 128-B requests at 64 B), WRITE_SIZE as reported; separate --pmc passes'}


def pmc_step_bytes(precision):
    """HBM bytes of one whole training step: sum over every kernel of the committed PMC summary."""
    tab, path = pmc_tables(precision)
    if not tab or '_meta' not in tab:
        return None
    steps = tab['_meta']['steps']
    tot = sum((v['fetch_bytes_per_launch_corrected'] + v['write_bytes_per_launch']) * v['launches']
              for k, v in tab.items() if k != '_meta')
    return tot / steps, os.path.relpath(path, ROOT)


def rocprof_avg_us(kernel, precision):
    """Average duration of `kernel` in the newest committed rocprofv3 --kernel-trace --stats summary of this same command."""
    path = _latest('r*_kernel_stats.csv')
    if precision != 'bf16' or not path:
        return None, None
    key = 'void ' + _kkey(kernel)
    for r in csv.DictReader(open(path)):
        if r['Name'].startswith(key):
            return float(r['AverageNs']) / 1e3, os.path.relpath(path, ROOT)
    return None, os.path.relpath(path, ROOT)


def family_of(kernel):
    """Kernel FAMILY of an instantiation name: every conv3x3_kernel<...> instantiation is one kernel with different tile constants,
    wgrad7_kernel<true> / <false> one kernel with a bool (round-4 review: the dominant consumer must not hide behind a template split)."""
    return kernel.split('<')[0] + '<*>' if '<' in kernel else kernel


def rocprof_family_avg_us(names, precision):
    """Launch-weighted average duration over the instantiations `names` in the newest committed kernel-stats summary."""
    path = _latest('r*_kernel_stats.csv')
    if precision != 'bf16' or not path:
        return None, None
    keys = ['void ' + _kkey(n) for n in names]
    calls = tot = 0.0
    for r in csv.DictReader(open(path)):
        if any(r['Name'].startswith(k) for k in keys):
            calls += float(r['Calls']); tot += float(r['TotalDurationNs'])
    return (tot / calls / 1e3 if calls else None), os.path.relpath(path, ROOT)


def pmc_family_traffic(names, per_step_launches, precision):
    """HBM bytes per launch of a family: launch-weighted mean over its instantiations in the committed PMC summary."""
    tab, path = pmc_tables(precision)
    if not tab:
        return None
    rd = wr = n = 0.0
    for nm in names:
        tr = pmc_traffic(nm, precision)
        if tr is None:
            return None
        k = per_step_launches[nm]
        rd += tr['hbm_read'] * k; wr += tr['hbm_write'] * k; n += k
    return {'unit': 'bytes/launch', 'hbm_read': rd / n, 'hbm_write': wr / n, 'source': os.path.relpath(path, ROOT),
            'correction': 'FETCH_SIZE x2 (gfx950 counts 128-B requests at 64 B), WRITE_SIZE as reported; separate --pmc passes; '
                          'launch-weighted mean over the family\'s instantiations'}


def leg_profile(leg, conv_launches, flop_per_unit_fwd, note):
    """rocprof evidence of a leg that is NOT the bf16 training loop (tools/profile_legs.sh: profiles/<tag>_<leg>_kstats.csv from rocprofv3
    --kernel-trace --stats, <tag>_<leg>_pmc.json from separate --pmc passes): the conv3x3_kernel<*> family's launch-weighted average
    duration and HBM bytes per launch, and the MFMA fraction they give for `conv_launches` launches doing `flop_per_unit_fwd` FLOP -- so a
    reader can recompute the leg's fraction from tracked files.  None when no such file is committed."""
    ks = sorted(glob.glob(os.path.join(ROOT, 'profiles', f'r*_{leg}_kstats.csv')))
    if not ks:
        return None
    calls = tot = 0.0
    inst = {}
    for r in csv.DictReader(open(ks[-1])):
        if r['Name'].startswith('void conv3x3_kernel<'):
            calls += float(r['Calls']); tot += float(r['TotalDurationNs'])
            inst[r['Name'].replace('unsigned short', 'bf16').replace('void ', '').replace('(ConvArgs)', '')] = \
                {'calls': int(r['Calls']), 'avg_us': float(r['AverageNs']) / 1e3}
    if not calls:
        return None
    avg = tot / calls / 1e3
    out = {'kernel': 'conv3x3_kernel<*>', 'rocprof_source': os.path.relpath(ks[-1], ROOT), 'rocprof_avg_launch_us': avg, 'rocprof_launches': int(calls),
           'instantiations': inst, 'note': note}
    if conv_launches and flop_per_unit_fwd:
        out['launches_per_unit'] = conv_launches
        out['achieved'] = flop_per_unit_fwd / (avg * 1e-6 * conv_launches) / 1e12
        out['peak'] = MFMA_BF16_PEAK / 1e12
        out['unit'] = 'TFLOP/s'
        out['frac'] = out['achieved'] / out['peak']
    pm = sorted(glob.glob(os.path.join(ROOT, 'profiles', f'r*_{leg}_pmc.json')))
    if pm:
        rd = wr = n = 0.0
        for k, v in json.load(open(pm[-1])).items():
            if k.startswith('conv3x3_kernel<') or k.startswith('void conv3x3_kernel<'):
                n += v['launches']; rd += v['fetch_bytes_per_launch_corrected'] * v['launches']; wr += v['write_bytes_per_launch'] * v['launches']
        if n:
            out['traffic'] = {'unit': 'bytes/launch', 'hbm_read': rd / n, 'hbm_write': wr / n, 'source': os.path.relpath(pm[-1], ROOT),
                              'correction': 'FETCH_SIZE x2 (gfx950), WRITE_SIZE as reported; separate --pmc passes; launch-weighted over the family'}
    return out


def mfma_ceiling():
    """tools/probe_power_wall (built by __graft_entry__.build()): a bare v_mfma_f32_32x32x16_bf16 loop on every CU with all-zero and with
    N(0,1) bf16 operands.  The chip clocks to its power budget, so the rate on random data -- not the data-sheet 2.5 PFLOP/s -- is what
    any kernel can reach on real activations.  Returns None when the probe binary is absent."""
    import subprocess
    exe = os.path.join(ROOT, 'tools', 'probe_power_wall')
    if not os.path.exists(exe):
        return None
    try:
        txt = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
        rows = {}
        for line in txt.splitlines():
            if 'TFLOP/s' in line:
                name = line[:48].strip()
                rows[name] = float(line.split('ms')[1].split('TFLOP/s')[0])
        rnd = rows.get('N(0,1) random')
        return {'unit': 'TFLOP/s', 'zero_operands': rows.get('all zero'), 'random_operands': rnd,
                'random_operands_srcB_shared_by_4': rows.get('N(0,1) random, srcB shared by 4 MFMAs (1x4 tile)'),
                'frac_of_nominal_peak': None if rnd is None else rnd / (MFMA_BF16_PEAK / 1e12),
                'how': 'bare v_mfma_f32_32x32x16_bf16 loop, one wave per SIMD on every CU, operands in registers, each row after three whole '
                       'warm-up launches (tools/probe_power_wall.hip): the chip clocks to its power budget; random_operands = both source '
                       'registers change every MFMA, random_operands_srcB_shared_by_4 = the order of the convolutions\' 1x4 wave tile (the '
                       'order moves the ceiling by 0...3 % only; rounds 3-4 quoted 1.53-1.61 PFLOP/s here from inside the clock ramp that '
                       'follows the host-side data fill: profiles/r5_operand_reuse.txt)'}
    except Exception as e:
        return {'error': f'{type(e).__name__}: {e}'}


# ---------------------------------------------------------------------------------------------- where the step's time goes
_CLASS_OF = {'bdn_conv3x3_dgrad_bs': 'conv_dgrad', 'bdn_conv3x3_dgrad_bb': 'conv_dgrad', 'bdn_conv3x3_wgrad_ex': 'wgrad', 'bdn_conv3x3_wgrad_bnbwd': 'wgrad',
             'bdn_bn_finalize': 'finalize', 'bdn_bn_bwd_finalize': 'finalize'}


def step_classes(ts, x1, x2, lbl, B, dev):
    """ONE instrumented, untimed step: every library call that takes a stream is bracketed by an event pair on that stream
    (fabric_amd/_lib.py PROFILE), then summed per class and per queue.  Every pair is a small bubble and the two queues crowd into
    each other's bubbles, so the sums run a few percent above an unprofiled step -- they say where a change landed, the headline says
    how much it is worth.  conv_* and wgrad carry the algorithmic FLOP of their class, hbm_bound the committed PMC bytes."""
    from fabric_amd import _lib, streams
    torch.cuda.synchronize()
    _lib.PROFILE = []
    try:
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        raw = _lib.PROFILE
    finally:
        _lib.PROFILE = None
    chain, side = ts.stream().cuda_stream, streams.get('wgrad', dev).cuda_stream
    cls, queues = {}, {'q0_chain': 0.0, 'q1_wgrad': 0.0, 'other': 0.0}
    for name, phase, h, e0, e1 in raw:
        c = _CLASS_OF.get(name) or (('conv_fwd' if phase == 'fwd' else 'conv_dgrad') if name in ('bdn_conv3x3', 'bdn_conv3x3_x3src') else 'hbm_bound')
        ms = e0.elapsed_time(e1)
        a = cls.setdefault(c, {'ms': 0.0, 'calls': 0})
        a['ms'] += ms; a['calls'] += 1
        queues['q0_chain' if h == chain else 'q1_wgrad' if h == side else 'other'] += ms
    flop = {'conv_fwd': FLOP_PER_PAIR_FWD * B, 'conv_dgrad': (FLOP_PER_PAIR_FWD - 0.491e9) * B, 'wgrad': FLOP_PER_PAIR_FWD * B}
    for c, f in flop.items():
        if c in cls and cls[c]['ms'] > 0:
            cls[c]['TFLOPs'] = f / cls[c]['ms'] / 1e9
    tab, path = pmc_tables('bf16')
    if tab and 'hbm_bound' in cls:
        steps = tab['_meta']['steps']
        nb = sum((v['fetch_bytes_per_launch_corrected'] + v['write_bytes_per_launch']) * v['launches'] for k, v in tab.items()
                 if k != '_meta' and not k.startswith(('conv3x3', 'wgrad7', 'wgrad_kernel', 'wgrad_first', 'reduce_rows', 'bn_finalize', 'bn_bwd_finalize'))) / steps
        cls['hbm_bound']['TBps'] = nb / cls['hbm_bound']['ms'] / 1e9
        cls['hbm_bound']['bytes_source'] = os.path.relpath(path, ROOT)
    for a in cls.values():
        a['ms'] = round(a['ms'], 4)
    return {'per_class': cls, 'queue_busy_ms': {k: round(v, 4) for k, v in queues.items() if v},
            'how': 'one instrumented untimed step, an event pair around every library call on its own stream; wgrad = GEMM + its split-K '
                   'reduction; finalize = the separately launched BatchNorm (backward) finalize calls; hbm_bound = everything else'}


# ---------------------------------------------------------------------------------------------- extra legs (rank 0, N = 1)
def _time_steps(ts, x1, x2, lbl, warm, n):
    # on the step's own stream, as the headline loop and fabric_amd/train.py run it (no cross-stream joins around every step)
    torch.cuda.synchronize()
    with torch.cuda.stream(ts.stream()):
        for _ in range(warm):
            ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n


def host_fed_leg(ts, dev, B, C, S, steps, warmup, x1, x2, lbl):
    """The step fed from pinned host memory: float32 NCHW pairs + uint8 labels cross PCIe every step on a copy stream, under the
    previous steps (fabric_amd/input_pipeline.py; reference train.py:83-85 copies on the compute stream).  Compared with the
    resident loop measured immediately before and after it in the same process state (the step has two stable speeds per
    process, DESIGN.md section 6, so the headline run minutes earlier is not the right denominator)."""
    from fabric_amd.input_pipeline import DeviceFeeder
    g = torch.Generator(device='cpu').manual_seed(7)
    pool = []
    for _ in range(3):
        h1 = torch.randn(B, C, S, S, generator=g)
        pool.append((h1.pin_memory(), (h1 + 0.3 * torch.randn(B, C, S, S, generator=g)).pin_memory(),
                     (torch.rand(B, S, S, generator=g) < 0.1).to(torch.uint8).pin_memory()))
    feeder = DeviceFeeder(dev)

    def batches(n):
        for i in range(n):
            yield pool[i % len(pool)]

    def fed(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in feeder(batches(n)):
            ts.step(*b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    fed(max(warmup, 80))                                   # slot allocation, first copies -- and the copy path's own warm-up: the first
                                                           # ~80 host-fed steps of a process run 4 % slower than the steady state that follows
    res_a = _time_steps(ts, x1, x2, lbl, 2, max(steps // 2, 10)) * 1e3
    ms = fed(steps)
    res_b = _time_steps(ts, x1, x2, lbl, 2, max(steps // 2, 10)) * 1e3
    res = 0.5 * (res_a + res_b)
    nbytes = sum(t.numel() * t.element_size() for t in pool[0])
    return {'value': B / ms * 1e3, 'unit': 'patch-pairs/s', 'ms_per_step': ms, 'resident_ms_per_step_adjacent': res,
            'vs_resident': res / ms, 'host_bytes_per_step': nbytes, 'pcie_GBps_sustained': nbytes / ms / 1e6,
            'how': 'pinned host batches -> DeviceFeeder (copy stream, 3 device slots, event hand-off) -> TrainStep; '
                   'PCIe-inclusive, never the headline value; vs_resident = resident loop timed right before and after / fed loop'}


def collectives_leg(ts, model, dev, x1, x2, lbl, steps):
    """The step with its five gradient-bucket all-reduces really issued through RCCL -- process group 'nccl' with ONE rank, the
    buckets forced (TrainStep(force_collectives=True)) -- on the stream arrangement an 8-GPU run uses: launched from the
    weight-gradient stream behind the GEMM that completes a bucket, the last one from the chain's stream.  With one rank RCCL has
    nothing to exchange, so this prices the launches, the stream hand-offs and RCCL's own kernels beside two busy queues, not the
    xGMI transfer (53.6 MB per step; DESIGN.md section 5 prices that from the link rate).  Timed against the local step right
    before and after it in the same process."""
    from fabric_amd.parallel import init_rccl
    from fabric_amd.train_step import TrainStep
    own_group = False
    try:
        if not dist.is_initialized():
            os.environ.setdefault('MASTER_PORT', str(29000 + os.getpid() % 3000))
            init_rccl(0, 1, dev)
            own_group = True
        forced = TrainStep(model, lr=1e-3, tversky_alpha=0.1, tversky_beta=0.9, force_collectives=True)
        n = max(steps // 2, 10)
        a = _time_steps(ts, x1, x2, lbl, 3, n) * 1e3
        f = _time_steps(forced, x1, x2, lbl, 5, n) * 1e3
        b = _time_steps(ts, x1, x2, lbl, 3, n) * 1e3
        local = 0.5 * (a + b)
        sizes = [(hi - lo) * 4 for lo, hi, _ in forced.bucketer.buckets]
        out = {'ms_per_step': f, 'local_ms_per_step_adjacent': local, 'overhead_frac': f / local - 1.0,
               'buckets': len(sizes), 'bucket_bytes': sizes, 'backend': 'nccl (RCCL), world size 1, all-reduces forced',
               'guard': forced.collectives_report,
               'what_it_prices': 'launch + stream ordering + RCCL kernels beside the two busy queues; NOT the xGMI transfer'}
        del forced
        return out
    except Exception as e:                                    # a bench line without this leg beats no bench line
        return {'error': f'{type(e).__name__}: {e}'}
    finally:
        if own_group:
            dist.destroy_process_group()


def parity_leg(dev, B, C, S):
    """The float32-class settings at the benchmark shape: pairs/s, and how far bf16x3 / bf16 logits sit from the exact-f32
    setting on the same weights and inputs (the f32 setting itself is pinned to the reference within 3e-5 by tests/)."""
    from fabric_amd import BiDateNet
    from fabric_amd.train_step import TrainStep
    g = torch.Generator(device='cpu').manual_seed(11)
    x1 = torch.randn(B, C, S, S, generator=g)
    x2 = (x1 + 0.3 * torch.randn(B, C, S, S, generator=g)).to(dev)
    x1 = x1.to(dev)
    lbl = (torch.rand(B, S, S, generator=g) < 0.1).to(torch.uint8).to(dev)
    torch.manual_seed(4321)
    sd = {k: v.clone() for k, v in BiDateNet(C, 2).state_dict().items()}
    out, logits = {}, {}
    for prec, warm, n in (('fp32', 2, 4), ('bf16x3', 5, 15), ('bf16', 2, 6)):
        m = BiDateNet(C, 2, precision=prec)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        with torch.no_grad():
            logits[prec] = m(x1[:8], x2[:8]).float().clone()
        if prec != 'bf16':
            ts = TrainStep(m, lr=1e-3)
            ms = _time_steps(ts, x1, x2, lbl, warm, n) * 1e3
            out[prec] = {'pairs_per_s': B / ms * 1e3, 'ms_per_step': ms}
            if prec == 'bf16x3':                                   # the same forward with two-term backward GEMMs: precision='bf16x3-fast'
                m.engine().x3_bwd_terms = 2
                ms2 = _time_steps(ts, x1, x2, lbl, 3, n) * 1e3
                out['bf16x3_fast'] = {'pairs_per_s': B / ms2 * 1e3, 'ms_per_step': ms2}
                out[prec]['three_term_backward'] = dict(out[prec])   # (the same numbers under the key round 5's line used)
            del ts
        del m
        torch.cuda.empty_cache()
    for prec in ('bf16x3', 'bf16'):
        out.setdefault(prec, {})['max_abs_dlogit_vs_fp32_setting'] = float((logits[prec] - logits['fp32']).abs().max())
    out['bf16x3_fast']['max_abs_dlogit_vs_fp32_setting'] = out['bf16x3']['max_abs_dlogit_vs_fp32_setting']      # the same forward
    out['tolerance'] = 'north_star: logits within 1e-3 of the reference; tests/test_gpu_model.py holds fp32 and bf16x3 to it on the golden vectors'
    out['bf16x3']['how'] = ('float32 tensors; GEMM operands split into bf16 hi + lo on the bf16 MFMA kernels, the split product fused into one reduction '
                            '(csrc/conv3x3.hip X3, csrc/x3.hip): three terms (a_hi*w_hi + a_lo*w_hi + a_hi*w_lo) in the forward AND in both backward GEMMs '
                            '-- the parity setting')
    out['bf16x3_fast']['how'] = ("precision='bf16x3-fast': the bf16x3 forward (the logits the 1e-3 bar is about) with TWO-term backward GEMMs (filter rounded to "
                                 'bf16 in the data gradient, dz in the weight gradient): gradients 2-5e-3 relative L2 from the three-term backward, '
                                 '1 - cosine <= 1.3e-5; an explicit opt-in, never the parity headline')
    out['fp32']['how'] = 'float32 tensors; v_mfma_f32_32x32x2_f32 (1/16 of the bf16 matrix rate)'
    return out


def scene_leg(dev, size=10000, batch=256, reps=2, band_rows=None):
    """BASELINE.json configs[4]: forward-only sliding-window inference of a 13-band size x size scene pair (6241 tiles at 10000:
    reference train.py:182-205 / utils/inference.py:134-236), scene planes resident in HBM as float32.  Tiles per forward batch: 256
    (the loop's `batch_size` is a free parameter of the reference; 64 -> 256 amortises the per-batch fixed cost: 32.9k -> 35.7k tiles/s)."""
    from fabric_amd import BiDateNet
    from fabric_amd.utils import inference as inf
    torch.manual_seed(0)
    model = BiDateNet(13, 2, precision='bf16').to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(3)
    d1 = torch.randn(13, size, size, device=dev, generator=g)
    d2 = d1 + 0.3 * torch.randn(13, size, size, device=dev, generator=g)
    n = len(inf.tile_origins(size, size, 128)[0])
    inf.predict_scene(model, d1, d2, 128, batch)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t = time.perf_counter()
        mask = inf.predict_scene(model, d1, d2, 128, batch)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    flops = n * FLOP_PER_PAIR_FWD
    act_bytes = n * 45.9e6 + 2 * 13 * size * size * 4           # ideal conv activation traffic + one read of the scene
    out = {'workload': f'13-band {size}x{size} scene pair, 128-px tiles, batch {batch}, forward only, bf16 (BASELINE configs[4])',
           'tiles': n, 'seconds': best, 'tiles_per_s': n / best, 'mpix_per_s': size * size / best / 1e6,
           'changed_fraction': float(mask.float().mean()),
           'roofline': {'bound': 'mfma', 'achieved': flops / best / 1e12, 'peak': MFMA_BF16_PEAK / 1e12, 'unit': 'TFLOP/s',
                        'frac': flops / best / MFMA_BF16_PEAK,
                        'note': 'BASELINE calls the regime HBM-bound; with the scene resident and tiles gathered on the device the forward '
                                'convolutions bound it (144 TFLOP vs 0.3 TB of ideal activation traffic)'},
           'hbm_algorithmic': {'bytes': act_bytes, 'GBps': act_bytes / best / 1e9, 'frac_of_peak': act_bytes / best / HBM_PEAK}}
    # the same scene fed from pinned HOST memory (the regime SURVEY n1 names: host -> device staging as long as the compute): the planes
    # go up in 256-row bands on the copy stream while tiles of the bands that have arrived run (fabric_amd/utils/inference.py)
    try:
        h1 = torch.empty(13, size, size, dtype=torch.float32, pin_memory=True)
        h2 = torch.empty(13, size, size, dtype=torch.float32, pin_memory=True)
        h1.copy_(d1); h2.copy_(d2)
        torch.cuda.synchronize()
        del d1, d2
        torch.cuda.empty_cache()
        nbytes = 2 * h1.numel() * 4
        tmp = torch.empty_like(h1, device=dev)                # a plain upload of one date into an existing buffer: the PCIe rate of this box
        tmp.copy_(h1, non_blocking=True); torch.cuda.synchronize()
        t = time.perf_counter()
        tmp.copy_(h1, non_blocking=True); torch.cuda.synchronize()
        pcie = h1.numel() * 4 / (time.perf_counter() - t)
        del tmp
        torch.cuda.empty_cache()
        inf.predict_scene(model, h1, h2, 128, batch, band_rows=band_rows)
        torch.cuda.synchronize()
        fed = 1e9
        for _ in range(reps):
            t = time.perf_counter()
            mask_h = inf.predict_scene(model, h1, h2, 128, batch, band_rows=band_rows)
            torch.cuda.synchronize()
            fed = min(fed, time.perf_counter() - t)
        bound = max(best, nbytes / pcie)
        out['host_fed'] = {'seconds': fed, 'tiles_per_s': n / fed, 'host_bytes': nbytes, 'pcie_GBps_plain_copy': pcie / 1e9,
                           'pcie_GBps_sustained': nbytes / fed / 1e9, 'bound_seconds': bound, 'frac_of_bound': bound / fed,
                           'mask_equals_resident': bool(torch.equal(mask_h, mask)),
                           'how': 'pinned [13,H,W] float32 host planes -> 256-row bands on the copy stream, one event per band, tile batches wait '
                                  'only for the last band they read; bound = max(resident compute time, bytes / plain-copy PCIe rate)'}
        del h1, h2
    except Exception as e:                                    # e.g. not enough pinnable host memory on the box
        out['host_fed'] = {'error': f'{type(e).__name__}: {e}'}
    del model
    torch.cuda.empty_cache()
    return out


def val_f1_leg(dev, steps=60, B=8, S=128, lr=0.02):
    """The other half of BASELINE.json's metric ("...; val F1"): does the benchmarked bf16 setting reach the same F1 as the float32 one?
    Synthetic OSCD-shaped scenes with change blobs (fabric_amd.utils.dataloaders.synthetic_onera: four 13-band 300 x 300 cities), `steps`
    fused train steps at batch `B` from identical random-init weights in each numerics setting on cities 0-2; reported per setting: the
    training loss / per-batch F1 averaged over the last 10 steps, and the VALIDATION F1 on the held-out city 3 with the reference's
    definitions (eval-mode forward, train.py:125-172; per-batch sklearn-style binary P/R/F1, utils/helpers.py:45-59 mean over batches)."""
    import numpy as np
    from fabric_amd import BiDateNet
    from fabric_amd.train import validate
    from fabric_amd.train_step import TrainStep
    from fabric_amd.utils.dataloaders import OneraPreloader, metadata_from_shapes, patch_origins, synthetic_onera
    from fabric_amd.utils.metrics import TverskyLoss, batch_prf_from_counts
    data = synthetic_onera(n_cities=4, bands=13, size=(300, 300), seed=5, change_fraction=0.15)
    cities = sorted(data)
    items = [(c, i, j) for c in cities[:3] for i, j in patch_origins(300, 300, S, 43)]
    order = np.random.default_rng(9).permutation(len(items))
    batches = []
    for st in range(steps):
        pick = [items[order[(st * B + k) % len(items)]] for k in range(B)]
        x = np.stack([data[c]['images'][:, :, i:i + S, j:j + S] for c, i, j in pick])
        y = np.stack([data[c]['labels'][i:i + S, j:j + S] for c, i, j in pick])
        batches.append((torch.from_numpy(x[:, 0].copy()).to(dev), torch.from_numpy(x[:, 1].copy()).to(dev), torch.from_numpy(y.copy()).to(dev)))
    val_meta = [[cities[3], i, j] for i, j in patch_origins(300, 300, S, 43)]
    val_ds = OneraPreloader('', val_meta, data, S, False)
    val_loader = torch.utils.data.DataLoader(val_ds, batch_size=B, shuffle=False)
    torch.manual_seed(1234)
    sd0 = {k: v.clone() for k, v in BiDateNet(13, 2).state_dict().items()}
    out = {}
    for prec in ('fp32', 'bf16x3', 'bf16x3-fast', 'bf16'):
        m = BiDateNet(13, 2, precision=prec)
        m.load_state_dict(sd0)
        m = m.to(dev).train()
        ts = TrainStep(m, lr=lr, tversky_alpha=0.1, tversky_beta=0.9)
        recs = []
        for x1, x2, y in batches:
            loss = ts.step(x1, x2, y)
            recs.append((loss, ts.last_counts.clone()))
        losses = [float(l.item()) for l, _ in recs]
        f1s = [batch_prf_from_counts(c.cpu())[2] for _, c in recs]
        v = validate(m, val_loader, dev, S, TverskyLoss(alpha=0.1, beta=0.9))
        out[prec] = {'first_loss': losses[0], 'tail_loss': float(np.mean(losses[-10:])), 'tail_train_f1': float(np.mean(f1s[-10:])),
                     'val_f1': float(v['cd_f1scores']), 'val_precision': float(v['cd_precisions']), 'val_recall': float(v['cd_recalls']),
                     'val_loss': float(v['cd_losses'])}
        del ts, m
        torch.cuda.empty_cache()
    for prec in ('bf16x3', 'bf16x3-fast', 'bf16'):
        out[prec]['abs_dF1_vs_fp32'] = {'val': abs(out[prec]['val_f1'] - out['fp32']['val_f1']),
                                        'tail_train': abs(out[prec]['tail_train_f1'] - out['fp32']['tail_train_f1'])}
    out['workload'] = (f'{steps} fused train steps, batch {B}, 13-band {S}x{S} patches cut from 3 synthetic change-blob cities (lr {lr}, Tversky 0.1/0.9), '
                       f'then eval-mode validation on {len(val_ds)} patches of a held-out city; identical init and batch order in every setting')
    out['definition'] = 'val_f1 = mean over validation batches of the binary F1 of argmax(logits) (reference train.py:150-160, utils/helpers.py:45-59)'
    out['data'] = 'synthetic (no OSCD download in this environment): F1 parity BETWEEN numerics settings, not an OSCD score'
    return out


def conv3d_leg(dev, samples=(2, 16), D=5, S=128, cin=13, cout=64, iters=5):
    """BASELINE.json configs[3] (multi-date stack, 5 dates x 13 bands x 128 x 128) as far as a reference exists for it -- it does not
    (UNetLSTM/ is an empty sub-module), so PARITY IS UNPINNED: the 3x3x3 convolution of the two full-resolution layers a 3-D U-Net with
    BiDateNet's widths starts with (13 -> 64 and 64 -> 64; tests/test_gpu_conv3d.py checks them against torch.nn.functional.conv3d /
    torch.nn.grad) -- forward, data gradient and weight gradient timed SEPARATELY, at the config's own 2 samples (10 slices = 640 blocks:
    1.25 rounds of the chip) and at 16 samples (80 slices: a chip-filling batch), plus the whole DoubleConv3d block forward + backward."""
    from fabric_amd.conv3d import Conv3d3x3, DoubleConv3d

    def timeit(fn):
        fn(); fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    out = {'workload': f'3x3x3 convolution {cin}->{cout} and {cout}->{cout} on {D} dates x {S} x {S}, bf16 (BASELINE configs[3] shapes), per direction',
           'parity': 'unpinned: the reference holds no 3-D model source; operator and block checked against torch.nn in tests/test_gpu_conv3d.py'}
    peak = MFMA_BF16_PEAK / 1e12
    for N in samples:
        for ci, co in ((cin, cout), (cout, cout)):
            g = torch.Generator(device='cpu').manual_seed(ci)
            w = (0.05 * torch.randn(co, ci, 3, 3, 3, generator=g)).to(dev)
            op = Conv3d3x3(w, torch.zeros(co, device=dev))
            cp = op.cp
            x = torch.zeros(N, D, S, S, cp, dtype=torch.bfloat16, device=dev)
            x[..., :ci] = torch.randn(N, D, S, S, ci, generator=g).to(dev).to(torch.bfloat16)
            dy = torch.randn(N, D, S, S, co, generator=g).to(dev).to(torch.bfloat16)
            fl = 2.0 * N * D * S * S * 27 * co * ci          # algorithmic FLOP of one direction (real input channels)
            rec = {'GFLOP_per_direction': fl / 1e9, 'slices': N * D}
            for what, fn in (('fwd', lambda: op.forward(x)), ('dgrad', (lambda: op.dgrad(dy)) if op.wd is not None else None),
                             ('wgrad', lambda: op.wgrad(dy, x))):
                if fn is None:
                    rec[what] = None                              # a 13-band first layer has no data gradient
                    continue
                ms = timeit(fn)
                rec[what] = {'ms': ms, 'TFLOPs': fl / ms / 1e9, 'frac_of_mfma_peak': fl / ms / 1e9 / peak}
            blk = DoubleConv3d(ci, co, precision='bf16')
            blk.load({'conv.0.weight': w.cpu(), 'conv.3.weight': 0.05 * torch.randn(co, co, 3, 3, 3, generator=g)})

            def fb():
                blk.forward(x)
                blk.backward(dy)
            ms = timeit(fb)
            vox = N * D * S * S
            flb = 2.0 * vox * 27 * (co * ci * (3 if cp % 64 == 0 else 2) + co * co * 3)
            rec['double_conv_fwd_bwd'] = {'ms': ms, 'GFLOP': flb / 1e9, 'TFLOPs': flb / ms / 1e9, 'frac_of_mfma_peak': flb / ms / 1e9 / peak,
                                          'samples_per_s': N / ms * 1e3}
            out.setdefault(f'{N}x{D}', {})[f'{ci}->{co}'] = rec
            del op, blk, x, dy
            torch.cuda.empty_cache()
    return out


DUMP_SAMPLE = 1 << 22                    # elements kept of an output larger than this (a fixed, seeded sample): <= 16 MB per array


def dump_outputs(out_dir, ts, loss):
    """`--dump-outputs DIR`: what the timed path handed its caller in its LAST timed step, as DIR/<name>.npy (float32 / float64), so
    that two builds run with the same arguments (same seeded inputs and weights) can be compared output for output:
      loss            the step's Tversky loss, shape (1,)
      logits          TrainStep.last_logits, [B, 2, H, W] (flattened sample of DUMP_SAMPLE, numpy default_rng(1), when larger)
      counts          TrainStep.last_counts (the loss's confusion counts), float64
      params, grads   the flat parameters after the step's SGD update and the gradients it applied (TrainStep.flat_params /
                      flat_grads): the same sorted sample of DUMP_SAMPLE positions of each (numpy default_rng(0)) when larger
      bn_buffers      every BatchNorm running mean / variance after the step, concatenated in state-dict order
    At most 3 x 16 MB plus a few kB."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()

    def sample(flat, idx):
        return flat if idx is None else flat[idx]

    n = ts.flat_params.numel()
    idx = None
    if n > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))
    logits = ts.last_logits.detach().float().cpu().numpy()
    if logits.size > DUMP_SAMPLE:
        logits = logits.reshape(-1)[np.sort(np.random.default_rng(1).choice(logits.size, DUMP_SAMPLE, replace=False))]
    bufs = [v.detach().float().reshape(-1).cpu() for k, v in ts.model.state_dict().items()
            if k.endswith('.running_mean') or k.endswith('.running_var')]
    arrays = {
        'loss': loss.detach().float().reshape(1).cpu().numpy(),
        'logits': logits,
        'counts': ts.last_counts.detach().cpu().numpy().astype(np.float64),
        'params': sample(ts.flat_params.detach().cpu().numpy(), idx),
        'grads': sample(ts.flat_grads.detach().cpu().numpy(), idx),
        'bn_buffers': torch.cat(bufs).numpy() if bufs else np.zeros(0, np.float32),
    }
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), np.ascontiguousarray(a))


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(('127.0.0.1', 0))
        return so.getsockname()[1]


def visible_devices():
    """GPUs this process could use.  BENCH_ASSUME_DEVICES overrides the probe (the CPU-only test of the launcher logic)."""
    if os.environ.get('BENCH_ASSUME_DEVICES'):
        return int(os.environ['BENCH_ASSUME_DEVICES'])
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def launch_plan(gpus, env, n_devices, argv):
    """What `bench.py --gpus N` does, decided before anything touches a device:
      ('run', None)      this process IS a rank (WORLD_SIZE == N, set by torch.distributed.run or by our own re-exec), or N == 1;
      ('spawn', cmd)     no launcher above us and N > 1: re-exec under torch.distributed.run with N ranks on 127.0.0.1;
      ('refuse', why)    fewer than N devices, or a launcher whose WORLD_SIZE differs from --gpus: a line whose n_gpus differs from
                         --gpus is never printed (round-3 review: `python bench.py --gpus 8` silently ran one rank)."""
    ws = env.get('WORLD_SIZE')
    if gpus < 1:
        return 'refuse', f'--gpus {gpus}'
    if ws is not None:
        if int(ws) != gpus:
            return 'refuse', f'--gpus {gpus} but the launcher set WORLD_SIZE={ws}'
        return 'run', None
    if gpus == 1:
        return 'run', None
    if n_devices < gpus:
        return 'refuse', f'--gpus {gpus} but only {n_devices} device(s) are visible'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(free_port()), os.path.abspath(__file__)] + list(argv)
    return 'spawn', cmd


def launcher_selftest(json_out):
    """`--launcher-selftest`: every rank the launcher logic produced joins a gloo group on the CPU and rank 0 prints the contract's
    keys with n_gpus = the number of ranks that really showed up (tests/test_host_cpu.py; no device is touched)."""
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        dist.init_process_group('gloo', rank=rank, world_size=world)
        t = torch.ones(1)
        dist.all_reduce(t)
        seen = int(t.item())
        dist.destroy_process_group()
    else:
        seen = 1
    if rank == 0:
        json_out.write(json.dumps({'metric': 'launcher-selftest', 'n_gpus': seen, 'world_size_env': world}) + '\n')
        json_out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=64, help='patch pairs per GPU')
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--channels', type=int, default=13)
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'bf16x3', 'bf16x3-fast', 'fp32'])
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline does not need: step_classes, cpu_baseline and (N = 1, bf16) the extra legs')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-roofline', action='store_true', help='skip the per-launch HIP events')
    ap.add_argument('--no-extras', action='store_true', help='with --full: skip the host_fed / parity_setting / scene legs')
    ap.add_argument('--scene-size', type=int, default=10000)
    ap.add_argument('--force-collectives', action='store_true',
                    help='N=1 only: the HEADLINE loop itself issues its gradient-bucket all-reduces through RCCL (world size 1)')
    ap.add_argument('--windows', type=int, default=3,
                    help='the --steps timed steps are split into this many consecutive windows (at most one per step); the headline '
                         'is the MEDIAN window\'s ms per step (all are reported)')
    ap.add_argument('--dump-outputs', metavar='DIR', default='',
                    help='after the timed steps, write what the last timed step computed to DIR/<name>.npy (rank 0; see dump_outputs)')
    ap.add_argument('--engine-set', default='', help='A/B runs only: engine attributes for the headline loop, e.g. fwd_chains=2,fwd_chain_levels=2')
    ap.add_argument('--launcher-selftest', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')

    # --gpus N without a launcher above us: become the launcher (N ranks under torch.distributed.run), or refuse
    what, detail = launch_plan(args.gpus, os.environ, visible_devices(), sys.argv[1:])
    if what == 'refuse':
        sys.stderr.write(f'bench.py: refusing to run: {detail}\n')
        raise SystemExit(2)
    if what == 'spawn':
        import subprocess
        env = dict(os.environ)
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        env.setdefault('OMP_NUM_THREADS', '8')
        raise SystemExit(subprocess.run(detail, env=env).returncode)

    # the contract is ONE JSON line on stdout: keep a private handle on the real stdout for it and point file descriptor 1 at stderr
    # for everything else (RCCL prints a version banner through C stdio, which would otherwise land after the JSON line at exit)
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), 'w')
    os.dup2(2, 1)

    if args.launcher_selftest:
        launcher_selftest(json_out)
        return
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a ROCm device (MI355X); there is no CPU path for the product')
    # BENCH_BACKEND=gloo (tests only): the N-rank code path of this file on a box with ONE device -- all ranks share cuda:0 and exchange
    # gradients over gloo, exactly as tests/test_gpu_ddp.py does (RCCL refuses two ranks on one device)
    backend = os.environ.get('BENCH_BACKEND', 'nccl')
    if backend == 'gloo':
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    if world > 1 and backend == 'gloo':
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo', rank=rank, world_size=world)
    elif world > 1:
        from fabric_amd.parallel import init_rccl
        init_rccl(rank, world, dev)
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'      # launch_plan() refused anything else
    if args.force_collectives and world == 1:
        os.environ.setdefault('MASTER_PORT', str(29000 + os.getpid() % 3000))
        from fabric_amd.parallel import init_rccl
        init_rccl(0, 1, dev)

    from fabric_amd import BiDateNet
    from fabric_amd.train_step import TrainStep

    torch.manual_seed(1234)                  # same random-init weights on every rank
    model = BiDateNet(args.channels, 2, precision=args.precision).to(dev).train()
    ts = TrainStep(model, lr=1e-3, tversky_alpha=0.1, tversky_beta=0.9, force_collectives=args.force_collectives)
    g = torch.Generator(device='cpu').manual_seed(100 + rank)     # each rank its own shard of synthetic pairs
    B, S, C = args.batch, args.size, args.channels
    x1 = torch.randn(B, C, S, S, generator=g)
    x2 = x1 + 0.3 * torch.randn(B, C, S, S, generator=g)
    lbl = (torch.rand(B, S, S, generator=g) < 0.1).to(torch.uint8)
    x1, x2, lbl = x1.to(dev), x2.to(dev), lbl.to(dev)     # resident in HBM before the timed region

    guard = None
    if world > 1 or args.force_collectives:
        # measure the collectives' cost on THIS stream arrangement before anything is timed, and repair it if it is the slow one
        # (TrainStep.guard_collectives: may replace the chain / weight-gradient stream, so it runs before the loop adopts the chain's)
        guard = ts.guard_collectives(B, S, S)
    torch.cuda.synchronize()
    torch.cuda.set_stream(ts.stream())       # the loop runs on the step's own high-priority stream, as fabric_amd/train.py's does:
                                             # no cross-stream joins at the step boundaries (~25 us of idle GPU per step)
    eng = model.engine()
    for item in filter(None, args.engine_set.split(',')):
        k_, v_ = item.split('=')
        if not hasattr(eng, k_):
            raise SystemExit(f'--engine-set: the engine has no attribute {k_!r}')
        setattr(eng, k_, int(v_) if v_.lstrip('-').isdigit() else v_)
    for _ in range(args.warmup):
        ts.step(x1, x2, lbl)
    # Which MFMA kernel (conv3x3 instantiation or weight-gradient GEMM) dominates?  One fully instrumented, UNTIMED step decides
    # (every event pair is a pipeline bubble, so the timed region brackets ONE launch of that kernel per step).
    conv_all = None
    if not args.no_roofline:
        torch.cuda.synchronize()
        eng.prof, eng.prof_filter = [], None
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        raw, eng.prof = eng.prof, None
        conv_all = {}
        for name, flops, e0, e1 in raw:
            a = conv_all.setdefault(name, [0, 0.0, 0.0])
            a[0] += 1; a[1] += flops; a[2] += e0.elapsed_time(e1) * 1e-3
        fam_all = {}
        for name, v in conv_all.items():
            a = fam_all.setdefault(family_of(name), [0, 0.0, 0.0, []])
            a[0] += v[0]; a[1] += v[1]; a[2] += v[2]; a[3].append(name)
        dom_family = max(fam_all.items(), key=lambda kv: kv[1][2])[0]
        eng.prof_filter = tuple(fam_all[dom_family][3])          # every instantiation of the family with the most time per step
    classes = None
    if not args.no_roofline and rank == 0 and args.full:
        try:
            classes = step_classes(ts, x1, x2, lbl, B, dev)
        except Exception as e:
            classes = {'error': f'{type(e).__name__}: {e}'}
    elif not args.no_roofline:
        # the other ranks, and without --full every rank, run the same step uninstrumented: collectives stay matched, and the timed
        # steps start from the same weights with or without --full
        ts.step(x1, x2, lbl)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    n_dom = fam_all[dom_family][0] if not args.no_roofline else 0
    if not args.no_roofline:
        eng.prof = []
    picks = []
    # EXACTLY --steps timed steps, split into `--windows` consecutive windows of (nearly) equal length, each bracketed by barrier +
    # synchronize on both sides and reduced with MAX over the ranks; the headline is the MEDIAN window's ms per step (all are reported),
    # so that a 1-2 % change is resolvable from one record: value = B * world / ms_per_step.
    n_win = max(1, min(args.windows, args.steps))
    win_steps = [args.steps // n_win + (1 if i < args.steps % n_win else 0) for i in range(n_win)]
    windows, enqueue_s, k = [], 0.0, 0
    for n_steps in win_steps:
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps):
            eng.prof_pick = k % n_dom if n_dom else None      # step k brackets the (k mod n)-th launch of the dominant kernel
            picks.append(eng.prof_pick)
            k += 1
            loss = ts.step(x1, x2, lbl)
        enq = time.perf_counter() - t0                         # host time to enqueue K steps (no sync inside the loop)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        w = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([w], dtype=torch.float64, device=dev if backend != 'gloo' else 'cpu')
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            w = float(t.item())
        windows.append(w / n_steps)
        enqueue_s += enq
    enqueue_max_s = enqueue_s
    if world > 1:                                              # the slowest rank's host loop (8 ranks share one host)
        t = torch.tensor([enqueue_s], dtype=torch.float64, device=dev if backend != 'gloo' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        enqueue_max_s = float(t.item())
    prof, eng.prof, eng.prof_pick = eng.prof, None, None
    loss_val = float(loss.item())
    ms_step = sorted(windows)[len(windows) // 2] * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ts, loss)

    roofline = None
    if prof:
        name = dom_family
        members = list(eng.prof_filter)
        per_step_launches = {m: conv_all[m][0] for m in members}
        # one sample per step, launch shapes round robin; every SHAPE gets the same weight whatever K mod n is:
        # achieved = sum over shapes of its FLOP / sum over shapes of its mean duration
        per = {}
        for (nm, flops, e0, e1), pk in zip(prof, picks):
            a = per.setdefault(pk, [flops, []])
            a[1].append(e0.elapsed_time(e1) * 1e-3)
        flop_sum = sum(v[0] for v in per.values())
        time_sum = sum(sum(v[1]) / len(v[1]) for v in per.values())
        peak = MFMA_F32_PEAK if args.precision == 'fp32' else MFMA_BF16_PEAK
        achieved = flop_sum / time_sum
        conv_total = sum(v[2] for v in conv_all.values())
        tr = pmc_family_traffic(members, per_step_launches, args.precision)
        ravg, rsrc = rocprof_family_avg_us(members, args.precision)
        step_s = ms_step * 1e-3
        families = {}
        for fam, (nl, fl, sec, names) in sorted(fam_all.items(), key=lambda kv: -kv[1][2]):
            fr, _ = rocprof_family_avg_us(names, args.precision)
            families[fam] = {'launches_per_step': nl, 'ms_per_step': round(sec * 1e3, 4), 'TFLOPs': fl / sec / 1e12, 'frac': fl / sec / peak,
                             'GFLOP_per_step': fl / 1e9, 'instantiations': sorted(names), 'rocprof_avg_launch_us': fr}
        roofline = {'bound': 'mfma', 'kernel': name, 'kernel_instantiations': sorted(members),
                    'achieved': achieved / 1e12, 'peak': peak / 1e12,
                    'unit': 'TFLOP/s', 'frac': achieved / peak,
                    'traffic': None if tr is None else tr['hbm_read'] + tr['hbm_write'], 'traffic_detail': tr,
                    'launches_per_step': n_dom, 'sampled_launches': len(prof), 'shapes_sampled': len(per),
                    'sampling': 'one launch of the family per timed step, round robin over its launches of a step; launches weighted equally',
                    'families': families,
                    'families_how': 'kernel FAMILY = all instantiations of one template (conv3x3_kernel<*>: forward + data gradient; wgrad7_kernel<*>: '
                                    'weight-gradient GEMM with / without BatchNorm+ReLU on load); `kernel` is the family with the most summed time in '
                                    'one fully instrumented untimed step, `families` lists every family with its ms / TFLOP/s / fraction of peak there',
                    'avg_launch_us': time_sum / len(per) * 1e6, 'rocprof_avg_launch_us': ravg, 'rocprof_source': rsrc,
                    'flop_per_launch': flop_sum / len(per),
                    'all_mfma_kernels': {'source': 'one fully instrumented untimed step (conv3x3 fwd/dgrad + weight-gradient GEMMs)',
                                         'per_kernel_ms': {k: round(v[2] * 1e3, 3) for k, v in sorted(conv_all.items(), key=lambda kv: -kv[1][2])},
                                         'seconds_per_step': conv_total,
                                         'achieved': sum(v[1] for v in conv_all.values()) / conv_total / 1e12}}
        if name.startswith('wgrad') and name != 'wgrad_first_kernel':
            roofline['note'] = ('the weight-gradient GEMMs run on the second stream CONCURRENTLY with the dz chain on a half-chip grid: the in-step '
                                'launch duration (and so `frac`) is what the GEMM gets beside the chain, not its stand-alone rate')
            # the weight-gradient GEMMs run on the second stream beside the dz chain, on a grid of HALF the CUs by design
            # (fabric_amd/csrc/wgrad.hip wgrad_plan; engine.wgrad_blocks overrides): `frac` above is against the FULL-chip peak
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            blocks = eng.wgrad_blocks or 128
            roofline['grid'] = {'blocks': blocks, 'cus': cus, 'concurrent_with': 'the dz chain (data-gradient convs, BatchNorm / unpool / upsample backward) on the other stream',
                                'frac_of_occupied_cus': achieved / peak * cus / min(blocks, cus)}
    if rank == 0:
        value = B * world / (ms_step * 1e-3)
        peak = MFMA_F32_PEAK if args.precision == 'fp32' else MFMA_BF16_PEAK
        out = {
            'metric': 'patch-pairs/sec (fwd+bwd) 13-band 128x128', 'value': value, 'unit': 'patch-pairs/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': ms_step, 'windows_ms_per_step': [w * 1e3 for w in windows],
            'timing': f'{args.steps} timed steps in {len(windows)} consecutive windows of {win_steps} steps: ms per step of the median window '
                      f'(barrier + synchronize around each, max over ranks)',
            'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': args.precision, 'data': 'synthetic',
            'config': {'workload': f'BiDateNet({C},2) {C}-band {S}x{S} patch pairs, batch {B}/GPU, '
                                   f'fwd + Tversky + bwd + grad all-reduce + SGD (BASELINE configs[{1 if world == 1 else 2}])',
                       'global_batch': B * world, 'patch': S, 'bands': C,
                       'parallelism': f'dp{world}', 'precision': args.precision, 'inputs': 'resident in HBM',
                       **({'collectives': 'forced through RCCL with one rank'} if args.force_collectives and world == 1 else {})},
            'step_mfma_frac': value * FLOP_PER_PAIR_FWD_BWD / (world * peak),
            'final_loss': loss_val,
            'host_enqueue_ms_per_step': enqueue_s / args.steps * 1e3,
            'host_enqueue_ms_per_step_max_over_ranks': enqueue_max_s / args.steps * 1e3,
            'roofline': roofline,
            'step_classes': classes,
        }
        if guard is not None:
            out['collectives'] = {'overhead_frac': guard.get('overhead_frac'), 'guard': guard,
                                  'what_it_prices': 'the step with its bucket all-reduces vs the same step without them, measured on synthetic '
                                                    'inputs before the timed region (max over ranks); with N > 1 this includes the xGMI transfer'}
        hb = pmc_step_bytes(args.precision)
        if hb is not None:
            out['hbm_bytes_per_step'] = hb[0]
            out['hbm_frac'] = hb[0] / (ms_step * 1e-3) / HBM_PEAK
            out['hbm_source'] = hb[1] + ' (PMC FETCH_SIZE x2 + WRITE_SIZE summed over every kernel of a step; bytes/step divided by this run\'s step time and 8 TB/s)'
        if world == 1 and args.full and not args.no_extras and args.precision == 'bf16':
            mc = mfma_ceiling()
            if mc is not None:
                out['mfma_ceiling'] = mc
                if mc.get('random_operands'):
                    out['step_frac_of_mfma_ceiling'] = value * FLOP_PER_PAIR_FWD_BWD / (mc['random_operands'] * 1e12)
            if not args.force_collectives:
                out['collectives'] = collectives_leg(ts, model, dev, x1, x2, lbl, args.steps)
            out['host_fed'] = host_fed_leg(ts, dev, B, C, S, args.steps, args.warmup, x1, x2, lbl)
            del ts, model, eng, x1, x2, lbl
            torch.cuda.empty_cache()
            out['parity_setting'] = parity_leg(dev, B, C, S)
            # (the profiled command is `bench.py --precision bf16x3`: three-term backward; algorithmic FLOP of the 35 forward + data-gradient launches)
            out['parity_setting']['bf16x3']['roofline'] = leg_profile(
                'x3', 35, (FLOP_PER_PAIR_FWD + FLOP_PER_PAIR_FWD - 0.491e9) * 64,
                'bf16x3 step at B = 64: ALGORITHMIC conv FLOP (one product per multiply-add; the kernels execute three bf16 MFMAs per product) over '
                'the family\'s profiled time, against the bf16 dense peak')
            for key, leg in (('val_f1', val_f1_leg), ('conv3d', conv3d_leg)):
                try:
                    out[key] = leg(dev)
                except Exception as e:                            # a bench line without a side leg beats no bench line
                    out[key] = {'error': f'{type(e).__name__}: {e}'}
                torch.cuda.empty_cache()
            out['scene'] = scene_leg(dev, size=args.scene_size)
            lp = leg_profile('scene', 18, FLOP_PER_PAIR_FWD * 256,
                             'eval-shaped forward of one 256-tile batch: 18 convolution launches (10 encoder incl. 5 date-paired, 8 decoder) for 256 x 23.14 GFLOP; '
                             'profiled on ONE lane (tools/bench_scene.py --one-lane: clean per-kernel durations; the timed leg above runs two lanes, whose '
                             'kernels overlap), so rocprof_frac is the convolutions\' own MFMA fraction, without gather / upsample launches and lane overlap')
            if lp is not None and isinstance(out['scene'].get('roofline'), dict):
                out['scene']['roofline'].update({'rocprof_' + k if not k.startswith('rocprof_') else k: v for k, v in lp.items()})
            if isinstance(out.get('conv3d'), dict) and 'error' not in out['conv3d']:
                out['conv3d']['rocprof'] = leg_profile('conv3d', 0, 0, 'tools/bench_conv3d_block.py under rocprofv3: per-instantiation average launch times (CKB = 32: the '
                                                       '13 -> 64 layers, 128: the 64 -> 64 layers; D3 = true marks the 3x3x3 walk); the 2 x 5 and 16 x 5 batches share an instantiation')
        if world == 1 and args.full and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline()
        json_out.write(json.dumps(out) + '\n')
        json_out.flush()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
