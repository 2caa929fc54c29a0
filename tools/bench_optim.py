"""Micro-benchmark (test infrastructure) of the fused step's update rules:
  (a) each update kernel alone at BiDateNet(13, 2)'s flat buffer size (13,401,156 floats), HIP events over --reps back-to-back launches
      after a warm-up: us per launch and TB/s of the bytes the rule moves (plain SGD 3, momentum SGD 5, Adam / AdamW 7 buffer passes);
  (b) the bf16 B=64 128x128 train step in ms for sgd, sgd + momentum, adam and adamw, interleaved in one process like tools/ab_cfg.py
      (--rounds rounds of 5 warm-up + --steps timed steps per rule), median and difference to plain SGD.
  (c) --groups: the grouped Adam kernel (bdn_adam_step_grouped; BiDateNet(13, 2)'s real segment tables: weights / norms and biases,
      and the same with the encoder's segments frozen) against bdn_adam_step in one process, the whole interleaving repeated --rounds
      times (the spread between repeats of the ungrouped kernel is the margin), and the bf16 B=64 128x128 AdamW step with no groups, two
      groups, the encoder frozen, and the encoder frozen + bn='frozen', interleaved like (b).
  (d) --clip: bdn_grad_norm (no table; the model's two-group table; the same with the encoder frozen) and bdn_grad_accumulate (add = 0,
      add = 1) at the model's size beside launches that move the same bytes on the same card in the same process (torch's vector_norm:
      one read; torch's copy_: read + write; torch's add_: two reads + write), bdn_adam_step_grouped_ex beside bdn_adam_step_grouped, and
      the bf16 B=64 128x128 AdamW step plain / with max_grad_norm=1.0 / with accumulate=4 (per update of four micro-steps, against
      four plain steps), interleaved like (b).
  (e) --ema: bdn_ema_update (no table; the model's two-group table; the same with the encoder frozen: 3 buffer passes over the vectors
      that count) and bdn_swap_segments (4 passes) at the model's size, with bdn_adam_step and bdn_adam_step_grouped (7 passes) from
      the same library interleaved in the same run as the bandwidth yardstick, the whole interleaving repeated --rounds times; and the
      bf16 B=64 128x128 AdamW step with averaging off, on (ema_decay=0.999) and on with ema_every=4, interleaved like (b).
    python tools/bench_optim.py [--reps 200] [--rounds 4] [--steps 20] [--skip-step] [--groups | --clip | --ema]
Prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.train_step import TrainStep

N = 13_401_156                     # FlatLayout(BiDateNet(13, 2)).total: 13,401,154 parameters, each tensor padded to 4 floats
HBM_PEAK = 8.0                     # TB/s, MI355X spec


def kernels(reps):
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(0)
    p = torch.randn(N, generator=g).to(dev)
    gr = (torch.randn(N, generator=g) * 1e-3).to(dev)
    buf, m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    st = _lib.stream_ptr()
    step = [0]

    def adam(decoupled):
        def f():
            step[0] += 1
            _lib.call('bdn_adam_step', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-2,
                      decoupled, step[0], N, st)
        return f
    cases = [
        ('sgd', 3, lambda: _lib.call('bdn_sgd_step', p.data_ptr(), gr.data_ptr(), 1e-3, 1.0, N, st)),
        ('sgd_momentum', 5, lambda: _lib.call('bdn_sgd_momentum_step', p.data_ptr(), gr.data_ptr(), buf.data_ptr(), 1e-3, 1.0, 0.9, 0.0,
                                              0.0, 0, 0, N, st)),
        ('sgd_nesterov_wd', 5, lambda: _lib.call('bdn_sgd_momentum_step', p.data_ptr(), gr.data_ptr(), buf.data_ptr(), 1e-3, 1.0, 0.9,
                                                 0.0, 1e-4, 1, 0, N, st)),
        ('adam', 7, adam(0)),
        ('adamw', 7, adam(1)),
    ]
    out = {}
    for name, passes, fn in cases:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        tbs = passes * 4 * N / us * 1e-6
        out[name] = {'us': round(us, 2), 'MB': round(passes * 4 * N / 1e6, 1), 'TB_s': round(tbs, 2), 'frac_of_8TBs': round(tbs / HBM_PEAK, 3)}
        print(f'{name:18s} {us:8.1f} us  {passes * 4 * N / 1e6:6.1f} MB  {tbs:5.2f} TB/s  ({tbs / HBM_PEAK * 100:4.1f} % of 8 TB/s)', flush=True)
    return out


def steps(rounds, n_steps, batch=64):
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    x1 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    x2 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    lbl = (torch.rand(batch, 128, 128, generator=g) < 0.1).to(torch.uint8).to(dev)
    rules = [('sgd', {}), ('sgd_momentum', dict(optimizer='sgd', momentum=0.9)), ('adam', dict(optimizer='adam')),
             ('adamw', dict(optimizer='adamw'))]
    ts = {}
    for name, kw in rules:
        torch.manual_seed(0)
        ts[name] = TrainStep(BiDateNet(13, 2, precision='bf16').to(dev).train(), lr=1e-4, **kw)
    res = {name: [] for name, _ in rules}
    with torch.cuda.stream(ts['sgd'].stream()):                # every TrainStep shares the process's chain stream
        for _ in range(rounds):
            for name, _ in rules:
                s = ts[name]
                for _ in range(5):
                    s.step(x1, x2, lbl)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_steps):
                    s.step(x1, x2, lbl)
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) / n_steps)
    base = statistics.median(res['sgd'])
    out = {}
    for name, _ in rules:
        med = statistics.median(res[name])
        out[name] = {'ms': round(med, 4), 'delta_us': round((med - base) * 1e3, 1), 'rounds_ms': [round(t, 4) for t in res[name]]}
        print(f'step {name:14s} median {med:.4f} ms  ({(med - base) * 1e3:+7.1f} us vs sgd)  {out[name]["rounds_ms"]}', flush=True)
    return out


ENCODER = ('inc.', 'down1.', 'down2.', 'down3.', 'down4.')


def _two_groups(model, frozen_encoder):
    """{weights} / {norms and biases: no decay, lr x 0.1} by name; the encoder's parameters get requires_grad=False when asked."""
    for k, p in model.named_parameters():
        p.requires_grad_(not (frozen_encoder and k.startswith(ENCODER)))
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    return [{'params': [k for k, p in named if p.dim() > 1]},
            {'params': [k for k, p in named if p.dim() == 1], 'weight_decay': 0.0, 'lr': 1e-4}]


def grouped_kernels(reps, rounds):
    """us per launch of bdn_adam_step and of bdn_adam_step_grouped on the real tables, interleaved, `rounds` times over."""
    from fabric_amd import optim as O
    from fabric_amd.engine import param_order
    from fabric_amd.parallel import FlatLayout
    dev = torch.device('cuda', 0)
    model = BiDateNet(13, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(13))
    assert layout.total == N
    cfg = O.OptimConfig('adamw', lr=1e-3)
    tables, moved = {}, {}
    for name, frozen_encoder in (('two_groups', False), ('two_groups_encoder_frozen', True)):
        groups = _two_groups(model, frozen_encoder)
        pg = O.ParamGroups(cfg, names, groups, {k for k, p in named if not p.requires_grad})
        ends, ids = O.segment_table(layout, pg)
        tables[name] = (torch.tensor(ends, dtype=torch.int64).to(torch.int32).to(dev), torch.tensor(ids, dtype=torch.int32).to(dev), len(ends))
        starts = [0] + ends[:-1]
        moved[name] = 7 * 16 * sum(b - a for a, b, g in zip(starts, ends, ids) if g != O.FROZEN)
    g = torch.Generator(device='cpu').manual_seed(0)
    p = torch.randn(N, generator=g).to(dev)
    gr = (torch.randn(N, generator=g) * 1e-3).to(dev)
    m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    st = _lib.stream_ptr()
    step = [0]
    lr, wd = _lib.floats([1e-3, 1e-4]), _lib.floats([1e-2, 0.0])

    def plain():
        step[0] += 1
        _lib.call('bdn_adam_step', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-2, 1, step[0], N, st)

    def grouped(name):
        ends, ids, n_seg = tables[name]

        def f():
            step[0] += 1
            _lib.call('bdn_adam_step_grouped', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), ends.data_ptr(), ids.data_ptr(), n_seg,
                      2, lr, wd, 1.0, 0.9, 0.999, 1e-8, 1, step[0], N, st)
        return f
    cases = [('adamw_ungrouped', 7 * 4 * N, plain)] + [(name, moved[name], grouped(name)) for name in tables]
    res = {name: [] for name, _, _ in cases}
    for _ in range(rounds):
        for name, _, fn in cases:
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / reps * 1e3)
    out = {}
    for name, nbytes, _ in cases:
        med = statistics.median(res[name])
        out[name] = {'us': round(med, 2), 'MB': round(nbytes / 1e6, 1), 'TB_s': round(nbytes / med * 1e-6, 2),
                     'segments': tables[name][2] if name in tables else None, 'rounds_us': [round(t, 2) for t in res[name]]}
        print(f'{name:28s} median {med:8.2f} us  {nbytes / 1e6:6.1f} MB  {nbytes / med * 1e-6:5.2f} TB/s  {out[name]["rounds_us"]}', flush=True)
    return out


def grouped_steps(rounds, n_steps, batch=64):
    """ms per bf16 B=64 128x128 AdamW step: no groups, two groups, encoder frozen, encoder frozen + bn='frozen'; interleaved."""
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    x1 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    x2 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    lbl = (torch.rand(batch, 128, 128, generator=g) < 0.1).to(torch.uint8).to(dev)
    cases = [('no_groups', None, 'batch'), ('two_groups', False, 'batch'), ('encoder_frozen', True, 'batch'),
             ('encoder_frozen_bn_frozen', True, 'frozen')]
    ts = {}
    for name, frozen_encoder, bn in cases:
        torch.manual_seed(0)
        model = BiDateNet(13, 2, precision='bf16').to(dev).train()
        groups = None if frozen_encoder is None else _two_groups(model, frozen_encoder)
        ts[name] = TrainStep(model, lr=1e-4, optimizer='adamw', param_groups=groups, bn=bn)
    res = {name: [] for name, _, _ in cases}
    with torch.cuda.stream(ts['no_groups'].stream()):
        for _ in range(rounds):
            for name, _, _ in cases:
                s = ts[name]
                for _ in range(5):
                    s.step(x1, x2, lbl)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_steps):
                    s.step(x1, x2, lbl)
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) / n_steps)
    base = statistics.median(res['no_groups'])
    out = {}
    for name, _, _ in cases:
        med = statistics.median(res[name])
        out[name] = {'ms': round(med, 4), 'delta_us': round((med - base) * 1e3, 1), 'rounds_ms': [round(t, 4) for t in res[name]]}
        print(f'step {name:26s} median {med:.4f} ms  ({(med - base) * 1e3:+8.1f} us vs no_groups)  {out[name]["rounds_ms"]}', flush=True)
    return out


def clip_kernels(reps, rounds):
    """us per launch (median of `rounds` interleaved repeats) of the norm, accumulate and _ex kernels and of their byte-for-byte
    references."""
    from fabric_amd import optim as O
    from fabric_amd.engine import param_order
    from fabric_amd.parallel import FlatLayout
    dev = torch.device('cuda', 0)
    model = BiDateNet(13, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(13))
    assert layout.total == N
    cfg = O.OptimConfig('adamw', lr=1e-3)
    tables, counted = {}, {}
    for name, frozen_encoder in (('two_groups', False), ('two_groups_encoder_frozen', True)):
        groups = _two_groups(model, frozen_encoder)
        pg = O.ParamGroups(cfg, names, groups, {k for k, p in named if not p.requires_grad})
        ends, ids = O.segment_table(layout, pg)
        tables[name] = (torch.tensor(ends, dtype=torch.int64).to(torch.int32).to(dev), torch.tensor(ids, dtype=torch.int32).to(dev), len(ends))
        counted[name] = 16 * sum(b - a for a, b, g in zip([0] + ends[:-1], ends, ids) if g != O.FROZEN)
    g = torch.Generator(device='cpu').manual_seed(0)
    p = torch.randn(N, generator=g).to(dev)
    gr = (torch.randn(N, generator=g) * 1e-3).to(dev)
    acc, m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    ws = torch.empty(_lib.load().bdn_grad_norm_workspace_bytes(N) // 8, dtype=torch.float64, device=dev)
    out2 = torch.ones(2, device=dev)
    one = torch.ones(1, device=dev)
    st = _lib.stream_ptr()
    step = [0]
    lr, wd = _lib.floats([1e-3, 1e-4]), _lib.floats([1e-2, 0.0])

    def norm(name):
        t = (None, None, 0) if name is None else (tables[name][0].data_ptr(), tables[name][1].data_ptr(), tables[name][2])
        return lambda: _lib.call('bdn_grad_norm', gr.data_ptr(), *t, 1.0, 1.0, ws.data_ptr(), out2.data_ptr(), N, st)

    def adam(ex):
        ends, ids, n_seg = tables['two_groups']

        def f():
            step[0] += 1
            if ex:
                _lib.call('bdn_adam_step_grouped_ex', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), ends.data_ptr(), ids.data_ptr(),
                          n_seg, 2, lr, wd, 1.0, one.data_ptr(), 0.9, 0.999, 1e-8, 1, step[0], N, st)
            else:
                _lib.call('bdn_adam_step_grouped', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), ends.data_ptr(), ids.data_ptr(),
                          n_seg, 2, lr, wd, 1.0, 0.9, 0.999, 1e-8, 1, step[0], N, st)
        return f
    cases = [
        ('ref_read_torch_vector_norm', 4 * N, lambda: torch.linalg.vector_norm(gr)),
        ('grad_norm', 4 * N, norm(None)),
        ('grad_norm_two_groups', counted['two_groups'], norm('two_groups')),
        ('grad_norm_encoder_frozen', counted['two_groups_encoder_frozen'], norm('two_groups_encoder_frozen')),
        ('ref_read_write_torch_copy', 8 * N, lambda: acc.copy_(gr)),
        ('grad_accumulate_copy', 8 * N, lambda: _lib.call('bdn_grad_accumulate', acc.data_ptr(), gr.data_ptr(), N, 0, st)),
        ('ref_2read_write_torch_add', 12 * N, lambda: acc.add_(gr)),
        ('grad_accumulate_add', 12 * N, lambda: _lib.call('bdn_grad_accumulate', acc.data_ptr(), gr.data_ptr(), N, 1, st)),
        ('adamw_grouped', 28 * N, adam(False)),
        ('adamw_grouped_ex', 28 * N, adam(True)),
    ]
    res = {name: [] for name, _, _ in cases}
    for _ in range(rounds):
        for name, _, fn in cases:
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / reps * 1e3)
    out = {}
    for name, nbytes, _ in cases:
        med = statistics.median(res[name])
        out[name] = {'us': round(med, 2), 'MB': round(nbytes / 1e6, 1), 'TB_s': round(nbytes / med * 1e-6, 2), 'rounds_us': [round(t, 2) for t in res[name]]}
        print(f'{name:30s} median {med:8.2f} us  {nbytes / 1e6:6.1f} MB  {nbytes / med * 1e-6:5.2f} TB/s  {out[name]["rounds_us"]}', flush=True)
    for a, b in (('grad_norm', 'ref_read_torch_vector_norm'), ('grad_accumulate_copy', 'ref_read_write_torch_copy'),
                 ('grad_accumulate_add', 'ref_2read_write_torch_add'), ('adamw_grouped_ex', 'adamw_grouped')):
        out[f'{a}/{b}'] = round(out[a]['us'] / out[b]['us'], 3)
        print(f'{a} / {b} = {out[f"{a}/{b}"]}', flush=True)
    return out


def clip_steps(rounds, n_steps, batch=64):
    """ms per bf16 B=64 128x128 AdamW step: plain, with max_grad_norm=1.0, and with accumulate=4 (n_steps is rounded to a multiple of 4;
    reported per micro-step and per update); interleaved."""
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    x1 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    x2 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    lbl = (torch.rand(batch, 128, 128, generator=g) < 0.1).to(torch.uint8).to(dev)
    n_steps = max(4, n_steps // 4 * 4)
    cases = [('plain', {}), ('max_grad_norm_1', dict(max_grad_norm=1.0)), ('accumulate_4', dict(accumulate=4)),
             ('accumulate_4_max_grad_norm_1', dict(accumulate=4, max_grad_norm=1.0))]
    ts = {}
    for name, kw in cases:
        torch.manual_seed(0)
        ts[name] = TrainStep(BiDateNet(13, 2, precision='bf16').to(dev).train(), lr=1e-4, optimizer='adamw', **kw)
    res = {name: [] for name, _ in cases}
    with torch.cuda.stream(ts['plain'].stream()):
        for _ in range(rounds):
            for name, _ in cases:
                s = ts[name]
                for _ in range(8):
                    s.step(x1, x2, lbl)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_steps):
                    s.step(x1, x2, lbl)
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) / n_steps)
    base = statistics.median(res['plain'])
    out = {}
    for name, kw in cases:
        med = statistics.median(res[name])
        k = kw.get('accumulate', 1)
        out[name] = {'ms_per_call': round(med, 4), 'delta_us_per_call': round((med - base) * 1e3, 1), 'ms_per_update': round(med * k, 4),
                     'delta_us_per_update_vs_plain_steps': round((med - base) * k * 1e3, 1), 'rounds_ms': [round(t, 4) for t in res[name]]}
        print(f'step {name:30s} median {med:.4f} ms/call  ({(med - base) * 1e3:+7.1f} us vs plain; per update of {k}: '
              f'{(med - base) * k * 1e3:+7.1f} us)  {out[name]["rounds_ms"]}', flush=True)
    return out


def _tables(dev):
    """BiDateNet(13, 2)'s layout and its real segment tables: {name: (ends, ids, n_seg, vectors that count)}."""
    from fabric_amd import optim as O
    from fabric_amd.engine import param_order
    from fabric_amd.parallel import FlatLayout
    model = BiDateNet(13, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(13))
    assert layout.total == N
    cfg = O.OptimConfig('adamw', lr=1e-3)
    tables = {}
    for name, frozen_encoder in (('two_groups', False), ('encoder_frozen', True)):
        groups = _two_groups(model, frozen_encoder)
        pg = O.ParamGroups(cfg, names, groups, {k for k, p in named if not p.requires_grad})
        ends, ids = O.segment_table(layout, pg)
        count = sum(b - a for a, b, g in zip([0] + ends[:-1], ends, ids) if g != O.FROZEN)
        tables[name] = (torch.tensor(ends, dtype=torch.int64).to(torch.int32).to(dev), torch.tensor(ids, dtype=torch.int32).to(dev), len(ends), count)
    return tables


def ema_kernels(reps, rounds):
    """us per launch, bytes moved and TB/s of bdn_ema_update and bdn_swap_segments beside bdn_adam_step / bdn_adam_step_grouped,
    interleaved, `rounds` times over."""
    dev = torch.device('cuda', 0)
    tables = _tables(dev)
    g = torch.Generator(device='cpu').manual_seed(0)
    p = torch.randn(N, generator=g).to(dev)
    gr = (torch.randn(N, generator=g) * 1e-3).to(dev)
    m, v, avg = torch.zeros(N, device=dev), torch.zeros(N, device=dev), p.clone()
    st = _lib.stream_ptr()
    step = [0]
    lr, wd = _lib.floats([1e-3, 1e-4]), _lib.floats([1e-2, 0.0])

    def table(name):
        if name is None:
            return None, None, 0
        ends, ids, n_seg, _ = tables[name]
        return ends.data_ptr(), ids.data_ptr(), n_seg

    def adam():
        step[0] += 1
        _lib.call('bdn_adam_step', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-2, 1, step[0], N, st)

    def adam_grouped():
        step[0] += 1
        _lib.call('bdn_adam_step_grouped', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), *table('two_groups'), 2, lr, wd, 1.0,
                  0.9, 0.999, 1e-8, 1, step[0], N, st)

    def ema(name):
        return lambda: _lib.call('bdn_ema_update', avg.data_ptr(), p.data_ptr(), *table(name), 1e-3, 0, N, st)

    def swap(name):
        return lambda: _lib.call('bdn_swap_segments', p.data_ptr(), avg.data_ptr(), *table(name), N, st)
    vec = lambda name: N // 4 if name is None else tables[name][3]          # noqa: E731
    cases = [('adamw_ungrouped', 7 * 4 * N, adam), ('adamw_two_groups', 7 * 16 * vec('two_groups'), adam_grouped),
             ('ema_no_table', 3 * 4 * N, ema(None)), ('ema_two_groups', 3 * 16 * vec('two_groups'), ema('two_groups')),
             ('ema_encoder_frozen', 3 * 16 * vec('encoder_frozen'), ema('encoder_frozen')),
             ('swap_no_table', 4 * 4 * N, swap(None)), ('swap_two_groups', 4 * 16 * vec('two_groups'), swap('two_groups'))]
    res = {name: [] for name, _, _ in cases}
    for _ in range(rounds):
        for name, _, fn in cases:
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / reps * 1e3)
    out = {}
    for name, nbytes, _ in cases:
        med = statistics.median(res[name])
        out[name] = {'us': round(med, 2), 'MB': round(nbytes / 1e6, 1), 'TB_s': round(nbytes / med * 1e-6, 2),
                     'TB_s_rounds': [round(nbytes / t * 1e-6, 2) for t in res[name]], 'rounds_us': [round(t, 2) for t in res[name]]}
        print(f'{name:22s} median {med:8.2f} us  {nbytes / 1e6:6.1f} MB  {nbytes / med * 1e-6:5.2f} TB/s  {out[name]["rounds_us"]}', flush=True)
    return out


def ema_steps(rounds, n_steps, batch=64):
    """ms per bf16 B=64 128x128 AdamW step with averaging off, on, and on with ema_every=4; interleaved."""
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    x1 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    x2 = torch.randn(batch, 13, 128, 128, generator=g).to(dev)
    lbl = (torch.rand(batch, 128, 128, generator=g) < 0.1).to(torch.uint8).to(dev)
    cases = [('off', {}), ('ema', dict(ema_decay=0.999)), ('ema_every_4', dict(ema_decay=0.999, ema_every=4))]
    ts = {}
    for name, kw in cases:
        torch.manual_seed(0)
        ts[name] = TrainStep(BiDateNet(13, 2, precision='bf16').to(dev).train(), lr=1e-4, optimizer='adamw', **kw)
    res = {name: [] for name, _ in cases}
    with torch.cuda.stream(ts['off'].stream()):
        for _ in range(rounds):
            for name, _ in cases:
                s = ts[name]
                for _ in range(5):
                    s.step(x1, x2, lbl)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_steps):
                    s.step(x1, x2, lbl)
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) / n_steps)
    base = statistics.median(res['off'])
    out = {}
    for name, _ in cases:
        med = statistics.median(res[name])
        out[name] = {'ms': round(med, 4), 'delta_us': round((med - base) * 1e3, 1), 'rounds_ms': [round(t, 4) for t in res[name]]}
        print(f'step {name:12s} median {med:.4f} ms  ({(med - base) * 1e3:+8.1f} us vs off)  {out[name]["rounds_ms"]}', flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--groups', action='store_true', help='(c): the grouped update kernel and the grouped / frozen steps only')
    ap.add_argument('--clip', action='store_true', help='(d): the norm / accumulate / _ex kernels and the clipped / accumulating steps only')
    ap.add_argument('--ema', action='store_true', help='(e): the averaging / exchange kernels beside the Adam kernels, and the step with averaging off / on')
    a = ap.parse_args()
    if a.ema:
        res = {'n': N, 'ema_kernels': ema_kernels(max(a.reps, 200), a.rounds)}
        if not a.skip_step:
            res['ema_step_bf16_b64'] = ema_steps(a.rounds, a.steps)
        print(json.dumps(res))
        return
    if a.clip:
        res = {'n': N, 'clip_kernels': clip_kernels(max(a.reps, 200), a.rounds)}
        if not a.skip_step:
            res['clip_step_bf16_b64'] = clip_steps(a.rounds, a.steps)
        print(json.dumps(res))
        return
    if a.groups:
        res = {'n': N, 'grouped_kernels': grouped_kernels(max(a.reps, 200), a.rounds)}
        if not a.skip_step:
            res['grouped_step_bf16_b64'] = grouped_steps(a.rounds, a.steps)
        print(json.dumps(res))
        return
    res = {'n': N, 'kernels': kernels(max(a.reps, 200))}
    if not a.skip_step:
        res['step_bf16_b64'] = steps(a.rounds, a.steps)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
