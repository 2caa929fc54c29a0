"""Micro-benchmark (test infrastructure) of the layer-wise adaptive updates: bdn_lamb_step and bdn_lars_step on BiDateNet(13, 2)'s real
per-tensor table (74 tensors, 13,401,156 floats, one implicit group, adapt_1d off) beside bdn_adam_step_grouped_ex and
bdn_sgd_momentum_step_grouped_ex on the model's one-segment table, in one process: --reps back-to-back launches between two HIP events
after a warm-up, the arms interleaved and the whole interleaving repeated --rounds times (the spread between the repeats of one arm is
the margin).  Per arm: us per update (median of the rounds), the bytes the rule moves per element, TB/s, and the ratio to the Adam / momentum
SGD update of the same build on the same card; and the share of the 6.0 ms fused step an update takes.

Bytes per element (4-byte floats; the partial sums, the table and trust_out are kilobytes):
  adamw 28 (p g m v read, p m v written)      lamb 40 (pass 1: p g m v read, m v written; pass 3: p m v read, p written)
  sgd momentum 20 (p g buf read, p buf written)   lars 28 (pass 1: p g read; pass 3: p g buf read, p buf written)

    python tools/bench_layerwise.py [--reps 200] [--rounds 4] [--out profiles/layerwise_bench.txt]
Prints the table and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd import optim as O
from fabric_amd.engine import param_order
from fabric_amd.parallel import FlatLayout

STEP_MS = 6.0                      # the bf16 B=64 128x128 fused step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    model = BiDateNet(13, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(13))
    n = layout.total
    pg = O.ParamGroups(O.OptimConfig('lamb'), names, None, ())
    table = tuple(t.to(dev) for t in O.tensor_table(layout, pg, False))
    n_ten = len(layout.order)
    ends, ids = O.segment_table(layout, pg)
    seg = (torch.tensor(ends, dtype=torch.int64).to(torch.int32).to(dev), torch.tensor(ids, dtype=torch.int32).to(dev), len(ends))
    g = torch.Generator(device='cpu').manual_seed(0)
    p = torch.randn(n, generator=g).to(dev)
    gr = (torch.randn(n, generator=g) * 1e-3).to(dev)
    m, v, buf = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ws = torch.empty(_lib.load().bdn_layerwise_workspace_bytes(n, n_ten) // 8, dtype=torch.float64, device=dev)
    trust = torch.zeros(n_ten, 3, device=dev)
    one = torch.ones(1, device=dev)
    st = _lib.stream_ptr()
    step = [0]
    lr, wd = _lib.floats([1e-3]), _lib.floats([1e-2])
    tab = tuple(t.data_ptr() for t in table) + (n_ten, 1)
    sg = (seg[0].data_ptr(), seg[1].data_ptr(), seg[2], 1)

    def adamw():
        step[0] += 1
        _lib.call('bdn_adam_step_grouped_ex', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), *sg, lr, wd, 1.0, one.data_ptr(),
                  0.9, 0.999, 1e-8, 1, step[0], n, st)

    def lamb():
        step[0] += 1
        _lib.call('bdn_lamb_step', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), *tab, lr, wd, 1.0, one.data_ptr(), 0.9, 0.999,
                  1e-8, 0.0, step[0], ws.data_ptr(), trust.data_ptr(), n, st)

    def sgdm():
        _lib.call('bdn_sgd_momentum_step_grouped_ex', p.data_ptr(), gr.data_ptr(), buf.data_ptr(), *sg, lr, wd, 1.0, one.data_ptr(), 0.9,
                  0.0, 0, 0, n, st)

    def lars():
        _lib.call('bdn_lars_step', p.data_ptr(), gr.data_ptr(), buf.data_ptr(), *tab, lr, wd, 1.0, one.data_ptr(), 0.9, 0.0, 0, 0, 1e-3,
                  1e-8, 0.0, ws.data_ptr(), trust.data_ptr(), n, st)

    cases = [('adamw_grouped_ex', 28, adamw), ('lamb', 40, lamb), ('sgd_momentum_grouped_ex', 20, sgdm), ('lars', 28, lars)]
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
    out, lines = {}, []
    lines.append(f'layer-wise updates on BiDateNet(13, 2): n = {n} floats, {n_ten} tensors; {a.reps} back-to-back launches, {a.rounds} rounds, '
                 f'{torch.cuda.get_device_name(0)}')
    for name, bpe, _ in cases:
        med = statistics.median(res[name])
        out[name] = {'us': round(med, 2), 'bytes_per_element': bpe, 'TB_s': round(bpe * n / med * 1e-6, 2),
                     'share_of_6ms_step': round(med / (STEP_MS * 1e3), 4), 'rounds_us': [round(t, 2) for t in res[name]]}
        lines.append(f'{name:26s} median {med:8.2f} us  {bpe:2d} B/element  {bpe * n / med * 1e-6:5.2f} TB/s  '
                     f'{med / (STEP_MS * 10):5.2f} % of a {STEP_MS} ms step  {out[name]["rounds_us"]}')
    for rule, base in (('lamb', 'adamw_grouped_ex'), ('lars', 'sgd_momentum_grouped_ex')):
        r = out[rule]['us'] / out[base]['us']
        b = out[rule]['bytes_per_element'] / out[base]['bytes_per_element']
        out[f'{rule}/{base}'] = {'time': round(r, 3), 'bytes': round(b, 3)}
        lines.append(f'{rule} / {base}: time x{r:.3f}, bytes x{b:.3f}')
    print('\n'.join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    print(json.dumps({'n': n, 'tensors': n_ten, 'layerwise': out}))


if __name__ == '__main__':
    main()
