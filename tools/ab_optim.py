"""A/B (test infrastructure) of two builds of libbidate_hip.so on the table-driven kernels of csrc/optim.hip, in one process on one card:
the three libraries -- the base, a second copy of the base file (a library loaded twice from one path is one library) and the new one --
are loaded side by side with ctypes.

1. Bits.  Every entry point whose kernel stages a segment / tensor table -- the six grouped / _ex updates, bdn_ema_update,
   bdn_swap_segments, bdn_grad_norm, bdn_lamb_step, bdn_lars_step, bdn_sam_perturb (SAM and ASAM), bdn_sam_restore -- three consecutive
   calls from the same seeded inputs through the base and through the new library, every output buffer (parameters, state, out,
   trust_out, saved; never the workspace, whose unowned slots are undefined) compared bit for bit.  Two sizes: a 21,524-float layout of
   five tensors (a 16-vector one, one that ends 3 vectors into a block of 256, a frozen one, the last end 5 vectors short of n / 4) and
   BiDateNet(13, 2)'s real tables at 13,401,156 floats with two groups and the encoder frozen.
2. Time.  The kernel arms of tools/bench_optim.py --groups / --clip / --ema, tools/bench_layerwise.py and tools/bench_sam.py at the
   model's size: --reps back-to-back launches between two HIP events after a warm-up, base / new / base copy alternated inside every
   round, --rounds rounds.  Per arm: the median of each library, new - base beside base copy - base, and whether the new median lies
   inside the range of the base's rounds (both copies): the spread of the base against itself is the margin.

    python tools/ab_optim.py --base BASE.so --base-copy COPY.so [--new fabric_amd/csrc/libbidate_hip.so] [--reps 200] [--rounds 5] [--out FILE]
Exit status 1 when a bit differs."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd import optim as O
from fabric_amd.engine import param_order
from fabric_amd.parallel import FlatLayout
from bench_optim import N, _two_groups

dev = torch.device('cuda', 0)


class Lib:
    def __init__(self, path):
        self.path, self.lib = path, C.CDLL(os.path.abspath(path))
        for name, (res, args) in _lib.SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args

    def __call__(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise RuntimeError(f'{self.path}: {name} failed (rc={rc}): {self.lib.bdn_last_error().decode(errors="replace")}')


def as32(v):
    return torch.tensor(v, dtype=torch.int64).to(torch.int32).to(dev)


class Layout:
    """n floats, a segment table (ends, ids), a tensor table (ends, lens, ids, adapt) and the number of groups."""

    def __init__(self, n, seg, ten, n_groups):
        self.n, self.n_groups = n, n_groups
        self.seg = tuple(as32(t) for t in seg)
        self.ten = tuple(t.to(dev) if torch.is_tensor(t) else as32(t) for t in ten)
        self.n_seg, self.n_ten = len(seg[0]), len(ten[0])


def small_layout():
    sizes, ids = [61, 4042, 7997, 1199, 8195], [0, 1, -1, 0, 1]
    ends, off = [], 0
    for s in sizes:
        off += (s + 3) // 4
        ends.append(off)
    n = 4 * (4096 + 1024 + 256 + 5)
    assert ends[-1] == n // 4 - 5 and ends[1] % 256 == 3
    return Layout(n, (ends, ids), (ends, sizes, ids, [1, 1, 1, 0, 1]), 2)


def model_layouts():
    """BiDateNet(13, 2): {two_groups, encoder_frozen: two groups with their segment and tensor tables; one_group: the implicit group}."""
    model = BiDateNet(13, 2)
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    layout = FlatLayout([(k, p.shape) for k, p in named], param_order(13))
    assert layout.total == N
    out = {}
    for name, frozen_encoder in (('two_groups', False), ('encoder_frozen', True)):
        groups = _two_groups(model, frozen_encoder)
        pg = O.ParamGroups(O.OptimConfig('adamw', lr=1e-3), names, groups, {k for k, p in named if not p.requires_grad})
        out[name] = Layout(N, O.segment_table(layout, pg), O.tensor_table(layout, pg), 2)
    pg = O.ParamGroups(O.OptimConfig('lamb'), names, None, ())
    out['one_group'] = Layout(N, O.segment_table(layout, pg), O.tensor_table(layout, pg, False), 1)
    return out


class Bufs:
    """Seeded inputs for one layout, fresh per library: p, g (x3), the states, and the small outputs."""
    _host = {}

    def __init__(self, lay, lib):
        n = lay.n
        if n not in Bufs._host:
            gen = torch.Generator(device='cpu').manual_seed(n)
            Bufs._host[n] = [torch.randn(n, generator=gen) * s for s in (1.0, 0.3, 1.3, 2.3, 1.0)]
        self.p, g0, g1, g2, self.q = (t.to(dev) for t in Bufs._host[n])         # q: the second buffer of ema / swap
        self.g = [g0, g1, g2]
        self.m, self.v, self.buf, self.saved = (torch.zeros(n, device=dev) for _ in range(4))
        self.ds = torch.tensor([0.37], device=dev)
        self.out = torch.zeros(2, device=dev)
        self.trust = torch.zeros(lay.n_ten, 3, device=dev)
        self.nws = torch.zeros(lib.lib.bdn_grad_norm_workspace_bytes(n) // 8 + 2, dtype=torch.float64, device=dev)
        self.lws = torch.zeros(lib.lib.bdn_layerwise_workspace_bytes(n, lay.n_ten) // 8 + 2, dtype=torch.float64, device=dev)


def bit_cases(lay):
    """{name: f(lib, b, it) -> the output tensors of call `it` (0, 1, 2)}"""
    n, st = lay.n, _lib.stream_ptr()
    lrs, wds = [1e-2, 1e-3][:lay.n_groups], [1e-2, 0.0][:lay.n_groups]
    lr, wd = _lib.floats(lrs), _lib.floats(wds)
    seg = (lay.seg[0].data_ptr(), lay.seg[1].data_ptr(), lay.n_seg)
    ten = tuple(t.data_ptr() for t in lay.ten) + (lay.n_ten, lay.n_groups)
    sam_t = (lay.ten[0].data_ptr(), lay.ten[1].data_ptr(), lay.ten[2].data_ptr(), lay.n_ten)
    P = lambda t: t.data_ptr()                                                   # noqa: E731
    cases = {}

    def sgd(ex):
        def f(lib, b, it):
            if ex:
                lib('bdn_sgd_step_grouped_ex', P(b.p), P(b.g[it]), *seg, lay.n_groups, lr, 0.5, P(b.ds), n, st)
            else:
                lib('bdn_sgd_step_grouped', P(b.p), P(b.g[it]), *seg, lay.n_groups, lr, 0.5, n, st)
            return [b.p]
        return f

    def sgdm(ex, mom, nesterov):
        def f(lib, b, it):
            buf = P(b.buf) if mom else None
            tail = (mom, 0.0, nesterov, int(it == 0), n, st)
            if ex:
                lib('bdn_sgd_momentum_step_grouped_ex', P(b.p), P(b.g[it]), buf, *seg, lay.n_groups, lr, wd, 0.5, P(b.ds), *tail)
            else:
                lib('bdn_sgd_momentum_step_grouped', P(b.p), P(b.g[it]), buf, *seg, lay.n_groups, lr, wd, 0.5, *tail)
            return [b.p, b.buf]
        return f

    def adam(ex, decoupled):
        def f(lib, b, it):
            tail = (0.9, 0.999, 1e-8, decoupled, it + 1, n, st)
            if ex:
                lib('bdn_adam_step_grouped_ex', P(b.p), P(b.g[it]), P(b.m), P(b.v), *seg, lay.n_groups, lr, wd, 0.5, P(b.ds), *tail)
            else:
                lib('bdn_adam_step_grouped', P(b.p), P(b.g[it]), P(b.m), P(b.v), *seg, lay.n_groups, lr, wd, 0.5, *tail)
            return [b.p, b.m, b.v]
        return f
    for ex in (0, 1):
        x = '_ex' if ex else ''
        cases[f'sgd_step_grouped{x}'] = sgd(ex)
        cases[f'sgd_momentum_step_grouped{x} momentum'] = sgdm(ex, 0.9, 1)
        cases[f'sgd_momentum_step_grouped{x} no momentum'] = sgdm(ex, 0.0, 0)
        cases[f'adam_step_grouped{x} adamw'] = adam(ex, 1)
        cases[f'adam_step_grouped{x} adam'] = adam(ex, 0)

    def ema(table, w, copy):
        t = seg if table else (None, None, 0)

        def f(lib, b, it):
            lib('bdn_ema_update', P(b.q), P(b.p), *t, w, copy if it == 0 else 0, n, st)
            return [b.q, b.p]
        return f

    def swap(table):
        t = seg if table else (None, None, 0)

        def f(lib, b, it):
            lib('bdn_swap_segments', P(b.p), P(b.q), *t, n, st)
            return [b.p, b.q]
        return f

    def norm(table):
        t = seg if table else (None, None, 0)

        def f(lib, b, it):
            lib('bdn_grad_norm', P(b.g[it]), *t, 0.5, 1.0, P(b.nws), P(b.out), n, st)
            return [b.out]
        return f
    for table in (1, 0):
        x = 'table' if table else 'no table'
        cases[f'ema_update {x} w=1e-3'] = ema(table, 1e-3, 0)
        cases[f'ema_update {x} w=0.75 copy first'] = ema(table, 0.75, 1)
        cases[f'swap_segments {x}'] = swap(table)
        cases[f'grad_norm {x}'] = norm(table)

    def lamb(ds):
        def f(lib, b, it):
            lib('bdn_lamb_step', P(b.p), P(b.g[it]), P(b.m), P(b.v), *ten, lr, wd, 0.5, P(b.ds) if ds else None, 0.9, 0.999, 1e-8, 0.0,
                it + 1, P(b.lws), P(b.trust), n, st)
            return [b.p, b.m, b.v, b.trust]
        return f

    def lars(mom, nesterov):
        def f(lib, b, it):
            lib('bdn_lars_step', P(b.p), P(b.g[it]), P(b.buf) if mom else None, *ten, lr, wd, 0.5, P(b.ds), mom, 0.0, nesterov, int(it == 0),
                0.02, 1e-8, 0.0, P(b.lws), P(b.trust), n, st)
            return [b.p, b.buf, b.trust]
        return f
    cases['lamb_step'] = lamb(0)
    cases['lamb_step dev_scale'] = lamb(1)
    cases['lars_step nesterov'] = lars(0.9, 1)
    cases['lars_step no momentum'] = lars(0.0, 0)

    def sam(adaptive):
        def f(lib, b, it):
            lib('bdn_sam_perturb', P(b.p), P(b.saved), P(b.g[it]), *sam_t, 0.5 if adaptive else 0.05, adaptive, 1e-12, P(b.nws), P(b.out), n, st)
            outs = [b.p.clone(), b.saved.clone(), b.out.clone()]
            if it == 1:                                                          # perturb, perturb + restore, perturb
                lib('bdn_sam_restore', P(b.p), P(b.saved), sam_t[0], sam_t[2], lay.n_ten, n, st)
                outs.append(b.p)
            return outs
        return f
    cases['sam_perturb / sam_restore'] = sam(0)
    cases['asam_perturb / sam_restore'] = sam(1)
    return cases


def bits(base, new, layouts, lines):
    bad = 0
    for lname, lay in layouts.items():
        for cname, fn in bit_cases(lay).items():
            res = []
            for lib in (base, new):
                b = Bufs(lay, lib)
                got = []
                for it in range(3):
                    got += [t.clone().view(torch.int32) for t in fn(lib, b, it)]
                torch.cuda.synchronize()
                res.append(got)
            same = len(res[0]) == len(res[1]) and all(torch.equal(x, y) for x, y in zip(*res))
            moved = any(bool((x != x[0]).any()) for x in res[0] if x.numel() > 2)       # not a run of equal words: something was computed
            bad += not same
            lines.append(f'bits {lname:15s} {cname:45s} {len(res[0]):2d} buffers  {"equal" if same else "DIFFERENT"}{"" if moved else "  (constant?)"}')
    return bad


def time_arms(lays):
    """[(name, f(lib))] at the model's size, the arms of the bench tools."""
    st = _lib.stream_ptr()
    g = torch.Generator(device='cpu').manual_seed(0)
    p = torch.randn(N, generator=g).to(dev)
    gr = (torch.randn(N, generator=g) * 1e-3).to(dev)
    m, v, buf, avg, saved = torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev), p.clone(), p.clone()
    one, out2 = torch.ones(1, device=dev), torch.ones(2, device=dev)
    og = lays['one_group']
    ws = torch.empty(_lib.load().bdn_layerwise_workspace_bytes(N, og.n_ten) // 8 + 2, dtype=torch.float64, device=dev)
    trust = torch.zeros(og.n_ten, 3, device=dev)
    step = [0]
    lr2, wd2 = _lib.floats([1e-3, 1e-4]), _lib.floats([1e-2, 0.0])
    lr1, wd1 = _lib.floats([1e-3]), _lib.floats([1e-2])
    P = lambda t: t.data_ptr()                                                   # noqa: E731

    def seg(name):
        if name is None:
            return None, None, 0
        return P(lays[name].seg[0]), P(lays[name].seg[1]), lays[name].n_seg

    def adam(name, ex):
        def f(lib):
            step[0] += 1
            if ex:
                lib('bdn_adam_step_grouped_ex', P(p), P(gr), P(m), P(v), *seg(name), 2, lr2, wd2, 1.0, P(one), 0.9, 0.999, 1e-8, 1, step[0], N, st)
            else:
                lib('bdn_adam_step_grouped', P(p), P(gr), P(m), P(v), *seg(name), 2, lr2, wd2, 1.0, 0.9, 0.999, 1e-8, 1, step[0], N, st)
        return f
    ten = tuple(P(t) for t in og.ten) + (og.n_ten, 1)
    sam_t = (P(og.ten[0]), P(og.ten[1]), P(og.ten[2]), og.n_ten)

    def lamb(lib):
        step[0] += 1
        lib('bdn_lamb_step', P(p), P(gr), P(m), P(v), *ten, lr1, wd1, 1.0, P(one), 0.9, 0.999, 1e-8, 0.0, step[0], P(ws), P(trust), N, st)

    def adam_one(lib):
        step[0] += 1
        lib('bdn_adam_step_grouped_ex', P(p), P(gr), P(m), P(v), *seg('one_group'), 1, lr1, wd1, 1.0, P(one), 0.9, 0.999, 1e-8, 1, step[0], N, st)
    arms = [
        ('groups  adamw two_groups', adam('two_groups', 0)),
        ('groups  adamw encoder_frozen', adam('encoder_frozen', 0)),
        ('clip    adamw_grouped_ex two_groups', adam('two_groups', 1)),
    ]
    for name in (None, 'two_groups', 'encoder_frozen'):
        arms.append((f'clip    grad_norm {name or "no table"}',
                     lambda lib, t=seg(name): lib('bdn_grad_norm', P(gr), *t, 1.0, 1.0, P(ws), P(out2), N, st)))
    for name in (None, 'two_groups', 'encoder_frozen'):
        arms.append((f'ema     ema_update {name or "no table"}', lambda lib, t=seg(name): lib('bdn_ema_update', P(avg), P(p), *t, 1e-3, 0, N, st)))
    for name in (None, 'two_groups'):
        arms.append((f'ema     swap_segments {name or "no table"}', lambda lib, t=seg(name): lib('bdn_swap_segments', P(p), P(avg), *t, N, st)))
    arms += [
        ('layerw  adamw_grouped_ex one segment', adam_one),
        ('layerw  lamb', lamb),
        ('layerw  sgd_momentum_grouped_ex one segment',
         lambda lib: lib('bdn_sgd_momentum_step_grouped_ex', P(p), P(gr), P(buf), *seg('one_group'), 1, lr1, wd1, 1.0, P(one), 0.9, 0.0, 0, 0, N, st)),
        ('layerw  lars', lambda lib: lib('bdn_lars_step', P(p), P(gr), P(buf), *ten, lr1, wd1, 1.0, P(one), 0.9, 0.0, 0, 0, 1e-3, 1e-8, 0.0,
                                         P(ws), P(trust), N, st)),
        ('sam     sam_perturb', lambda lib: lib('bdn_sam_perturb', P(p), P(saved), P(gr), *sam_t, 0.05, 0, 1e-12, P(ws), P(out2), N, st)),
        ('sam     asam_perturb', lambda lib: lib('bdn_sam_perturb', P(p), P(saved), P(gr), *sam_t, 0.05, 1, 1e-12, P(ws), P(out2), N, st)),
        ('sam     sam_restore', lambda lib: lib('bdn_sam_restore', P(p), P(saved), sam_t[0], sam_t[2], og.n_ten, N, st)),
    ]
    return arms


def times(libs, lays, reps, rounds, lines):
    arms = time_arms(lays)
    res = {name: {k: [] for k in libs} for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            for k, lib in libs.items():
                for _ in range(20):
                    fn(lib)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn(lib)
                e1.record()
                torch.cuda.synchronize()
                res[name][k].append(e0.elapsed_time(e1) / reps * 1e3)
    lines.append(f'us per call, median of {rounds} rounds of {reps} launches; base / new / base copy alternated inside every round')
    lines.append(f'{"arm":46s} {"base":>8s} {"copy":>8s} {"new":>8s}  {"copy-base":>9s} {"new-base":>9s}  base rounds min..max   new in range')
    slow = 0
    for name, _ in arms:
        r = res[name]
        b, c, w = (statistics.median(r[k]) for k in ('base', 'copy', 'new'))
        lo, hi = min(r['base'] + r['copy']), max(r['base'] + r['copy'])
        ok = w <= hi
        slow += not ok
        lines.append(f'{name:46s} {b:8.2f} {c:8.2f} {w:8.2f}  {c - b:+9.2f} {w - b:+9.2f}  {lo:8.2f}..{hi:8.2f}   '
                     f'{"yes" if lo <= w <= hi else ("faster" if w < lo else "SLOWER")}')
    return slow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--base', required=True)
    ap.add_argument('--base-copy', required=True, help='a copy of the base library under another file name')
    ap.add_argument('--new', default=_lib.LIB_PATH)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    libs = {'base': Lib(a.base), 'new': Lib(a.new), 'copy': Lib(a.base_copy)}
    lines = [f'{torch.cuda.get_device_name(0)}; base {os.path.relpath(a.base)}, new {os.path.relpath(a.new)}']
    lays = model_layouts()
    bad = bits(libs['base'], libs['new'], {'small_21524': small_layout(), 'model_enc_frozen': lays['encoder_frozen']}, lines)
    lines.append(f'bits: {"every buffer equal" if bad == 0 else f"{bad} case(s) DIFFER"}')
    print('\n'.join(lines), flush=True)
    n0 = len(lines)
    slow = times(libs, lays, a.reps, a.rounds, lines)
    lines.append('time: every arm inside or below the range of the base library\'s own rounds' if slow == 0
                 else f'time: {slow} arm(s) above the range of the base library\'s own rounds')
    print('\n'.join(lines[n0:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
