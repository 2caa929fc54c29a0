"""-m gpu: gradient accumulation and global-norm clipping in the fused step (TrainStep(accumulate=, max_grad_norm=), flush();
include/bidate_hip.h bdn_grad_accumulate, bdn_grad_norm, bdn_*_step_grouped_ex).

The defaults on today's launches, call for call; the clipped update against the float64 rules of tests/optim_ref.py with the
coefficient of tests/grad_clip_ref.py; frozen parameters left out of the norm; the accumulator's summation order bit for bit against a
twin step; flush(); two gloo ranks (one exchange per update); train.py's flags; and one schedule-stress case."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet, _lib, streams
from fabric_amd.train_step import TrainStep
from oracle import filler
from tests import grad_clip_ref as G
from tests import optim_ref as R
from tests import sched_stress as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
EPS32 = G.EPS32
NEW = ('bdn_grad_accumulate', 'bdn_grad_norm', 'bdn_sgd_step_grouped_ex', 'bdn_sgd_momentum_step_grouped_ex', 'bdn_adam_step_grouped_ex')
B_, C_, S_ = 4, 3, 32


def _inputs(seed=3, b=B_, c=C_, s=S_):
    return tuple(torch.from_numpy(v).to(dev) for v in filler.make_inputs(b, c, s, seed=seed))


def _model(prec='fp32', c=C_):
    return filler.fill_module(BiDateNet(c, 2, precision=prec)).to(dev).train()


class _Spy:
    """Names of every library call made inside the block, the engine's launches included: the hook _lib.call consults before each one."""

    def __enter__(self):
        assert _lib.SKIP is None
        self.calls = []
        _lib.SKIP = lambda name, args: bool(self.calls.append(name))
        return self

    def __exit__(self, *exc):
        _lib.SKIP = None
        return False


def _rule(kw, lr, p, g, state, step, grad_scale):
    """tests/optim_ref.py's rule for the TrainStep keywords `kw` on flat buffers -> (params, |params| magnitude)."""
    if kw['optimizer'] == 'sgd':
        out = R.sgd(p, g, state.get('momentum_buffer'), lr, grad_scale, kw.get('momentum', 0.0), kw.get('dampening', 0.0),
                    kw.get('weight_decay') or 0.0, kw.get('nesterov', False), first=step == 1)
        return out[0], out[2]
    wd = kw.get('weight_decay')
    wd = (1e-2 if kw['optimizer'] == 'adamw' else 0.0) if wd is None else wd
    out = R.adam(p, g, state['exp_avg'], state['exp_avg_sq'], step, lr, grad_scale, kw.get('betas', (0.9, 0.999)), 1e-8, wd,
                 kw['optimizer'] == 'adamw')
    return out[0], out[3]


# ---------------------------------------------------------------- the defaults are today's step
def test_defaults_issue_todays_launches_call_for_call():
    x1, x2, lbl = _inputs()
    lists, outs = [], []
    for kw in (dict(), dict(), dict(accumulate=1, max_grad_norm=None)):      # (the first run creates what a process creates once: streams, events)
        model = _model('bf16')
        with _Spy() as spy:
            ts = TrainStep(model, lr=1e-2, optimizer='adamw', **kw)
            for _ in range(3):
                ts.step(x1, x2, lbl)
            assert ts.flush() is False
            torch.cuda.synchronize()
        lists.append(spy.calls)
        outs.append(ts.flat_params.clone())
        assert ts.flat_accum is None and ts.last_grad_norm is None and ts.last_clip_coef is None and ts.micro == 0 and ts.opt_step == 3
    assert lists[1] == lists[2] and torch.equal(outs[1], outs[2])
    assert not set(lists[2]) & set(NEW), set(lists[2]) & set(NEW)
    assert lists[2].count('bdn_adam_step') == 3 and len(lists[2]) > 300


# ---------------------------------------------------------------- clipping
_RULES = [
    ('sgd_nesterov_wd', dict(optimizer='sgd', momentum=0.9, nesterov=True, weight_decay=1e-2)),
    ('adamw', dict(optimizer='adamw')),
]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('name,kw', _RULES, ids=[r[0] for r in _RULES])
def test_clipped_step_matches_the_rule_with_the_coefficient(name, kw, prec):
    """N = the norm a max_grad_norm=inf step reports; with max_grad_norm = N / 4 the clip is active.  Two steps, each from the step's own
    pre-step parameters, state and gradients: last_grad_norm within 2 EPS32 of the float64 norm of the trainable views of ts.grads,
    last_clip_coef within an ulp of torch's formula on that norm, post-step parameters within 2 R.ULPS + 1 of the rule applied with
    grad_scale * coefficient.  max_grad_norm = 4 N updates bit for bit like max_grad_norm = inf; p.grad keeps the unclipped sum."""
    lr = 5e-3
    x1, x2, lbl = _inputs()
    probe = TrainStep(_model(prec), lr=lr, max_grad_norm=float('inf'), **kw)
    assert float(probe.last_grad_norm) == 0.0                  # nothing measured yet
    probe.step(x1, x2, lbl)
    torch.cuda.synchronize()
    N = float(probe.last_grad_norm)
    assert math.isfinite(N) and N > 0 and float(probe.last_clip_coef) == 1.0
    print(f'{name} {prec}: unclipped norm {N!r}')
    loose = TrainStep(_model(prec), lr=lr, max_grad_norm=4 * N, **kw)
    loose.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert float(loose.last_clip_coef) == 1.0 and torch.equal(loose.flat_params, probe.flat_params)
    for k in probe.opt_state:
        assert torch.equal(loose.opt_state[k], probe.opt_state[k]), k

    model = _model(prec)
    with _Spy() as spy:
        ts = TrainStep(model, lr=lr, max_grad_norm=N / 4, **kw)
        for it in range(2):
            p_in = ts.flat_params.clone()
            s_in = {k: v.clone() for k, v in ts.opt_state.items()}
            ts.step(x1, x2, lbl)
            torch.cuda.synchronize()
            norm, coef = ts.last_grad_norm.cpu().numpy(), ts.last_clip_coef.cpu().numpy()
            ref = math.sqrt(sum(float((g.double() ** 2).sum()) for k, g in ts.grads.items()))
            print(f'  step {it}: norm {norm!r} (float64 {ref!r}, rel err {abs(float(norm) - ref) / ref:.3e}) coef {coef!r}')
            assert abs(float(norm) - ref) <= 2 * EPS32 * ref
            want = G.coef32(norm, N / 4)
            assert abs(float(coef) - float(want)) <= float(np.spacing(want)) and float(coef) < 0.5
            if it == 0:
                assert abs(float(norm) - N) <= 2 * EPS32 * N and 0.24 < float(coef) < 0.26
            rp, mp = _rule(kw, lr, p_in, ts.flat_grads, s_in, it + 1, float(np.float32(1.0)) * float(coef))
            R.check(ts.flat_params, rp, mp, f'{name} {prec} step {it} params', ulps=2 * R.ULPS + 1)
            assert not torch.equal(ts.flat_params, p_in)
    assert ts.opt_step == 2 and spy.calls.count('bdn_grad_norm') == 2
    assert sum(c in NEW[2:] for c in spy.calls) == 2 and not any(c.endswith('_grouped') or c in ('bdn_adam_step', 'bdn_sgd_momentum_step') for c in spy.calls)
    k0, p0 = next(iter(model.named_parameters()))
    assert p0.grad.data_ptr() == ts.grads[k0].data_ptr(), 'p.grad is the view of flat_grads, which keeps the unclipped sum'


def test_frozen_parameters_are_left_out_of_the_norm():
    """inc.* frozen, two groups, the frozen gradients NaN-filled before the step: the norm is finite and equals the trainable views'
    norm, the frozen parameters keep their bits."""
    x1, x2, lbl = _inputs()
    model = _model('fp32')
    for k, p in model.named_parameters():
        p.requires_grad_(not k.startswith('inc.'))
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    groups = [{'params': [k for k, p in named if p.dim() > 1], 'weight_decay': 1e-2}, {'params': [k for k, p in named if p.dim() == 1], 'lr': 1e-4}]
    ts = TrainStep(model, lr=1e-3, optimizer='adamw', param_groups=groups, max_grad_norm=1e-3)
    frozen = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert frozen
    before = {k: dict(model.named_parameters())[k].detach().clone() for k in frozen}
    for k in frozen:
        ts.grads[k].fill_(float('nan'))
    p_in = ts.flat_params.clone()
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    norm = float(ts.last_grad_norm)
    ref = math.sqrt(sum(float((ts.grads[k].double() ** 2).sum()) for k, _ in named))
    assert math.isfinite(norm) and abs(norm - ref) <= 2 * EPS32 * ref and float(ts.last_clip_coef) < 1.0
    for k in frozen:
        assert torch.equal(dict(model.named_parameters())[k].detach(), before[k]), k
        assert bool(torch.isnan(ts.grads[k]).all())
    assert not bool(torch.isnan(ts.flat_params).any()) and not torch.equal(ts.flat_params, p_in)


# ---------------------------------------------------------------- accumulation
def _twin_grads(batches, prec='fp32'):
    """A twin model stepped with lr = 0 on the same batches: clones of its flat_grads per batch, and its BatchNorm buffers after them."""
    twin = _model(prec)
    tb = TrainStep(twin, lr=0.0)
    gs, losses = [], []
    for b in batches:
        losses.append(tb.step(*b))
        gs.append(tb.flat_grads.clone())
    torch.cuda.synchronize()
    buffers = {k: v.clone() for k, v in twin.state_dict().items() if 'running' in k or 'num_batches' in k}
    return gs, buffers, losses


def test_three_micro_batches_accumulate_in_the_documented_order():
    kw = dict(optimizer='sgd', momentum=0.9, nesterov=True, weight_decay=1e-2)
    lr = 5e-3
    batches = [_inputs(seed=s) for s in (3, 4, 5)]
    (g1, g2, g3), buffers, losses = _twin_grads(batches)
    assert not torch.equal(g1, g2) and not torch.equal(g2, g3)
    model = _model('fp32')
    eng = model.engine()
    invalidated, real = [], eng.invalidate_weights
    eng.invalidate_weights = lambda: (invalidated.append(1), real())[1]
    with _Spy() as spy:
        ts = TrainStep(model, lr=lr, accumulate=3, **kw)
        p0 = ts.flat_params.clone()
        s0 = {k: v.clone() for k, v in ts.opt_state.items()}
        micro = []
        for i, b in enumerate(batches):
            n_before = len(spy.calls)
            loss = ts.step(*b)
            torch.cuda.synchronize()
            micro.append(ts.micro)
            assert torch.equal(loss, losses[i]), 'step() returns the micro-batch\'s own unscaled loss'
            if i < 2:
                assert torch.equal(ts.flat_params, p0) and all(torch.equal(ts.opt_state[k], s0[k]) for k in s0) and ts.opt_step == 0
                assert not invalidated, 'a micro-step invalidated the packed weights'
                assert not any(c.startswith(('bdn_sgd', 'bdn_adam')) for c in spy.calls[n_before:])
    assert micro == [1, 2, 0] and ts.opt_step == 1 and len(invalidated) == 1
    total = g3 + ((g1) + g2)
    assert torch.equal(ts.flat_grads, total), float((ts.flat_grads - total).abs().max())
    for k, v in model.state_dict().items():
        if 'running' in k or 'num_batches' in k:
            assert torch.equal(v, buffers[k]), k
    rp, mp = _rule(kw, lr, p0, total, s0, 1, float(np.float32(1 / 3)))
    R.check(ts.flat_params, rp, mp, 'accumulate=3 params', ulps=2 * R.ULPS)
    assert spy.calls.count('bdn_grad_accumulate') == 3 and spy.calls.count('bdn_sgd_momentum_step') == 1
    # with clipping: the norm is that of the mean gradient
    tc = TrainStep(_model('fp32'), lr=lr, accumulate=3, max_grad_norm=float('inf'), **kw)
    for b in batches:
        tc.step(*b)
    torch.cuda.synchronize()
    ref = G.norm(total, None, 1 / 3)
    assert abs(float(tc.last_grad_norm) - ref) <= 2 * EPS32 * ref and float(tc.last_clip_coef) == 1.0
    assert torch.equal(tc.flat_params, ts.flat_params), 'a coefficient of 1.0 changed the update'


def test_flush_applies_or_drops_an_incomplete_accumulation():
    kw = dict(optimizer='adam', weight_decay=1e-3)
    lr = 2e-3
    batches = [_inputs(seed=s) for s in (3, 4)]
    (g1, g2), _, _ = _twin_grads(batches)
    ts = TrainStep(_model('fp32'), lr=lr, accumulate=3, **kw)
    p0 = ts.flat_params.clone()
    s0 = {k: v.clone() for k, v in ts.opt_state.items()}
    ts.step(*batches[0])
    assert ts.micro == 1
    for refused in (ts.optimizer_state_dict, lambda: ts.load_optimizer_state_dict({}), lambda: ts.set_param_groups(None)):
        with pytest.raises(RuntimeError, match=r'flush\(\)'):
            refused()
    ts.step(*batches[1])
    assert ts.micro == 2 and ts.flush() is True and ts.micro == 0 and ts.opt_step == 1
    torch.cuda.synchronize()
    assert torch.equal(ts.flat_grads, g1 + g2)
    rp, mp = _rule(kw, lr, p0, g1 + g2, s0, 1, 0.5)
    R.check(ts.flat_params, rp, mp, 'flush of two micro-steps', ulps=2 * R.ULPS)
    with _Spy() as spy:
        assert ts.flush() is False and ts.flush(apply=False) is False
    assert spy.calls == []
    ts.optimizer_state_dict()                                 # nothing pending: allowed again
    p1 = ts.flat_params.clone()
    ts.step(*batches[0])
    with _Spy() as spy:
        assert ts.flush(apply=False) is False
    torch.cuda.synchronize()
    assert spy.calls == [] and ts.micro == 0 and ts.opt_step == 1 and torch.equal(ts.flat_params, p1)
    # the dropped gradient left nothing behind: the next full accumulation is that of a fresh one
    for b in (batches[1], batches[0], batches[1]):
        ts.step(*b)
    torch.cuda.synchronize()
    assert ts.micro == 0 and ts.opt_step == 2


# ---------------------------------------------------------------- data parallel, in fresh child processes
_GLOO = r'''
import os, sys, math, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[3])
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = sys.argv[4]
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
from fabric_amd import BiDateNet
from fabric_amd.train_step import TrainStep
from oracle import filler
b, c, s = 4, 3, 32
EPS32 = float(torch.finfo(torch.float32).eps)
data = [[torch.from_numpy(v).cuda() for v in filler.make_inputs(b * world, c, s, seed=13 + i)] for i in range(2)]
sl = slice(rank * b, (rank + 1) * b)
model = filler.fill_module(BiDateNet(c, 2, precision='fp32')).cuda().train()
ts = TrainStep(model, lr=1e-3, optimizer='adam', weight_decay=1e-3, n_buckets=3, accumulate=2, max_grad_norm=MAXNORM)
assert ts.world == world and ts.bucketer.active()
n_buckets = len(ts.bucketer.buckets)
assert n_buckets >= 3
count = [0]
real = dist.all_reduce
def counting(*a, **k):
    count[0] += 1
    return real(*a, **k)
dist.all_reduce = counting
for upd in range(2):
    count[0] = 0
    ts.step(*[t[sl] for t in data[0]])
    assert count[0] == 0 and ts.micro == 1, 'a collective on the first micro-step'
    ts.step(*[t[sl] for t in data[1]])
    assert count[0] == n_buckets and ts.micro == 0, (count[0], n_buckets)
    torch.cuda.synchronize()
    ref = math.sqrt(float((ts.flat_grads.double() ** 2).sum())) / (world * 2)
    norm = float(ts.last_grad_norm)
    assert abs(norm - ref) <= 2 * EPS32 * ref, (norm, ref)
    assert float(ts.last_clip_coef) < 1.0, 'the clip is not active'
dist.all_reduce = real
assert ts.opt_step == 2
for t in (ts.flat_params, ts.opt_state['exp_avg'], ts.opt_state['exp_avg_sq'], ts._norm[1], ts.flat_grads):
    mine = t.cpu()
    assert bool(mine.abs().sum() > 0)
    others = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(others, mine)
    assert all(torch.equal(o, mine) for o in others), 'ranks diverged'
dist.barrier(); dist.destroy_process_group()
print('ok', rank, norm)
'''


def test_two_gloo_ranks_exchange_once_per_update(tmp_path):
    """accumulate=2 with an active clip, Adam, two updates: no all-reduce on the first micro-step, exactly one per bucket on the second;
    parameters, Adam state, summed gradients and the norm buffer bit-identical across ranks; the norm that of flat_grads / (world 2)."""
    script = tmp_path / 'accum_ddp_worker.py'
    script.write_text(_GLOO.replace('MAXNORM', '1e-4'))
    port = str(41000 + (os.getpid() * 7) % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', ROOT, port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=280)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(outs)
    assert all('ok' in o for o in outs)


_RCCL = r'''
import os, sys, torch
sys.path.insert(0, sys.argv[1])
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = sys.argv[2]
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)
from fabric_amd.parallel import init_rccl
init_rccl(0, 1, dev)
from fabric_amd import BiDateNet
from fabric_amd.train_step import TrainStep
from oracle import filler
batches = [[torch.from_numpy(v).cuda() for v in filler.make_inputs(4, 3, 32, seed=17 + i)] for i in range(2)]
kw = dict(lr=1e-3, optimizer='adam', accumulate=2, max_grad_norm=1e-4)
local = TrainStep(filler.fill_module(BiDateNet(3, 2, precision='fp32')).cuda().train(), distributed=False, **kw)
ts = TrainStep(filler.fill_module(BiDateNet(3, 2, precision='fp32')).cuda().train(), force_collectives=True, guard=False, **kw)
assert ts.bucketer.active() and not local.bucketer.active()
for s in (local, ts):
    for b in batches:
        s.step(*b)
    s.step(*batches[0])                                      # one micro-step pending
torch.cuda.synchronize()
assert ts.micro == 1 and ts.opt_step == 1
# a world of one: the all-reduce is the identity, so the bucket-by-bucket add gives the bits of the one launch behind backward
for name in ('flat_params', 'flat_grads', 'flat_accum'):
    assert torch.equal(getattr(ts, name), getattr(local, name)), name
assert torch.equal(ts._norm[1], local._norm[1]) and float(ts.last_clip_coef) < 1.0
before = (ts.flat_params.clone(), ts.opt_state['exp_avg'].clone(), ts.opt_state['exp_avg_sq'].clone(), ts.flat_accum.clone(), ts._norm[1].clone())
rep = ts.guard_collectives(4, 32, 32, steps=2)
assert rep['active'], rep
torch.cuda.synchronize()
after = (ts.flat_params, ts.opt_state['exp_avg'], ts.opt_state['exp_avg_sq'], ts.flat_accum, ts._norm[1])
for name, u, v in zip(('params', 'exp_avg', 'exp_avg_sq', 'flat_accum', 'norm buffer'), before, after):
    assert torch.equal(u, v), name
assert ts.accumulate == 2 and ts.micro == 1 and ts.opt_step == 1
for s in (local, ts):
    s.step(*batches[1])
torch.cuda.synchronize()
assert ts.micro == 0 and ts.opt_step == 2 and torch.equal(ts.flat_params, local.flat_params) and torch.equal(ts.flat_grads, local.flat_grads)
import torch.distributed as dist
dist.barrier(); dist.destroy_process_group()
print('ok')
'''


def test_bucketed_add_over_rccl_and_guard_collectives_restore(tmp_path):
    """One rank with forced collectives over RCCL: the pending sum added bucket by bucket from inside backward (on the stream each
    all-reduce is issued from) gives the bits of the local step's single launch; guard_collectives measures with accumulation off and
    puts accumulate, micro, flat_accum and the norm buffer back beside what it restored before."""
    script = tmp_path / 'accum_rccl_worker.py'
    script.write_text(_RCCL)
    port = str(43000 + (os.getpid() * 3) % 2000)
    p = subprocess.Popen([sys.executable, str(script), ROOT, port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.communicate(timeout=280)[0].decode()
    assert p.returncode == 0 and 'ok' in out, out


# ---------------------------------------------------------------- train.py --accumulate / --max_grad_norm
def test_train_cli_accumulates_and_clips(tmp_path):
    import json
    from fabric_amd.train import make_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    bs = 8
    train_loader, _ = make_loaders(synthetic_onera(n_cities=6, bands=13, size=(360, 360)), ['city4', 'city5'], 90, 90, bs, True)
    per_epoch = len(train_loader)
    assert per_epoch > 1
    log = tmp_path / 'log'
    flags = ['--accumulate', '2', '--max_grad_norm', '1.0', '--epochs', '1', '--num_workers', '0', '--batch_size', str(bs)]
    common = [sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--log_dir', str(log)]
    r = subprocess.run(common + ['--fused_step', 'true', '--optimizer', 'adam'] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sd = torch.load(log / 'optimizer_epoch_0.pt', weights_only=True)
    assert all(float(s['step']) == math.ceil(per_epoch / 2) for s in sd['state'].values()) and len(sd['state']) == 74
    rec = next(json.loads(line) for line in r.stdout.splitlines() if line.startswith('{"epoch"'))
    assert {'train_grad_norm_mean', 'train_grad_norm_max', 'train_clipped_frac'} <= set(rec), sorted(rec)
    assert 0 < rec['train_grad_norm_mean'] <= rec['train_grad_norm_max'] and 0.0 <= rec['train_clipped_frac'] <= 1.0
    r = subprocess.run(common + ['--loss_function', 'dice'] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and '--fused_step true' in r.stderr


# ---------------------------------------------------------------- stream timing cannot change the result
def test_accumulating_clipped_step_bits_do_not_depend_on_stream_timing(monkeypatch):
    """bf16, momentum SGD, accumulate=2 with an active clip, four calls = two updates on the chain stream: under the natural schedule, a
    lagging weight-gradient stream, a lagging chain and a seeded random pattern the results are those of the run with a device
    synchronisation in front of every launch.  An accumulate or norm launch that read a gradient before the weight-gradient stream
    had written it would differ here."""
    from tests.test_gpu_sched_stress import P_RANDOM, STEP_CASES, _Cal, _diff, _Steps
    monkeypatch.setitem(STEP_CASES, 'accum-clip', dict(prec='bf16', kw=dict(optimizer='sgd', momentum=0.9, accumulate=2, max_grad_norm=1e-3)))
    chain, wgrad = streams.get('chain'), streams.get('wgrad')
    assert not (streams.serialised(chain, wgrad) or streams.serialised(wgrad, chain)), 'the two streams share a hardware queue'

    class Steps(_Steps):
        def enqueue(self, ts):
            out = super().enqueue(ts)
            with torch.cuda.stream(ts.stream()):
                out.update(grad_norm=ts.last_grad_norm.clone(), clip_coef=ts.last_clip_coef.clone(), flat_grads=ts.flat_grads.clone(),
                           flat_accum=ts.flat_accum.clone(), micro=torch.tensor(ts.micro))
            return out
    cal = _Cal()
    sub = Steps('accum-clip', True)
    sizes = cal.measure('step accum-clip chain', lambda: sub.enqueue(sub.prepare()))
    ref, h_ref = sub.run(ss.sync(), sizes)
    names = [n for n, _ in h_ref.trace]
    assert names.count('bdn_grad_accumulate') == 4 and names.count('bdn_grad_norm') == 2 and names.count('bdn_sgd_momentum_step_grouped_ex') == 2
    assert int(ref['opt_step']) == 2 and int(ref['micro']) == 0 and 0 < float(ref['clip_coef']) < 1 and math.isfinite(float(ref['grad_norm']))
    bad = {}
    for pat in (ss.none(), ss.none(queued=True), ss.lag('wgrad', queued=True), ss.lag('chain', queued=True), ss.random(11, P_RANDOM, queued=True)):
        got, h = sub.run(pat, sizes)
        assert pat.kind in ('none', 'random') or h.log, f'{pat}: delayed nothing'
        d = _diff(got, ref)
        if d:
            bad[repr(pat)] = d
    assert not bad, f'results differ from the synchronised run under {bad}'
