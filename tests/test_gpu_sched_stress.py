"""-m gpu: stream timing cannot change results.  Every subject below -- engine.backward, TrainStep, the autograd route, scene inference,
the feeder and the device loader -- is run under the launch perturbations of tests/sched_stress.py (sleep kernels in front of the
library's own launches, on the launches' own streams) and must give, bit for bit, what it gives with a device synchronisation in front
of every launch (`sync`: race-free whatever the streams).  Two runs at the natural timing show determinism; only a run whose timing was
MOVED shows that a missing wait is not merely hidden by it.

Sleep lengths are measured here, not fixed: one timed _sleep gives cycles per microsecond, one profiled unperturbed run of each subject
its longest single launch and its duration; the short sleep is 3 x the longest launch (after a handful of launches the lagging stream
is more than a layer behind), the long one 2 x the subject's duration (the other stream runs to its join with nothing of the stalled one
done).  At these shapes the host, not the device, paces the launches, so every perturbed run starts behind a head sleep of twice the long
one on each of its streams (sched_stress: queued): the device then runs from full queues, as in a full-size step.  For engine.backward
every lag / stall run must also show that it moved the schedule (Perturb.join_lag_us / idle_before_launch).

The two mutant tests at the end remove waits (never a pointer, a size or a launch) and prove that the patterns catch it.
"""
import copy
import functools
import os
import random as pyrandom
import time

import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet, _lib, streams
from fabric_amd.train_step import TrainStep
from fabric_amd.utils import inference as inf
from oracle import filler
from tests import sched_stress as ss

pytestmark = pytest.mark.gpu

C = 13
MAIN, ODD = (2, 32, 48), (3, 16, 16)          # (B, H, W): the smallest shapes at which the default step's own paths engage; odd B: one-image tiles
SEEDS = (11, 12, 13)
P_RANDOM = 0.3


def _report(*a):
    print('[sched]', *a, flush=True)


# ---------------------------------------------------------------------------------------------------------------- calibration
class _Cal:
    def __init__(self):
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20_000_000
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        torch.cuda.synchronize()
        self.rate = n / (e0.elapsed_time(e1) * 1e3)            # _sleep cycles per microsecond
        self.sizes = {}
        _report(f'_sleep rate {self.rate:.1f} cycles/us ({n} cycles = {e0.elapsed_time(e1):.3f} ms)')

    def measure(self, key, run):
        """(short, long) sleep cycles for a subject: run() enqueues it once, unperturbed, and may be called repeatedly."""
        if key not in self.sizes:
            run()
            torch.cuda.synchronize()
            _lib.PROFILE = prof = []
            try:
                run()
                torch.cuda.synchronize()
            finally:
                _lib.PROFILE = None
            longest, name = max((e0.elapsed_time(e1) * 1e3, nm) for nm, _, _, e0, e1 in prof)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            dur = (time.perf_counter() - t0) * 1e6
            short, long_ = int(3 * longest * self.rate), int(2 * dur * self.rate)
            self.sizes[key] = (short, long_)
            _report(f'{key}: longest launch {longest:.1f} us ({name}), duration {dur:.0f} us, {len(prof)} launches -> '
                    f'short sleep {3 * longest:.0f} us = {short} cycles, long sleep {2 * dur:.0f} us = {long_} cycles')
        return self.sizes[key]


@pytest.fixture(scope='module')
def cal():
    t0 = time.perf_counter()
    yield _Cal()
    torch.cuda.synchronize()
    if QUEUED:
        _report(f'{len(QUEUED)} queued runs: {sum(q[0] == 1.0 for q in QUEUED)} enqueued wholly under their head sleeps; the least: '
                f'{[(t, p, round(q, 3)) for q, t, p in sorted(QUEUED)[:12]]}')
    _report(f'file wall time {time.perf_counter() - t0:.1f} s')


@pytest.fixture(scope='module')
def queues():
    """streams.py promises the chain and the weight-gradient stream hardware queues of their own; on a shared queue nothing can be
    reordered and every test here would pass vacuously."""
    chain, wgrad = streams.get('chain'), streams.get('wgrad')
    shared = streams.serialised(chain, wgrad) or streams.serialised(wgrad, chain)
    assert not shared, 'streams.serialised(chain, wgrad) is true: the two streams share a hardware queue, nothing can be reordered'
    return chain, wgrad


def _inputs(shape, seed=0, c=C):
    B, H, W = shape
    g = torch.Generator(device='cpu').manual_seed(seed)
    x1 = torch.randn(B, c, H, W, generator=g)
    x2 = x1 + 0.3 * torch.randn(B, c, H, W, generator=g)
    lbl = (torch.rand(B, H, W, generator=g) < 0.2).to(torch.uint8)
    return x1.cuda(), x2.cuda(), lbl.cuda()


@functools.lru_cache(maxsize=None)
def _filled(c):
    return filler.fill_module(BiDateNet(c, 2, precision='fp32'))


def _model(prec, c=C):
    """A fresh filled model (the fill takes a second on the host: one per band count, copied)."""
    model = copy.deepcopy(_filled(c))
    model.precision = prec
    return model.cuda().train()


def _P(model):
    return {k: v.detach() for k, v in model.state_dict(keep_vars=True).items()}


def _diff(got, ref):
    """Names of the entries of two {name: tensor} dicts that are not bit-equal."""
    assert got.keys() == ref.keys()
    return [k for k in ref if not torch.equal(got[k], ref[k])]


def _stream_patterns(trace, roles, queued=True):
    """lag and stall patterns for the streams of `roles` ({name: handle}) that the subject uses (trace: Perturb.trace of its natural
    run), stalls at the first, second and middle launch of each, plus the three seeded random patterns.  The natural schedule runs as it
    is and once more behind a head sleep (the streams start on full queues, as in a full-size step); every perturbed run is behind it too:
    at these shapes the host paces the launches otherwise, a stream that is delayed before every launch catches up between two of
    them, and whether a stall outlasts the other stream depends on how fast the host happens to enqueue.  queued=False: a subject that waits for the device itself, in front of which no queue can be formed."""
    pats = [ss.none()] + ([ss.none(queued=True)] if queued else [])
    for role, h in roles.items():
        n = sum(1 for _, s in trace if s == h)
        if n:
            pats.append(ss.lag(role, queued=queued))
            pats += [ss.stall(role, k, queued=queued) for k in sorted({0, min(1, n - 1), n // 2})]
    return pats + [ss.random(s, P_RANDOM, queued=queued) for s in SEEDS]


# ---------------------------------------------------------------------------------------------------------------- (a) engine.backward
VARIANTS = ['full', 'dx', 'frozen_encoder', 'frozen_middle', 'only_outc', 'running', 'twice']


class _Backward:
    """One forward, then engine.backward under any pattern on the same workspace (backward leaves the activations as they are)."""

    def __init__(self, prec, shape, variant, seed=0):
        self.prec, self.shape, self.variant = prec, shape, variant
        B, H, W = shape
        self.chain, self.wgrad = streams.get('chain'), streams.get('wgrad')
        self.model = _model(prec)
        self.eng, self.P = self.model.engine(), _P(self.model)
        x1, x2, _ = _inputs(shape, seed)
        self.running = variant == 'running'
        torch.cuda.synchronize()
        with torch.cuda.stream(self.chain):
            _, self.ws = self.eng.forward(x1, x2, self.P, training=not self.running, frozen=self.running)
        g = torch.Generator(device='cpu').manual_seed(seed + 5)
        self.dl = (torch.randn(B, 2, H, W, generator=g) * 1e-2).cuda()
        names = [k for k, _ in self.model.named_parameters()]
        by = {L.name: L for L in self.eng.layers}
        keys = lambda L: {f'{L.conv}.weight', f'{L.conv}.bias', f'{L.bn}.weight', f'{L.bn}.bias'}
        self.need = None
        if variant == 'frozen_encoder':
            self.need = {k for k in names if not k.startswith(('inc.', 'down'))}
        elif variant == 'frozen_middle':
            self.need = set(names) - keys(by['d2a'])
        elif variant == 'only_outc':
            self.need = {'outc.conv.weight', 'outc.conv.bias'}
        torch.cuda.synchronize()

    def prepare(self, dl=None):
        """Output buffers of one run, made and filled BEFORE the perturbation opens: nothing in enqueue() may wait for the device."""
        B, H, W = self.shape
        dl = self.dl if dl is None else dl
        fresh = lambda: {k: torch.full_like(p, 0.5, dtype=torch.float32) for k, p in self.model.named_parameters()}
        bufs = dict(dl=dl, grads=fresh(), chk=torch.zeros(40, dtype=torch.float64, device='cuda'),
                    dx=tuple(torch.full((B, C, H, W), 0.5, device='cuda') for _ in range(2)) if self.variant == 'dx' else None)
        if self.variant == 'twice':
            bufs.update(dl2=dl * 2.0, grads2=fresh())
        torch.cuda.synchronize()
        return bufs

    def enqueue(self, bufs):
        grads, chk, dx, n = bufs['grads'], bufs['chk'], bufs['dx'], [0]

        def on_ready(ks):
            # stands in for an all-reduce bucket: a checksum of the gradients it was handed, on the stream current at the call
            chk[n[0]].copy_(torch.stack([grads[k].double().sum() for k in ks]).sum())
            n[0] += 1
        with torch.cuda.stream(self.chain):
            self.eng.backward(self.ws, bufs['dl'], self.P, grads, on_ready=on_ready, dx=dx, need=self.need,
                              bn_mode='running' if self.running else 'batch')
            if self.variant == 'twice':          # the same workspace again without a host sync: hand-off events and the 'wgrad' scratch are reused
                self.eng.backward(self.ws, bufs['dl2'], self.P, bufs['grads2'])
        out = dict(grads, ready_checksums=chk, ready_calls=torch.tensor(n[0]))
        if dx is not None:
            out['dx1'], out['dx2'] = dx
        if self.variant == 'twice':
            out.update({f'second.{k}': v for k, v in bufs['grads2'].items()})
        return out

    def run(self, pattern, sizes, dl=None):
        bufs = self.prepare(dl)
        with ss.Perturb(pattern, *sizes, probe=('chain', 'wgrad'), head=2 * sizes[1], head_roles=('chain', 'wgrad')) as h:
            out = self.enqueue(bufs)
        torch.cuda.synchronize()
        _assert_queued(pattern, h)
        return out, h


QUEUED = []          # per queued run: fraction of the subject's launches that were enqueued while the head sleeps still ran


def _assert_queued(pat, h):
    """A queued run really started from queues: the head sleeps were still running when the subject's first launch was enqueued (a host
    synchronisation in front of it would have waited them out).  How much of the subject was enqueued under the head is reported."""
    if pat.queued:
        assert h.queued and h.queued[0], f'{pat}: the head sleep was over before the first launch was enqueued'
        QUEUED.append((sum(h.queued) / len(h.queued), os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1].split(' ')[0], repr(pat)))


def _assert_moved(pat, h, roles):
    """The effectiveness condition of a lag / stall run of engine.backward; returns the margin it was met by in microseconds."""
    assert h.log, f'{pat}: delayed nothing'
    if pat.role == 'wgrad':
        lag_us = max(h.join_lag_us(i) for i in range(len(h.joins)))          # the join the chain had to wait longest at (two passes: either's)
        assert lag_us > 0, f'{pat}: the second stream finished {-lag_us:.0f} us BEFORE the chain reached its join: the perturbation did not move the schedule'
        return lag_us
    else:
        idle = h.idle_before_launch()
        if pat.kind == 'stall':
            idle = [(n, us) for n, us in idle if n > pat.k][:1]          # the first hand-off behind the stall
        else:
            idle = idle[1:]                                               # (at the first one the second stream has had nothing to do yet)
        assert idle, f'{pat}: no hand-off behind the perturbation'
        busy = [(n, round(us)) for n, us in idle if us < 0]
        assert not busy, f'{pat}: the second stream was still busy at the hand-offs (chain launches before it, us): {busy}: the perturbation did not move the schedule'
        return min(us for _, us in idle)


def _check_paths(eng, shape):
    """The paths under test are taken at this shape (the engine's own predicates)."""
    B, H, W = shape
    by = {L.name: L for L in eng.layers}
    if eng.precision in ('bf16', 'bf16x3', 'bf16x3-fast'):
        assert eng.first_wgrad_dtype(2 * B, H, W, B) is not None, f'first-layer fused weight gradient not taken at {shape}'
    if eng.precision == 'bf16':
        assert eng.folds_bn_bwd(by['e1b'], H, W) and eng.folds_bn_bwd(by['d4a'], H, W), f'BatchNorm-backward fold not taken at {shape}'
    if eng.x3:
        assert eng.x3_src_f32 is True, 'the bf16x3 float32-source convolutions are off'


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('prec', ['fp32', 'bf16', 'bf16x3', 'bf16x3-fast'])
def test_backward_bits_do_not_depend_on_stream_timing(cal, queues, prec, variant):
    shapes = [MAIN, ODD] if variant in ('full', 'dx') else [MAIN]
    for shape in shapes:
        sub = _Backward(prec, shape, variant)
        _check_paths(sub.eng, shape)
        sizes = cal.measure(f'backward {prec} {variant} {shape}', lambda: sub.enqueue(sub.prepare()))
        ref, _ = sub.run(ss.sync(), sizes)
        nat, h0 = sub.run(ss.none(), sizes)
        roles = {'wgrad': sub.wgrad.cuda_stream, 'chain': sub.chain.cuda_stream}
        if variant == 'full' and shape == MAIN:
            assert any(s == roles['wgrad'] for _, s in h0.trace) and h0.handoffs, 'no weight gradient ran on the second stream'
        pats = _stream_patterns(h0.trace, roles)
        if h0.handoffs:                          # a stall right behind the first hand-off to the second queue, and one at the first encoder layer
            chain_trace = [nm for nm, s in h0.trace if s == roles['chain']]
            ks = {h0.handoffs[0][0]}
            if 'bdn_enc_skip_bwd' in chain_trace:
                ks.add(chain_trace.index('bdn_enc_skip_bwd'))
            have = {(p.role, p.k) for p in pats if p.kind == 'stall'}
            pats += [ss.stall('chain', k, queued=True) for k in sorted(ks) if ('chain', k) not in have]
        bad, margins = {}, {}
        d = _diff(nat, ref)
        if d:
            bad['none'] = d
        for pat in pats[1:]:
            got, h = sub.run(pat, sizes)
            if pat.kind == 'random':
                pass
            elif pat.role == 'wgrad' or (pat.kind == 'lag' and len(h.handoffs) > 1) or (pat.kind == 'stall' and any(n > pat.k for n, _, _ in h.handoffs)):
                margins[repr(pat)] = round(_assert_moved(pat, h, roles))           # (a chain perturbation behind the last hand-off has no second-stream launch to move)
            d = _diff(got, ref)
            if d:
                bad[repr(pat)] = d
        _report(f'backward {prec} {variant} {shape}: schedule moved by (us) {margins}')
        assert not bad, f'{prec} {variant} {shape}: results differ from the synchronised run under {bad}'
        assert int(ref['ready_calls']) > 0 and torch.isfinite(ref['ready_checksums']).all()
        del sub
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- (b) TrainStep
STEP_CASES = {
    'sgd-bf16': dict(prec='bf16', kw=dict(optimizer='sgd', momentum=0.9)),
    'adamw-bf16': dict(prec='bf16', kw=dict(optimizer='adamw')),
    'sgd-bf16x3': dict(prec='bf16x3', kw=dict(optimizer='sgd', momentum=0.9)),
    'adamw-bf16x3': dict(prec='bf16x3', kw=dict(optimizer='adamw')),
    'groups-frozen-stem-frozen-bn': dict(prec='bf16', kw=dict(optimizer='adamw', bn='frozen'), groups=True),
    'focal+dice': dict(prec='bf16', kw=dict(optimizer='sgd', criterion='focal+dice')),
    'two-shapes': dict(prec='bf16x3', kw=dict(optimizer='sgd', momentum=0.9), alternate=True),
}


class _Steps:
    """Four consecutive steps with no host sync between them, on one model whose state is put back before every run."""

    def __init__(self, case, on_chain, n_steps=4):
        cfg = STEP_CASES[case]
        self.cfg, self.on_chain, self.n_steps = cfg, on_chain, n_steps
        self.model = _model(cfg['prec'])
        if cfg.get('groups'):
            for k, p in self.model.named_parameters():
                if k.startswith('inc.'):
                    p.requires_grad_(False)                      # a frozen stem: the chain ends early
        self.sd0 = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        self.batches = [_inputs(MAIN, 0), _inputs(ODD if cfg.get('alternate') else MAIN, 1)]
        torch.cuda.synchronize()

    def prepare(self):
        """The model back at its first state and a new TrainStep on it, BEFORE the perturbation opens."""
        self.model.load_state_dict(self.sd0)
        self.model.train()
        kw = dict(self.cfg['kw'])
        if 'criterion' in kw:
            from fabric_amd.criterion import Criterion
            kw['criterion'] = Criterion.parse(kw['criterion'], focal_gamma=2.0)
        if self.cfg.get('groups'):
            names = [k for k, p in self.model.named_parameters() if p.requires_grad]
            kw['param_groups'] = [{'params': [k for k in names if k.endswith('.bias') or '.1.' in k or '.4.' in k], 'lr': 2e-3, 'weight_decay': 0.0},
                                  {'params': [k for k in names if not (k.endswith('.bias') or '.1.' in k or '.4.' in k)], 'weight_decay': 1e-2}]
        ts = TrainStep(self.model, lr=1e-2, distributed=False, **kw)
        # the parameters moved into the step's flat buffer: the engine uploads its packing descriptor for the new addresses with a blocking
        # copy (once per re-pointing, in a real run inside the first step), which would wait the head sleeps out
        eng = self.model.engine()
        eng._check_packed(ts._P)
        eng._weights(eng.layers[0], ts._P, False)
        torch.cuda.synchronize()
        return ts

    def enqueue(self, ts):
        order = [0, 1, 0, 0] if self.cfg.get('alternate') else [0, 0, 1, 0]
        losses = []
        ctx = torch.cuda.stream(ts.stream()) if self.on_chain else torch.cuda.stream(torch.cuda.default_stream())
        with ctx:
            for i, b in enumerate(order[:self.n_steps]):
                losses.append(ts.step(*self.batches[b]))
                if self.cfg.get('alternate') and i == 1:
                    self.model.eval()                            # drops the bf16x3 split buffers (release_split) the last GEMMs may still read
                    self.model.train()
            out = {'losses': torch.stack(losses), 'last_logits': ts.last_logits.clone(), 'last_counts': ts.last_counts.clone()}
        return out

    def run(self, pattern, sizes):
        ts = self.prepare()
        with ss.Perturb(pattern, *sizes, head=2 * sizes[1], head_roles=('chain', 'wgrad') + (() if self.on_chain else (0,))) as h:
            out = self.enqueue(ts)
        torch.cuda.synchronize()
        _assert_queued(pattern, h)
        out['flat_params'] = ts.flat_params.clone()
        out.update({f'state.{k}': v.detach().clone() for k, v in self.model.state_dict().items()})
        out.update({f'opt.{k}': v.clone() for k, v in ts.opt_state.items()})
        out['opt_step'] = torch.tensor(ts.opt_step)
        torch.cuda.synchronize()
        return out, h


@pytest.mark.parametrize('on_chain', [False, True], ids=['default-stream', 'chain-stream'])
@pytest.mark.parametrize('case', list(STEP_CASES))
def test_train_step_bits_do_not_depend_on_stream_timing(cal, queues, case, on_chain):
    sub = _Steps(case, on_chain)
    if case in ('sgd-bf16', 'sgd-bf16x3'):
        _check_paths(sub.model.engine(), MAIN)
    sizes = cal.measure(f'step {case} {"chain" if on_chain else "default"}', lambda: sub.enqueue(sub.prepare()))
    ref, _ = sub.run(ss.sync(), sizes)
    nat, h0 = sub.run(ss.none(), sizes)
    roles = {'wgrad': queues[1].cuda_stream, 'chain': queues[0].cuda_stream}
    assert {s for _, s in h0.trace} >= set(roles.values()), 'the step did not use both of its streams'
    bad = {}
    d = _diff(nat, ref)
    if d:
        bad['none'] = d
    for pat in _stream_patterns(h0.trace, roles)[1:]:
        got, h = sub.run(pat, sizes)
        assert pat.kind in ('none', 'random') or h.log, f'{pat}: delayed nothing'
        d = _diff(got, ref)
        if d:
            bad[repr(pat)] = d
    assert not bad, f'{case}: results differ from the synchronised run under {bad}'
    assert torch.isfinite(ref['losses']).all() and torch.isfinite(ref['flat_params']).all()


# ---------------------------------------------------------------------------------------------------------------- (c) the autograd route
def _tversky(logits, labels, alpha=0.1, beta=0.9, eps=1e-7):
    one_hot = torch.eye(2, device=logits.device, dtype=logits.dtype)[labels.long()].permute(0, 3, 1, 2)
    probas = torch.softmax(logits, dim=1)
    inter = torch.sum(probas * one_hot, (0, 2))
    fps = torch.sum(probas * (1 - one_hot), (0, 2))
    fns = torch.sum((1 - probas) * one_hot, (0, 2))
    return 1 - (inter / (inter + alpha * fps + beta * fns + eps)).mean()


def _autograd(model, sd0, scenario, batches):
    """One scenario of the autograd route on the caller's (default) stream; returns every gradient it produced."""
    model.load_state_dict(sd0)
    model.train()
    model.zero_grad(set_to_none=True)
    (x1, x2, lbl), (y1, y2, lbl2) = batches
    out = {}
    a1, a2 = x1.clone().requires_grad_(), x2.clone().requires_grad_()
    if scenario == 'input-grads':
        _tversky(model(a1, a2), lbl).backward()
    elif scenario == 'two-forwards':                 # the second forward finds the workspace leased and takes its own
        b1 = y1.clone().requires_grad_()
        la = _tversky(model(a1, a2), lbl)
        lb = _tversky(model(b1, y2), lbl2)
        (la + lb).backward()
        out['b1.grad'] = b1.grad
    else:                                            # an eval-mode forward + backward between a training forward and its backward
        loss = _tversky(model(a1, a2), lbl)
        model.eval()
        xe = y1.clone().requires_grad_()
        _tversky(model(xe, y2), lbl2).backward()
        out['eval.x.grad'] = xe.grad
        out.update({f'eval.{k}': p.grad.clone() for k, p in model.named_parameters()})
        model.zero_grad(set_to_none=True)
        model.train()
        loss.backward()
    out['x1.grad'], out['x2.grad'] = a1.grad, a2.grad
    out.update({k: p.grad for k, p in model.named_parameters()})
    out.update({f'buf.{k}': v.clone() for k, v in model.state_dict().items() if 'running_' in k})
    return out


@pytest.mark.parametrize('scenario', ['input-grads', 'two-forwards', 'eval-backward-between'])
@pytest.mark.parametrize('prec', ['bf16', 'bf16x3'])
def test_autograd_route_bits_do_not_depend_on_stream_timing(cal, queues, prec, scenario):
    model = _model(prec)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batches = [_inputs(MAIN, 0), _inputs(MAIN, 1)]
    torch.cuda.synchronize()
    sizes = cal.measure(f'autograd {prec} {scenario}', lambda: _autograd(model, sd0, scenario, batches))

    def run(pat):
        torch.cuda.synchronize()
        with ss.Perturb(pat, *sizes, head=2 * sizes[1], head_roles=(0, 'wgrad')) as h:
            out = _autograd(model, sd0, scenario, batches)
        torch.cuda.synchronize()
        _assert_queued(pat, h)
        return {k: v.clone() for k, v in out.items()}, h
    ref, _ = run(ss.sync())
    nat, h0 = run(ss.none())
    roles = {'wgrad': queues[1].cuda_stream, 0: 0}                # the caller's stream here is the default stream
    assert {s for _, s in h0.trace} == {0, roles['wgrad']}
    bad = {}
    if _diff(nat, ref):
        bad['none'] = _diff(nat, ref)
    for pat in _stream_patterns(h0.trace, roles)[1:]:
        got, h = run(pat)
        assert pat.kind in ('none', 'random') or h.log, f'{pat}: delayed nothing'
        if _diff(got, ref):
            bad[repr(pat)] = _diff(got, ref)
    assert not bad, f'{prec} {scenario}: results differ from the synchronised run under {bad}'
    assert ref['x1.grad'].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------- (d) scene inference
def _scene(c, h, w, seed):
    r = np.random.default_rng(seed)
    d1 = r.standard_normal((c, h, w)).astype(np.float32)
    d2 = (d1 + 0.5 * r.standard_normal((c, h, w))).astype(np.float32)
    d2[:, h // 4:h // 2, w // 3:w // 2] += 2.0
    return d1, d2


@functools.lru_cache(maxsize=None)
def _scene_state(c, h, w, p, seed):
    """As tests/test_gpu_scene.py calibrates its model: running statistics that have seen the scene, so the mask has both classes."""
    d1, d2 = _scene(c, h, w, seed)
    model = _model('fp32', c)
    t1 = torch.from_numpy(np.ascontiguousarray(inf._get_patches(d1.transpose(1, 2, 0), p)[0].transpose(0, 3, 1, 2))).cuda()
    t2 = torch.from_numpy(np.ascontiguousarray(inf._get_patches(d2.transpose(1, 2, 0), p)[0].transpose(0, 3, 1, 2))).cuda()
    with torch.no_grad():
        for _ in range(25):
            model(t1, t2)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize('bs', [5, 64])
@pytest.mark.parametrize('blended', [False, True], ids=['mask', 'blended'])
@pytest.mark.parametrize('prec', ['bf16', 'bf16x3'])
def test_scene_inference_bits_do_not_depend_on_stream_timing(cal, queues, prec, blended, bs):
    c, h, w, p = 3, 88, 75, 32
    d1, d2 = _scene(c, h, w, 3)
    model = _model(prec, c)
    model.load_state_dict(_scene_state(c, h, w, p, 3))
    model.eval()
    t1, t2 = torch.from_numpy(d1).pin_memory(), torch.from_numpy(d2).pin_memory()       # host scenes: the band feeder and both copy streams run

    def scan(two):
        if blended:
            proba, mask = inf.predict_scene_blended(model, t1, t2, patch_size=p, stride=16, batch_size=bs, band_rows=32, two_streams=two)
            return {'proba': proba, 'mask': mask}
        return {'mask': inf.predict_scene(model, t1, t2, patch_size=p, batch_size=bs, band_rows=32, two_streams=two)}
    torch.cuda.synchronize()
    sizes = cal.measure(f'scene {prec} {"blended" if blended else "mask"} bs={bs}', lambda: scan(True))

    def run(pat, two=True):
        torch.cuda.synchronize()
        with ss.Perturb(pat, *sizes) as hh:
            out = scan(two)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}, hh
    ref, _ = run(ss.sync(), two=False)                              # the ground truth is the synchronised single-lane scan
    nat, h0 = run(ss.none())
    roles = {0: 0, 'wgrad': queues[1].cuda_stream, 'copy': streams.get('copy').cuda_stream, 'copy2': streams.get('copy2').cuda_stream}
    used = {s for _, s in h0.trace}
    assert roles['copy'] in used and roles['copy2'] in used, 'the band feeder did not run on the copy streams'
    n_img = len(inf.blend_tile_origins(h, w, p, 16)[0]) if blended else len(inf.tile_origins(h, w, p)[0])
    assert (roles['wgrad'] in used) == (n_img > bs), 'the second lane runs exactly when there is more than one batch'
    bad = {}
    if _diff(nat, ref):
        bad['none'] = _diff(nat, ref)
    # not queued: the scan uploads its tile origins with a blocking copy, i.e. it waits for its own stream before its first launch
    for pat in _stream_patterns(h0.trace, roles, queued=False)[1:]:
        got, hh = run(pat)
        assert pat.kind in ('none', 'random') or hh.log, f'{pat}: delayed nothing'
        if _diff(got, ref):
            bad[repr(pat)] = _diff(got, ref)
    assert not bad, f'{prec} bs={bs}: results differ from the synchronised single-lane scan under {bad}'
    assert 0.02 < ref['mask'].float().mean().item() < 0.98, 'degenerate scene: the mask has a single class'


# ---------------------------------------------------------------------------------------------------------------- (e) feeder, device loader
@pytest.mark.parametrize('depth', [2, 3])
def test_feeder_batches_do_not_depend_on_copy_stream_timing(cal, depth):
    """DeviceFeeder's copies are torch copies on the 'copy' stream, not library launches: the same sleeps are enqueued on that stream
    from the batch source, i.e. right before the feeder issues the copies of a batch (the existing test lags only the consumer)."""
    from fabric_amd.input_pipeline import DeviceFeeder
    n, shape = 9, (4, C, 32, 32)
    g = torch.Generator().manual_seed(3)
    host = [(torch.randn(shape, generator=g).pin_memory(), torch.randn(shape, generator=g).pin_memory(),
             torch.randint(0, 2, (4, 32, 32), generator=g, dtype=torch.uint8).pin_memory()) for _ in range(n)]
    copy = streams.get('copy').cuda_stream
    feeder = DeviceFeeder('cuda', depth=depth, stage_threads=1)

    def feed(delays):
        """delays: {batch index: cycles slept on the copy stream before the batch is issued}; the consumer reads every batch late too."""
        def source():
            for i, b in enumerate(host):
                if delays.get(i):
                    ss.device_sleep(copy, delays[i])
                yield b
        got = []
        cons = streams.get('chain')
        with torch.cuda.stream(cons):
            for a, b, y in feeder(source()):
                if delays.get('consumer'):
                    ss.device_sleep(cons.cuda_stream, delays['consumer'])
                got.append((a.clone(), b.clone(), y.clone()))
        torch.cuda.synchronize()
        return got
    feed({})                                      # (the first pass allocates the slots)
    t0 = time.perf_counter()
    feed({})
    dur = (time.perf_counter() - t0) * 1e6
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(streams.get('copy')):
        e0.record()
        d = host[0][0].cuda(non_blocking=True)
        e1.record()
    torch.cuda.synchronize()
    short, long_ = int(3 * e0.elapsed_time(e1) * 1e3 * cal.rate), int(2 * dur * cal.rate)
    _report(f'feeder depth {depth}: one copy {e0.elapsed_time(e1) * 1e3:.0f} us, pass {dur:.0f} us -> short {short} long {long_} cycles')
    rng = pyrandom.Random(5)
    cases = {'none': {}, "lag('copy')": {i: short for i in range(n)}, "stall('copy', 0)": {0: long_}, "stall('copy', 4)": {4: long_},
             'consumer+copy': dict({i: short for i in range(n) if rng.random() < 0.5}, consumer=short)}
    bad = []
    for name, delays in cases.items():
        got = feed(delays)
        assert len(got) == n
        bad += [(name, k) for k in range(n) for t, r in zip(got[k], host[k]) if not torch.equal(t.cpu(), r)]
    assert not bad, f'batches arrived damaged: {bad}'
    feeder.close()
    del d


def test_device_loader_batches_do_not_depend_on_stream_timing(cal):
    """make_device_loaders promises the host loader's batches bit for bit; its launch (descriptors through a pinned ring of `depth` slots)
    runs on the consumer's stream, which is perturbed here while the host runs ahead."""
    from fabric_amd.train import make_device_loaders, make_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    data = synthetic_onera(n_cities=3, bands=C, size=(100, 90), seed=2)
    bs, S, stride = 5, 32, 16
    pyrandom.seed(3)
    h_tr, _ = make_loaders(data, ['city2'], S, stride, bs, True, num_workers=0, seed=9)
    pyrandom.seed(3)
    d_tr, _ = make_device_loaders(data, ['city2'], S, stride, bs, True, seed=9)
    pyrandom.seed(100)
    want = [tuple(t.clone() for t in b) for b in h_tr]
    assert len(want) > 3 + 2, 'fewer batches than exercise the reuse of the three ring slots'
    cons = streams.get('chain')

    def epoch():
        pyrandom.seed(100)
        with torch.cuda.stream(cons):
            return [tuple(t.clone() for t in b) for b in d_tr]
    torch.cuda.synchronize()
    sizes = cal.measure('device loader epoch', epoch)
    bad = []
    for pat in [ss.sync(), ss.none(), ss.none(queued=True), ss.lag('chain', queued=True), ss.stall('chain', 0, queued=True), ss.stall('chain', 3, queued=True)] + \
            [ss.random(s, P_RANDOM, queued=True) for s in SEEDS]:
        torch.cuda.synchronize()
        with ss.Perturb(pat, *sizes, head=2 * sizes[1], head_roles=('chain',)) as h:
            got = epoch()
        torch.cuda.synchronize()
        _assert_queued(pat, h)
        assert pat.kind in ('sync', 'none', 'random') or h.log, f'{pat}: delayed nothing'
        assert len(got) == len(want)
        bad += [(repr(pat), k) for k in range(len(want)) for t, r in zip(got[k], want[k])
                if not torch.equal(t.cpu().view(torch.uint8), r.contiguous().view(torch.uint8))]
    assert not bad, f'device batches differ from the host loader\'s: {bad}'


# ---------------------------------------------------------------------------------------------------------------- the tests can fail
def test_mutant_a_weight_gradient_without_its_wait_is_caught(cal, queues, monkeypatch):
    """Mutant A: hand-off waits whose destination is the weight-gradient stream do nothing, so a GEMM no longer waits for its dz.  A
    chain-lagging pattern must then change some gradient.  The gradient seed is one no earlier run used: a GEMM that runs too early
    reads what an earlier pass left in the buffer, which after an identical pass would be the right values."""
    chain, wgrad = queues
    sub = _Backward('bf16', MAIN, 'full')
    sizes = cal.measure(f'backward bf16 full {MAIN}', lambda: sub.enqueue(sub.prepare()))
    g = torch.Generator(device='cpu').manual_seed(77)
    dl = (torch.randn(sub.dl.shape, generator=g) * 1e-2).cuda()
    _, h0 = sub.run(ss.none(), sizes)
    first = h0.handoffs[0][0]
    pats = [ss.lag('chain', queued=True), ss.stall('chain', first, queued=True), ss.stall('chain', 0, queued=True)]
    real = streams.HandOff.wait
    caught = {}
    for i, pat in enumerate(pats):
        dl_i = dl * float(2 ** i)                 # never the values the previous pass left behind
        monkeypatch.setattr(streams.HandOff, 'wait', lambda self, dst: None if dst.cuda_stream == wgrad.cuda_stream else real(self, dst))
        try:
            got, _ = sub.run(pat, sizes, dl_i)
        finally:
            monkeypatch.setattr(streams.HandOff, 'wait', real)
        ref, _ = sub.run(ss.sync(), sizes, dl_i)
        d = _diff(got, ref)
        if d:
            caught[repr(pat)] = len(d)
    torch.cuda.synchronize()
    del sub
    _report(f'mutant A (no wait in front of the weight-gradient GEMMs) caught by {caught}')
    assert caught, f'mutant A was caught by none of {pats}: the chain-lagging patterns are too weak'


def test_mutant_b_step_without_its_final_join_is_caught(cal, queues, monkeypatch):
    """Mutant B: hand-off waits whose destination is the chain's stream do nothing, so the final join of backward is gone and the
    optimizer update no longer waits for the weight gradients.  A pattern that makes the weight-gradient stream lag must then change
    the result of two back-to-back steps."""
    chain, wgrad = queues
    sub = _Steps('sgd-bf16', True, n_steps=2)
    sizes = cal.measure('step sgd-bf16 chain 2 steps', lambda: sub.enqueue(sub.prepare()))
    ref, h0 = sub.run(ss.sync(), sizes)
    n = sum(1 for _, s in h0.trace if s == wgrad.cuda_stream)
    pats = [ss.lag('wgrad', queued=True), ss.stall('wgrad', 0, queued=True), ss.stall('wgrad', n // 4, queued=True)]
    real = streams.HandOff.wait
    caught = {}
    for pat in pats:
        monkeypatch.setattr(streams.HandOff, 'wait', lambda self, dst: None if dst.cuda_stream == chain.cuda_stream else real(self, dst))
        try:
            got, _ = sub.run(pat, sizes)
        finally:
            monkeypatch.setattr(streams.HandOff, 'wait', real)
        d = _diff(got, ref)
        if d:
            caught[repr(pat)] = len(d)
    torch.cuda.synchronize()
    del sub
    _report(f'mutant B (no final join behind the weight-gradient stream) caught by {caught}')
    assert caught, f'mutant B was caught by none of {pats}: the wgrad-lagging patterns are too weak'
