"""-m gpu: the fused step's momentum SGD / Adam / AdamW (include/bidate_hip.h bdn_sgd_momentum_step, bdn_adam_step; fabric_amd/optim.py).

Kernels against the float64 restatement (tests/optim_ref.py, pinned against CPU torch.optim in tests/test_optim_cpu.py); TrainStep against
CUDA torch.optim on the step's own gradients; state interchange with torch.optim in both directions; the default rule unchanged; a short
AdamW trajectory against the autograd route; data parallel; train.py's --optimizer / --resume."""
import os
import subprocess
import sys

import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.metrics import TverskyLoss
from oracle import filler
from tests import optim_ref as R
from tests import guard
from tests.guard import guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)


# ---------------------------------------------------------------- kernels against the float64 restatement
_KERNEL_CASES = [
    ('sgd_m', dict(kind='sgd', momentum=0.9), 1.0),
    ('sgd_m_damp', dict(kind='sgd', momentum=0.9, dampening=0.1), 0.5),
    ('sgd_nesterov', dict(kind='sgd', momentum=0.9, nesterov=True), 1.0),
    ('sgd_nesterov_wd', dict(kind='sgd', momentum=0.9, nesterov=True, weight_decay=1e-2), 0.5),
    ('sgd_m_wd', dict(kind='sgd', momentum=0.8, weight_decay=1e-2), 1.0),
    ('sgd_wd_only', dict(kind='sgd', weight_decay=1e-2), 0.5),
    ('adam', dict(kind='adam'), 1.0),
    ('adam_l2', dict(kind='adam', weight_decay=1e-2), 0.5),
    ('adamw', dict(kind='adamw', weight_decay=1e-2), 1.0),
    ('adamw_gs', dict(kind='adamw', weight_decay=1e-2, betas=(0.8, 0.99)), 0.5),
]
_SIZES = [1, 3, 4, 1023, 4_000_003]
_LR = 0.01


def _run_kernel(case, gs, p, grads, state):
    """len(grads) steps of the kernel on p / state in place; returns the per-step (inputs, outputs) for checking."""
    st = _lib.stream_ptr()
    n = p.numel()
    hist = []
    for it, g in enumerate(grads):
        before = (p.clone(), {k: v.clone() for k, v in state.items()})
        if case['kind'] == 'sgd':
            buf = state.get('buf')
            _lib.call('bdn_sgd_momentum_step', p.data_ptr(), g.data_ptr(), _lib.ptr(buf), _LR, gs, case.get('momentum', 0.0),
                      case.get('dampening', 0.0), case.get('weight_decay', 0.0), int(case.get('nesterov', False)), int(it == 0), n, st)
        else:
            b1, b2 = case.get('betas', (0.9, 0.999))
            _lib.call('bdn_adam_step', p.data_ptr(), g.data_ptr(), state['m'].data_ptr(), state['v'].data_ptr(), _LR, gs, b1, b2, 1e-8,
                      case.get('weight_decay', 0.0), int(case['kind'] == 'adamw'), it + 1, n, st)
        hist.append((before, p.clone(), {k: v.clone() for k, v in state.items()}))
    return hist


@pytest.mark.parametrize('n', _SIZES)
@pytest.mark.parametrize('name,case,gs', _KERNEL_CASES, ids=[c[0] for c in _KERNEL_CASES])
@guarded
def test_update_kernel_matches_float64_restatement(name, case, gs, n):
    """Three steps (the first-step momentum branch and two after it), each checked from the kernel's own float32 inputs: every element
    of the parameters and the state within R.ULPS float32 epsilons of the magnitude R computes (at least max(|p|, |dp|)).  A repeat of the
    whole run from the same inputs is bit-identical."""
    gen = torch.Generator(device='cpu').manual_seed(n * 31 + len(name))
    p0 = guard.guard(torch.randn(n, generator=gen), dev)
    p0[::7] *= 1e-3                                           # parameters much smaller than their update
    grads = [guard.guard(torch.randn(n, generator=gen) * (0.3 + it), dev) for it in range(3)]
    grads[1][::5] = 0.0                                       # zero gradients: Adam's m / (sqrt(v) + eps) with a decayed m
    runs = []
    for _ in range(2):
        p = guard.clone(p0)
        if case['kind'] == 'sgd':
            state = {'buf': guard.full((n,), float('nan'), device=dev)} if case.get('momentum', 0.0) else {}   # first step must not read it
        else:
            state = {'m': guard.zeros(n, device=dev), 'v': guard.zeros(n, device=dev)}
        runs.append(_run_kernel(case, gs, p, grads, state))
    torch.cuda.synchronize()
    for it, ((p_in, s_in), p_out, s_out) in enumerate(runs[0]):
        g = grads[it]
        if case['kind'] == 'sgd':
            rp, rb, mp, mb = R.sgd(p_in, g, s_in.get('buf'), _LR, gs, case.get('momentum', 0.0), case.get('dampening', 0.0),
                                   case.get('weight_decay', 0.0), case.get('nesterov', False), first=it == 0)
            if rb is not None:
                R.check(s_out['buf'], rb, mb, f'{name} n={n} step {it} momentum_buffer')
        else:
            rp, rm, rv, mp, mm, mv = R.adam(p_in, g, s_in['m'], s_in['v'], it + 1, _LR, gs, case.get('betas', (0.9, 0.999)), 1e-8,
                                            case.get('weight_decay', 0.0), case['kind'] == 'adamw')
            R.check(s_out['m'], rm, mm, f'{name} n={n} step {it} exp_avg')
            R.check(s_out['v'], rv, mv, f'{name} n={n} step {it} exp_avg_sq')
        R.check(p_out, rp, mp, f'{name} n={n} step {it} params')
        assert bool((p_out != p_in).any()), 'the step changed nothing'
    for (_, pa, sa), (_, pb, sb) in zip(*runs):
        assert torch.equal(pa, pb) and all(torch.equal(sa[k], sb[k]) for k in sa), 'repeat run differs'


# ---------------------------------------------------------------- TrainStep against CUDA torch.optim on the step's gradients
def _inputs(b=4, c=3, s=32, seed=3):
    return tuple(torch.from_numpy(v).to(dev) for v in filler.make_inputs(b, c, s, seed=seed))


_RULES = [
    ('sgd_nesterov_wd', dict(optimizer='sgd', momentum=0.9, nesterov=True, weight_decay=1e-2),
     lambda ps, lr: torch.optim.SGD(ps, lr=lr, momentum=0.9, nesterov=True, weight_decay=1e-2, foreach=False)),
    ('sgd_m_damp', dict(optimizer='sgd', momentum=0.9, dampening=0.1),
     lambda ps, lr: torch.optim.SGD(ps, lr=lr, momentum=0.9, dampening=0.1, foreach=False)),
    ('adam', dict(optimizer='adam', weight_decay=1e-3),
     lambda ps, lr: torch.optim.Adam(ps, lr=lr, weight_decay=1e-3, foreach=False)),
    ('adamw', dict(optimizer='adamw'),
     lambda ps, lr: torch.optim.AdamW(ps, lr=lr, foreach=False)),
]


def _bound(opt, q, grads, lr, it):
    """R's magnitude of this step for every parameter, from torch's pre-step state (q: pre-step parameters)."""
    g0 = opt.param_groups[0]
    mags = []
    for p, g in zip(q, grads):
        s = opt.state.get(p, {})
        if 'betas' in g0:
            m = s.get('exp_avg', torch.zeros_like(p))
            v = s.get('exp_avg_sq', torch.zeros_like(p))
            mags.append(R.adam(p.detach(), g, m, v, it + 1, lr, 1.0, g0['betas'], g0['eps'], g0['weight_decay'],
                               g0['decoupled_weight_decay'])[3])
        else:
            mags.append(R.sgd(p.detach(), g, s.get('momentum_buffer'), lr, 1.0, g0['momentum'], g0['dampening'], g0['weight_decay'],
                              g0['nesterov'], first='momentum_buffer' not in s)[2])
    return mags


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('name,kw,make', _RULES, ids=[r[0] for r in _RULES])
def test_train_step_matches_torch_optim_on_its_own_gradients(name, kw, make, prec):
    """Four steps: CUDA torch.optim (foreach=False) applied to clones of the pre-step parameters, in model.parameters() order, with the
    step's own flat_grads, gives the fused step's post-step parameters within twice the kernel bound (two float32 evaluations of the
    same exact value).  Pins layout, order, state, step count and grad scale without the gradients' own sensitivity."""
    lr = 5e-3
    model = filler.fill_module(BiDateNet(3, 2, precision=prec)).to(dev).train()
    ts = TrainStep(model, lr=lr, **kw)
    names = [k for k, _ in model.named_parameters()]
    q = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    opt = make(q, lr)
    x1, x2, lbl = _inputs()
    for it in range(4):
        with torch.no_grad():
            for a, p in zip(q, model.parameters()):
                a.copy_(p)
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        grads = [ts.grads[k].clone() for k in names]
        mags = _bound(opt, q, grads, lr, it)
        for a, g in zip(q, grads):
            a.grad = g
        opt.step()
        for k, a, p, mg in zip(names, q, model.parameters(), mags):
            R.check(p, a.detach(), mg, f'{name} {prec} step {it} {k}', ulps=2 * R.ULPS)
    assert ts.opt_step == 4
    sd = ts.optimizer_state_dict()
    for i, a in enumerate(q):
        for key, v in opt.state[a].items():
            if key == 'step':
                assert float(sd['state'][i]['step']) == float(v) == 4.0
            else:
                assert torch.allclose(sd['state'][i][key], v, rtol=1e-4, atol=1e-7), (i, key)


# ---------------------------------------------------------------- torch.optim <-> TrainStep state interchange
def _autograd_step(model, opt, x1, x2, lbl):
    crit = TverskyLoss(alpha=0.1, beta=0.9)
    opt.zero_grad()
    loss = crit(model(x1, x2), lbl.long())
    loss.backward()
    opt.step()
    model.engine().invalidate_weights()
    return float(loss.detach())


def test_torch_adam_state_continues_in_the_fused_step():
    """Adam state from 3 autograd-route steps loads into TrainStep; its fused 4th step equals torch's 4th step on the same gradients."""
    lr = 2e-3
    model = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-3, foreach=False)
    x1, x2, lbl = _inputs()
    for _ in range(3):
        _autograd_step(model, opt, x1, x2, lbl)
    sd = opt.state_dict()
    ts = TrainStep(model, lr=0.5, optimizer='adam', weight_decay=0.0)        # the saved group's lr and weight decay must be adopted
    ts.load_optimizer_state_dict(sd)
    assert ts.lr == lr and ts.optim.weight_decay == 1e-3 and ts.opt_step == 3
    names = [k for k, _ in model.named_parameters()]
    q = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    ref = torch.optim.Adam(q, lr=1.0, foreach=False)
    ref.load_state_dict(sd)
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    grads = [ts.grads[k].clone() for k in names]
    mags = _bound(ref, q, grads, lr, 3)
    for a, g in zip(q, grads):
        a.grad = g
    ref.step()
    for k, a, p, mg in zip(names, q, model.parameters(), mags):
        R.check(p, a.detach(), mg, f'4th step {k}', ulps=2 * R.ULPS)
    assert float(ref.state[q[0]]['step']) == 4 and ts.opt_step == 4
    # a state of the other family is refused
    with pytest.raises(ValueError):
        ts.load_optimizer_state_dict(torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9).state_dict())


def test_fused_state_loads_into_torch_adam():
    model = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()
    ts = TrainStep(model, lr=1e-3, optimizer='adamw', betas=(0.85, 0.995))
    x1, x2, lbl = _inputs()
    for _ in range(2):
        ts.step(x1, x2, lbl)
    sd = ts.optimizer_state_dict()
    names = [k for k, _ in model.named_parameters()]
    live = ts.opt_state['exp_avg'].clone()
    keep = sd['state'][0]['exp_avg'].clone()
    sd['state'][0]['exp_avg'].add_(1.0)                      # copies, not views of the live buffers
    assert torch.equal(ts.opt_state['exp_avg'], live)
    sd['state'][0]['exp_avg'].copy_(keep)
    opt = torch.optim.Adam(model.parameters())
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g['decoupled_weight_decay'] and g['betas'] == (0.85, 0.995) and g['weight_decay'] == 1e-2
    for i, (k, p) in enumerate(model.named_parameters()):
        s = opt.state[p]
        assert float(s['step']) == 2.0
        assert torch.equal(s['exp_avg'], ts.layout.view(ts.opt_state['exp_avg'], k))
        assert torch.equal(s['exp_avg_sq'], ts.layout.view(ts.opt_state['exp_avg_sq'], k))
    assert len(opt.state) == len(names)


# ---------------------------------------------------------------- the default rule is today's
def test_default_rule_is_plain_sgd_without_state():
    x1, x2, lbl = _inputs(c=13, seed=5)
    outs = []
    calls = []
    orig = _lib.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    _lib.call = spy
    try:
        for kw in (dict(), dict(optimizer='sgd', momentum=0, weight_decay=0)):
            model = filler.fill_module(BiDateNet(13, 2, precision='bf16')).to(dev).train()
            ts = TrainStep(model, lr=1e-2, **kw)
            assert ts.opt_state == {} and ts.optim.plain
            for _ in range(3):
                ts.step(x1, x2, lbl)
            torch.cuda.synchronize()
            outs.append(ts.flat_params.clone())
            assert ts.optimizer_state_dict()['state'] == {}
    finally:
        _lib.call = orig
    assert torch.equal(outs[0], outs[1])
    assert calls.count('bdn_sgd_step') == 6 and 'bdn_sgd_momentum_step' not in calls and 'bdn_adam_step' not in calls


# ---------------------------------------------------------------- a short trajectory against the autograd route
def test_fused_adamw_trajectory_follows_the_autograd_route():
    """fp32 setting, 6 steps, lr 1e-3: fused AdamW against model(x1, x2) + TverskyLoss + backward + torch.optim.AdamW.  The two routes
    compute the same gradients to float32 rounding (the fp32 parity bar: logits within 1e-3 of float64), but Adam normalises every gradient
    element, so an element whose gradient is rounding noise may move by up to ~lr in either route; summed over the network that bounds the
    loss difference, not the parameters.  The loss change over the 6 steps is checked to be well above the tolerance."""
    lr = 1e-3
    x1, x2, lbl = _inputs(b=4, c=3, s=32, seed=9)
    a = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()
    b = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()
    ts = TrainStep(a, lr=lr, optimizer='adamw')
    opt = torch.optim.AdamW(b.parameters(), lr=lr, foreach=False)
    fused, auto = [], []
    for _ in range(6):
        fused.append(float(ts.step(x1, x2, lbl)))
        auto.append(_autograd_step(b, opt, x1, x2, lbl))
    print('fused', fused, '\nautograd', auto)
    assert abs(fused[0] - auto[0]) < 1e-5                    # same weights: the fp32 loss parity
    assert abs(fused[0] - fused[-1]) > 5e-3, 'the loss barely moved: the comparison below would show nothing'
    for k in range(6):
        assert abs(fused[k] - auto[k]) < 1e-3, (k, fused, auto)


# ---------------------------------------------------------------- data parallel, in fresh child processes
_GLOO = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[3])
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = sys.argv[4]
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
from fabric_amd import BiDateNet
from fabric_amd.train_step import TrainStep
from oracle import filler
b, c, s = 4, 3, 32
x1, x2, lbl = (torch.from_numpy(v).cuda() for v in filler.make_inputs(b * world, c, s, seed=13))
sl = slice(rank * b, (rank + 1) * b)
model = filler.fill_module(BiDateNet(c, 2, precision='fp32')).cuda().train()
ts = TrainStep(model, lr=1e-3, optimizer='adam', weight_decay=1e-3, n_buckets=3)
assert ts.world == world
for _ in range(2):
    ts.step(x1[sl], x2[sl], lbl[sl])
torch.cuda.synchronize()
assert ts.opt_step == 2
for t in (ts.flat_params, ts.opt_state['exp_avg'], ts.opt_state['exp_avg_sq']):
    mine = t.cpu()
    assert bool(mine.abs().sum() > 0)
    others = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(others, mine)
    assert all(torch.equal(o, mine) for o in others), 'ranks diverged'
dist.barrier(); dist.destroy_process_group()
print('ok', rank)
'''


def test_two_gloo_ranks_hold_identical_adam_state(tmp_path):
    script = tmp_path / 'adam_ddp_worker.py'
    script.write_text(_GLOO)
    port = str(35000 + (os.getpid() * 5) % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', ROOT, port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=280)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(outs)
    assert all('ok' in o for o in outs)


_GUARD = r'''
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
x1, x2, lbl = (torch.from_numpy(v).cuda() for v in filler.make_inputs(4, 3, 32, seed=17))
model = filler.fill_module(BiDateNet(3, 2, precision='fp32')).cuda().train()
ts = TrainStep(model, lr=1e-3, optimizer='adam', force_collectives=True, guard=False)
for _ in range(2):
    ts.step(x1, x2, lbl)
torch.cuda.synchronize()
before = (ts.flat_params.clone(), ts.opt_state['exp_avg'].clone(), ts.opt_state['exp_avg_sq'].clone(), ts.opt_step)
rep = ts.guard_collectives(4, 32, 32, steps=2)
assert rep['active'], rep
torch.cuda.synchronize()
after = (ts.flat_params, ts.opt_state['exp_avg'], ts.opt_state['exp_avg_sq'])
for name, u, v in zip(('params', 'exp_avg', 'exp_avg_sq'), before[:3], after):
    assert torch.equal(u, v), name
assert ts.opt_step == before[3] == 2, ts.opt_step
ts.step(x1, x2, lbl)
torch.cuda.synchronize()
assert ts.opt_step == 3
import torch.distributed as dist
dist.barrier(); dist.destroy_process_group()
print('ok')
'''


def test_guard_collectives_restores_adam_state_over_rccl(tmp_path):
    script = tmp_path / 'adam_guard_worker.py'
    script.write_text(_GUARD)
    port = str(37000 + (os.getpid() * 3) % 2000)
    p = subprocess.Popen([sys.executable, str(script), ROOT, port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.communicate(timeout=280)[0].decode()
    assert p.returncode == 0 and 'ok' in out, out


# ---------------------------------------------------------------- train.py --optimizer / --resume
def test_train_cli_writes_optimizer_state_and_resumes(tmp_path):
    from fabric_amd.train import make_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    bs = 8
    train_loader, _ = make_loaders(synthetic_onera(n_cities=6, bands=13, size=(360, 360)), ['city4', 'city5'], 90, 90, bs, True)
    per_epoch = len(train_loader)
    assert per_epoch > 0
    log = tmp_path / 'log'
    common = [sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--optimizer', 'adam', '--batch_size', str(bs),
              '--num_workers', '0', '--log_dir', str(log)]
    r = subprocess.run(common + ['--epochs', '1'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sd = torch.load(log / 'optimizer_epoch_0.pt', weights_only=True)
    assert sd['param_groups'][0]['decoupled_weight_decay'] is False and len(sd['state']) == 74
    assert all(float(s['step']) == per_epoch for s in sd['state'].values())
    r = subprocess.run(common + ['--epochs', '2', '--resume', str(log / 'checkpoint_epoch_0.state_dict.pt')], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert '"epoch": 1' in r.stdout and '"epoch": 0' not in r.stdout
    sd1 = torch.load(log / 'optimizer_epoch_1.pt', weights_only=True)
    assert all(float(s['step']) == 2 * per_epoch for s in sd1['state'].values())
