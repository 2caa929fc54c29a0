"""-m gpu: TrainStep with optimizer='lamb' / 'lars' (fabric_amd/train_step.py) on BiDateNet(3, 2), B=4, 32x32.

Every update is checked against the float64 twin (tests/layerwise_ref.py: check_update) applied to the step's own gradients, with the
element and norm bounds of tests/test_gpu_layerwise.py; then the compositions: groups and frozen parameters, accumulation, clipping, the
averaged weights, the state exchange, the launches of the existing rules, two ranks, and train.py's flags."""
import json
import os
import subprocess
import sys

import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.train_step import TrainStep
from oracle import filler
from tests import layerwise_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)

_RULES = {
    'lamb': dict(optimizer='lamb', weight_decay=0.01, max_trust=10.0),
    'lars': dict(optimizer='lars', momentum=0.9, nesterov=True, weight_decay=1e-3, trust_coef=0.02),
}
_STATE = {'lamb': {'m': 'exp_avg', 'v': 'exp_avg_sq'}, 'lars': {'buf': 'momentum_buffer'}}


def _inputs(b=4, c=3, s=32, seed=3):
    return tuple(torch.from_numpy(v).to(dev) for v in filler.make_inputs(b, c, s, seed=seed))


def _model():
    return filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()


def _split(ts, flat):
    flat = flat.detach().cpu()
    return [flat[o:o + n] for o, n, _ in (ts.layout.slices[k] for k in ts.layout.order)]


def _snapshot(ts):
    torch.cuda.synchronize()
    return ts.flat_params.clone(), {k: ts.opt_state[v].clone() for k, v in _STATE[ts.optim.kind].items() if v in ts.opt_state}


def _check(ts, it, before, grads, grad_scale=1.0, lrs=None, wds=None, what=''):
    """The update that just ran against the twin: `before` = _snapshot() taken in front of it, `grads` = the flat gradient it read."""
    o = ts.optim
    order = ts.layout.order
    pg = ts._layerwise_table()[0]
    frozen = {i for i, k in enumerate(order) if pg.group_id(k) < 0}
    lr_t = lrs or [pg.groups[max(pg.group_id(k), 0)]['lr'] for k in order]
    wd_t = wds or [pg.groups[max(pg.group_id(k), 0)]['weight_decay'] for k in order]
    adapt = [int(o.adapt_1d or len(ts.layout.slices[k][2]) > 1) for k in order]
    hyper = dict(grad_scale=grad_scale, betas=o.betas, eps=o.eps, max_trust=o.max_trust, momentum=o.momentum, dampening=o.dampening,
                 nesterov=o.nesterov, trust_coef=o.trust_coef, lars_eps=o.lars_eps)
    p_in, s_in = before
    p_out, s_out = _snapshot(ts)
    L.check_update(o.kind, hyper, it, _split(ts, p_in), _split(ts, grads), {k: _split(ts, v) for k, v in s_in.items()}, _split(ts, p_out),
                   {k: _split(ts, v) for k, v in s_out.items()}, ts.last_trust, lr_t, wd_t, adapt, frozen, what or o.kind)
    return p_out


@pytest.mark.parametrize('name', list(_RULES))
def test_three_updates_match_the_twin_on_the_steps_own_gradients(name):
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=1e-2, **_RULES[name])
    assert ts.trust_ratios() == {} and ts.last_trust.shape == (len(ts.layout.order), 3)
    for it in range(3):
        before = _snapshot(ts)
        ts.step(x1, x2, lbl)
        p_out = _check(ts, it, before, ts.flat_grads.clone())
        assert bool((p_out != before[0]).any()) and ts.opt_step == it + 1
    ratios = ts.trust_ratios()
    assert set(ratios) == set(ts.layout.order)
    for k, r in ratios.items():
        if len(ts.layout.slices[k][2]) <= 1:
            assert r == 1.0, (k, r)                          # adapt_1d=False: biases, BatchNorm weight and bias
    assert any(r != 1.0 for k, r in ratios.items() if len(ts.layout.slices[k][2]) > 1)
    assert set(ts.trust_ratios(adapted_only=True)) == {k for k in ts.layout.order if len(ts.layout.slices[k][2]) > 1}


@pytest.mark.parametrize('name', list(_RULES))
def test_groups_and_a_frozen_first_block(name):
    x1, x2, lbl = _inputs()
    model = _model()
    names = [k for k, _ in model.named_parameters()]
    for k, p in model.named_parameters():
        if k.startswith('inc.'):
            p.requires_grad_(False)
    one_d = [k for k, p in model.named_parameters() if p.dim() <= 1]
    groups = [{'params': [k for k in names if k not in one_d], 'lr': 2e-2}, {'params': one_d, 'weight_decay': 0.0}]
    ts = TrainStep(model, lr=1e-2, param_groups=groups, **_RULES[name])
    frozen = [k for k in names if k.startswith('inc.')]
    p0 = {k: ts.layout.view(ts.flat_params, k).clone() for k in frozen}
    for it in range(2):
        before = _snapshot(ts)
        ts.step(x1, x2, lbl)
        _check(ts, it, before, ts.flat_grads.clone())
    for k in frozen:
        assert torch.equal(ts.layout.view(ts.flat_params, k), p0[k]), k
        assert all(not bool(ts.layout.view(t, k).any()) for t in ts.opt_state.values()), k
    ratios = ts.trust_ratios()
    assert set(ratios) == set(names) - set(frozen)
    assert all(ratios[k] == 1.0 for k in one_d if k in ratios)
    sd = ts.optimizer_state_dict()
    assert len(sd['param_groups']) == 2 and all(g['layer_adapt'] == name for g in sd['param_groups'])
    assert not any(names.index(k) in sd['state'] for k in frozen)
    # set_param_groups rebuilds and uploads the table: with everything released the first block trains
    for p in model.parameters():
        p.requires_grad_(True)
    ts.set_param_groups(None)
    before = _snapshot(ts)
    ts.step(x1, x2, lbl)
    _check(ts, 2, before, ts.flat_grads.clone())
    assert all(not torch.equal(ts.layout.view(ts.flat_params, k), p0[k]) for k in frozen if k.endswith('.weight'))


@pytest.mark.parametrize('name', list(_RULES))
def test_accumulate_two_is_one_update_on_the_mean_gradient(name):
    x1, x2, lbl = _inputs(8)
    ts = TrainStep(_model(), lr=1e-2, accumulate=2, **_RULES[name])
    before = _snapshot(ts)
    ts.step(x1[:4], x2[:4], lbl[:4])
    torch.cuda.synchronize()
    assert ts.opt_step == 0 and ts.micro == 1 and torch.equal(ts.flat_params, before[0])          # a micro-step: no update
    ts.step(x1[4:], x2[4:], lbl[4:])
    assert ts.opt_step == 1 and ts.micro == 0
    _check(ts, 0, before, ts.flat_grads.clone(), grad_scale=0.5)                                    # flat_grads holds the SUM of the two


@pytest.mark.parametrize('name', list(_RULES))
def test_clipping_reaches_the_rule_on_the_device(name):
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=1e-2, max_grad_norm=1e-3, **_RULES[name])
    for it in range(2):
        before = _snapshot(ts)
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        coef = float(ts.last_clip_coef)
        assert 0.0 < coef < 1.0, coef                                                               # the clip is active
        _check(ts, it, before, ts.flat_grads.clone(), grad_scale=coef)                              # 1.0f * coef is exact


def test_the_average_follows_the_rule():
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=1e-2, ema_decay=0.9, **_RULES['lamb'])
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert ts.n_averaged == 1 and torch.equal(ts.flat_avg, ts.flat_params)                          # the first averaging update is a copy
    avg1 = ts.flat_avg.double().clone()
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    want = avg1 + (1.0 - 0.9) * (ts.flat_params.double() - avg1)
    tol = 4 * L.EPS32 * (avg1.abs() + ts.flat_params.double().abs()) + 1e-38
    assert ts.n_averaged == 2 and bool(((ts.flat_avg.double() - want).abs() <= tol).all())
    assert not torch.equal(ts.flat_avg, ts.flat_params)


@pytest.mark.parametrize('name', list(_RULES))
def test_saved_state_continues_bit_for_bit(name):
    x1, x2, lbl = _inputs()
    a = TrainStep(_model(), lr=1e-2, **_RULES[name])
    for _ in range(2):
        a.step(x1, x2, lbl)
    torch.cuda.synchronize()
    sd = a.optimizer_state_dict()
    assert sd['param_groups'][0]['layer_adapt'] == name and len(sd['state']) == 74
    model_b = _model()
    model_b.load_state_dict(a.model.state_dict())
    b = TrainStep(model_b, lr=5e-2, **_RULES[name])
    b.load_optimizer_state_dict(sd)
    assert b.opt_step == (2 if name == 'lamb' else 1) and b.lr == 1e-2
    a.step(x1, x2, lbl)
    b.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert torch.equal(a.flat_params, b.flat_params) and torch.equal(a.last_trust, b.last_trust)
    assert all(torch.equal(a.opt_state[k], b.opt_state[k]) for k in a.opt_state)
    other = TrainStep(_model(), lr=1e-2, optimizer='adamw' if name == 'lamb' else 'sgd', **({} if name == 'lamb' else {'momentum': 0.9}))
    with pytest.raises(ValueError, match='optimizer state of'):
        other.load_optimizer_state_dict(sd)                                                          # another family
    with pytest.raises(ValueError, match='optimizer state of'):
        a.load_optimizer_state_dict(other.optimizer_state_dict())


_UPDATE_CALLS = ('bdn_sgd', 'bdn_adam', 'bdn_lamb', 'bdn_lars', 'bdn_layerwise', 'bdn_grad_', 'bdn_ema', 'bdn_swap')


def _update_calls(**kw):
    """The update-side library calls of two steps of a TrainStep built with `kw`, recorded through _lib.call's hook."""
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=1e-3, **kw)
    seen = []
    assert _lib.SKIP is None
    _lib.SKIP = lambda name, args: seen.append(name) and False
    try:
        for _ in range(2):
            ts.step(x1, x2, lbl)
    finally:
        _lib.SKIP = None
    torch.cuda.synchronize()
    return [n for n in seen if n.startswith(_UPDATE_CALLS)]


def test_existing_rules_keep_their_launches():
    """The default step and adamw issue the update calls they always did -- one ungrouped entry point per step, nothing of the layer-wise
    route -- and the new rules issue exactly one call of their own."""
    assert _update_calls() == ['bdn_sgd_step'] * 2
    assert _update_calls(optimizer='adamw') == ['bdn_adam_step'] * 2
    assert _update_calls(optimizer='sgd', momentum=0.9) == ['bdn_sgd_momentum_step'] * 2
    assert _update_calls(optimizer='adamw', max_grad_norm=1.0) == ['bdn_grad_norm', 'bdn_adam_step_grouped_ex'] * 2
    assert _update_calls(**_RULES['lamb']) == ['bdn_lamb_step'] * 2
    assert _update_calls(max_grad_norm=1.0, **_RULES['lars']) == ['bdn_grad_norm', 'bdn_lars_step'] * 2


_DDP = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[3])
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = sys.argv[4]
torch.cuda.set_device(rank)
dist.init_process_group('gloo', rank=rank, world_size=world)
from fabric_amd import BiDateNet
from fabric_amd.train_step import TrainStep
from oracle import filler
b, c, s = 4, 3, 32
x1, x2, lbl = (torch.from_numpy(v).cuda() for v in filler.make_inputs(b * world, c, s, seed=13))
sl = slice(rank * b, (rank + 1) * b)
for kw in (dict(optimizer='lamb', weight_decay=0.01), dict(optimizer='lars', momentum=0.9, weight_decay=1e-3, trust_coef=0.02)):
    model = filler.fill_module(BiDateNet(c, 2, precision='fp32')).cuda().train()
    ts = TrainStep(model, lr=1e-2, n_buckets=3, **kw)
    assert ts.world == world
    for _ in range(2):
        ts.step(x1[sl], x2[sl], lbl[sl])
    torch.cuda.synchronize()
    assert ts.opt_step == 2
    for t in [ts.flat_params, ts.last_trust] + list(ts.opt_state.values()):
        mine = t.cpu()
        assert bool(mine.abs().sum() > 0)
        others = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(others, mine)
        assert all(torch.equal(o, mine) for o in others), 'ranks diverged'
dist.barrier(); dist.destroy_process_group()
print('ok', rank)
'''


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason=f'needs 2 GPUs (one device per rank), found {torch.cuda.device_count()}')
def test_two_ranks_hold_bit_equal_parameters(tmp_path):
    script = tmp_path / 'layerwise_ddp_worker.py'
    script.write_text(_DDP)
    port = str(39000 + (os.getpid() * 7) % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', ROOT, port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=280)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(outs)
    assert all('ok' in o for o in outs)


def test_train_cli_runs_lamb_with_warmup_and_cosine(tmp_path):
    cmd = [sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', '--fused_step', 'true', '--optimizer', 'lamb',
           '--lr_warmup_updates', '4', '--lr_schedule', 'cosine', '--num_workers', '0', '--log_dir', str(tmp_path / 'log')]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = next(json.loads(line) for line in r.stdout.splitlines() if line.startswith('{"epoch"'))
    assert rec['epoch'] == 0 and 'train_trust_min' in rec and 'train_trust_max' in rec, rec
    assert 0.0 < rec['train_trust_min'] <= rec['train_trust_max'] and rec['train_trust_max'] != 1.0
    loss = next(v for k, v in rec.items() if k.startswith('train_') and 'loss' in k)
    assert loss == loss and abs(loss) != float('inf'), rec
    sd = torch.load(tmp_path / 'log' / 'optimizer_epoch_0.pt', weights_only=True)
    assert sd['param_groups'][0]['layer_adapt'] == 'lamb'
    # the learning rate the run ended on is saved with the state: the schedule's value at the epoch's last update
    from fabric_amd.schedule import LRSchedule
    from fabric_amd.train import DEFAULTS, make_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    loader, _ = make_loaders(synthetic_onera(n_cities=6, bands=13, size=(360, 360)), ['city4', 'city5'], DEFAULTS['patch_size'],
                             DEFAULTS['stride'] // 2, DEFAULTS['batch_size'], True)
    n = len(loader)
    want = LRSchedule(DEFAULTS['learning_rate'], n, 4, 'cosine').lr(n - 1)
    assert n > 0 and sd['param_groups'][0]['lr'] == pytest.approx(want, rel=1e-12) and want != DEFAULTS['learning_rate']
    assert all(float(s['step']) == n for s in sd['state'].values())
