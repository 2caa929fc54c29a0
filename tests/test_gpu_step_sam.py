"""-m gpu: TrainStep(sam_rho=...) (fabric_amd/train_step.py) on BiDateNet(3, 2, precision='fp32'), B=4, 32x32.

The oracle is exact: the library is bit-reproducible, so a SAM step must leave the BITS a plain step leaves that is driven by hand through
"step with lr 0 -> bdn_sam_perturb -> step with lr 0 -> copy the weights back -> bdn_sgd_step".  The other update rules are held to their
float64 twins on the step's own (pass-2) gradient; then the compositions, the default-off launches, two ranks and train.py's flags."""
import json
import os
import subprocess
import sys

import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd import optim as O
from fabric_amd.train_step import TrainStep
from oracle import filler
from tests import layerwise_ref as L
from tests import optim_ref as R
from tests import stale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
LR = 1e-2


def _inputs(b=4, c=3, s=32, seed=3):
    return tuple(torch.from_numpy(v).to(dev) for v in filler.make_inputs(b, c, s, seed=seed))


def _model():
    return filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()


def _buffers(ts):
    return {k: v.clone() for k, v in ts._P.items() if k not in ts.layout.slices}


def _perturb(ts, rho, adaptive, eps=1e-12):
    """bdn_sam_perturb called directly on a plain step's buffers, with the per-tensor table of the step's own groups -> (saved, out);
    the engine's packed images are marked stale."""
    pg = ts._groups if ts._groups is not None else O.ParamGroups(ts.optim, ts._names, None, ())
    ends, lens, ids, _ = (t.to(dev) for t in O.tensor_table(ts.layout, pg))
    saved = torch.empty_like(ts.flat_params)
    ws = torch.empty(_lib.load().bdn_sam_workspace_bytes(ts.layout.total, len(ts.layout.order)) // 8, dtype=torch.float64, device=dev)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _lib.call('bdn_sam_perturb', ts.flat_params.data_ptr(), saved.data_ptr(), ts.flat_grads.data_ptr(), ends.data_ptr(), lens.data_ptr(),
              ids.data_ptr(), len(ts.layout.order), rho, int(adaptive), eps, ws.data_ptr(), out.data_ptr(), ts.layout.total,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    ts.model.engine().invalidate_weights()
    return saved, out


def _sam_gradient_by_hand(b, x1, x2, lbl, rho, adaptive):
    """Drive the plain step `b` through one SAM gradient: -> (loss at w, loss at w + e, norm, g1, buffers after the first pass).  On
    return flat_grads holds the gradient at w + e and flat_params is w again."""
    snap = b.flat_params.clone()
    lr, b.lr = b.lr, 0.0
    loss1 = b.step(x1, x2, lbl)
    torch.cuda.synchronize()
    b.flat_params.copy_(snap)
    g1, bufs = b.flat_grads.clone(), _buffers(b)
    _, out = _perturb(b, rho, adaptive)
    loss2 = b.step(x1, x2, lbl)
    torch.cuda.synchronize()
    b.flat_params.copy_(snap)
    b.model.engine().invalidate_weights()
    b.lr = lr
    return loss1, loss2, out, g1, bufs


@pytest.mark.parametrize('adaptive', [False, True])
def test_a_sam_step_is_the_plain_step_driven_by_hand_bit_for_bit(adaptive):
    x1, x2, lbl = _inputs()
    rho = 0.5 if adaptive else 0.05
    a = TrainStep(_model(), lr=LR, sam_rho=rho, sam_adaptive=adaptive)
    b = TrainStep(stale.twin(a.model), lr=LR)
    assert a.flat_sam is not None and a.flat_sam.shape == a.flat_params.shape and b.flat_sam is None
    for it in range(2):
        loss_a = a.step(x1, x2, lbl)
        loss1, loss2, out, g1, bufs = _sam_gradient_by_hand(b, x1, x2, lbl, rho, adaptive)
        _lib.call('bdn_sgd_step', b.flat_params.data_ptr(), b.flat_grads.data_ptr(), LR, 1.0, b.layout.total, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(a.flat_grads, b.flat_grads), f'step {it}: the pass-2 gradient differs'
        assert torch.equal(a.flat_params, b.flat_params), f'step {it}: the updated parameters differ'
        assert torch.equal(loss_a, loss1) and torch.equal(a.last_sam_loss, loss2), f'step {it}: a loss differs'
        assert torch.equal(a.last_sam_norm, out[0]) and torch.equal(a.last_sam_scale, out[1])
        assert float(a.last_sam_norm) > 0 and float(a.last_sam_loss) != float(loss_a)
        stale.same_bits(_buffers(a), bufs, f'step {it}: BatchNorm buffers after pass 1 (pass 2 must move nothing)')
        assert not torch.equal(b.flat_grads, g1), 'the perturbation did not change the gradient: the test proves nothing'
        for k, v in _buffers(a).items():                      # B's second forward moved them a second time: bring B back to A
            b._P[k].copy_(v)


def _split(ts, flat):
    flat = flat.detach().cpu()
    return [flat[o:o + n] for o, n, _ in (ts.layout.slices[k] for k in ts.layout.order)]


@pytest.mark.parametrize('rule', ['adam', 'sgdm', 'lamb'])
def test_other_update_rules_apply_the_pass_two_gradient_at_w(rule):
    """Snapshot, step, then the rule's float64 twin on the step's own flat_grads, from the snapshot (so the update started at the restored
    w, not at w + e), with the twins' own bounds."""
    x1, x2, lbl = _inputs()
    kw = dict(adam=dict(optimizer='adamw', weight_decay=0.01), sgdm=dict(optimizer='sgd', momentum=0.9, nesterov=True, weight_decay=1e-3),
              lamb=dict(optimizer='lamb', weight_decay=0.01, max_trust=10.0))[rule]
    ts = TrainStep(_model(), lr=LR, sam_rho=0.05, **kw)
    for it in range(2):
        torch.cuda.synchronize()
        p0, s0 = ts.flat_params.clone(), {k: v.clone() for k, v in ts.opt_state.items()}
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        g = ts.flat_grads
        if rule == 'adam':
            rp, rm, rv, mp, mm, mv = R.adam(p0, g, s0['exp_avg'], s0['exp_avg_sq'], it + 1, LR, weight_decay=0.01, decoupled=True)
            R.check(ts.flat_params, rp, mp, f'adamw step {it} p')
            R.check(ts.opt_state['exp_avg'], rm, mm, f'adamw step {it} m')
            R.check(ts.opt_state['exp_avg_sq'], rv, mv, f'adamw step {it} v')
        elif rule == 'sgdm':
            rp, rb, mp, mb = R.sgd(p0, g, s0['momentum_buffer'], LR, momentum=0.9, weight_decay=1e-3, nesterov=True, first=it == 0)
            R.check(ts.flat_params, rp, mp, f'sgd step {it} p')
            R.check(ts.opt_state['momentum_buffer'], rb, mb, f'sgd step {it} buf')
        else:
            o, order = ts.optim, ts.layout.order
            hyper = dict(grad_scale=1.0, betas=o.betas, eps=o.eps, max_trust=o.max_trust, momentum=0.0, dampening=0.0, nesterov=False,
                         trust_coef=o.trust_coef, lars_eps=o.lars_eps)
            L.check_update('lamb', hyper, it, _split(ts, p0), _split(ts, g), {'m': _split(ts, s0['exp_avg']), 'v': _split(ts, s0['exp_avg_sq'])},
                           _split(ts, ts.flat_params), {'m': _split(ts, ts.opt_state['exp_avg']), 'v': _split(ts, ts.opt_state['exp_avg_sq'])},
                           ts.last_trust, [LR] * len(order), [0.01] * len(order), [int(len(ts.layout.slices[k][2]) > 1) for k in order],
                           set(), f'lamb step {it}')
        assert bool((ts.flat_params != p0).any())


def test_a_frozen_block_is_not_perturbed_and_not_in_the_norm():
    x1, x2, lbl = _inputs()
    model = _model()
    for k, p in model.named_parameters():
        if k.startswith('inc.'):
            p.requires_grad_(False)
    a = TrainStep(model, lr=LR, sam_rho=0.05)
    b = TrainStep(stale.twin(model), lr=LR)
    frozen = [k for k in a.layout.order if k.startswith('inc.')]
    assert frozen and b._groups is not None and set(b._groups.frozen) == set(frozen)
    p0 = {k: a.layout.view(a.flat_params, k).clone() for k in frozen}
    a.step(x1, x2, lbl)
    _, _, out, g1, _ = _sam_gradient_by_hand(b, x1, x2, lbl, 0.05, False)
    torch.cuda.synchronize()
    assert torch.equal(a.last_sam_norm, out[0]) and torch.equal(a.flat_grads, b.flat_grads)
    trainable = [k for k in a.layout.order if k not in frozen]
    want = torch.sqrt(sum((b.layout.view(g1, k).double() ** 2).sum() for k in trainable))
    assert abs(float(out[0]) - float(want)) <= 2.0 ** -23 * float(want)                  # the norm of the trainable tensors alone
    for k in frozen:
        assert torch.equal(a.layout.view(a.flat_params, k), p0[k]), k
    # set_param_groups rebuilds the table: released, the block is perturbed and trained
    for p in model.parameters():
        p.requires_grad_(True)
    a.set_param_groups(None)
    a.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert all(not torch.equal(a.layout.view(a.flat_params, k), p0[k]) for k in frozen if k.endswith('.weight'))


def test_accumulate_two_sums_two_sam_gradients():
    x1, x2, lbl = _inputs(8)
    a = TrainStep(_model(), lr=LR, sam_rho=0.05, accumulate=2)
    b = TrainStep(stale.twin(a.model), lr=LR)
    w0 = a.flat_params.clone()
    a.step(x1[:4], x2[:4], lbl[:4])
    torch.cuda.synchronize()
    assert a.micro == 1 and torch.equal(a.flat_params, w0)                                 # a micro-step: restored, not updated
    a.step(x1[4:], x2[4:], lbl[4:])
    _sam_gradient_by_hand(b, x1[:4], x2[:4], lbl[:4], 0.05, False)
    acc = b.flat_grads.clone()
    _sam_gradient_by_hand(b, x1[4:], x2[4:], lbl[4:], 0.05, False)
    total = b.flat_grads + acc                                                             # flat_grads = g2 + acc, one float32 add
    _lib.call('bdn_sgd_step', b.flat_params.data_ptr(), total.data_ptr(), LR, 0.5, b.layout.total, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert a.micro == 0 and torch.equal(a.flat_grads, total) and torch.equal(a.flat_params, b.flat_params)


def test_clipping_measures_the_pass_two_gradient():
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=LR, sam_rho=0.05, max_grad_norm=1e-3)
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    want = float(ts.flat_grads.double().norm())
    assert abs(float(ts.last_grad_norm) - want) <= 2.0 ** -23 * want and 0.0 < float(ts.last_clip_coef) < 1.0
    assert float(ts.last_grad_norm) != float(ts.last_sam_norm)                             # pass 1's norm is the perturbation's


def test_the_average_follows_the_restored_and_updated_weights():
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=LR, sam_rho=0.05, ema_decay=0.9)
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert ts.n_averaged == 1 and torch.equal(ts.flat_avg, ts.flat_params)                # the first averaging update is a copy
    avg1 = ts.flat_avg.double().clone()
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    want = avg1 + (1.0 - 0.9) * (ts.flat_params.double() - avg1)
    tol = 4 * L.EPS32 * (avg1.abs() + ts.flat_params.double().abs()) + 1e-38
    assert ts.n_averaged == 2 and bool(((ts.flat_avg.double() - want).abs() <= tol).all())


def test_frozen_batchnorm_leaves_the_buffers_untouched():
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=LR, sam_rho=0.05, bn='frozen')
    before, w0 = _buffers(ts), ts.flat_params.clone()
    ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    stale.same_bits(_buffers(ts), before, 'bn=frozen under SAM')
    assert not torch.equal(ts.flat_params, w0) and float(ts.last_sam_norm) > 0


@pytest.mark.parametrize('adaptive', [False, True])
def test_a_twin_built_after_three_steps_continues_bit_for_bit(adaptive):
    x1, x2, lbl = _inputs()
    rho = 0.5 if adaptive else 0.05
    a = TrainStep(_model(), lr=LR, sam_rho=rho, sam_adaptive=adaptive, optimizer='sgd', momentum=0.9)
    for _ in range(3):
        a.step(x1, x2, lbl)
    torch.cuda.synchronize()
    t = stale.twin_step(a, sam_rho=rho, sam_adaptive=adaptive)
    la, lt = a.step(x1, x2, lbl), t.step(x1, x2, lbl)
    torch.cuda.synchronize()
    stale.same_bits(dict(p=t.flat_params, g=t.flat_grads, loss=lt, sam=t.last_sam_loss, out=t._sam[4], buf=_buffers(t)),
                    dict(p=a.flat_params, g=a.flat_grads, loss=la, sam=a.last_sam_loss, out=a._sam[4], buf=_buffers(a)), 'the step after the twin point')
    plain = stale.twin_step(a)                                                             # the keyword matters: without it the twin is a plain step
    assert plain.sam_rho is None and plain.flat_sam is None


def test_an_eval_forward_between_two_steps_sees_the_unperturbed_weights():
    x1, x2, lbl = _inputs()
    a = TrainStep(_model(), lr=LR, sam_rho=0.05)
    a.step(x1, x2, lbl)
    torch.cuda.synchronize()
    a.model.eval()
    with torch.no_grad():
        got = a.model(x1, x2).clone()
    torch.cuda.synchronize()
    fresh = stale.twin(a.model)                                                            # packs its images from the state dict: w, never w + e
    with torch.no_grad():
        want = fresh(x1, x2)
    stale.same_bits(got, want, 'eval forward after a SAM step')
    a.model.train()
    w = a.flat_params.clone()
    a.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert not torch.equal(a.flat_params, w)


_UPDATE_CALLS = ('bdn_sgd', 'bdn_adam', 'bdn_lamb', 'bdn_lars', 'bdn_layerwise', 'bdn_grad_', 'bdn_ema', 'bdn_swap', 'bdn_sam')


def _calls(**kw):
    """Every library call of two steps of a TrainStep built with `kw`, recorded through _lib.call's hook."""
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
    return ts, seen


def test_default_off_issues_the_launches_of_the_plain_step():
    """sam_rho=None allocates nothing and issues exactly the calls of a step built without the keyword; with it, one step is two passes, the
    two kernels and one more repack, and the second pass finalizes BatchNorm as often as the first."""
    _, base = _calls()
    ts1, off = _calls(sam_rho=None)
    assert off == base and ts1.flat_sam is None and ts1._sam is None and ts1.last_sam_loss is None and ts1.last_sam_norm is None
    assert [n for n in base if n.startswith(_UPDATE_CALLS)] == ['bdn_sgd_step'] * 2
    _, on = _calls(sam_rho=0.05)
    assert [n for n in on if n.startswith(_UPDATE_CALLS)] == ['bdn_sam_perturb', 'bdn_sam_restore', 'bdn_sgd_step'] * 2
    count = lambda seen, name: sum(n == name for n in seen)
    assert count(base, 'bdn_pack_weights_multi') == 2 and count(on, 'bdn_pack_weights_multi') == 4      # one more repack per step
    for name in set(base) - {'bdn_sgd_step', 'bdn_pack_weights_multi'}:      # forward, criterion, backward and their hand-offs: twice
        if name not in ('bdn_event_create', 'bdn_stream_create'):            # (the pooled events and streams are made once)
            assert count(on, name) == 2 * count(base, name), name
    assert count(base, 'bdn_bn_finalize') > 0 and count(base, 'bdn_tversky') == 2
    _, adamw = _calls(optimizer='adamw', max_grad_norm=1.0, sam_rho=0.05)
    assert [n for n in adamw if n.startswith(_UPDATE_CALLS)] == ['bdn_sam_perturb', 'bdn_sam_restore', 'bdn_grad_norm', 'bdn_adam_step_grouped_ex'] * 2


_DDP = r'''
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
ts = TrainStep(model, lr=1e-2, n_buckets=3, sam_rho=0.05)
assert ts.world == world and ts.bucketer.active()
n_reduce = [0]
real = dist.all_reduce
def counted(*a, **k):
    n_reduce[0] += 1
    return real(*a, **k)
dist.all_reduce = counted
for _ in range(3):
    ts.step(x1[sl], x2[sl], lbl[sl])
torch.cuda.synchronize()
dist.all_reduce = real
assert n_reduce[0] == 3 * len(ts.bucketer.buckets), (n_reduce[0], len(ts.bucketer.buckets))      # one set per update, none in pass 1
norms = [torch.empty(1) for _ in range(world)]
dist.all_gather(norms, ts.last_sam_norm.cpu().reshape(1))
assert norms[0].item() != norms[1].item(), 'm-sharpness: every rank perturbs with its own gradient'
mine = ts.flat_params.cpu()
others = [torch.empty_like(mine) for _ in range(world)]
dist.all_gather(others, mine)
assert all(torch.equal(o, mine) for o in others), 'ranks diverged'
dist.barrier(); dist.destroy_process_group()
print('ok', rank)
'''


def test_two_gloo_ranks_hold_bit_equal_parameters_with_one_exchange_per_update(tmp_path):
    """Two processes on one device, different batches, three SAM steps: every rank perturbs with its own gradient (the norms differ), one
    set of bucket all-reduces per update and none in pass 1, and the restore is exact, so the parameters stay bit-equal across the ranks."""
    script = tmp_path / 'sam_ddp_worker.py'
    script.write_text(_DDP)
    port = str(41000 + (os.getpid() * 7) % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', ROOT, port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=280)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(outs)
    assert all('ok' in o for o in outs)


def test_training_loop_reports_the_sharpness(tmp_path, capsys):
    from fabric_amd import train as T
    T.main(['--synthetic', '--batch_size', '8', '--patch_size', '64', '--stride', '128', '--num_workers', '0', '--learning_rate', '0.002',
            '--fused_step', 'true', '--sam_rho', '0.05', '--epochs', '2', '--log_dir', str(tmp_path)])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith('{"epoch"')]
    assert [l['epoch'] for l in lines] == [0, 1]
    for rec in lines:
        assert {'train_sam_sharpness_mean', 'train_sam_norm_mean'} <= set(rec), sorted(rec)
        s, n = rec['train_sam_sharpness_mean'], rec['train_sam_norm_mean']
        assert s == s and abs(s) != float('inf') and n == n and 0.0 < n < float('inf'), rec
