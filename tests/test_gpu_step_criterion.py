"""-m gpu: the fused train step with an explicit criterion (TrainStep(criterion=...), fabric_amd/criterion.py) and the --fused_step
route of the training CLI.

The oracle's step for a criterion is O.train_step's with the loss swapped for tests/criterion_ref.py's restatement: O.bidate_forward ->
loss -> torch.autograd.grad -> SGD.  The bars on logits, loss, gradients and the logits after the update are those of
tests/test_gpu_model.py::test_train_step_matches_reference for fp32 and bf16x3, unchanged."""
import json
import os
import subprocess
import sys

import pytest
import torch

from fabric_amd import BiDateNet
from fabric_amd.criterion import Criterion
from fabric_amd.train_step import TrainStep
from oracle import bidate_oracle as O
from oracle import filler
from tests import criterion_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODER = ('inc.', 'down1.', 'down2.', 'down3.', 'down4.')
dev = 'cuda'


def _inputs(b=4, c=3, s=32, seed=3):
    return tuple(torch.from_numpy(v) for v in filler.make_inputs(b, c, s, seed=seed))


def _bn_buffers(model):
    return {k: v for k, v in model.state_dict().items() if 'running_' in k or 'num_batches' in k}


# ---------------------------------------------------------------- tversky by name is the default step
@pytest.mark.parametrize('prec', ['fp32', 'bf16x3', 'bf16'])
def test_tversky_by_name_is_the_default_step_bit_for_bit(prec):
    x1, x2, lbl = (t.to(dev) for t in _inputs())
    models = [filler.fill_module(BiDateNet(3, 2, precision=prec)).to(dev).train() for _ in range(2)]
    named = TrainStep(models[0], lr=0.05, criterion='tversky', tversky_alpha=.1, tversky_beta=.9)
    plain = TrainStep(models[1], lr=0.05)
    assert named.criterion is not None and plain.criterion is None
    for it in range(3):
        la, lb = named.step(x1, x2, lbl), plain.step(x1, x2, lbl)
        torch.cuda.synchronize()
        if it in (0, 2):
            assert torch.equal(la, lb), (it, la.item(), lb.item())
            assert torch.equal(named.last_logits, plain.last_logits) and torch.equal(named.last_counts, plain.last_counts), it
            assert torch.equal(named.flat_grads, plain.flat_grads) and torch.equal(named.flat_params, plain.flat_params), it
            ba, bb = _bn_buffers(models[0]), _bn_buffers(models[1])
            assert ba and all(torch.equal(ba[k], bb[k]) for k in ba), it
    assert torch.equal(named.last_terms.cpu(), torch.tensor([la.item(), 0.0])) and plain.last_terms is None


# ---------------------------------------------------------------- one step against the oracle's step with the same criterion
def _oracle_step(c, sd, x1, x2, lbl, lr):
    """O.train_step with the criterion's restatement for the loss."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running_' not in k}
    full = dict(sd)
    full.update(params)
    logits, new_buf = O.bidate_forward(full, x1, x2, training=True)
    loss = CR.loss(c, logits, lbl)[0]
    names = list(params)
    grads = torch.autograd.grad(loss, [params[k] for k in names])
    new_sd = {k: v.clone() for k, v in sd.items()}
    for k, g in zip(names, grads):
        new_sd[k] = (sd[k] - lr * g).detach()
    for k, v in new_buf.items():
        new_sd[k] = v.detach()
    return dict(logits=logits.detach(), loss=float(loss.detach()), grads=dict(zip(names, [g.detach() for g in grads])), new_sd=new_sd)


def _grad_errors(got, ref):
    """test_gpu_model._grad_errors on whole tensors: worst per-parameter max(relative L2 error, relative error of the norm), and the
    cosine of the whole gradient."""
    worst, worst_key, allg, allr = 0.0, None, [], []
    for k, r in ref.items():
        g, r = got[k].detach().cpu().double().reshape(-1), r.double().reshape(-1)
        if float(r.norm()) < 1e-6:          # conv biases feeding a BatchNorm: the reference holds only rounding noise
            assert float(g.norm()) < 1e-6, k
            continue
        e = max(float((g - r).norm() / r.norm()), abs(float(g.norm()) - float(r.norm())) / float(r.norm()))
        allg.append(g)
        allr.append(r)
        if e > worst:
            worst, worst_key = e, k
    ag, ar = torch.cat(allg), torch.cat(allr)
    return worst, worst_key, float((ag * ar).sum() / (ag.norm() * ar.norm()))


_CRITERIA = {'dice': lambda: Criterion.parse('dice'), 'jaccard': lambda: Criterion.parse('jaccard'),
             'focal2': lambda: Criterion.parse('focal', focal_gamma=2.0),
             'focal2+dice': lambda: Criterion.parse('focal+dice', focal_gamma=2.0, weights=(1, 1))}


@pytest.mark.parametrize('prec', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', list(_CRITERIA))
def test_first_step_matches_the_oracle_step(name, prec):
    c, lr = _CRITERIA[name](), 1e-3
    x1, x2, lbl = _inputs()
    model = filler.fill_module(BiDateNet(3, 2, precision=prec))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ref = _oracle_step(c, sd, x1, x2, lbl, lr)
    model = model.to(dev).train()
    ts = TrainStep(model, lr=lr, criterion=c)
    dx1, dx2, dl = x1.to(dev), x2.to(dev), lbl.to(dev)
    loss = ts.step(dx1, dx2, dl)
    torch.cuda.synchronize()
    got = ts.last_logits.cpu()
    d = (got - ref['logits']).abs()
    gerr, gkey, gcos = _grad_errors(ts.grads, ref['grads'])
    print(f'\n[{name} {prec}] max|dlogit|={d.max():.3e} loss={loss.item():.7f} (oracle {ref["loss"]:.7f}) worst grad err={gerr:.3e} @ {gkey} '
          f'cos={gcos:.6f}')
    assert d.max() <= 1e-3
    margin = (ref['logits'][:, 0] - ref['logits'][:, 1]).abs()
    assert ((got.argmax(1) == ref['logits'].argmax(1)) | (margin < 2e-3)).all()
    assert abs(loss.item() - ref['loss']) < (1e-5 if prec == 'fp32' else 5e-5)
    assert gerr < (2e-2 if prec == 'fp32' else 6e-2) and gcos > 0.9999, (gkey, gerr, gcos)
    # the step's own loss gradient is what Criterion.evaluate gives on the step's logits, bit for bit
    _, terms, counts, dlogits = c.evaluate(ts.last_logits, dl)
    assert torch.equal(ts.last_dlogits, dlogits) and torch.equal(ts.last_terms, terms) and torch.equal(ts.last_counts, counts)
    # the updated parameters: forward again in train mode, as test_train_step_matches_reference does after opt.step()
    logits2 = model(dx1, dx2).detach().cpu()
    ref2, _ = O.bidate_forward(ref['new_sd'], x1, x2, training=True)
    assert (logits2 - ref2).abs().max() <= 1e-3


def test_label_rank_does_not_decide_the_reduction():
    x1, x2, lbl = (t.to(dev) for t in _inputs())
    out = []
    for labels in (lbl, lbl[:, None]):
        model = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()
        ts = TrainStep(model, lr=1e-3, criterion=Criterion.parse('dice', reduce='image'))
        out.append((ts.step(x1, x2, labels), ts.flat_grads.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    ref = CR.reference(Criterion.parse('dice', reduce='image'), ts.last_logits.cpu(), lbl.cpu())
    assert abs(out[0][0].item() - ref['loss']) < 5e-6


# ---------------------------------------------------------------- the rest of the step composes
def test_compound_criterion_composes_with_groups_frozen_encoder_and_frozen_bn():
    x1, x2, lbl = (t.to(dev) for t in _inputs(c=13, seed=5))
    model = filler.fill_module(BiDateNet(13, 2, precision='bf16')).to(dev).train()
    for k, p in model.named_parameters():
        p.requires_grad_(not k.startswith(ENCODER))
    named = list(model.named_parameters())
    w = [k for k, p in named if p.requires_grad and p.dim() > 1]
    nb = [k for k, p in named if p.requires_grad and p.dim() == 1]
    frozen = [k for k, p in named if not p.requires_grad]
    groups = [{'params': w, 'weight_decay': 5e-2}, {'params': nb, 'weight_decay': 0.0, 'lr': 1e-3}]
    ts = TrainStep(model, lr=1e-2, optimizer='adamw', param_groups=groups, bn='frozen',
                   criterion=Criterion.parse('focal+dice', focal_gamma=2.0))
    start = {k: p.detach().clone() for k, p in named}
    buf0 = {k: v.clone() for k, v in _bn_buffers(model).items()}
    g0 = {k: ts.grads[k].clone() for k in frozen}
    for _ in range(3):
        loss = ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(ts.last_terms).all()
    assert abs(loss.item() - float(ts.last_terms.sum())) < 1e-6            # weights (1, 1)
    for k in frozen:
        assert torch.equal(dict(named)[k].detach(), start[k]) and torch.equal(ts.grads[k], g0[k]), k
        for key, t in ts.opt_state.items():
            assert not bool(ts.layout.view(t, k).any()), (k, key)
    buf1 = _bn_buffers(model)
    assert buf0 and all(torch.equal(buf0[k], buf1[k]) for k in buf0)
    assert all(not torch.equal(dict(named)[k].detach(), start[k]) for k in w)
    sd = ts.optimizer_state_dict()
    by = dict(named)
    opt = torch.optim.AdamW([dict(g, params=[by[k] for k in g['params']]) for g in groups], lr=1e-2)
    opt.load_state_dict(sd)
    index = {k: i for i, (k, _) in enumerate(named)}
    assert set(sd['state']) == {index[k] for k in w + nb} and len(sd['param_groups']) == 2
    assert all(float(s['step']) == 3 for s in sd['state'].values())
    assert all(opt.state[by[k]] for k in w + nb) and not any(by[k] in opt.state and opt.state[by[k]] for k in frozen)


# ---------------------------------------------------------------- the command line
@pytest.mark.parametrize('loss_function', ['focal+dice', 'dice'])
def test_cli_fused_step_with_a_frozen_stem(tmp_path, loss_function):
    """python -m fabric_amd.train --synthetic --epochs 1 --fused_step true --loss_function L --focal_gamma 2 --freeze inc --optimizer adamw.
    The run starts from a state dict written here (--init_from), so that "the initial inc.* tensors" are known to the test."""
    from fabric_amd.utils.helpers import load_checkpoint
    torch.manual_seed(4)
    init = {'module.' + k: v.clone() for k, v in BiDateNet(13, 2).state_dict().items()}
    torch.save(init, tmp_path / 'init.state_dict.pt')
    r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', '--fused_step', 'true', '--loss_function',
                        loss_function, '--focal_gamma', '2', '--freeze', 'inc', '--optimizer', 'adamw', '--num_workers', '0',
                        '--init_from', str(tmp_path / 'init.state_dict.pt'), '--log_dir', str(tmp_path / 'log')],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"epoch"')][-1])
    assert line['epoch'] == 0
    for k in ('train_cd_losses', 'validate_cd_losses'):
        assert line[k] == line[k] and abs(line[k]) < float('inf'), (k, line[k])
    got = load_checkpoint(str(tmp_path / 'log' / 'checkpoint_epoch_0.state_dict.pt')).state_dict()
    for k, v in got.items():
        if k.startswith('inc.') and v.is_floating_point() and 'running_' not in k:
            assert torch.equal(v, init['module.' + k]), k
    assert not torch.equal(got['outc.conv.weight'], init['module.outc.conv.weight'])
