"""-m gpu: the fused train step and the training CLI with an ignore label (TrainStep(criterion=Criterion(..., ignore_index=255)),
python -m fabric_amd.train --ignore_label).

The oracle's step is tests/test_gpu_step_criterion.py's with tests/ignore_ref.py's restatement for the loss: O.bidate_forward -> masked
loss -> torch.autograd.grad -> SGD, held to the bars of test_first_step_matches_the_oracle_step, unchanged."""
import json
import math
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
from tests import ignore_ref as IR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = 'cuda'


def _inputs(b=4, c=3, s=32, seed=3, masked=True):
    """filler inputs; the labels carry a rectangular unlabelled region (another one per image) painted 255."""
    x1, x2, lbl = (torch.from_numpy(v) for v in filler.make_inputs(b, c, s, seed=seed))
    if masked:
        lbl = lbl.clone()
        for i in range(b):
            lbl[i, 3 + 2 * i:15 + 3 * i, 5 * i:s // 2 + 4 * i] = 255
        assert (lbl == 255).any() and (lbl == 1).any() and (lbl == 0).any()
    return x1, x2, lbl


def _oracle_step(c, sd, x1, x2, lbl, lr):
    """O.train_step with the masked criterion's restatement for the loss."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running_' not in k}
    full = dict(sd)
    full.update(params)
    logits, new_buf = O.bidate_forward(full, x1, x2, training=True)
    loss = IR.loss(c, logits, lbl)[0]
    names = list(params)
    grads = torch.autograd.grad(loss, [params[k] for k in names])
    new_sd = {k: v.clone() for k, v in sd.items()}
    for k, g in zip(names, grads):
        new_sd[k] = (sd[k] - lr * g).detach()
    for k, v in new_buf.items():
        new_sd[k] = v.detach()
    return dict(logits=logits.detach(), loss=float(loss.detach()), grads=dict(zip(names, [g.detach() for g in grads])), new_sd=new_sd)


def _grad_errors(got, ref):
    """tests/test_gpu_step_criterion.py's: worst per-parameter max(relative L2 error, relative error of the norm), cosine of the whole."""
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


_CRITERIA = {'dice': lambda: Criterion.parse('dice', ignore_index=255),
             'focal2+dice': lambda: Criterion.parse('focal+dice', focal_gamma=2.0, weights=(1, 1), ignore_index=255)}


@pytest.mark.parametrize('prec', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', list(_CRITERIA))
def test_first_masked_step_matches_the_oracle_step(name, prec):
    c, lr = _CRITERIA[name](), 1e-3
    x1, x2, lbl = _inputs()
    ignored = lbl == 255
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
    # the step's own loss gradient is what Criterion.evaluate gives on the step's logits, bit for bit; five counts; zero where ignored
    _, terms, counts, dlogits = c.evaluate(ts.last_logits, dl)
    assert torch.equal(ts.last_dlogits, dlogits) and torch.equal(ts.last_terms, terms) and torch.equal(ts.last_counts, counts)
    assert ts.last_counts.shape == (5,) and ts.last_counts.cpu().tolist() == IR.counts(got, lbl, 255)
    assert int(ts.last_counts[4]) == int((~ignored).sum())
    assert not ts.last_dlogits.cpu()[ignored[:, None].expand(-1, 2, -1, -1)].any() and ts.last_dlogits.any()
    logits2 = model(dx1, dx2).detach().cpu()
    ref2, _ = O.bidate_forward(ref['new_sd'], x1, x2, training=True)
    assert (logits2 - ref2).abs().max() <= 1e-3


def test_default_step_is_untouched_by_the_feature():
    x1, x2, lbl = (t.to(dev) for t in _inputs(masked=False))
    ts = TrainStep(filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train(), lr=1e-3)
    ts.step(x1, x2, lbl)
    assert ts.criterion is None and ts.last_counts.shape == (4,) and ts.last_terms is None
    named = TrainStep(filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train(), lr=1e-3, criterion='dice')
    named.step(x1, x2, lbl)
    assert named.criterion.ignore_index is None and named.last_counts.shape == (4,)


# ---------------------------------------------------------------- a batch without a valid pixel
def test_an_all_ignored_batch_leaves_plain_sgd_parameters_unchanged():
    x1, x2, lbl = _inputs()
    lbl = torch.full_like(lbl, 255)
    for extra in ({}, {'max_grad_norm': float('inf')}):
        model = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()
        ts = TrainStep(model, lr=0.05, criterion=Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255), **extra)
        before = ts.flat_params.clone()
        loss = ts.step(x1.to(dev), x2.to(dev), lbl.to(dev))
        torch.cuda.synchronize()
        assert loss.item() == 1.0 and ts.last_terms.cpu().tolist() == [1.0, 0.0] and ts.last_counts.cpu().tolist() == [0] * 5
        assert not ts.last_dlogits.any() and not ts.flat_grads.any()
        assert torch.equal(ts.flat_params, before), extra
        if extra:
            assert float(ts.last_grad_norm) == 0.0 and math.isfinite(float(ts.last_clip_coef))


# ---------------------------------------------------------------- accumulation
def test_accumulate_over_a_masked_and_an_unmasked_micro_batch():
    c = lambda: Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255)
    batches = [tuple(t.to(dev) for t in _inputs(seed=3, masked=True)), tuple(t.to(dev) for t in _inputs(seed=4, masked=False))]
    twin = TrainStep(filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train(), lr=0.0, criterion=c())
    gs, valid = [], []
    for b in batches:
        twin.step(*b)
        gs.append(twin.flat_grads.clone())
        valid.append(int(twin.last_counts[4]))
    assert valid[0] < valid[1] == batches[1][2].numel() and not torch.equal(gs[0], gs[1])
    ts = TrainStep(filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train(), lr=1e-3, accumulate=2, criterion=c())
    p0 = ts.flat_params.clone()
    ts.step(*batches[0])
    torch.cuda.synchronize()
    assert ts.micro == 1 and torch.equal(ts.flat_accum, gs[0]) and torch.equal(ts.flat_params, p0)
    ts.step(*batches[1])
    torch.cuda.synchronize()
    total = gs[1] + gs[0]                                   # micro-step K: flat_grads = gK + acc, one float32 add per element
    assert ts.micro == 0 and ts.opt_step == 0 and torch.equal(ts.flat_grads, total), float((ts.flat_grads - total).abs().max())
    assert torch.isfinite(ts.flat_params).all() and not torch.equal(ts.flat_params, p0)


# ---------------------------------------------------------------- metrics over valid pixels
def test_validate_reports_accuracy_over_the_valid_pixels():
    from fabric_amd.train import validate
    from fabric_amd.utils.metrics import CompoundLoss
    c = Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255)
    model = filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev)
    x1, x2, lbl = _inputs(seed=5)
    none = torch.full_like(lbl, 255)                        # a batch without a valid pixel contributes 0
    va = validate(model, [(x1, x2, lbl), (x1, x2, none)], dev, 32, CompoundLoss(c), ignore_index=255)
    model.eval()
    with torch.no_grad():
        pred = model(x1.to(dev), x2.to(dev)).argmax(1).cpu()
    v = lbl != 255
    want = 100.0 * int(((pred == lbl) & v).sum()) / int(v.sum())
    assert abs(va['cd_corrects'] - (want + 0.0) / 2) < 1e-9, (va, want)
    assert want > 100.0 * int((pred == lbl).sum()) / lbl.numel()         # over all pixels it would read lower
    assert all(math.isfinite(float(x)) for x in va.values())


# ---------------------------------------------------------------- the command line
def test_cli_fused_step_with_an_ignore_label(tmp_path):
    """python -m fabric_amd.train --synthetic --fused_step true --loss_function focal+dice --focal_gamma 2 --ignore_label 255: one epoch
    on synthetic_onera(ignore_frac > 0) data, in a fresh child process."""
    r = subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', '--fused_step', 'true', '--loss_function',
                        'focal+dice', '--focal_gamma', '2', '--ignore_label', '255', '--num_workers', '0', '--log_dir', str(tmp_path / 'log')],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"epoch"')][-1])
    assert line['epoch'] == 0
    for k, v in line.items():
        assert math.isfinite(v), (k, v)
    for k in ('train_cd_corrects', 'validate_cd_corrects'):
        assert 0.0 <= line[k] <= 100.0, (k, line[k])
    for k in ('train_cd_losses', 'validate_cd_losses'):
        assert line[k] > 0.0, (k, line[k])
