"""-m gpu: the fused train step and the autograd route with top-k hard-pixel mining (TrainStep(criterion=Criterion(..., topk=f)),
utils.metrics.CompoundLoss).  The step against the autograd route is held to the bars tests/test_gpu_step_criterion.py holds a step to
(fp32: |loss| 1e-5, worst per-parameter gradient error 2e-2, cosine > 0.9999)."""
import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.criterion import Criterion
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.metrics import CompoundLoss
from oracle import filler
from tests import topk_ref as TR

pytestmark = pytest.mark.gpu

dev = 'cuda'


def _criterion(**kw):
    return Criterion.parse('focal+dice', focal_gamma=2, topk=0.25, ignore_index=255, **kw)


def _inputs(b=2, c=3, s=32, seed=3):
    """filler inputs; the labels carry a rectangular unlabelled region (another one per image) painted 255."""
    x1, x2, lbl = (torch.from_numpy(v) for v in filler.make_inputs(b, c, s, seed=seed))
    lbl = lbl.clone()
    for i in range(b):
        lbl[i, 3 + 2 * i:15 + 3 * i, 5 * i:s // 2 + 4 * i] = 255
    return x1.to(dev), x2.to(dev), lbl.to(dev)


def _model():
    return filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()


def _grad_errors(got, ref):
    """tests/test_gpu_step_criterion.py's: worst per-parameter max(relative L2 error, relative error of the norm), cosine of the whole."""
    worst, worst_key, allg, allr = 0.0, None, [], []
    for k, r in ref.items():
        g, r = got[k].detach().cpu().double().reshape(-1), r.detach().cpu().double().reshape(-1)
        if float(r.norm()) < 1e-6:
            assert float(g.norm()) < 1e-6, k
            continue
        e = max(float((g - r).norm() / r.norm()), abs(float(g.norm()) - float(r.norm())) / float(r.norm()))
        allg.append(g)
        allr.append(r)
        if e > worst:
            worst, worst_key = e, k
    ag, ar = torch.cat(allg), torch.cat(allr)
    return worst, worst_key, float((ag * ar).sum() / (ag.norm() * ar.norm()))


def test_step_with_topk_reports_k_and_the_threshold_and_agrees_with_the_autograd_route():
    c = _criterion()
    x1, x2, lbl = _inputs()
    ts = TrainStep(_model(), lr=0.0, criterion=c)
    loss = ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    n_valid = int((lbl != 255).sum())
    assert ts.last_counts.shape == (6,) and ts.last_terms.shape == (3,)
    assert ts.last_counts.cpu().tolist()[4:] == [n_valid, TR.kept_count(n_valid, 250_000)]
    # the step's loss gradient is what Criterion.evaluate gives on the step's logits, bit for bit; terms[2] is the K-th largest exported term
    pt = torch.empty(lbl.numel(), device=dev)
    kept = torch.empty(lbl.numel(), dtype=torch.uint8, device=dev)
    l2, terms, counts, dlogits = c.evaluate(ts.last_logits, lbl, pixel_terms=pt, kept=kept)
    assert torch.equal(ts.last_dlogits, dlogits) and torch.equal(ts.last_terms, terms) and torch.equal(ts.last_counts, counts)
    assert torch.equal(loss, l2) and int(kept.sum()) == int(counts[5])
    assert ts.last_terms[2].item() == pt[kept.bool()].min().item() > 0
    ignored = (lbl == 255)[:, None].expand(-1, 2, -1, -1)
    assert not ts.last_dlogits[ignored].any() and ts.last_dlogits.any()
    # two steps from the same state are the same bits
    other = TrainStep(_model(), lr=0.0, criterion=_criterion())
    loss_b = other.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_b) and torch.equal(ts.flat_grads, other.flat_grads) and torch.equal(ts.last_dlogits, other.last_dlogits)
    assert torch.equal(ts.last_counts, other.last_counts) and torch.equal(ts.last_terms, other.last_terms)
    # the autograd route: the module's own backward under CompoundLoss(criterion)
    model = _model()
    mod = CompoundLoss(c)
    v = mod(model(x1, x2), lbl)
    v.backward()
    torch.cuda.synchronize()
    ref = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    gerr, gkey, gcos = _grad_errors(ts.grads, ref)
    print(f'\nstep loss {loss.item():.7f} autograd {v.item():.7f} worst grad err {gerr:.3e} @ {gkey} cos {gcos:.6f}')
    assert abs(loss.item() - v.item()) < 1e-5
    assert gerr < 2e-2 and gcos > 0.9999, (gkey, gerr, gcos)
    assert mod.last_counts.shape == (6,) and mod.last_counts.cpu().tolist()[4:] == ts.last_counts.cpu().tolist()[4:]


def test_accumulate_selects_per_micro_step():
    batches = [_inputs(seed=3), _inputs(seed=4)]
    twin = TrainStep(_model(), lr=0.0, criterion=_criterion())
    gs, ks = [], []
    for b in batches:
        twin.step(*b)
        gs.append(twin.flat_grads.clone())
        ks.append(twin.last_counts.cpu().tolist()[4:])
    for (valid, K), b in zip(ks, batches):
        assert valid == int((b[2] != 255).sum()) and K == TR.kept_count(valid, 250_000)
    ts = TrainStep(_model(), lr=1e-3, accumulate=2, criterion=_criterion())
    p0 = ts.flat_params.clone()
    ts.step(*batches[0])
    torch.cuda.synchronize()
    assert ts.micro == 1 and torch.equal(ts.flat_accum, gs[0]) and torch.equal(ts.flat_params, p0)
    assert ts.last_counts.cpu().tolist()[4:] == ks[0]
    ts.step(*batches[1])
    torch.cuda.synchronize()
    total = gs[1] + gs[0]                                   # micro-step 2: flat_grads = g2 + acc, one float32 add per element
    assert ts.micro == 0 and torch.equal(ts.flat_grads, total), float((ts.flat_grads - total).abs().max())
    assert ts.last_counts.cpu().tolist()[4:] == ks[1]       # its own K, from its own batch
    # plain SGD: the update is lr times the mean of the two separately evaluated gradients
    want = p0 - 1e-3 * (total / 2)
    assert (ts.flat_params - want).abs().max().item() <= 1e-7 * max(1.0, p0.abs().max().item())


def test_a_step_without_topk_launches_the_entry_point_it_always_did(monkeypatch):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    x1, x2, lbl = _inputs()
    for kw, entry in (({}, 'bdn_criterion'), ({'ignore_index': 255}, 'bdn_criterion_masked')):
        del names[:]
        for crit in (Criterion.parse('focal+dice', focal_gamma=2, **kw), Criterion.parse('focal+dice', focal_gamma=2, topk=None, **kw)):
            ts = TrainStep(_model(), lr=1e-3, criterion=crit)
            ts.step(x1, x2, lbl if kw else lbl.clamp(max=1))
            assert ts.last_counts.shape == (5 if kw else 4,) and ts.last_terms.shape == (2,)
        crits = [n for n in names if n.startswith('bdn_criterion')]
        assert crits == [entry] * 2, crits
    del names[:]
    ts = TrainStep(_model(), lr=1e-3, criterion=_criterion())
    ts.step(x1, x2, lbl)
    assert [n for n in names if n.startswith('bdn_criterion')] == ['bdn_criterion_topk']
