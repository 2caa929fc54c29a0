"""-m gpu: soft targets through the Python surface -- Criterion.evaluate's routing, TrainStep.step(weights=) and float targets, the add-on
terms behind the soft entry point, and CompoundLoss under autograd.  The float64 yardsticks are tests/soft_ref.py, tests/lovasz_ref.py
and tests/edt_ref.py with the bars of tests/test_gpu_soft.py."""
import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd.criterion import Criterion
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.metrics import CompoundLoss
from oracle import filler
from tests import edt_ref as ER
from tests import lovasz_ref as LR
from tests import soft_ref as SR

pytestmark = pytest.mark.gpu

dev = 'cuda'
LOSS_TOL, GRAD_TOL = 5e-6, 3e-4


def _inputs(b=4, c=3, s=32, seed=3, masked=False):
    """filler inputs (tests/test_gpu_step_ignore.py's); `masked` paints a rectangular unlabelled region per image with 255."""
    x1, x2, lbl = (torch.from_numpy(v) for v in filler.make_inputs(b, c, s, seed=seed))
    lbl = lbl.clone()
    if masked:
        for i in range(b):
            lbl[i, 3 + 2 * i:15 + 3 * i, 5 * i:s // 2 + 4 * i] = 255
    return x1.to(dev), x2.to(dev), lbl.to(dev)


def _soft_inputs(b=4, s=32, seed=7):
    """float32 [B,2,H,W] Dirichlet(0.5) targets and [B,H,W] weights (30 % zeros, the rest in (0, 2)) on the device."""
    r = np.random.default_rng(seed)
    q = np.ascontiguousarray(r.dirichlet([0.5, 0.5], (b, s, s)).astype(np.float32).transpose(0, 3, 1, 2))
    w = r.uniform(1e-3, 2.0, (b, s, s)).astype(np.float32)
    w[r.random((b, s, s)) < 0.3] = 0.0
    return torch.from_numpy(q).to(dev), torch.from_numpy(w).to(dev)


def _model():
    return filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()


def _names(monkeypatch):
    """Record the entry points _lib.call is asked for."""
    names, real = [], _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    return names


# ---------------------------------------------------------------- routing
def test_evaluate_routes_soft_inputs_to_the_soft_entry_point_and_nothing_else(monkeypatch):
    _, _, lbl = _inputs()
    q, w = _soft_inputs()
    lg = torch.randn(4, 2, 32, 32, device=dev)
    names = _names(monkeypatch)
    old = [(Criterion.parse('focal+dice', focal_gamma=2.0), 'bdn_criterion'),
           (Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255), 'bdn_criterion_masked'),
           (Criterion.parse('focal+dice', focal_gamma=2.0, topk=0.5), 'bdn_criterion_topk')]
    for c, want in old:                                     # the defaults take the entry points they always took
        del names[:]
        out = c.evaluate(lg, lbl)
        assert names == [want] and out[2].shape[0] == {'bdn_criterion': 4, 'bdn_criterion_masked': 5, 'bdn_criterion_topk': 6}[want]
    plain, smooth = old[0][0], Criterion.parse('focal+dice', focal_gamma=2.0, label_smoothing=0.1)
    for c, kw in ((smooth, dict(labels=lbl)), (plain, dict(labels=lbl, weights=w)), (plain, dict(labels=q)), (plain, dict(labels=q, weights=w)),
                  (old[1][0], dict(labels=lbl, weights=w)), (smooth, dict(labels=lbl[:, None], weights=w[:, None]))):
        del names[:]
        loss, terms, counts, dl = c.evaluate(lg, **kw)
        assert names == ['bdn_criterion_soft'] and counts.shape == (5,) and terms.shape == (2,) and torch.isfinite(dl).all()
    del names[:]
    lov = Criterion.parse('focal+lovasz', label_smoothing=0.1, w_boundary=0.1)
    assert lov.evaluate(lg, lbl)[1].shape == (4,) and names == ['bdn_criterion_soft', 'bdn_lovasz_softmax', 'bdn_boundary_loss']
    # buffers of the hard-label route are refused by the soft one, not overrun
    with pytest.raises(RuntimeError, match='soft=True'):
        plain.evaluate(lg, lbl, weights=w, out=plain.buffers(lg.shape, lg.device))
    out = plain.buffers(lg.shape, lg.device, soft=True)
    assert out[3].shape == (5,) and plain.evaluate(lg, lbl, weights=w, out=out)[0] is out[1]
    assert smooth.buffers(lg.shape, lg.device)[3].shape == (5,)
    # the values: weights of one and smoothing 0 are the masked criterion's function
    a, b = plain.evaluate(lg, lbl, weights=torch.ones_like(w)), old[1][0].evaluate(lg, lbl)
    assert abs(a[0].item() - b[0].item()) <= 1e-5 and torch.equal(a[2], b[2])


# ---------------------------------------------------------------- the train step
def test_step_with_label_smoothing_is_the_criterion_on_its_logits():
    x1, x2, lbl = _inputs(masked=True)
    c = Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255, label_smoothing=0.1)
    ts = TrainStep(_model(), lr=1e-3, criterion=c)
    loss = ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    l2, terms, counts, dlogits = c.evaluate(ts.last_logits, lbl)
    assert torch.equal(loss, l2) and torch.equal(ts.last_dlogits, dlogits) and torch.equal(ts.last_terms, terms)
    assert torch.equal(ts.last_counts, counts) and ts.last_counts.shape == (5,) and ts.last_terms.shape == (2,)
    assert not ts.last_dlogits[(lbl == 255)[:, None].expand(-1, 2, -1, -1)].any() and ts.last_dlogits.any()
    ref = SR.reference(c, ts.last_logits.cpu(), lbl.cpu())
    assert abs(loss.item() - ref['loss']) <= LOSS_TOL * (c.w_overlap * max(1.0, abs(ref['overlap'])) + c.w_focal * max(1.0, abs(ref['focal'])))
    plain = Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255)
    assert abs(loss.item() - plain.evaluate(ts.last_logits, lbl)[0].item()) > 1e-3      # the smoothing is in the loss
    # a second step of the same object, with float targets and weights
    q, w = _soft_inputs()
    ts2 = TrainStep(_model(), lr=1e-3, criterion=Criterion.parse('focal+dice', focal_gamma=2.0))
    ts2.step(x1, x2, lbl.clamp(max=1))
    assert ts2.last_counts.shape == (4,)
    before = ts2.flat_params.clone()
    loss2 = ts2.step(x1, x2, q, weights=w)
    torch.cuda.synchronize()
    lg = ts2.last_logits.cpu()
    assert ts2.last_counts.cpu().tolist() == SR.counts(ts2.criterion, lg, q.cpu(), w.cpu()) and ts2.last_terms.shape == (2,)
    l3, _, _, dl3 = ts2.criterion.evaluate(ts2.last_logits, q, weights=w)
    assert torch.equal(loss2, l3) and torch.equal(ts2.last_dlogits, dl3) and not ts2.last_dlogits[(w == 0)[:, None].expand(-1, 2, -1, -1)].any()
    assert torch.isfinite(ts2.flat_params).all() and not torch.equal(ts2.flat_params, before)
    ts2.step(x1, x2, lbl.clamp(max=1))                      # and back: the hard-label buffers are still there
    assert ts2.last_counts.shape == (4,)


def test_sam_and_accumulation_see_the_same_targets_and_weights():
    x1, x2, _ = _inputs()
    q, w = _soft_inputs()
    mk = lambda lr=1e-3, **kw: TrainStep(_model(), lr=lr, criterion=Criterion.parse('focal+dice', focal_gamma=2.0), **kw)
    one = mk(lr=0.0)
    one.step(x1, x2, q, weights=w)
    acc = mk(accumulate=2)
    acc.step(x1, x2, q, weights=w)
    torch.cuda.synchronize()
    assert acc.micro == 1 and torch.equal(acc.flat_accum, one.flat_grads)
    sam = mk(sam_rho=0.05)
    loss = sam.step(x1, x2, q, weights=w)
    torch.cuda.synchronize()
    assert torch.equal(sam.last_counts, one.last_counts) and torch.isfinite(sam.last_sam_loss) and torch.isfinite(loss)
    assert sam._weights is None


def test_default_step_refuses_soft_inputs_before_any_launch(monkeypatch):
    x1, x2, lbl = _inputs()
    q, w = _soft_inputs()
    ts = TrainStep(_model(), lr=1e-3)
    names = _names(monkeypatch)
    with pytest.raises(ValueError, match="criterion='tversky'"):
        ts.step(x1, x2, lbl, weights=w)
    with pytest.raises(ValueError, match="criterion='tversky'"):
        ts.step(x1, x2, q)
    assert names == []


# ---------------------------------------------------------------- the add-on terms behind the soft entry point
@pytest.mark.parametrize('addon', ['lovasz', 'boundary', 'lovasz+weights'])
def test_add_on_terms_compose_with_smoothing_and_weights(addon):
    _, _, lbl = _inputs(masked=True)
    _, w = _soft_inputs()
    lg = 2 * torch.randn(4, 2, 32, 32, device=dev, generator=torch.Generator(dev).manual_seed(5))
    kw = dict(w_overlap=0.5, alpha=0.5, beta=0.5, w_focal=1.0, gamma=2.0, ignore_index=255)
    if addon == 'boundary':
        c, base = Criterion(w_boundary=0.2, label_smoothing=0.1, **kw), Criterion(label_smoothing=0.1, **kw)
    elif addon == 'lovasz':
        c, base = Criterion(w_lovasz=0.75, label_smoothing=0.1, **kw), Criterion(label_smoothing=0.1, **kw)
    else:
        c, base = Criterion(w_lovasz=0.75, **kw), Criterion(**kw)
    weights = w if addon == 'lovasz+weights' else None
    loss, terms, counts, dl = c.evaluate(lg, lbl, weights=weights)
    torch.cuda.synchronize()
    assert terms.shape == (3,) and counts.shape == (5,)
    lg_c, lbl_c = lg.cpu(), lbl.cpu()
    ref = SR.reference(base, lg_c, lbl_c, None if weights is None else weights.cpu())
    if addon == 'boundary':
        t64, d64, _ = ER.boundary_loss_ref(lg_c.numpy(), lbl_c.numpy().astype('uint8'), 255, False, None)
        d64, w_add = torch.from_numpy(np.asarray(d64)), c.w_boundary
    else:
        r = LR.evaluate(lg_c, lbl_c, 255, 'present')
        t64, d64, w_add = r['term'], r['dlogits'], c.w_lovasz
    want = ref['loss'] + w_add * t64
    lb = LOSS_TOL * (c.w_overlap * max(1.0, abs(ref['overlap'])) + c.w_focal * max(1.0, abs(ref['focal'])) + w_add * max(1.0, abs(t64)))
    gb = GRAD_TOL * (c.w_overlap * ref['doverlap'].abs().max().item() + c.w_focal * ref['dfocal'].abs().max().item()
                     + w_add * d64.abs().max().item())
    e_loss, e_grad = abs(loss.item() - want), (dl.cpu().double() - (ref['dloss'] + w_add * d64)).abs().max().item()
    print(f'{addon}: |loss err| {e_loss:.3e} (bound {lb:.3e}) max|dlogits err| {e_grad:.3e} (bound {gb:.3e})')
    assert e_loss <= lb and e_grad <= gb
    t = terms.cpu().tolist()
    assert abs(t[0] - ref['overlap']) <= LOSS_TOL * max(1.0, abs(ref['overlap'])) and abs(t[1] - ref['focal']) <= LOSS_TOL * max(1.0, abs(ref['focal']))
    assert abs(t[2] - t64) <= LOSS_TOL * max(1.0, abs(t64))
    assert counts.cpu().tolist() == SR.counts(base, lg_c, lbl_c, None if weights is None else weights.cpu())
    with pytest.raises(ValueError, match='do not take float targets'):
        c.evaluate(lg, _soft_inputs()[0])


# ---------------------------------------------------------------- autograd
def test_compound_loss_takes_soft_inputs_under_autograd():
    _, _, lbl = _inputs(masked=True)
    q, w = _soft_inputs()
    lg = torch.randn(4, 2, 32, 32, device=dev)
    for c, true, weights in ((Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255, label_smoothing=0.1), lbl, None),
                             (Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255), lbl, w),
                             (Criterion.parse('focal+tversky', focal_gamma=0.0), q, w), (Criterion.parse('dice'), q, None)):
        loss, terms, counts, dl = c.evaluate(lg, true, weights=weights)
        mod = CompoundLoss(c)
        x = lg.clone().requires_grad_(True)
        v = mod(x, true) if weights is None else mod(x, true, weights)
        (3.0 * v).backward()
        assert torch.equal(v.detach(), loss) and torch.equal(x.grad, dl * 3.0)
        assert torch.equal(mod.last_counts, counts) and torch.equal(mod.last_terms, terms) and mod.last_counts.shape == (5,)
        with torch.no_grad():
            assert torch.equal(mod(lg, true, weights), loss)
