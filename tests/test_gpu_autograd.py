"""-m gpu: gradients on the input images and backward after model.eval() through BiDateNet's autograd node, against the float64
oracle (oracle.bidate_oracle.bidate_forward + tversky_loss(alpha=0.1, beta=0.9)), and the invariances the feature promises: a backward
with input gradients changes nothing else, the eval forward is the eval forward, an eval backward leaves the running buffers alone and
does not disturb a live training graph, frozen layers launch no weight-gradient GEMM."""
import functools
import os

import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet, _lib
from oracle import bidate_oracle as O
from oracle import filler

pytestmark = pytest.mark.gpu

CASES = ['g1_c3_b4_s32', 'g4_c13_b2_s90', 'g6_c3_b4_s32_diffdates', 'g8_c13_b3_h40_w72']
PRECS = ['fp32', 'bf16x3', 'bf16x3-fast', 'bf16']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _inputs(name):
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    c, b, s, sw, dd = [int(v) for v in g['meta']]
    x1, x2, lbl = filler.make_inputs(b, c, s, seed=0, different_dates=bool(dd), size_w=sw)
    return c, torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(lbl)


def _tversky(logits, labels, alpha=0.1, beta=0.9, eps=1e-7):
    nc = logits.shape[1]
    one_hot = torch.eye(nc, device=logits.device, dtype=logits.dtype)[labels.long()].permute(0, 3, 1, 2)
    probas = torch.softmax(logits, dim=1)
    inter = torch.sum(probas * one_hot, (0, 2))
    fps = torch.sum(probas * (1 - one_hot), (0, 2))
    fns = torch.sum((1 - probas) * one_hot, (0, 2))
    return 1 - (inter / (inter + alpha * fps + beta * fns + eps)).mean()


@functools.lru_cache(maxsize=None)
def _oracle(name, training):
    """float64 gradients of the Tversky loss on the inputs and every parameter (the oracle's own autograd)."""
    c, x1, x2, lbl = _inputs(name)
    sd = filler.fill_module(BiDateNet(c, 2)).state_dict()
    sd = {k: (v.double() if v.is_floating_point() else v).clone() for k, v in sd.items()}
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running_' not in k}
    x1d, x2d = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    logits, _ = O.bidate_forward(sd, x1d, x2d, training=training)
    loss = O.tversky_loss(logits, lbl.long(), 0.1, 0.9)
    names = list(params)
    gr = torch.autograd.grad(loss, [x1d, x2d] + [params[k] for k in names])
    return {'x1': gr[0], 'x2': gr[1], **dict(zip(names, gr[2:]))}


def _bounds(prec):
    """(relative L2 bound, cosine bound) per gradient tensor.  The relative L2 bounds are test_train_step_matches_reference's for the
    weight gradients.  The cosine bounds are looser than that test's whole-vector ones: the input gradient is the END of the chain
    (every dz rounding of the 18 layers lands on it).  Measured minima over these cases: bf16x3 / bf16x3-fast 0.99979 (x2 on
    g8, train), 0.99989 for a parameter (inc.conv.conv.1.weight, eval); bf16 0.907 (x1 on g6) -- the deep encoder's weight gradients
    of the bf16 reference itself deviate 0.30-0.43 relative L2 from float32."""
    return {'fp32': (2e-2, None), 'bf16x3': (6e-2, 0.9995), 'bf16x3-fast': (6e-2, 0.9995), 'bf16': (0.8, 0.85)}[prec]


def _check(key, got, ref, prec):
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    rn = float(ref.norm())
    assert torch.isfinite(got).all(), key
    if rn < 1e-12:                                       # conv biases in front of a training-mode BatchNorm: identically zero
        assert float(got.norm()) < 1e-6, (key, float(got.norm()))
        return
    rel = float((got - ref).norm()) / rn
    cos = float((got * ref).sum()) / (float(got.norm()) * rn + 1e-300)
    lim, cmin = _bounds(prec)
    assert rel < lim, f'{key}: relative L2 {rel:.3e} >= {lim}'
    if cmin is not None:
        assert cos >= cmin, f'{key}: cosine {cos:.6f} < {cmin}'


def _model(name, prec, training):
    c, x1, x2, lbl = _inputs(name)
    model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda()
    model.train(training)
    return model, x1.cuda(), x2.cuda(), lbl.cuda()


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', CASES)
def test_train_mode_input_gradient_matches_oracle(name, prec):
    model, x1, x2, lbl = _model(name, prec, True)
    x1.requires_grad_()
    x2.requires_grad_()
    loss = _tversky(model(x1, x2), lbl)
    loss.backward()
    ref = _oracle(name, True)
    assert x1.grad is not None and x2.grad is not None
    assert x1.grad.shape == x1.shape and x1.grad.dtype == torch.float32
    _check('x1', x1.grad, ref['x1'], prec)
    _check('x2', x2.grad, ref['x2'], prec)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', CASES)
def test_eval_mode_backward_matches_oracle(name, prec):
    model, x1, x2, lbl = _model(name, prec, False)
    x1.requires_grad_()
    x2.requires_grad_()
    bufs = {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k or 'num_batches' in k}
    loss = _tversky(model(x1, x2), lbl)
    loss.backward()
    ref = _oracle(name, False)
    _check('x1', x1.grad, ref['x1'], prec)
    _check('x2', x2.grad, ref['x2'], prec)
    n = 0
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        _check(k, p.grad, ref[k], prec)
        n += 1
    assert n == 74
    for k, v in model.state_dict().items():
        if k in bufs:
            assert torch.equal(v, bufs[k]), f'{k} moved in an eval-mode backward'


def test_input_grad_first_call_sites():
    """The plain autograd surface: x.grad after loss.backward() and torch.autograd.grad in eval mode."""
    model, x1, x2, lbl = _model('g1_c3_b4_s32', 'bf16', True)
    x1.requires_grad_()
    _tversky(model(x1, x2), lbl).backward()
    assert x1.grad is not None and x2.grad is None
    model.eval()
    xe = x1.detach().clone().requires_grad_()
    (gx,) = torch.autograd.grad(_tversky(model(xe, x2), lbl), xe)
    assert gx.shape == xe.shape and torch.isfinite(gx).all() and float(gx.abs().max()) > 0


@pytest.mark.parametrize('prec', ['bf16', 'bf16x3'])
def test_same_tensor_as_both_dates_sums_the_two_gradients(prec):
    model, x1, _, lbl = _model('g1_c3_b4_s32', prec, True)
    xa = x1.clone().requires_grad_()
    _tversky(model(xa, xa), lbl).backward()
    model2, _, _, _ = _model('g1_c3_b4_s32', prec, True)
    xb, xc = x1.clone().requires_grad_(), x1.clone().requires_grad_()
    _tversky(model2(xb, xc), lbl).backward()
    assert torch.equal(xa.grad, xb.grad + xc.grad)


@pytest.mark.parametrize('prec', PRECS)
def test_training_backward_unchanged_by_input_gradients(prec):
    """Parameter gradients, logits and BatchNorm buffers are bit-identical with and without input gradients."""
    out = []
    for want in (False, True):
        model, x1, x2, lbl = _model('g8_c13_b3_h40_w72', prec, True)
        if want:
            x1.requires_grad_()
            x2.requires_grad_()
        logits = model(x1, x2)
        _tversky(logits, lbl).backward()
        torch.cuda.synchronize()
        out.append((logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()},
                    {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k or 'num_batches' in k}))
    (l0, g0, b0), (l1, g1, b1) = out
    assert torch.equal(l0, l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


@pytest.mark.parametrize('prec', PRECS)
def test_eval_forward_with_grad_is_the_eval_forward(prec):
    model, x1, x2, lbl = _model('g4_c13_b2_s90', prec, False)
    P = {k: v.detach() for k, v in model.state_dict(keep_vars=True).items()}
    ref, _ = model.engine().forward(x1, x2, P, training=False)
    ref = ref.clone()
    x1.requires_grad_()
    logits = model(x1, x2)
    assert logits.requires_grad
    assert torch.equal(logits.detach(), ref)


@pytest.mark.parametrize('prec', ['bf16', 'bf16x3'])
def test_eval_backward_between_a_training_forward_and_its_backward(prec):
    """A live training graph keeps its activations across an eval forward + backward of the same shape; both results equal
    those of separate runs."""
    def train_run(model, x1, x2, lbl):
        model.train()
        loss = _tversky(model(x1, x2), lbl)
        return loss

    def eval_run(model, x1, x2, lbl):
        model.eval()
        xe = x1.detach().clone().requires_grad_()
        _tversky(model(xe, x2), lbl).backward()
        g = {k: p.grad.clone() for k, p in model.named_parameters()}
        model.zero_grad(set_to_none=True)
        return xe.grad.clone(), g

    # separate runs
    m_a, x1, x2, lbl = _model('g1_c3_b4_s32', prec, True)
    train_run(m_a, x1, x2, lbl).backward()
    ref_train = {k: p.grad.clone() for k, p in m_a.named_parameters()}
    m_b, _, _, _ = _model('g1_c3_b4_s32', prec, True)
    with torch.no_grad():                                # the running statistics move as the interleaved run's training forward moves them
        m_b(x1, x2)
    ref_eval = eval_run(m_b, x1, x2, lbl)
    # interleaved on one model: training forward, eval forward + backward, training backward
    m, _, _, _ = _model('g1_c3_b4_s32', prec, True)
    loss = train_run(m, x1, x2, lbl)
    ev = eval_run(m, x1, x2, lbl)
    m.train()
    loss.backward()
    assert torch.equal(ev[0], ref_eval[0])
    for k in ref_eval[1]:
        assert torch.equal(ev[1][k], ref_eval[1][k]), k
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, ref_train[k]), k


def _record_launches(monkeypatch):
    names = []
    real = _lib.call

    def rec(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    import fabric_amd.engine as E
    monkeypatch.setattr(E, 'call', rec)
    return names


WGRAD_GEMMS = ('bdn_conv3x3_wgrad_ex', 'bdn_conv3x3_wgrad_bnbwd', 'bdn_conv3x3_wgrad')


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('training', [False, True])
def test_frozen_model_input_gradient(monkeypatch, prec, training):
    """Attribution on a frozen model: the input gradient is bit-identical to the unfrozen run, p.grad stays None and no
    weight-gradient GEMM is launched."""
    model, x1, x2, lbl = _model('g8_c13_b3_h40_w72', prec, training)
    xa = x1.clone().requires_grad_()
    _tversky(model(xa, x2), lbl).backward()
    ref = xa.grad.clone()
    model, _, _, _ = _model('g8_c13_b3_h40_w72', prec, training)
    for p in model.parameters():
        p.requires_grad_(False)
    xb = x1.clone().requires_grad_()
    names = _record_launches(monkeypatch)
    _tversky(model(xb, x2), lbl).backward()
    torch.cuda.synchronize()
    assert torch.equal(xb.grad, ref)
    assert all(p.grad is None for p in model.parameters())
    assert 'bdn_conv3x3_dgrad_first' in names
    assert not [n for n in names if n in WGRAD_GEMMS], [n for n in names if n in WGRAD_GEMMS]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('training', [False, True])
def test_frozen_encoder_leaves_decoder_gradients_unchanged(prec, training):
    out = []
    for freeze in (False, True):
        model, x1, x2, lbl = _model('g1_c3_b4_s32', prec, training)
        if freeze:
            for name, p in model.named_parameters():
                if name.startswith(('inc.', 'down')):
                    p.requires_grad_(False)
        _tversky(model(x1, x2), lbl).backward()
        torch.cuda.synchronize()
        out.append({k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()})
    full, part = out
    for k, g in part.items():
        if k.startswith(('inc.', 'down')):
            assert g is None, k
        else:
            assert torch.equal(g, full[k]), k
