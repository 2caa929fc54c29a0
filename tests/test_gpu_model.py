"""-m gpu whole-model parity: fabric_amd.BiDateNet on the HIP library vs golden vectors captured from
the reference itself (tests/golden, oracle/make_golden.py) through the drop-in module surface:
BiDateNet(n_channels, n_classes), forward(x_d1, x_d2), autograd backward, torch.optim.SGD.

Stated tolerances:
  fp32 setting : per-pixel logits within 1e-3 of the reference (train mode), identical argmax except
                 where the reference's own top-2 margin is < 2e-3, loss within 1e-5, BatchNorm running
                 buffers within 1e-4, weight gradients within 2e-2 relative L2 (two float32
                 implementations differ by ~2e-3 already, see oracle/make_golden.py).
  bf16 setting : max |dlogit| <= 0.25, mean |dlogit| <= 0.03, argmax agreement >= 96 %, loss within
                 5e-3.  Gradients: the REFERENCE ITSELF under torch.autocast(bfloat16) deviates from its
                 own float32 gradients by 0.30-0.43 relative L2 on the deep encoder parameters (median
                 0.25-0.30 over parameters, whole-vector cosine 0.99; measured in the build container, see
                 DESIGN.md "tolerances"), so the bound here is per-parameter relative L2 <= 0.8 on the
                 sampled entries and cosine >= 0.97 over all sampled entries.  Kernel-level bf16
                 correctness is pinned separately and tightly in test_gpu_kernels.py.
"""
import os

import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet
from oracle import filler

pytestmark = pytest.mark.gpu

CASES = ['g1_c3_b4_s32', 'g2_c13_b2_s128', 'g4_c13_b2_s90', 'g6_c3_b4_s32_diffdates', 'g8_c13_b3_h40_w72']


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    c, b, s, sw, dd = [int(v) for v in g['meta']]
    x1, x2, lbl = filler.make_inputs(b, c, s, seed=0, different_dates=bool(dd), size_w=sw)
    return g, c, torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda(), torch.from_numpy(lbl).cuda()


def _tversky_torch(logits, labels, alpha=0.1, beta=0.9, eps=1e-7):
    # plain torch restatement of train.py's criterion so the test exercises BiDateNet's own autograd node
    from oracle.bidate_oracle import tversky_loss
    lg = logits
    true = labels.long()
    nc = lg.shape[1]
    one_hot = torch.eye(nc, device=lg.device)[true].permute(0, 3, 1, 2)
    probas = torch.softmax(lg, dim=1)
    dims = (0, 2)
    inter = torch.sum(probas * one_hot, dims)
    fps = torch.sum(probas * (1 - one_hot), dims)
    fns = torch.sum((1 - probas) * one_hot, dims)
    return 1 - (inter / (inter + alpha * fps + beta * fns + eps)).mean()


def _grad_errors(model, g):
    """relative L2 error of the sampled gradient entries per parameter, and of the norms."""
    worst, worst_key = 0.0, None
    allg, allr = [], []
    for k, p in model.named_parameters():
        ref = torch.from_numpy(g['gsamp/' + k]).double()
        refnorm = float(g['gnorm/' + k])
        if refnorm < 1e-6:          # conv biases feeding a BatchNorm: reference holds only rounding noise (~1e-9)
            assert float(p.grad.norm()) < 1e-6, k
            continue
        got = p.grad.detach().reshape(-1).cpu().double()[torch.from_numpy(g['gidx/' + k])]
        rel = float((got - ref).norm() / (ref.norm() + 1e-30))
        allg.append(got)
        allr.append(ref)
        nrel = abs(float(p.grad.double().norm()) - refnorm) / refnorm
        e = max(rel, nrel)
        if e > worst:
            worst, worst_key = e, k
    ag, ar = torch.cat(allg), torch.cat(allr)
    cos = float((ag * ar).sum() / (ag.norm() * ar.norm()))
    return worst, worst_key, cos


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('prec', ['fp32', 'bf16x3', 'bf16'])
def test_train_step_matches_reference(golden_dir, name, prec):
    g, c, x1, x2, lbl = _load(golden_dir, name)
    model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda()
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)           # train.py:55
    opt.zero_grad()
    logits = model(x1, x2)                                        # train.py:91
    loss = _tversky_torch(logits, lbl)                            # train.py:92
    loss.backward()                                               # train.py:94
    ref = torch.from_numpy(g['logits'])
    got = logits.detach().cpu()
    d = (got - ref).abs()
    agree = (got.argmax(1) == ref.argmax(1)).float().mean().item()
    gerr, gkey, gcos = _grad_errors(model, g)
    print(f'\n[{name} {prec}] max|dlogit|={d.max():.3e} mean={d.mean():.3e} argmax agree={agree:.4f} '
          f'loss={loss.item():.6f} (ref {float(g["loss"]):.6f}) worst grad err={gerr:.3e} @ {gkey} cos={gcos:.4f}')
    if prec in ('fp32', 'bf16x3'):
        # the 1e-3 parity bar of north_star holds in BOTH float32-class settings: exact f32 MFMA, and bf16 hi/lo split operands
        # (three bf16 MFMAs per product; 2^-16 relative per product, measured <= 2e-4 on the logits)
        assert d.max() <= 1e-3
        margin = (ref[:, 0] - ref[:, 1]).abs()
        assert ((got.argmax(1) == ref.argmax(1)) | (margin < 2e-3)).all()
        assert abs(loss.item() - float(g['loss'])) < (1e-5 if prec == 'fp32' else 5e-5)
        # per-parameter relative L2 on 64 sampled entries: fp32 measured <= 1.6e-2, bf16x3 <= 4.2e-2 (small decoder gradients;
        # whole-vector cosine 1.0000 in both)
        assert gerr < (2e-2 if prec == 'fp32' else 6e-2) and gcos > 0.9999, (gkey, gerr, gcos)
    else:
        assert d.max() <= 0.25 and d.mean() <= 0.03
        assert agree >= 0.96
        assert abs(loss.item() - float(g['loss'])) < 5e-3
        assert gerr < 0.8 and gcos >= 0.99, (gkey, gerr, gcos)      # measured: per-parameter 0.35-0.62, whole-vector cosine >= 0.995
    # BatchNorm running buffers after ONE forward: updated twice (date 1 then date 2)
    sd = model.state_dict()
    btol = 2e-2 if prec == 'bf16' else 1e-4
    for k in sd:
        if 'running_' in k:
            ref_b = torch.from_numpy(g['buf/' + k])
            assert (sd[k].cpu() - ref_b).abs().max() <= btol * max(1.0, ref_b.abs().max().item()), k
        if 'num_batches_tracked' in k:      # shared encoder BN modules run once per date, decoder ones once
            assert int(sd[k]) == (1 if k.startswith('up') else 2), k
    # one SGD step with torch's own optimizer, then forward again (train mode)
    opt.step()
    logits2 = model(x1, x2).detach().cpu()
    d2 = (logits2 - torch.from_numpy(g['logits_after_step'])).abs()
    assert d2.max() <= (0.25 if prec == 'bf16' else 1e-3)


def _whole_grad(model):
    return torch.cat([p.grad.flatten() for p in model.parameters()]).double()


@pytest.mark.parametrize('name', CASES)
def test_bf16x3_backward_two_and_three_terms(golden_dir, name):
    """precision='bf16x3' (the parity setting) keeps all three split-product terms in the backward GEMMs; precision='bf16x3-fast' is the
    explicit opt-in to two (BDN_BF16X2: the filter rounded to bf16 in the data gradient, dz in the weight gradient).  The forward -- the
    logits of north_star's 1e-3 bar -- is the same in both.  Both meet the golden gradient bounds of test_train_step_matches_reference
    (autograd of models/unet_parts.py:13,16).  Against the SAME engine in the exact-f32 setting the whole gradient of either form sits
    5-11e-3 relative L2 away -- that distance is dominated by the forward (ReLU masks and batch statistics that flip on 1e-4 differences of
    the activations), not by the backward's split terms, so it cannot be held to 1e-4; what IS held: both within 1.5e-2 of the fp32
    setting, the two forms within 1e-2 of each other (measured 1.9-5.2e-3, 1 - cosine <= 1.3e-5), and the three-term gradient the CLOSER
    one to the fp32 setting on every golden case (measured 5.4-9.5e-3 against 5.9-10.7e-3) -- a default that silently dropped a term
    fails the x3_bwd_terms assertions below, a regression of the three-term kernels the ordering.  The kernels themselves are pinned
    against exact gradients in tests/test_gpu_kernels.py (test_conv3x3_bf16x3_forward_dgrad_wgrad, test_conv3x3_bf16x2_backward_gemms)."""
    g, c, x1, x2, lbl = _load(golden_dir, name)
    grads = {}
    for prec, terms in (('fp32', None), ('bf16x3', 3), ('bf16x3-fast', 2)):
        model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda().train()
        if terms is not None:
            assert model.engine().x3_bwd_terms == terms            # the defaults of the two settings
        logits = model(x1, x2)
        _tversky_torch(logits, lbl).backward()
        assert (logits.detach().cpu() - torch.from_numpy(g['logits'])).abs().max() <= 1e-3
        gerr, gkey, gcos = _grad_errors(model, g)
        assert gerr < (2e-2 if prec == 'fp32' else 6e-2) and gcos > 0.9999, (prec, gkey, gerr, gcos)
        grads[prec] = _whole_grad(model)
    rel3 = ((grads['bf16x3'] - grads['fp32']).norm() / grads['fp32'].norm()).item()
    rel2 = ((grads['bf16x3-fast'] - grads['fp32']).norm() / grads['fp32'].norm()).item()
    rel23 = ((grads['bf16x3-fast'] - grads['bf16x3']).norm() / grads['bf16x3'].norm()).item()
    cos = torch.nn.functional.cosine_similarity(grads['bf16x3-fast'], grads['bf16x3'], dim=0).item()
    print(f'\n[{name}] whole-gradient relative L2 vs the fp32 setting: three-term {rel3:.2e}, two-term {rel2:.2e}; two vs three {rel23:.2e}, 1 - cosine {1 - cos:.1e}')
    assert rel3 <= 1.5e-2 and rel2 <= 1.5e-2, (rel3, rel2)
    assert rel23 <= 1e-2 and 1 - cos <= 1e-4
    assert rel3 < rel2, (rel3, rel2)                   # three terms is the form closer to the exact-f32 setting


@pytest.mark.parametrize('name', ['g2_c13_b2_s128', 'g8_c13_b3_h40_w72'])
def test_bf16x3_split_inside_the_conv_staging_is_bit_identical(golden_dir, name):
    """bf16x3: the second convolution of every double_conv reads the float32 z of the first and applies BatchNorm+ReLU and the hi / lo split in
    its staging (bdn_conv3x3_x3src, engine.x3_src_f32), leaving the split operand for the weight-gradient GEMM as a by-product; the step with
    a bdn_split_pack pass in front of those convolutions (rounds 3-5) gives the same logits and the same gradients bit for bit, in train
    and in eval mode."""
    g, c, x1, x2, lbl = _load(golden_dir, name)
    res = {}
    for fused in (True, False):
        model = filler.fill_module(BiDateNet(c, 2, precision='bf16x3')).cuda().train()
        model.engine().x3_src_f32 = fused
        logits = model(x1, x2)
        _tversky_torch(logits, lbl).backward()
        model.eval()
        with torch.no_grad():
            ev = model(x1, x2).clone()
        res[fused] = (logits.detach().clone(), _whole_grad(model), ev)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('prec', ['bf16x3', 'bf16x3-fast'])
def test_bf16x3_first_layer_weight_gradient_fused(golden_dir, prec):
    """bf16x3 settings, round 6: the first convolution's weight gradient with its BatchNorm backward (and the hi / lo split of dz) applied on
    load (bdn_conv3x3_wgrad_bnbwd, engine.first_wgrad_fused) against bn_bwd_apply_split + the generic GEMM: every other gradient bit for bit,
    inc.conv.conv.0.weight's within 1e-4 of its magnitude (same products, another summation order)."""
    g, c, x1, x2, lbl = _load(golden_dir, 'g2_c13_b2_s128')
    grads, ran = {}, {}
    for fused in (True, False):
        model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda().train()
        eng = model.engine()
        eng.first_wgrad_fused, eng.prof = fused, []
        _tversky_torch(model(x1, x2), lbl).backward()
        ran[fused] = 'wgrad_first_kernel' in [name for name, *_ in eng.prof]
        eng.prof = None
        grads[fused] = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    assert ran == {True: True, False: False}                       # the fused launch ran, and only where asked for
    for k in grads[True]:
        a, b = grads[True][k], grads[False][k]
        if k == 'inc.conv.conv.0.weight':
            assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item(), k
        else:
            assert torch.equal(a, b), k


def test_bf16x3_fast_loss_trajectory_follows_fp32(golden_dir):
    """Twelve SGD steps (train.py:83-96) from the same initial state on the 13-band golden inputs in the fp32, bf16x3 and bf16x3-fast
    settings at lr 1e-2: the loss of every step stays within 1e-5 of the fp32 setting's in both split settings (measured 1.2e-7), and the
    logits after the twelfth step within 1e-2 (measured 2.5e-3: twelve steps amplify the 1e-4 forward differences through ReLU masks)."""
    from fabric_amd.train_step import TrainStep
    g, c, x1, x2, lbl = _load(golden_dir, 'g2_c13_b2_s128')
    traj, last = {}, {}
    for prec in ('fp32', 'bf16x3', 'bf16x3-fast'):
        model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda().train()
        ts = TrainStep(model, lr=1e-2, tversky_alpha=0.1, tversky_beta=0.9)
        traj[prec] = [float(ts.step(x1, x2, lbl).item()) for _ in range(12)]
        last[prec] = ts.last_logits.detach().float().cpu()
    for prec, ltol in (('bf16x3', 1e-2), ('bf16x3-fast', 1e-2)):
        dl = max(abs(a - b) for a, b in zip(traj[prec], traj['fp32']))
        dlog = (last[prec] - last['fp32']).abs().max().item()
        print(f'\n[{prec}] max |dloss| over 12 steps {dl:.2e}, max |dlogit| after step 12 {dlog:.2e}')
        assert dl <= 1e-5 and dlog <= ltol, (prec, dl, dlog)
    assert traj['fp32'][-1] < traj['fp32'][0]                      # the steps do train


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_two_forwards_before_backward_keep_their_own_activations(golden_dir, prec):
    """Plain autograd usage the reference supports: two micro-batches (and an eval forward in between) before one backward.
    Each live graph owns its workspace, so the summed loss gives the sum of the separately computed gradients."""
    g, c, x1, x2, lbl = _load(golden_dir, 'g1_c3_b4_s32')
    y1, y2, lb2 = x2.flip(0).contiguous(), x1.flip(0).contiguous(), lbl.flip(0).contiguous()
    sep = []
    for a, b, l in ((x1, x2, lbl), (y1, y2, lb2)):
        model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda().train()
        _tversky_torch(model(a, b), l).backward()
        sep.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda().train()
    la = _tversky_torch(model(x1, x2), lbl)
    model.eval()
    with torch.no_grad():
        model(y1, y2)                                   # a validation forward of the same shape between forward and backward
    model.train()
    lb = _tversky_torch(model(y1, y2), lb2)
    assert len(model.engine()._ws[(x1.shape[0], x1.shape[2], x1.shape[3], str(x1.device), 0)]) == 2
    (la + lb).backward()
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        want = sep[0][k] + sep[1][k]
        if k.endswith('running_mean') or 'num_batches' in k:
            continue
        assert (p.grad - want).abs().max() <= 1e-5 * want.abs().max() + 1e-9, k
    # backward is over: the leases are released although `la` / `lb` (and their graphs) are still bound -- the usual training
    # loop keeps the previous iteration's loss alive while the next forward runs and must not ping-pong between two workspaces
    ws_pool = model.engine()._ws[(x1.shape[0], x1.shape[2], x1.shape[3], str(x1.device), 0)]
    assert not any(w.leased for w in ws_pool)
    lc = _tversky_torch(model(x1, x2), lbl)
    assert len(ws_pool) == 2 and ws_pool[0].leased
    lc.backward(retain_graph=True)
    model(y1, y2)                                       # reuses the released workspace ...
    with pytest.raises(RuntimeError, match='overwritten'):
        lc.backward()                                   # ... so a second backward through the old graph must refuse
    del la, lb, lc


@pytest.mark.parametrize('name', ['g1_c3_b4_s32', 'g4_c13_b2_s90'])
@pytest.mark.parametrize('prec', ['fp32', 'bf16x3', 'bf16'])
def test_eval_mode_matches_reference(golden_dir, name, prec):
    g, c, x1, x2, _ = _load(golden_dir, name)
    model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda().eval()
    with torch.no_grad():
        got = model(x1, x2).cpu()
    ref = torch.from_numpy(g['eval_logits'])
    scale = ref.abs().max().item()             # the filler's running statistics give O(100) eval logits
    d = (got - ref).abs().max().item()
    print(f'\n[{name} {prec} eval] max|dlogit|={d:.3e} of scale {scale:.1f}')
    assert d <= {'fp32': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}[prec] * scale
    sd = model.state_dict()
    assert all(int(sd[k]) == 0 for k in sd if 'num_batches_tracked' in k)    # eval must not touch the buffers


def test_cpu_tensors_are_refused():
    model = BiDateNet(3, 2)
    with pytest.raises(RuntimeError, match='no CPU path'):
        model(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))


def test_f1_definition_on_device_counts(golden_dir):
    """train.py:103-106 per-batch binary P/R/F1 from the on-device TP/FP/FN counts (G1's prf fixture)."""
    from fabric_amd.utils.metrics import batch_prf_from_counts, TverskyLoss
    g, c, x1, x2, lbl = _load(golden_dir, 'g1_c3_b4_s32')
    model = filler.fill_module(BiDateNet(c, 2, precision='fp32')).cuda().train()
    logits = model(x1, x2)
    crit = TverskyLoss(alpha=0.1, beta=0.9)
    loss = crit(logits, lbl.long())
    assert abs(loss.item() - float(g['loss'])) < 1e-5
    p, r, f = batch_prf_from_counts(crit.last_counts)
    assert np.allclose([p, r, f], g['prf'], atol=2e-3)


def test_model_loaded_from_a_reference_style_pickle_reproduces_g1(golden_dir, monkeypatch):
    """SURVEY.md 8b, reference train.py:222: a whole-module pickle of DataParallel(BiDateNet) WITHOUT the attributes this build adds
    (what a reference-written file holds after its class paths resolve through the root shims) is loaded by load_checkpoint AND used
    directly after torch.load(...).module; both reproduce golden G1 (train-mode logits within 1e-3, loss within 1e-5)."""
    import io
    import models.bidate_model as shim
    from fabric_amd.models.bidate_model import BiDateNet as B
    from fabric_amd.utils.helpers import load_checkpoint
    g, c, x1, x2, lbl = _load(golden_dir, 'g1_c3_b4_s32')
    added = ('_engine', 'precision', 'n_channels', 'n_classes')
    monkeypatch.setattr(B, '__getstate__', lambda self: {k: v for k, v in self.__dict__.items() if k not in added})
    buf = io.BytesIO()
    torch.save(torch.nn.DataParallel(filler.fill_module(shim.BiDateNet(c, 2))), buf)
    monkeypatch.undo()
    ref = torch.from_numpy(g['logits'])
    monkeypatch.setenv('BIDATE_PRECISION', 'fp32')            # a reference pickle carries no numerics setting: the environment decides
    raw = torch.load(io.BytesIO(buf.getvalue()), weights_only=False).module.cuda().train()
    loaded = load_checkpoint(io.BytesIO(buf.getvalue()), device='cuda', precision='fp32').train()
    for m in (raw, loaded):
        assert m.precision == 'fp32' and m.n_channels == c
        logits = m(x1, x2)
        loss = _tversky_torch(logits, lbl)
        loss.backward()
        assert (logits.detach().cpu() - ref).abs().max() <= 1e-3
        assert abs(loss.item() - float(g['loss'])) < 1e-5
        assert int(m.state_dict()['inc.conv.conv.1.num_batches_tracked']) == 2
