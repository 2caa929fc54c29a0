"""-m gpu: bdn_criterion (include/bidate_hip.h; fabric_amd/criterion.py) on guard-banded buffers.

Single terms must reproduce bdn_overlap_loss / bdn_focal bit for bit; the compound losses are held to the float64 restatement
(tests/criterion_ref.py: the weighted sum of the oracle's terms) with the project's per-term bars (tests/test_gpu_losses.py: loss values
5e-6 x max(1, |v|), gradients 3e-4 of the gradient's max magnitude) combined by the triangle inequality:

    |loss - L64|          <= 5e-6 (w_o max(1, |O64|) + w_f max(1, |F64|))
    max|dlogits - dL64|   <= 3e-4 (w_o max|dO64| + w_f max|dF64|)
"""
import os

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import REDUCE, Criterion
from fabric_amd.utils import metrics as M
from gpu_util import dev, st
from tests import criterion_ref as CR
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(64, 2, 128, 128), (3, 2, 90, 77), (1, 8, 16, 300), (2, 3, 1, 5)]          # test_losses_match_oracle_on_other_shapes
LOSS_TOL, GRAD_TOL = 5e-6, 3e-4
NAN = float('nan')


def _inputs(shape, seed=11):
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy((3 * r.standard_normal(shape)).astype(np.float32))
    labels = torch.from_numpy(r.integers(0, C, (B, H, W)).astype(np.int64))
    return logits, labels


def _class_alpha(C):
    return [0.25, 0.75] if C == 2 else [round(0.1 + 0.8 * k / (C - 1), 3) for k in range(C)]


def _run(c, lg_d, lb_d, alpha_d=None, want_dl=True, want_counts=True, want_terms=True):
    """bdn_criterion straight through the C ABI on fresh guarded outputs and a workspace of exactly the size the query returns."""
    B, C, H, W = lg_d.shape
    ws = guard.alloc_bytes(_lib.load().bdn_criterion_workspace_bytes(B, C, H, W, REDUCE[c.reduce]), label='criterion workspace')
    loss = guard.full((1,), NAN)
    terms = guard.full((2,), NAN) if want_terms else None
    counts = guard.full((4,), -1, dtype=torch.int32) if want_counts else None
    dl = guard.full(tuple(lg_d.shape), NAN) if want_dl else None
    if c.class_alpha is not None and alpha_d is None:
        alpha_d = dev(torch.tensor(c.class_alpha[:C]))
    _lib.call('bdn_criterion', lg_d.data_ptr(), lb_d.data_ptr(), c.w_overlap, c.alpha, c.beta, c.eps, REDUCE[c.reduce], c.w_focal, c.gamma,
              _lib.ptr(alpha_d), int(c.size_average), ws.data_ptr(), loss.data_ptr(), _lib.ptr(terms), _lib.ptr(counts), _lib.ptr(dl),
              B, C, H, W, st())
    return loss, terms, counts, dl


def _bounds(c, ref):
    return (LOSS_TOL * (c.w_overlap * max(1.0, abs(ref['overlap'])) + c.w_focal * max(1.0, abs(ref['focal']))),
            GRAD_TOL * (c.w_overlap * ref['doverlap'].abs().max().item() + c.w_focal * ref['dfocal'].abs().max().item()))


# ---------------------------------------------------------------- single terms: the existing entry points, bit for bit
@pytest.mark.parametrize('reduce', ['columns', 'image'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_single_overlap_term_has_the_bits_of_bdn_overlap_loss(shape, reduce):
    B, C, H, W = shape
    logits, labels = _inputs(shape)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for name in ('tversky', 'dice', 'jaccard'):
        c = Criterion.parse(name, tversky_alpha=0.1, tversky_beta=0.9, reduce=reduce)
        loss, terms, counts, dl = _run(c, lg_d, lb_d)
        ws = guard.alloc_bytes(_lib.load().bdn_overlap_workspace_bytes(B, C, H, W, REDUCE[reduce]), label='overlap workspace')
        loss0, counts0, dl0 = guard.full((1,), NAN), guard.full((4,), -1, dtype=torch.int32), guard.full(shape, NAN)
        _lib.call('bdn_overlap_loss', lg_d.data_ptr(), lb_d.data_ptr(), c.alpha, c.beta, c.eps, REDUCE[reduce], ws.data_ptr(),
                  loss0.data_ptr(), counts0.data_ptr(), dl0.data_ptr(), B, C, H, W, st())
        torch.cuda.synchronize()
        assert torch.equal(loss, loss0) and torch.equal(counts, counts0) and torch.equal(dl, dl0), (name, loss.item(), loss0.item())
        assert torch.equal(terms.cpu(), torch.tensor([loss0.item(), 0.0])), name
        assert counts.cpu().tolist() == CR.counts(logits, labels)


FOCAL_FORMS = [(g, a, sa) for g in (0.0, 2.0, 1.5) for a in (False, True) for sa in (1, 0)]


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_single_focal_term_has_the_bits_of_bdn_focal(shape):
    B, C, H, W = shape
    logits, labels = _inputs(shape)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    a_d = dev(torch.tensor(_class_alpha(C)))
    for gamma, with_alpha, sa in FOCAL_FORMS:
        c = Criterion(w_overlap=0.0, w_focal=1.0, gamma=gamma, class_alpha=_class_alpha(C) if with_alpha else None, size_average=bool(sa))
        loss, terms, counts, dl = _run(c, lg_d, lb_d, a_d if with_alpha else None)
        ws = guard.alloc_bytes(_lib.load().bdn_focal_workspace_bytes(), label='focal workspace')
        loss0, counts0, dl0 = guard.full((1,), NAN), guard.full((4,), -1, dtype=torch.int32), guard.full(shape, NAN)
        _lib.call('bdn_focal', lg_d.data_ptr(), lb_d.data_ptr(), gamma, a_d.data_ptr() if with_alpha else None, sa, ws.data_ptr(),
                  loss0.data_ptr(), counts0.data_ptr(), dl0.data_ptr(), B, C, H, W, st())
        torch.cuda.synchronize()
        form = (gamma, with_alpha, sa)
        assert torch.equal(dl, dl0) and torch.equal(counts, counts0), form
        ref = CR.reference(c, logits, labels)
        print(f'focal {shape} {form}: loss {loss.item():.9g} oracle {ref["loss"]:.9g}')
        assert abs(loss.item() - ref['loss']) <= LOSS_TOL * max(1.0, abs(ref['loss'])), (form, loss.item(), ref['loss'])
        assert torch.equal(terms.cpu(), torch.tensor([0.0, loss.item()])), form
        assert counts.cpu().tolist() == CR.counts(logits, labels)


# ---------------------------------------------------------------- compound against the float64 restatement
def _compound_cases(C, reduce):
    ca = 0.25 if C == 2 else _class_alpha(C)
    return [('focal(2)+dice', lambda w: Criterion.parse('focal+dice', focal_gamma=2.0, weights=w, reduce=reduce)),
            ('focal(2,alpha)+tversky(0.1,0.9)', lambda w: Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0,
                                                                          focal_alpha=ca, weights=w, reduce=reduce)),
            ('focal(0)+jaccard', lambda w: Criterion.parse('focal+jaccard', focal_gamma=0.0, weights=w, reduce=reduce))]


def _check_against(c, ref, logits, labels, loss, terms, counts, dl, what):
    lb, gb = _bounds(c, ref)
    e_loss = abs(loss.item() - ref['loss'])
    e_grad = (dl.cpu().double() - ref['dloss']).abs().max().item()
    t = terms.cpu().tolist()
    print(f'{what}: |loss err| {e_loss:.3e} (bound {lb:.3e})  max|dlogits err| {e_grad:.3e} (bound {gb:.3e})  '
          f'terms err {abs(t[0] - ref["overlap"]):.3e} {abs(t[1] - ref["focal"]):.3e}')
    assert torch.isfinite(dl).all() and e_loss <= lb and e_grad <= gb, (what, e_loss, lb, e_grad, gb)
    assert abs(t[0] - ref['overlap']) <= LOSS_TOL * max(1.0, abs(ref['overlap'])), (what, t, ref['overlap'])
    assert abs(t[1] - ref['focal']) <= LOSS_TOL * max(1.0, abs(ref['focal'])), (what, t, ref['focal'])
    assert counts.cpu().tolist() == CR.counts(logits, labels), what


@pytest.mark.parametrize('reduce', ['columns', 'image'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_compound_matches_the_float64_restatement(shape, reduce):
    logits, labels = _inputs(shape)
    lg_d = dev(logits)
    lb_d = guard.guard((labels if reduce == 'columns' else labels[:, None]).to(torch.uint8))       # both label ranks: the same bytes
    for name, make in _compound_cases(shape[1], reduce):
        for w in ((1, 1), (0.25, 2), (3, 0.5)):
            c = make(w)
            out = _run(c, lg_d, lb_d)
            torch.cuda.synchronize()
            _check_against(c, CR.reference(c, logits, labels), logits, labels, *out, f'{name} w={w} {shape} {reduce}')


@guarded
def test_compound_matches_the_reference_fixtures(golden_dir):
    """G9 records the reference's focal and overlap values on the same inputs: the compound value is their weighted sum.  G5 records
    overlap values only: there the overlap term of a compound run (terms[0]) and the overlap-only weighted forms that take the compound
    kernels (weight != 1) are compared."""
    g = np.load(os.path.join(golden_dir, 'g9_losses_more.npz'))
    for tag in ('c2', 'c5'):
        logits, lbl = torch.from_numpy(g[f'{tag}/logits']), torch.from_numpy(g[f'{tag}/labels'].astype(np.int64))
        lg_d, lb_d = dev(logits), guard.guard(lbl.to(torch.uint8))
        focal_forms = [('g0', 0.0, None), ('g2', 2.0, None)] + ([('g2_a0.25', 2.0, 0.25)] if tag == 'c2' else
                                                               [('g2_alist', 2.0, [0.1, 0.2, 0.3, 0.15, 0.25])])
        for rank, reduce in (('r3', 'columns'), ('r4', 'image')):
            for oname, pname, ta, tb in (('dice', 'dice', 0.5, 0.5), ('jaccard', 'jaccard', 0.5, 0.5), ('tversky_0.3_0.7', 'tversky', 0.3, 0.7)):
                for fname, gamma, fa in focal_forms:
                    for wf, wo in ((1, 1), (0.25, 2), (3, 0.5)):
                        c = Criterion.parse('focal+' + pname, tversky_alpha=ta, tversky_beta=tb, focal_gamma=gamma, focal_alpha=fa,
                                            weights=(wf, wo), reduce=reduce)
                        loss, terms, _, _ = _run(c, lg_d, lb_d, want_dl=False)
                        O_ref, F_ref = float(g[f'{tag}/{oname}_{rank}']), float(g[f'{tag}/focal_{fname}'])
                        bound = LOSS_TOL * (wo * max(1.0, abs(O_ref)) + wf * max(1.0, abs(F_ref)))
                        assert abs(loss.item() - (wo * O_ref + wf * F_ref)) <= bound, (tag, oname, rank, fname, wf, wo, loss.item())
                        t = terms.cpu().tolist()
                        assert abs(t[0] - O_ref) <= LOSS_TOL * max(1.0, abs(O_ref)) and abs(t[1] - F_ref) <= LOSS_TOL * max(1.0, abs(F_ref))
    g = np.load(os.path.join(golden_dir, 'g5_losses.npz'))
    logits, lbl = torch.from_numpy(g['logits']), torch.from_numpy(g['labels'].astype(np.int64))
    lg_d, lb_d = dev(logits), guard.guard(lbl.to(torch.uint8))
    for rank, reduce in (('r3', 'columns'), ('r4', 'image')):
        for oname, pname, ta, tb in (('dice', 'dice', 0.5, 0.5), ('jaccard', 'jaccard', 0.5, 0.5), ('tversky_0.1_0.9', 'tversky', 0.1, 0.9),
                                     ('tversky_0.5_0.5', 'tversky', 0.5, 0.5)):
            O_ref = float(g[f'{oname}_{rank}'])
            base = Criterion.parse(pname, tversky_alpha=ta, tversky_beta=tb, reduce=reduce)
            for wo in (2.0, 0.5):                                  # overlap alone with a weight: the compound kernels, focal weight 0
                c = Criterion(wo, base.alpha, base.beta, base.eps, reduce)
                loss, terms, _, _ = _run(c, lg_d, lb_d, want_dl=False)
                assert abs(loss.item() - wo * O_ref) <= LOSS_TOL * wo * max(1.0, abs(O_ref)), (oname, rank, wo, loss.item())
            c = Criterion(1.0, base.alpha, base.beta, base.eps, reduce, w_focal=1.0, gamma=2.0)
            _, terms, _, _ = _run(c, lg_d, lb_d, want_dl=False)
            assert abs(terms.cpu()[0].item() - O_ref) <= LOSS_TOL * max(1.0, abs(O_ref)), (oname, rank)


# ---------------------------------------------------------------- determinism and optional outputs
@pytest.mark.parametrize('shape', [(64, 2, 128, 128), (1, 8, 16, 300)], ids=str)
@guarded
def test_compound_is_deterministic_and_outputs_are_optional(shape):
    logits, labels = _inputs(shape, seed=5)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for reduce in ('columns', 'image'):
        c = Criterion.parse('focal+dice', focal_gamma=2.0, focal_alpha=_class_alpha(shape[1]), weights=(0.25, 2), reduce=reduce)
        a, b = _run(c, lg_d, lb_d), _run(c, lg_d, lb_d)
        torch.cuda.synchronize()
        for x, y, what in zip(a, b, ('loss', 'terms', 'counts', 'dlogits')):
            assert torch.equal(x, y), (what, reduce)
        loss, terms, counts, dl = _run(c, lg_d, lb_d, want_dl=False)                      # validation: no gradient pass
        assert dl is None and torch.equal(loss, a[0]) and torch.equal(counts, a[2]) and torch.equal(terms, a[1])
        loss, terms, counts, dl = _run(c, lg_d, lb_d, want_counts=False, want_terms=False)
        assert counts is None and terms is None and torch.equal(loss, a[0]) and torch.equal(dl, a[3])
    for c in (Criterion.parse('dice'), Criterion.parse('focal', focal_gamma=2.0)):          # the dispatched single terms take NULLs too
        full = _run(c, lg_d, lb_d)
        loss, terms, counts, dl = _run(c, lg_d, lb_d, want_dl=False, want_counts=False, want_terms=False)
        assert (terms, counts, dl) == (None, None, None) and torch.equal(loss, full[0])


# ---------------------------------------------------------------- the Python surface
def test_criterion_evaluate_and_compound_loss_module():
    shape = (3, 2, 90, 77)
    logits, labels = _inputs(shape, seed=7)
    c = Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=0.25, weights=(0.25, 2))
    ref = CR.reference(c, logits, labels)
    lb, gb = _bounds(c, ref)
    lg = logits.cuda()
    loss, terms, counts, dl = c.evaluate(lg, labels.cuda())
    out = c.buffers(shape, lg.device)
    loss2, terms2, counts2, dl2 = c.evaluate(lg, labels[:, None].cuda().to(torch.uint8), out=out)     # the label rank does not decide
    assert loss2 is out[1] and torch.equal(loss, loss2) and torch.equal(dl, dl2) and torch.equal(counts, counts2)
    assert c.evaluate(lg, labels.cuda(), want_grad=False)[3] is None
    assert abs(loss.item() - ref['loss']) <= lb and (dl.cpu().double() - ref['dloss']).abs().max().item() <= gb
    mod = M.CompoundLoss(c)
    x = lg.clone().requires_grad_(True)
    v = mod(x, labels.cuda())
    (3.0 * v).backward()
    assert torch.equal(v.detach(), loss) and torch.equal(x.grad, dl * 3.0)
    assert torch.equal(mod.last_counts, counts) and torch.equal(mod.last_terms, terms)
    with torch.no_grad():
        assert torch.equal(mod(lg, labels.cuda()), loss)
    with pytest.raises(RuntimeError, match='labels must be'):
        c.evaluate(lg, labels[:, :5].cuda())
