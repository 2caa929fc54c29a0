"""-m gpu: bdn_criterion_masked (include/bidate_hip.h; Criterion(ignore_index=)) through the C ABI on guard-banded buffers.

The yardstick is the float64 restatement tests/ignore_ref.py (pinned to the oracle's functions by tests/test_ignore_cpu.py) with the
project's per-term bars and their combination, as tests/test_gpu_criterion.py states them:

    |loss - L64|          <= 5e-6 (w_o max(1, |O64|) + w_f max(1, |F64|))          terms: 5e-6 max(1, |v|) each
    max|dlogits - dL64|   <= 3e-4 (w_o max|dO64| + w_f max|dF64|)

Counts are exact; dlogits is exactly 0 at every ignored pixel; the logits of ignored pixels change no bit of any output.
"""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import REDUCE, Criterion
from fabric_amd.utils import metrics as M
from gpu_util import dev, st
from tests import guard
from tests import ignore_ref as IR
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 90, 77),       # W not a power of two, a row tail, 135 row blocks
          (1, 8, 16, 300),      # two column blocks, the 8-class instantiation
          (2, 3, 1, 5), (4, 2, 32, 32)]
MASKS = ['random', 'column', 'image', 'none', 'all']
LOSS_TOL, GRAD_TOL = 5e-6, 3e-4
NAN = float('nan')
POISON = [1e30, float('inf'), -float('inf'), NAN, -1e30, 0.0]


@functools.lru_cache(maxsize=None)
def _inputs(shape, mask, ignore=255, seed=11):
    """float32 logits, int64 labels [B,H,W] with the ignored pixels painted `ignore`, the bool mask of ignored pixels.  Shared between
    the tests: never modified."""
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy((3 * r.standard_normal(shape)).astype(np.float32))
    labels = torch.from_numpy(r.integers(0, C, (B, H, W)).astype(np.int64))
    m = torch.zeros(B, H, W, dtype=torch.bool)
    if mask == 'random':
        m = torch.from_numpy(r.random((B, H, W)) < 0.3)
    elif mask == 'column':
        m[:, :, W // 2] = True
    elif mask == 'image':                                   # whole blocks of the statistics pass then hold only zeros
        m[0] = True
    elif mask == 'all':
        m[:] = True
    if ignore < C:
        assert mask == 'class'                              # ignoring a real class: its pixels are the mask
        return logits, labels, labels == ignore
    return logits, torch.where(m, torch.full_like(labels, ignore), labels), m


def _class_alpha(C):
    return [0.25, 0.75] if C == 2 else [round(0.1 + 0.8 * k / (C - 1), 3) for k in range(C)]


def _criteria(C, reduce, ignore=255):
    kw = dict(reduce=reduce, ignore_index=ignore)
    ca = 0.25 if C == 2 else _class_alpha(C)
    out = [(n, Criterion.parse(n, tversky_alpha=0.1, tversky_beta=0.9, **kw)) for n in ('tversky', 'dice', 'jaccard')]
    for g in (0.0, 2.0):
        for a in (None, _class_alpha(C)):
            for sa in (True, False):
                out.append((f'focal({g},{"alpha" if a else "-"},{"mean" if sa else "sum"})',
                            Criterion(w_overlap=0.0, w_focal=1.0, gamma=g, class_alpha=a, size_average=sa, **kw)))
    for w in ((1, 1), (0.25, 2)):
        out.append((f'focal(2)+dice w={w}', Criterion.parse('focal+dice', focal_gamma=2.0, weights=w, **kw)))
        out.append((f'focal(2,alpha)+tversky(0.1,0.9) w={w}', Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9,
                                                                             focal_gamma=2.0, focal_alpha=ca, weights=w, **kw)))
    return out


def _run(c, lg_d, lb_d, alpha_d=None, want_dl=True, want_counts=True, want_terms=True):
    """bdn_criterion_masked straight through the C ABI on fresh guarded outputs and a workspace of exactly the size the query returns."""
    B, C, H, W = lg_d.shape
    ws = guard.alloc_bytes(_lib.load().bdn_criterion_masked_workspace_bytes(B, C, H, W, REDUCE[c.reduce]), label='masked criterion workspace')
    loss = guard.full((1,), NAN)
    terms = guard.full((2,), NAN) if want_terms else None
    counts = guard.full((5,), -1, dtype=torch.int32) if want_counts else None
    dl = guard.full(tuple(lg_d.shape), NAN) if want_dl else None
    if c.class_alpha is not None and alpha_d is None:
        alpha_d = dev(torch.tensor(c.class_alpha[:C]))
    _lib.call('bdn_criterion_masked', lg_d.data_ptr(), lb_d.data_ptr(), c.ignore_index, c.w_overlap, c.alpha, c.beta, c.eps,
              REDUCE[c.reduce], c.w_focal, c.gamma, _lib.ptr(alpha_d), int(c.size_average), ws.data_ptr(), loss.data_ptr(), _lib.ptr(terms),
              _lib.ptr(counts), _lib.ptr(dl), B, C, H, W, st())
    return loss, terms, counts, dl


def _unmasked(c, lg_d, lb_d):
    """bdn_criterion on the same inputs (no pixel ignored): loss and dlogits."""
    B, C, H, W = lg_d.shape
    ws = guard.alloc_bytes(_lib.load().bdn_criterion_workspace_bytes(B, C, H, W, REDUCE[c.reduce]), label='criterion workspace')
    loss, dl = guard.full((1,), NAN), guard.full(tuple(lg_d.shape), NAN)
    alpha_d = dev(torch.tensor(c.class_alpha[:C])) if c.class_alpha is not None else None
    _lib.call('bdn_criterion', lg_d.data_ptr(), lb_d.data_ptr(), c.w_overlap, c.alpha, c.beta, c.eps, REDUCE[c.reduce], c.w_focal, c.gamma,
              _lib.ptr(alpha_d), int(c.size_average), ws.data_ptr(), loss.data_ptr(), None, None, dl.data_ptr(), B, C, H, W, st())
    return loss, dl


def _check(c, logits, labels, ignored, out, what):
    loss, terms, counts, dl = out
    ref = IR.reference(c, logits, labels)
    lb = LOSS_TOL * (c.w_overlap * max(1.0, abs(ref['overlap'])) + c.w_focal * max(1.0, abs(ref['focal'])))
    gb = GRAD_TOL * (c.w_overlap * ref['doverlap'].abs().max().item() + c.w_focal * ref['dfocal'].abs().max().item())
    dl_c = dl.cpu()
    e_loss = abs(loss.item() - ref['loss'])
    e_grad = (dl_c.double() - ref['dloss']).abs().max().item()
    t = terms.cpu().tolist()
    print(f'{what}: |loss err| {e_loss:.3e} (bound {lb:.3e})  max|dlogits err| {e_grad:.3e} (bound {gb:.3e})  '
          f'terms err {abs(t[0] - ref["overlap"]):.3e} {abs(t[1] - ref["focal"]):.3e}')
    assert torch.isfinite(dl_c).all(), what
    assert (dl_c[ignored[:, None].expand_as(dl_c)] == 0).all(), what
    assert e_loss <= lb and e_grad <= gb, (what, e_loss, lb, e_grad, gb)
    assert abs(t[0] - ref['overlap']) <= LOSS_TOL * max(1.0, abs(ref['overlap'])), (what, t, ref['overlap'])
    assert abs(t[1] - ref['focal']) <= LOSS_TOL * max(1.0, abs(ref['focal'])), (what, t, ref['focal'])
    assert counts.cpu().tolist() == IR.counts(logits, labels, c.ignore_index), what


# ---------------------------------------------------------------- against the float64 restatement
@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_masked_criterion_matches_the_float64_restatement(shape, mask):
    logits, labels, ignored = _inputs(shape, mask)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for reduce in ('columns', 'image'):
        for name, c in _criteria(shape[1], reduce):
            out = _run(c, lg_d, lb_d)
            plain = _unmasked(c, lg_d, lb_d) if mask == 'none' else None
            torch.cuda.synchronize()
            _check(c, logits, labels, ignored, out, f'{name} {shape} {reduce} mask={mask}')
            if plain is not None:                           # informational: another instantiation may contract differently
                print(f'    bit-equal to bdn_criterion: loss {torch.equal(out[0], plain[0])} dlogits {torch.equal(out[3], plain[1])}')
    if mask == 'all':
        for _, c in _criteria(shape[1], 'columns')[-2:]:
            loss, terms, counts, dl = _run(c, lg_d, lb_d)
            assert terms.cpu().tolist() == [1.0, 0.0] and loss.item() == c.w_overlap and not dl.any() and counts.cpu().tolist() == [0] * 5


@pytest.mark.parametrize('shape', [(3, 2, 90, 77), (1, 8, 16, 300)], ids=str)
@guarded
def test_ignoring_a_real_class(shape):
    """ignore_label = 0: the pixels of class 0 are left out, the others keep their class index."""
    logits, labels, ignored = _inputs(shape, 'class', ignore=0)
    assert ignored.any() and not ignored.all()
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for reduce in ('columns', 'image'):
        for name, c in _criteria(shape[1], reduce, ignore=0):
            out = _run(c, lg_d, lb_d)
            torch.cuda.synchronize()
            _check(c, logits, labels, ignored, out, f'{name} {shape} {reduce} ignore_label=0')


# ---------------------------------------------------------------- the logits of ignored pixels reach no output
@pytest.mark.parametrize('mask', ['random', 'column', 'image', 'all'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_ignored_logits_change_no_bit(shape, mask):
    logits, labels, ignored = _inputs(shape, mask)
    sel = ignored[:, None].expand_as(logits)
    bad = logits.clone()
    bad[sel] = torch.tensor(POISON).repeat(logits.numel() // len(POISON) + 1)[:int(sel.sum())]
    other = logits.clone()
    other[sel] = -7.5 * logits[sel] + 3.0
    lb_d = guard.guard(labels.to(torch.uint8))
    first, lg_bad, lg_other = dev(logits), dev(bad), dev(other)
    for reduce in ('columns', 'image'):
        crit = dict(_criteria(shape[1], reduce))
        for name in ('dice', 'focal(2.0,alpha,mean)', 'focal(2,alpha)+tversky(0.1,0.9) w=(0.25, 2)'):
            c = crit[name]
            a = _run(c, first, lb_d)
            for lg_d in (lg_bad, lg_other):
                b = _run(c, lg_d, lb_d)
                torch.cuda.synchronize()
                for x, y, what in zip(a, b, ('loss', 'terms', 'counts', 'dlogits')):
                    assert torch.isfinite(y.float()).all() and torch.equal(x, y), (what, name, reduce)


# ---------------------------------------------------------------- determinism and optional outputs
@pytest.mark.parametrize('shape', [(3, 2, 90, 77), (1, 8, 16, 300)], ids=str)
@guarded
def test_masked_is_deterministic_and_outputs_are_optional(shape):
    logits, labels, _ = _inputs(shape, 'random')
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for reduce in ('columns', 'image'):
        crit = dict(_criteria(shape[1], reduce))
        for name in ('dice', 'focal(2.0,alpha,mean)', 'focal(2,alpha)+tversky(0.1,0.9) w=(0.25, 2)'):
            c = crit[name]
            a, b = _run(c, lg_d, lb_d), _run(c, lg_d, lb_d)
            torch.cuda.synchronize()
            for x, y, what in zip(a, b, ('loss', 'terms', 'counts', 'dlogits')):
                assert torch.equal(x, y), (what, name, reduce)
            loss, terms, counts, dl = _run(c, lg_d, lb_d, want_dl=False)                      # validation: no gradient pass
            assert dl is None and torch.equal(loss, a[0]) and torch.equal(counts, a[2]) and torch.equal(terms, a[1])
            loss, terms, counts, dl = _run(c, lg_d, lb_d, want_counts=False, want_terms=False)
            assert counts is None and terms is None and torch.equal(loss, a[0]) and torch.equal(dl, a[3])
            loss, terms, counts, dl = _run(c, lg_d, lb_d, want_dl=False, want_counts=False, want_terms=False)
            assert (terms, counts, dl) == (None, None, None) and torch.equal(loss, a[0])


# ---------------------------------------------------------------- the Python surface
def test_criterion_evaluate_compound_loss_and_confusion_counts_agree_with_the_c_abi():
    shape = (3, 2, 90, 77)
    logits, labels, ignored = _inputs(shape, 'random')
    c = Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=0.25, weights=(0.25, 2),
                        ignore_index=255)
    lg, lb = logits.cuda(), labels.cuda()
    want = [t.clone() for t in _run(c, lg, lb.to(torch.uint8))]
    loss, terms, counts, dl = c.evaluate(lg, lb)
    for x, y in zip((loss.view(1), terms, counts, dl), want):
        assert torch.equal(x, y)
    assert counts.shape == (5,) and counts.cpu().tolist() == IR.counts(logits, labels, 255)
    out = c.buffers(shape, lg.device)
    assert out[3].shape == (5,)
    loss2, _, counts2, dl2 = c.evaluate(lg, lb[:, None].to(torch.uint8), out=out)                     # the label rank does not decide
    assert loss2 is out[1] and torch.equal(loss, loss2) and torch.equal(dl, dl2) and torch.equal(counts, counts2)
    assert c.evaluate(lg, lb, want_grad=False)[3] is None
    mod = M.CompoundLoss(c)
    x = lg.clone().requires_grad_(True)
    v = mod(x, lb)
    (3.0 * v).backward()
    assert torch.equal(v.detach(), loss) and torch.equal(x.grad, dl * 3.0) and not x.grad[ignored[:, None].expand_as(x).cuda()].any()
    assert torch.equal(mod.last_counts, counts) and torch.equal(mod.last_terms, terms)
    assert torch.equal(M.confusion_counts(lg, lb, ignore_index=255), counts)
    # without an ignore_index: today's objects, four counts, and a pixel labelled 255 is a wrong prediction there
    plain = Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=0.25, weights=(0.25, 2))
    assert plain.buffers(shape, lg.device)[3].shape == (4,) and plain.evaluate(lg, lb)[2].shape == (4,)
    c4 = M.confusion_counts(lg, lb)
    mod4 = M.CompoundLoss(plain)
    mod4(lg, lb)
    assert c4.shape == (4,) and mod4.last_counts.shape == (4,) and torch.equal(mod4.last_counts, c4)
    assert c4.cpu().tolist()[3] == counts.cpu().tolist()[3]                                            # an ignored pixel was never correct
