"""-m gpu: bdn_lovasz_softmax (include/bidate_hip.h; Criterion(w_lovasz=)) through the C ABI on guard-banded buffers, with a workspace of
exactly the queried size (0xFF-filled: NaN-born).

Two yardsticks, as in tests/test_gpu_topk.py.  The ORDER is checked exactly, in integers: `ranks` must be the stable descending order of
the kernel's own exported `pixel_errors` under the key map (tests/lovasz_ref.order_from_errors), -1 at ignored pixels, on every input of
this file -- random float32 inputs already hold equal errors, so a gradient cannot be compared under the reference's own order.  The VALUES
are checked against the float64 restatement tests/lovasz_ref.py (pinned by tests/test_lovasz_cpu.py) with the project's bars
(tests/test_gpu_criterion.py, tests/test_gpu_topk.py):

    |pixel_errors - err64|  <= 5e-6
    |term - L64|            <= 5e-6 max(1, |L64|)      L64 fully independent, under the float64 order: the extension is 1-Lipschitz in the
                                                       max norm of the errors (the coefficients are >= 0 and sum to at most 1)
    max|dlogits - dL64|     <= 3e-4 max|dL64|          dL64 the float64 gradient under the KERNEL's order
"""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import REDUCE, Criterion
from gpu_util import dev, st
from tests import guard
from tests import lovasz_ref as LR
from tests import topk_ref as TR
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 90, 77),       # 20 790 pixels: six sort tiles with a tail, W not a power of two
          (1, 8, 16, 300),      # the 8-class loops, two tiles
          (4, 2, 32, 32),       # exactly one full tile
          (2, 3, 1, 5),         # ten pixels
          (2, 2, 128, 128)]     # eight full tiles
MASKS = ['none', 'random', 'image', 'all']
ERR_TOL, TERM_TOL, GRAD_TOL = 5e-6, 5e-6, 3e-4
NAN = float('nan')
POISON = [1e30, float('inf'), -float('inf'), NAN]
NAMES = ('loss', 'term', 'dlogits', 'pixel_errors', 'ranks')


def _mask(shape, mask, r):
    B, C, H, W = shape
    m = torch.zeros(B, H, W, dtype=torch.bool)
    if mask == 'random':
        m = torch.from_numpy(r.random((B, H, W)) < 0.3)
    elif mask == 'image':
        m[0] = True
    elif mask == 'all':
        m[:] = True
    return m


@functools.lru_cache(maxsize=None)
def _inputs(shape, mask, seed=0, scale=3.0, absent=None):
    """float32 logits, int64 labels [B,H,W] with the ignored pixels painted 255, the bool mask of ignored pixels.  Shared: never modified."""
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))
    labels = torch.from_numpy(r.integers(0, C, (B, H, W)).astype(np.int64))
    if absent is not None:
        labels = torch.where(labels == absent, torch.full_like(labels, (absent + 1) % C), labels)
    m = _mask(shape, mask, r)
    return logits, torch.where(m, torch.full_like(labels, 255), labels), m


def _ignore(mask):
    return None if mask == 'none' else 255


def _run(lg_d, lb_d, ignore, classes='present', weight=1.0, accumulate=0, loss=None, dl=None, want_dl=True, want_term=True, want_export=True,
         ws=None):
    """bdn_lovasz_softmax straight through the C ABI on guarded outputs (fresh unless given) and a workspace of exactly the queried size."""
    B, C, H, W = lg_d.shape
    if ws is None:
        ws = guard.alloc_bytes(_lib.load().bdn_lovasz_workspace_bytes(B, C, H, W), label='lovasz workspace')
    loss = guard.full((1,), NAN) if loss is None else loss
    term = guard.full((1,), NAN) if want_term else None
    if dl is None and want_dl:
        dl = guard.full(tuple(lg_d.shape), NAN)
    pe = guard.full((C, B * H * W), NAN) if want_export else None
    ranks = guard.full((C, B * H * W), -7, dtype=torch.int32) if want_export else None
    _lib.call('bdn_lovasz_softmax', lg_d.data_ptr(), lb_d.data_ptr(), -1 if ignore is None else ignore, int(classes == 'all'), weight,
              accumulate, ws.data_ptr(), loss.data_ptr(), _lib.ptr(term), _lib.ptr(dl), _lib.ptr(pe), _lib.ptr(ranks), B, C, H, W, st())
    return loss, term, dl, pe, ranks


def _check_order(out, ignored, what):
    """Check 1: per class, ranks == the stable descending order of the kernel's own errors under the key map; -1 at ignored pixels."""
    pe, ranks = out[3].cpu().numpy(), out[4].cpu().numpy()
    valid = ~ignored.reshape(-1).numpy()
    orders = []
    for c in range(pe.shape[0]):
        o = LR.order_from_errors(pe[c], valid)
        want = LR.ranks_of(o, valid.size)
        bad = int((ranks[c] != want).sum())
        assert bad == 0, (what, c, bad, 'ranks differ from the stable order of the exported errors')
        assert (ranks[c][~valid] == -1).all() and sorted(ranks[c][valid].tolist()) == list(range(int(valid.sum()))), (what, c)
        orders.append(o)
    return orders


def _check_values(logits, labels, ignored, ignore, classes, out, orders, what, weight=1.0, grad=True):
    """Check 2: errors and term against the independent float64 value, the gradient against float64 under the kernel's order (grad=False:
    the caller states what the gradient must be)."""
    loss, term, dl, pe, ranks = out
    ref = LR.evaluate(logits, labels, ignore, classes)
    refk = LR.evaluate(logits, labels, ignore, classes, orders=orders)
    v = ~ignored.reshape(-1)
    e_err = (pe.cpu().double() - ref['err']).abs()[:, v]
    e_term = abs(term.item() - ref['term'])
    tb = TERM_TOL * max(1.0, abs(ref['term']))
    dl_c = dl.cpu()
    gmax = refk['dlogits'].abs().max().item()
    e_grad = (dl_c.double() - weight * refk['dlogits']).abs().max().item()
    print(f'{what}: max|err err| {e_err.max().item() if e_err.numel() else 0.0:.3e} (bound {ERR_TOL:.1e})  |term err| {e_term:.3e} (bound '
          f'{tb:.3e}; term {ref["term"]:.6f})  max|dlogits err| {e_grad:.3e} (bound {GRAD_TOL * weight * gmax:.3e})')
    assert not e_err.numel() or e_err.max().item() <= ERR_TOL, (what, e_err.max().item())
    assert e_term <= tb, (what, term.item(), ref['term'])
    assert loss.item() == np.float32(weight) * np.float32(term.item()), (what, loss.item(), term.item())
    assert torch.isfinite(dl_c).all() and (not grad or e_grad <= GRAD_TOL * weight * gmax), (what, e_grad, gmax)
    assert (dl_c[ignored[:, None].expand_as(dl_c)] == 0).all(), what
    return ref


# ---------------------------------------------------------------- checks 1 and 2 on random inputs
@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_order_is_exact_and_values_match_the_float64_restatement(shape, mask):
    logits, labels, ignored = _inputs(shape, mask)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for classes, weight in (('present', 1.0), ('all', 0.375)):
        out = _run(lg_d, lb_d, _ignore(mask), classes, weight)
        torch.cuda.synchronize()
        what = f'{shape} mask={mask} classes={classes}'
        orders = _check_order(out, ignored, what)
        ref = _check_values(logits, labels, ignored, _ignore(mask), classes, out, orders, what, weight)
        if bool(ignored.all()):                             # (mask 'image' of a one-image batch too)
            assert out[1].item() == 0.0 and out[0].item() == 0.0 and not out[2].any() and (out[4] == -1).all(), what
        else:
            assert ref['term'] > 0 and out[2].any(), what


# ---------------------------------------------------------------- check 1 on inputs made of ties, saturation, one key, low bytes, non-finite values
def _special(kind, shape, mask):
    """(logits, labels, ignored, values_too) of one ill-conditioned input."""
    B, C, H, W = shape
    base, labels, ignored = _inputs(shape, mask)
    r = np.random.default_rng(7)
    if kind == 'saturated':                      # softmax is exactly one-hot in float32: every error is exactly 0 or 1
        pred = torch.from_numpy(r.integers(0, C, (B, H, W)))
        return 400.0 * torch.nn.functional.one_hot(pred, C).permute(0, 3, 1, 2).float() - 200.0, labels, ignored, True
    if kind == 'constant':                       # p = 1/C everywhere: two keys per class (foreground or not), massive ties
        return torch.zeros(shape), labels, ignored, True
    if kind == 'one key':                        # constant logits and labels outside the classes: one key, the order is the pixel index
        return torch.zeros(shape), torch.where(ignored, labels, torch.full_like(labels, 200)), ignored, True
    if kind == 'low byte':                       # errors within a few ulps of 1/C and 1 - 1/C
        return _inputs(shape, mask, 0, 1e-6)[0], labels, ignored, True
    assert kind == 'non-finite'
    logits = base.clone()
    valid_idx = np.nonzero(~ignored.reshape(-1).numpy())[0]
    flat = logits.view(B, C, H * W)
    for j, val in enumerate([float('inf'), -float('inf'), NAN, 1e38, -1e38, NAN] if len(valid_idx) else []):
        p = int(valid_idx[(j * 7919) % len(valid_idx)])
        b, q = divmod(p, H * W)
        flat[b, j % C, q] = val
        if j == 3:
            flat[b, :, q] = float('inf')         # inf - inf: a NaN softmax row
    return logits, labels, ignored, False


@pytest.mark.parametrize('kind', ['saturated', 'constant', 'one key', 'low byte', 'non-finite'])
@pytest.mark.parametrize('mask', ['none', 'random', 'image'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_order_is_exact_on_ill_conditioned_inputs(shape, mask, kind):
    logits, labels, ignored, values_too = _special(kind, shape, mask)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    out = _run(lg_d, lb_d, _ignore(mask), 'all')
    torch.cuda.synchronize()
    what = f'{kind} {shape} mask={mask}'
    orders = _check_order(out, ignored, what)        # (the permutation; the guard bands are checked by @guarded)
    valid = ~ignored.reshape(-1).numpy()
    pe = out[3].cpu().numpy()
    if not valid.any():                                     # a one-image batch whose image is ignored: the order above is all there is
        return
    if kind == 'saturated':
        # float32 softmax is exactly one-hot here, so p_j (q_j - sum_c q_c p_c) is exactly 0 everywhere; the float64 gradient, of the order of
        # exp(-400), lies below float32's smallest subnormal: no relative bar can be put on it
        assert set(np.unique(pe[:, valid]).tolist()) <= {0.0, 1.0} and not out[2].any(), what
    if kind == 'one key':
        assert len(np.unique(pe[:, valid])) == 1 and all((o == np.nonzero(valid)[0]).all() for o in orders), what
    if kind == 'constant':
        assert all(len(np.unique(pe[c, valid])) <= 2 for c in range(shape[1])), what
    if kind == 'low byte':
        k = TR.keys(pe[:, valid])
        assert len(np.unique(k >> np.uint64(8))) <= 4 and len(np.unique(k)) > 4, what      # 1/C and 1 - 1/C, each on one or two sides of a binade
    if values_too:
        _check_values(logits, labels, ignored, _ignore(mask), 'all', out, orders, what, grad=kind != 'saturated')


# ---------------------------------------------------------------- accumulate = 1 behind the masked criterion
def _masked(c, lg_d, lb_d):
    B, C, H, W = lg_d.shape
    ws = guard.alloc_bytes(_lib.load().bdn_criterion_masked_workspace_bytes(B, C, H, W, REDUCE[c.reduce]), label='masked criterion workspace')
    loss, dl = guard.full((1,), NAN), guard.full(tuple(lg_d.shape), NAN)
    _lib.call('bdn_criterion_masked', lg_d.data_ptr(), lb_d.data_ptr(), 255, c.w_overlap, c.alpha, c.beta, c.eps, REDUCE[c.reduce], c.w_focal,
              c.gamma, None, int(c.size_average), ws.data_ptr(), loss.data_ptr(), None, None, dl.data_ptr(), B, C, H, W, st())
    return loss, dl


@pytest.mark.parametrize('mask', ['none', 'random', 'image'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_accumulate_adds_the_weighted_term_to_a_criterion_that_has_run(shape, mask):
    logits, labels, ignored = _inputs(shape, mask)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    c = Criterion.parse('focal+jaccard', focal_gamma=2.0, ignore_index=255)
    w = 0.7
    loss_m, dl_m = _masked(c, lg_d, lb_d)
    sel = ignored[:, None].expand_as(logits).cuda()
    dl_m[sel] = 7.25                                        # a mark at the ignored pixels: accumulate = 1 must not touch them
    loss0, dl0 = loss_m.clone(), dl_m.clone()
    one = _run(lg_d, lb_d, 255, weight=1.0)
    same_w = _run(lg_d, lb_d, 255, weight=w)
    acc = _run(lg_d, lb_d, 255, weight=w, accumulate=1, loss=loss_m, dl=dl_m)
    torch.cuda.synchronize()
    for x, y, what in zip(acc[1:], same_w[1:], NAMES[1:]):
        if what != 'dlogits':
            assert torch.equal(x, y), what                  # term, errors and ranks do not depend on accumulate
    # one float32 add per element of accumulate = 0's value at the same weight: the same bits
    assert torch.equal(acc[0], loss0 + same_w[0])
    want = torch.where(sel, dl0, dl0 + same_w[2])
    assert torch.equal(acc[2], want), int((acc[2] != want).sum())
    assert (acc[2][sel] == 7.25).all()
    # and weight times the weight-1 outputs: the product is rounded to float32, then the sum is (2^-24 (|y| + |x + y|) <= 2^-23 max(|y|, |x + y|))
    x, y = dl0.double(), w * one[2].double()
    bound = 2.0 ** -23 * torch.maximum(y.abs(), (x + y).abs())
    assert ((acc[2].double() - (x + y)).abs() <= bound)[~sel].all()
    xl, yl = loss0.double().item(), w * one[0].double().item()
    assert abs(acc[0].item() - (xl + yl)) <= 2.0 ** -23 * max(abs(yl), abs(xl + yl))


# ---------------------------------------------------------------- the logits of ignored pixels reach no output
@pytest.mark.parametrize('mask', ['random', 'image', 'all'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_ignored_logits_change_no_bit(shape, mask):
    logits, labels, ignored = _inputs(shape, mask)
    sel = ignored[:, None].expand_as(logits)
    bad = logits.clone()
    bad[sel] = torch.tensor(POISON).repeat(logits.numel() // len(POISON) + 1)[:int(sel.sum())]
    lb_d = guard.guard(labels.to(torch.uint8))
    first, lg_bad = dev(logits), dev(bad)
    for classes in ('present', 'all'):
        a, b = _run(first, lb_d, 255, classes, 0.5), _run(lg_bad, lb_d, 255, classes, 0.5)
        torch.cuda.synchronize()
        for x, y, what in zip(a, b, NAMES):
            assert torch.isfinite(y.float()).all() and torch.equal(x, y), (what, classes)


# ---------------------------------------------------------------- determinism, the workspace, optional outputs
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_lovasz_is_deterministic_whatever_the_workspace_held_and_outputs_are_optional(shape):
    B, C, H, W = shape
    logits, labels, _ = _inputs(shape, 'random')
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    n = _lib.load().bdn_lovasz_workspace_bytes(B, C, H, W)
    ws = guard.alloc_bytes(n)                               # 0xFF bytes: NaN as float / double, -1 as an int
    a = _run(lg_d, lb_d, 255, ws=ws)
    b = _run(lg_d, lb_d, 255, ws=ws)                        # the same workspace again: whatever the first call left in it
    z = _run(lg_d, lb_d, 255, ws=guard.alloc_bytes(n).zero_())
    h = _run(lg_d, lb_d, 255, ws=guard.alloc_bytes(n).fill_(0x5A))
    torch.cuda.synchronize()
    for x, y, w, v, what in zip(a, b, z, h, NAMES):
        assert torch.equal(x, y) and torch.equal(x, w) and torch.equal(x, v), what
    loss, term, dl, pe, ranks = _run(lg_d, lb_d, 255, want_dl=False)                        # validation: no gradient pass
    assert dl is None and torch.equal(loss, a[0]) and torch.equal(term, a[1]) and torch.equal(pe, a[3]) and torch.equal(ranks, a[4])
    loss, term, dl, pe, ranks = _run(lg_d, lb_d, 255, want_term=False, want_export=False)
    assert (term, pe, ranks) == (None, None, None) and torch.equal(loss, a[0]) and torch.equal(dl, a[2])
    loss = _run(lg_d, lb_d, 255, want_dl=False, want_term=False, want_export=False)[0]
    assert torch.equal(loss, a[0])


# ---------------------------------------------------------------- classes: 'present' against 'all' with an absent class
@pytest.mark.parametrize('shape', [(3, 2, 90, 77), (1, 8, 16, 300), (2, 3, 1, 5)], ids=str)
@guarded
def test_present_leaves_an_absent_class_out_and_all_keeps_it(shape):
    C = shape[1]
    logits, labels, ignored = _inputs(shape, 'random', absent=1)
    assert not (labels == 1).any()
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    outs = {}
    for classes in ('present', 'all'):
        out = outs[classes] = _run(lg_d, lb_d, 255, classes)
        torch.cuda.synchronize()
        what = f'absent class {shape} classes={classes}'
        orders = _check_order(out, ignored, what)
        ref = _check_values(logits, labels, ignored, 255, classes, out, orders, what)
        assert ref['m'] == (C if classes == 'all' else C - 1)
    assert torch.equal(outs['present'][3], outs['all'][3]) and torch.equal(outs['present'][4], outs['all'][4])
    assert outs['present'][1].item() != outs['all'][1].item() and not torch.equal(outs['present'][2], outs['all'][2])


# ---------------------------------------------------------------- the Python surface
def test_criterion_evaluate_and_compound_loss_agree_with_the_c_abi():
    from fabric_amd.utils import metrics as M
    shape = (3, 2, 90, 77)
    logits, labels, ignored = _inputs(shape, 'random')
    lg, lb = logits.cuda(), labels.cuda()
    lb8 = lb.to(torch.uint8)
    n = lg.numel() // 2
    # focal + Lovasz with an ignore label: the masked criterion, then the term added behind it
    c = Criterion.parse('focal+lovasz', focal_gamma=2.0, weights=(0.25, 2), ignore_index=255, lovasz_classes='all')
    base = Criterion(w_overlap=0.0, w_focal=0.25, gamma=2.0, ignore_index=255)
    loss_m, _, counts_m, dl_m = base.evaluate(lg, lb)
    want = _run(lg, lb8, 255, 'all', 2.0, 1, loss=loss_m.view(1), dl=dl_m)
    pe, ranks = torch.empty(2, n, device='cuda'), torch.empty(2, n, dtype=torch.int32, device='cuda')
    loss, terms, counts, dl = c.evaluate(lg, lb, pixel_errors=pe, ranks=ranks)
    assert torch.equal(loss.view(1), want[0]) and torch.equal(dl, want[2]) and torch.equal(pe, want[3]) and torch.equal(ranks, want[4])
    assert terms.shape == (3,) and terms[0].item() == 0.0 and terms[1].item() > 0 and torch.equal(terms[2:], want[1])
    assert counts.shape == (5,) and torch.equal(counts, counts_m) and torch.equal(counts, M.confusion_counts(lg, lb, 255))
    out = c.buffers(shape, lg.device)
    loss2, terms2, counts2, dl2 = c.evaluate(lg, lb[:, None].to(torch.uint8), out=out)
    assert loss2 is out[1] and torch.equal(loss, loss2) and torch.equal(dl, dl2) and torch.equal(counts, counts2) and torch.equal(terms, terms2)
    assert c.evaluate(lg, lb, want_grad=False)[3] is None and torch.equal(c.evaluate(lg, lb, want_grad=False)[0], loss)
    # the term alone: accumulate = 0, the counts of confusion_counts, with and without an ignore label
    for ignore, lab in ((255, lb), (None, lb.clamp(max=1))):
        alone = Criterion.parse('lovasz', ignore_index=ignore)
        want = _run(lg, lab.to(torch.uint8), ignore)
        loss, terms, counts, dl = alone.evaluate(lg, lab)
        assert torch.equal(loss.view(1), want[0]) and torch.equal(dl, want[2]) and terms.cpu().tolist() == [0.0, 0.0, want[1].item()]
        assert torch.equal(counts, M.confusion_counts(lg, lab, ignore)) and counts.shape == ((5,) if ignore is not None else (4,))
    # topk composes: its own entry point, then the term
    tk = Criterion.parse('focal+lovasz', focal_gamma=0.0, ignore_index=255, topk=0.25)
    loss, terms, counts, dl = tk.evaluate(lg, lb)
    assert terms.shape == (4,) and counts.shape == (6,) and terms[3].item() == _run(lg, lb8, 255)[1].item()
    with pytest.raises(RuntimeError, match='pixel_errors'):
        c.evaluate(lg, lb, pixel_errors=torch.empty(3, device='cuda'))
    with pytest.raises(RuntimeError, match='w_lovasz'):
        Criterion.parse('focal+dice', focal_gamma=2.0).evaluate(lg, lb, ranks=ranks)
    mod = M.CompoundLoss(c)
    x = lg.clone().requires_grad_(True)
    v = mod(x, lb)
    (3.0 * v).backward()
    loss, terms, counts, dl = c.evaluate(lg, lb)
    assert torch.equal(v.detach(), loss) and torch.equal(x.grad, dl * 3.0) and not x.grad[ignored[:, None].expand_as(x).cuda()].any()
    assert torch.equal(mod.last_counts, counts) and torch.equal(mod.last_terms, terms)


def test_without_a_lovasz_weight_the_criterion_calls_what_it_always_did(monkeypatch):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    logits, labels, _ = _inputs((4, 2, 32, 32), 'random')
    lg, lb = logits.cuda(), labels.cuda()
    for kw, entry in (({}, 'bdn_criterion'), ({'ignore_index': 255}, 'bdn_criterion_masked'), ({'ignore_index': 255, 'topk': 0.25}, 'bdn_criterion_topk')):
        del names[:]
        c = Criterion.parse('focal+jaccard', focal_gamma=2.0, **kw)
        out = c.buffers(lg.shape, lg.device)
        n = getattr(_lib.load(), entry + '_workspace_bytes')(4, 2, 32, 32, 0)
        assert out[0].numel() == (n + 15) // 16 * 16 and out[2].shape == ((3,) if 'topk' in kw else (2,))
        c.evaluate(lg, lb if kw else lb.clamp(max=1), out=out)
        assert names == [entry], names
        del names[:]
        Criterion.parse('focal+lovasz', focal_gamma=2.0, **kw).evaluate(lg, lb if kw else lb.clamp(max=1))
        assert names == [entry, 'bdn_lovasz_softmax'], names
