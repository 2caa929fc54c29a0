"""-m gpu: bdn_criterion_topk (include/bidate_hip.h; Criterion(topk=)) through the C ABI on guard-banded buffers, with a workspace of
exactly the queried size (0xFF-filled: NaN-born).

Two yardsticks.  The SELECTION is checked exactly, in integers: `kept` must equal tests/topk_ref.select applied to the kernel's own exported
`pixel_terms` (key map and tie rule of the header), on every input of this file.  The VALUES are checked against the float64 restatement
tests/topk_ref.py (pinned by tests/test_topk_cpu.py) on inputs whose float64 selection is well separated -- the first seed in 0..63 for which
the gap between the K-th and the (K+1)-th largest term exceeds 1e-4 times the K-th -- with the project's bars (tests/test_gpu_criterion.py):

    |pixel_terms - t64|   <= 5e-6 max(1, |t64|)
    |loss - L64|          <= 5e-6 (w_o max(1, |O64|) + w_f max(1, |F64|))          terms: 5e-6 max(1, |v|) each
    max|dlogits - dL64|   <= 3e-4 (w_o max|dO64| + w_f max|dF64|)

"dlogits is nonzero at a kept pixel" is asserted where the kernel's own term is nonzero: a kept pixel whose pt rounds to 1 in float32 (or
whose class weight is 0) has the term -0 and, correctly, a zero focal gradient.
"""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import REDUCE, Criterion
from gpu_util import dev, st
from tests import guard
from tests import topk_ref as TR
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 90, 77),       # 82 chunks of 256 pixels, a row tail, W not a power of two
          (1, 8, 16, 300),      # two column blocks, the 8-class instantiation
          (4, 2, 32, 32), (2, 3, 1, 5)]
PPMS = [1_000_000, 250_000, 100_000, 1]
MASKS = ['none', 'random', 'image', 'all']
LOSS_TOL, GRAD_TOL, TERM_TOL = 5e-6, 3e-4, 5e-6
NAN = float('nan')
POISON = [1e30, float('inf'), -float('inf'), NAN]
NAMES = ('loss', 'terms', 'counts', 'dlogits', 'pixel_terms', 'kept')


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
def _inputs(shape, mask, seed=0, scale=3.0):
    """float32 logits, int64 labels [B,H,W] with the ignored pixels painted 255, the bool mask of ignored pixels.  Shared: never modified."""
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))
    labels = torch.from_numpy(r.integers(0, C, (B, H, W)).astype(np.int64))
    m = _mask(shape, mask, r)
    return logits, torch.where(m, torch.full_like(labels, 255), labels), m


def _class_alpha(C):
    return [0.25, 0.75] if C == 2 else [round(0.1 + 0.8 * k / (C - 1), 3) for k in range(C)]


def _crit(mask, ppm, **kw):
    return dict(ignore_index=None if mask == 'none' else 255, topk=ppm / 1e6, **kw)


def _criteria(C, mask, ppm):
    """[(name, criterion)]: focal gamma 0 / 2, with and without class weights, mean and sum; the two compound forms with both weightings and
    both reductions."""
    out = []
    for g in (0.0, 2.0):
        for a in (None, _class_alpha(C)):
            for sa in (True, False):
                out.append((f'focal({g},{"alpha" if a else "-"},{"mean" if sa else "sum"})',
                            Criterion(w_overlap=0.0, w_focal=1.0, gamma=g, class_alpha=a, size_average=sa, **_crit(mask, ppm))))
    ca = 0.25 if C == 2 else _class_alpha(C)
    for reduce in ('columns', 'image'):
        for w in ((1, 1), (0.25, 2)):
            out.append((f'focal(2)+dice w={w} {reduce}', Criterion.parse('focal+dice', focal_gamma=2.0, weights=w, reduce=reduce, **_crit(mask, ppm))))
            out.append((f'focal(2,alpha)+tversky(0.1,0.9) w={w} {reduce}',
                        Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=ca, weights=w,
                                        reduce=reduce, **_crit(mask, ppm))))
    return out


@functools.lru_cache(maxsize=None)
def _separated_seed(shape, mask, ppm, gamma, alpha, scale=3.0):
    """The first seed in 0..63 whose float64 selection is separated: (K-th - (K+1)-th largest term) > 1e-4 * K-th."""
    c = Criterion(w_overlap=0.0, w_focal=1.0, gamma=gamma, class_alpha=list(alpha) if alpha else None, **_crit(mask, ppm))
    for seed in range(64):
        logits, labels, _ = _inputs(shape, mask, seed, scale)
        kth, nxt = TR.gap(c, logits, labels)
        if kth is None or nxt is None or kth - nxt > 1e-4 * kth:
            return seed
    raise AssertionError(f'no separated input among seeds 0..63 for {shape} {mask} ppm={ppm} gamma={gamma} alpha={alpha}')


def _run(c, lg_d, lb_d, want_dl=True, want_counts=True, want_terms=True, want_export=True, ws=None):
    """bdn_criterion_topk straight through the C ABI on fresh guarded outputs and a workspace of exactly the size the query returns."""
    B, C, H, W = lg_d.shape
    if ws is None:
        ws = guard.alloc_bytes(_lib.load().bdn_criterion_topk_workspace_bytes(B, C, H, W, REDUCE[c.reduce]), label='topk criterion workspace')
    loss = guard.full((1,), NAN)
    terms = guard.full((3,), NAN) if want_terms else None
    counts = guard.full((6,), -1, dtype=torch.int32) if want_counts else None
    dl = guard.full(tuple(lg_d.shape), NAN) if want_dl else None
    pt = guard.full((B * H * W,), NAN) if want_export else None
    kept = guard.full((B * H * W,), 77, dtype=torch.uint8) if want_export else None
    alpha_d = dev(torch.tensor(c.class_alpha[:C])) if c.class_alpha is not None else None
    _lib.call('bdn_criterion_topk', lg_d.data_ptr(), lb_d.data_ptr(), -1 if c.ignore_index is None else c.ignore_index, c.w_overlap, c.alpha,
              c.beta, c.eps, REDUCE[c.reduce], c.w_focal, c.gamma, _lib.ptr(alpha_d), int(c.size_average), c.topk_ppm, ws.data_ptr(),
              loss.data_ptr(), _lib.ptr(terms), _lib.ptr(counts), _lib.ptr(dl), _lib.ptr(pt), _lib.ptr(kept), B, C, H, W, st())
    return loss, terms, counts, dl, pt, kept


def _masked(c, lg_d, lb_d):
    """bdn_criterion_masked with the same criterion (an ignore label no pixel carries when the criterion has none): loss and dlogits."""
    B, C, H, W = lg_d.shape
    ws = guard.alloc_bytes(_lib.load().bdn_criterion_masked_workspace_bytes(B, C, H, W, REDUCE[c.reduce]), label='masked criterion workspace')
    loss, dl = guard.full((1,), NAN), guard.full(tuple(lg_d.shape), NAN)
    alpha_d = dev(torch.tensor(c.class_alpha[:C])) if c.class_alpha is not None else None
    _lib.call('bdn_criterion_masked', lg_d.data_ptr(), lb_d.data_ptr(), 255, c.w_overlap, c.alpha, c.beta, c.eps, REDUCE[c.reduce], c.w_focal,
              c.gamma, _lib.ptr(alpha_d), int(c.size_average), ws.data_ptr(), loss.data_ptr(), None, None, dl.data_ptr(), B, C, H, W, st())
    return loss, dl


def _check_exact(c, logits, labels, ignored, out, what):
    """Check 1: counts (K included), the kept set against select() on the exported terms, terms[2], the zero pattern of dlogits."""
    loss, terms, counts, dl, pt, kept = out
    C = logits.shape[1]
    want_counts = TR.counts(logits, labels, c.ignore_index, c.topk_ppm)
    assert counts.cpu().tolist() == want_counts, (what, counts.cpu().tolist(), want_counts)
    K = want_counts[5]
    valid = ~ignored.reshape(-1).numpy()
    pt_c, kept_c = pt.cpu().numpy(), kept.cpu().numpy()
    assert set(np.unique(kept_c).tolist()) <= {0, 1}, what
    want = TR.select(pt_c, valid, K)
    assert int(kept_c.sum()) == K, (what, int(kept_c.sum()), K)
    assert (kept_c.astype(bool) == want).all(), (what, int((kept_c.astype(bool) != want).sum()))
    thr = terms.cpu().numpy()[2:3]
    if K:
        kth = pt_c[want][np.argmin(TR.keys(pt_c[want]))]
        assert thr.view(np.uint32)[0] == np.array([kth], np.float32).view(np.uint32)[0], (what, thr, kth)
    else:
        assert thr.view(np.uint32)[0] == 0, what
    if dl is not None:
        dl_c = dl.cpu()
        assert (dl_c[ignored[:, None].expand_as(dl_c)] == 0).all(), what
        if c.w_overlap == 0:
            nz = (dl_c != 0).any(1).reshape(-1).numpy()
            has_class = valid & (labels.reshape(-1).numpy() < C)
            assert not nz[~want].any(), (what, 'a focal gradient outside the kept set')
            assert nz[want & has_class & (pt_c != 0)].all(), (what, 'a kept pixel without a focal gradient')
    return want, K, pt_c


def _check_values(c, logits, labels, ignored, out, what):
    """Check 2: against the float64 restatement (the input is separated: the float64 selection is the kernel's)."""
    loss, terms, counts, dl, pt, kept = out
    ref = TR.reference(c, logits, labels)
    assert ref['K'] == int(counts.cpu()[5]), what
    assert (kept.cpu().bool() == ref['kept']).all(), (what, 'kept set differs from the float64 selection')
    v = ~ignored.reshape(-1)
    e_t = ((pt.cpu().double() - ref['terms']).abs() / ref['terms'].abs().clamp(min=1.0))[v]
    lb = LOSS_TOL * (c.w_overlap * max(1.0, abs(ref['overlap'])) + c.w_focal * max(1.0, abs(ref['focal'])))
    gb = GRAD_TOL * (c.w_overlap * ref['doverlap'].abs().max().item() + c.w_focal * ref['dfocal'].abs().max().item())
    dl_c = dl.cpu()
    e_loss = abs(loss.item() - ref['loss'])
    e_grad = (dl_c.double() - ref['dloss']).abs().max().item()
    t = terms.cpu().tolist()
    print(f'{what}: |loss err| {e_loss:.3e} (bound {lb:.3e})  max|dlogits err| {e_grad:.3e} (bound {gb:.3e})  terms err '
          f'{abs(t[0] - ref["overlap"] * (c.w_overlap > 0)):.3e} {abs(t[1] - ref["focal"]):.3e} {abs(t[2] - ref["threshold"]):.3e}  '
          f'pixel terms {e_t.max().item() if e_t.numel() else 0.0:.3e} (bound {TERM_TOL:.1e})')
    assert torch.isfinite(dl_c).all(), what
    assert not e_t.numel() or e_t.max().item() <= TERM_TOL, (what, e_t.max().item())
    assert e_loss <= lb and e_grad <= gb, (what, e_loss, lb, e_grad, gb)
    assert abs(t[0] - (ref['overlap'] if c.w_overlap > 0 else 0.0)) <= LOSS_TOL * max(1.0, abs(ref['overlap'])), (what, t, ref['overlap'])
    assert abs(t[1] - ref['focal']) <= LOSS_TOL * max(1.0, abs(ref['focal'])), (what, t, ref['focal'])
    assert abs(t[2] - ref['threshold']) <= TERM_TOL * max(1.0, abs(ref['threshold'])), (what, t, ref['threshold'])


# ---------------------------------------------------------------- checks 1 and 2: exact selection, parity on separated inputs
@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_topk_selection_is_exact_and_values_match_the_float64_restatement(shape, mask):
    C = shape[1]
    on_dev = {}
    for ppm in PPMS:
        for name, c in _criteria(C, mask, ppm):
            seed = _separated_seed(shape, mask, ppm, c.gamma, tuple(c.class_alpha) if c.class_alpha else None)
            logits, labels, ignored = _inputs(shape, mask, seed)
            if seed not in on_dev:
                on_dev[seed] = dev(logits), guard.guard(labels.to(torch.uint8))
            out = _run(c, *on_dev[seed])
            torch.cuda.synchronize()
            what = f'{name} {shape} mask={mask} ppm={ppm} seed={seed}'
            _check_exact(c, logits, labels, ignored, out, what)
            _check_values(c, logits, labels, ignored, out, what)
            if mask == 'all':
                loss, terms, counts, dl = out[:4]
                assert terms.cpu().tolist() == [1.0 if c.w_overlap else 0.0, 0.0, 0.0] and loss.item() == c.w_overlap, what
                assert not dl.any() and counts.cpu().tolist() == [0] * 6 and not out[5].any(), what


# ---------------------------------------------------------------- check 3: ties
@pytest.mark.parametrize('mask', ['none', 'random', 'image'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_ties_are_kept_in_pixel_index_order(shape, mask):
    C = shape[1]
    _, labels, ignored = _inputs(shape, mask)
    lb_d = guard.guard(labels.to(torch.uint8))
    zeros = torch.zeros(shape)
    quant = (torch.round(_inputs(shape, mask)[0] * 2) / 2).clamp(-1.5, 1.5)      # multiples of 0.5: many equal keys across the blocks
    for logits in (zeros, quant):
        lg_d = dev(logits)
        for ppm in PPMS:
            for c in (Criterion(w_overlap=0.0, w_focal=1.0, gamma=2.0, **_crit(mask, ppm)),
                      Criterion.parse('focal+dice', focal_gamma=0.0, weights=(0.25, 2), **_crit(mask, ppm))):
                out = _run(c, lg_d, lb_d)
                torch.cuda.synchronize()
                want, K, pt_c = _check_exact(c, logits, labels, ignored, out, f'ties {shape} mask={mask} ppm={ppm} zeros={logits is zeros}')
                if logits is zeros:                             # every valid pixel has the same term: the first K valid pixels
                    valid_idx = np.nonzero(~ignored.reshape(-1).numpy())[0]
                    assert len(np.unique(pt_c[valid_idx])) <= 1          # (none with every pixel ignored)
                    assert np.nonzero(out[5].cpu().numpy())[0].tolist() == valid_idx[:K].tolist()


# ---------------------------------------------------------------- check 4: the last radix level decides
@pytest.mark.parametrize('mask', ['none', 'random'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_keys_that_differ_in_the_low_digits_only(shape, mask):
    logits, labels, ignored = _inputs(shape, mask, 0, 1e-3)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for ppm in PPMS:
        for c in (Criterion(w_overlap=0.0, w_focal=1.0, gamma=0.0, **_crit(mask, ppm)),
                  Criterion.parse('focal+dice', focal_gamma=2.0, **_crit(mask, ppm))):
            out = _run(c, lg_d, lb_d)
            torch.cuda.synchronize()
            what = f'low digits {shape} mask={mask} ppm={ppm}'
            want, K, pt_c = _check_exact(c, logits, labels, ignored, out, what)
            k = TR.keys(pt_c[~ignored.reshape(-1).numpy()])
            assert len(np.unique(k >> np.uint64(21))) <= 2, what                  # sign, exponent and two mantissa bits are shared
            # the loss: the kept set is the kernel's (exact over its own terms), the values are held to float64 on that set
            kept = torch.from_numpy(want)
            total, ov, fo, _, _ = TR.loss(c, logits.double(), labels, kept)
            lb = LOSS_TOL * (c.w_overlap * max(1.0, abs(float(ov))) + c.w_focal * max(1.0, abs(float(fo))))
            print(f'{what}: |loss err| {abs(out[0].item() - float(total)):.3e} (bound {lb:.3e})')
            assert abs(out[0].item() - float(total)) <= lb, (what, out[0].item(), float(total))


# ---------------------------------------------------------------- check 5: one huge / infinite term
@pytest.mark.parametrize('value', [-1e30, -float('inf')], ids=['-1e30', '-inf'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_one_pixel_with_an_extreme_term_is_kept_and_exactly_k_pixels_are(shape, value):
    """A true-class logit of -1e30 gives the float32 term 1e30 a[t] (log pt = -1e30 is finite in float32); -inf gives the term +inf, the
    top key of all.  Either way that pixel ranks first and the select ends with exactly K kept pixels."""
    B, C, H, W = shape
    logits, labels, ignored = _inputs(shape, 'random')
    valid_idx = np.nonzero(~ignored.reshape(-1).numpy())[0]
    p = int(valid_idx[len(valid_idx) // 2])
    b, q = divmod(p, H * W)
    logits = logits.clone()
    logits.view(B, C, H * W)[b, int(labels.reshape(-1)[p]), q] = value
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for ppm in PPMS:
        for c in (Criterion(w_overlap=0.0, w_focal=1.0, gamma=2.0, **_crit('random', ppm)),
                  Criterion.parse('focal+dice', focal_gamma=0.0, **_crit('random', ppm))):
            out = _run(c, lg_d, lb_d)
            torch.cuda.synchronize()
            want, K, pt_c = _check_exact(c, logits, labels, ignored, out, f'extreme {value} {shape} ppm={ppm}')
            assert pt_c[p] == (np.float32(1e30) if value == -1e30 else np.float32(np.inf)), pt_c[p]
            assert out[5][p].item() == 1 and int(out[5].sum()) == K and out[1][2].item() <= pt_c[p]
            if ppm == 1:
                assert out[1][2].item() == pt_c[p]


# ---------------------------------------------------------------- check 6: the logits of ignored pixels reach no output
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
    for ppm in (250_000, 1):
        for reduce in ('columns', 'image'):
            for c in (Criterion(w_overlap=0.0, w_focal=1.0, gamma=2.0, class_alpha=_class_alpha(shape[1]), **_crit(mask, ppm)),
                      Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, weights=(0.25, 2), reduce=reduce,
                                      **_crit(mask, ppm))):
                a, b = _run(c, first, lb_d), _run(c, lg_bad, lb_d)
                torch.cuda.synchronize()
                for x, y, what in zip(a, b, NAMES):
                    assert torch.isfinite(y.float()).all() and torch.equal(x, y), (what, ppm, reduce)


# ---------------------------------------------------------------- check 7: determinism, the workspace, optional outputs, ppm = 1e6
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_topk_is_deterministic_whatever_the_workspace_held_and_outputs_are_optional(shape):
    B, C, H, W = shape
    logits, labels, _ = _inputs(shape, 'random')
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for ppm in (250_000, 1):
        for reduce in ('columns', 'image'):
            for c in (Criterion(w_overlap=0.0, w_focal=1.0, gamma=2.0, class_alpha=_class_alpha(C), **_crit('random', ppm)),
                      Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, weights=(0.25, 2), reduce=reduce,
                                      **_crit('random', ppm))):
                n = _lib.load().bdn_criterion_topk_workspace_bytes(B, C, H, W, REDUCE[c.reduce])
                ws = guard.alloc_bytes(n)                       # 0xFF bytes: NaN as float / double, -1 as an int
                a = _run(c, lg_d, lb_d, ws=ws)
                b = _run(c, lg_d, lb_d, ws=ws)                  # the same workspace again: whatever the first call left in it
                z = _run(c, lg_d, lb_d, ws=guard.alloc_bytes(n).zero_())
                torch.cuda.synchronize()
                for x, y, w, what in zip(a, b, z, NAMES):
                    assert torch.equal(x, y) and torch.equal(x, w), (what, ppm, reduce)
                loss, terms, counts, dl, pt, kept = _run(c, lg_d, lb_d, want_dl=False)          # validation: no gradient pass
                assert dl is None and torch.equal(loss, a[0]) and torch.equal(counts, a[2]) and torch.equal(terms, a[1]) and torch.equal(kept, a[5])
                loss, terms, counts, dl, pt, kept = _run(c, lg_d, lb_d, want_counts=False, want_terms=False, want_export=False)
                assert (terms, counts, pt, kept) == (None, None, None, None) and torch.equal(loss, a[0]) and torch.equal(dl, a[3])
                loss = _run(c, lg_d, lb_d, want_dl=False, want_counts=False, want_terms=False, want_export=False)[0]
                assert torch.equal(loss, a[0])


@pytest.mark.parametrize('mask', ['none', 'random'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_every_pixel_kept_agrees_with_the_masked_criterion(shape, mask):
    """ppm = 1 000 000: the same function as bdn_criterion_masked, within the two bars (the focal sum has another association)."""
    logits, labels, ignored = _inputs(shape, mask)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    for name, c in _criteria(shape[1], mask, 1_000_000):
        out, ref = _run(c, lg_d, lb_d), _masked(c, lg_d, lb_d)
        torch.cuda.synchronize()
        r64 = TR.reference(c, logits, labels)
        lb = LOSS_TOL * (c.w_overlap * max(1.0, abs(r64['overlap'])) + c.w_focal * max(1.0, abs(r64['focal'])))
        gb = GRAD_TOL * (c.w_overlap * r64['doverlap'].abs().max().item() + c.w_focal * r64['dfocal'].abs().max().item())
        e_loss, e_grad = abs(out[0].item() - ref[0].item()), (out[3] - ref[1]).abs().max().item()
        print(f'{name} {shape} mask={mask}: loss diff {e_loss:.3e} (bound {lb:.3e}) dlogits diff {e_grad:.3e} (bound {gb:.3e}) '
              f'bit-equal dlogits {torch.equal(out[3], ref[1])}')
        assert e_loss <= lb and e_grad <= gb, (name, e_loss, lb, e_grad, gb)
        assert out[2].cpu().tolist()[4] == out[2].cpu().tolist()[5] == int((~ignored).sum())


# ---------------------------------------------------------------- the Python surface
def test_criterion_evaluate_and_compound_loss_agree_with_the_c_abi():
    from fabric_amd.utils import metrics as M
    shape = (3, 2, 90, 77)
    logits, labels, ignored = _inputs(shape, 'random')
    c = Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=0.25, weights=(0.25, 2),
                        ignore_index=255, topk=0.25)
    lg, lb = logits.cuda(), labels.cuda()
    want = [t.clone() for t in _run(c, lg, lb.to(torch.uint8))]
    pt, kept = torch.empty(lg.numel() // 2, device='cuda'), torch.empty(lg.numel() // 2, dtype=torch.uint8, device='cuda')
    loss, terms, counts, dl = c.evaluate(lg, lb, pixel_terms=pt, kept=kept)
    for x, y in zip((loss.view(1), terms, counts, dl, pt, kept), want):
        assert torch.equal(x, y)
    assert terms.shape == (3,) and counts.shape == (6,) and counts.cpu().tolist() == TR.counts(logits, labels, 255, 250_000)
    out = c.buffers(shape, lg.device)
    assert out[2].shape == (3,) and out[3].shape == (6,)
    loss2, _, counts2, dl2 = c.evaluate(lg, lb[:, None].to(torch.uint8), out=out)
    assert loss2 is out[1] and torch.equal(loss, loss2) and torch.equal(dl, dl2) and torch.equal(counts, counts2)
    assert c.evaluate(lg, lb, want_grad=False)[3] is None
    with pytest.raises(RuntimeError, match='pixel_terms'):
        c.evaluate(lg, lb, pixel_terms=torch.empty(3, device='cuda'))
    with pytest.raises(RuntimeError, match='topk'):
        Criterion.parse('focal+dice', focal_gamma=2.0).evaluate(lg, lb, kept=kept)
    mod = M.CompoundLoss(c)
    x = lg.clone().requires_grad_(True)
    v = mod(x, lb)
    (3.0 * v).backward()
    assert torch.equal(v.detach(), loss) and torch.equal(x.grad, dl * 3.0) and not x.grad[ignored[:, None].expand_as(x).cuda()].any()
    assert torch.equal(mod.last_counts, counts) and torch.equal(mod.last_terms, terms)
    # without topk: today's objects and entry points
    plain = Criterion.parse('focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=0.25, weights=(0.25, 2),
                            ignore_index=255)
    assert plain.buffers(shape, lg.device)[2].shape == (2,) and plain.evaluate(lg, lb)[2].shape == (5,)
