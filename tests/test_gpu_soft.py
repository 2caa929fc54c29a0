"""-m gpu: bdn_criterion_soft (include/bidate_hip.h; label smoothing, pixel weights, float targets) through the C ABI on guard-banded
buffers and a workspace of exactly the queried size.

The yardstick is the float64 restatement tests/soft_ref.py (pinned by tests/test_soft_cpu.py) with the project's bars, as
tests/test_gpu_ignore.py states them:

    |loss - L64|          <= 5e-6 (w_o max(1, |O64|) + w_f max(1, |F64|))          terms: 5e-6 max(1, |v|) each
    max|dlogits - dL64|   <= 3e-4 (w_o max|dO64| + w_f max|dF64|)

Counts are exact; dlogits is exactly 0 at every pixel whose weight is not > 0; what such a pixel holds changes no bit of any output.
"""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import REDUCE, Criterion
from gpu_util import dev, st
from tests import guard
from tests import soft_ref as SR
from tests.guard import guarded
from tests.test_gpu_ignore import GRAD_TOL, LOSS_TOL, MASKS, NAN, POISON, SHAPES, _class_alpha, _inputs

pytestmark = pytest.mark.gpu

CASES = [f'smooth-{m}' for m in MASKS] + ['weights', 'targets', 'targets+weights']
E = 0.1


@functools.lru_cache(maxsize=None)
def _weights(shape, seed=23):
    """float32 [B,H,W]: 30 % zeros, the rest in (0, 2).  Shared: never modified."""
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    w = r.uniform(1e-3, 2.0, (B, H, W)).astype(np.float32)
    w[r.random((B, H, W)) < 0.3] = 0.0
    return torch.from_numpy(w)


@functools.lru_cache(maxsize=None)
def _targets(shape, seed=29):
    """float32 [B,C,H,W] Dirichlet(0.5) targets.  Shared: never modified."""
    B, C, H, W = shape
    q = np.random.default_rng(seed).dirichlet([0.5] * C, (B, H, W)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(q.transpose(0, 3, 1, 2)))


@functools.lru_cache(maxsize=None)
def _case(shape, case):
    """(logits, labels or targets, weights or None, smoothing, ignore_index) of one source, CPU tensors."""
    if case.startswith('smooth-'):
        logits, labels, _ = _inputs(shape, case[len('smooth-'):])
        return logits, labels, None, E, 255
    logits, labels, _ = _inputs(shape, 'none')
    if case == 'weights':
        return logits, labels, _weights(shape), 0.0, None
    return logits, _targets(shape), _weights(shape) if case == 'targets+weights' else None, 0.0, None


def _criteria(C, reduce, ignore=None, smoothing=0.0):
    kw = dict(reduce=reduce, ignore_index=ignore, label_smoothing=smoothing)
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


THREE = ('dice', 'focal(2.0,alpha,mean)', 'focal(2,alpha)+tversky(0.1,0.9) w=(0.25, 2)')
_REF = {}


def _reference(key, c, logits, labels, weights):
    """SR.reference, computed once per (criterion, inputs) key and shared between the tests: never modified."""
    if key not in _REF:
        _REF[key] = SR.reference(c, logits, labels, weights)
    return _REF[key]


def _run(c, lg_d, labels_d=None, targets_d=None, weights_d=None, want_dl=True, want_counts=True, want_terms=True, ws_fill=None,
         ignore=None, smoothing=None):
    """bdn_criterion_soft straight through the C ABI on fresh guarded outputs and a workspace of exactly the size the query returns
    (born 0xFF: NaN as float32 and float64; ws_fill overwrites it)."""
    B, C, H, W = lg_d.shape
    ws = guard.alloc_bytes(_lib.load().bdn_criterion_soft_workspace_bytes(B, C, H, W, REDUCE[c.reduce]), label='soft criterion workspace')
    if ws_fill is not None:
        ws.fill_(ws_fill)
    loss = guard.full((1,), NAN)
    terms = guard.full((2,), NAN) if want_terms else None
    counts = guard.full((5,), -1, dtype=torch.int32) if want_counts else None
    dl = guard.full(tuple(lg_d.shape), NAN) if want_dl else None
    alpha_d = dev(torch.tensor(c.class_alpha[:C])) if c.class_alpha is not None else None
    ignore = (-1 if c.ignore_index is None else c.ignore_index) if ignore is None else ignore
    _lib.call('bdn_criterion_soft', lg_d.data_ptr(), _lib.ptr(labels_d), _lib.ptr(targets_d), _lib.ptr(weights_d), ignore,
              c.label_smoothing if smoothing is None else smoothing, c.w_overlap, c.alpha, c.beta, c.eps, REDUCE[c.reduce], c.w_focal,
              c.gamma, _lib.ptr(alpha_d), int(c.size_average), ws.data_ptr(), loss.data_ptr(), _lib.ptr(terms), _lib.ptr(counts),
              _lib.ptr(dl), B, C, H, W, st())
    return loss, terms, counts, dl


def _source(labels, weights):
    """The device arguments (labels_d, targets_d, weights_d) of CPU labels-or-targets and weights."""
    lab_d = tg_d = None
    if labels.is_floating_point():
        tg_d = dev(labels)
    else:
        lab_d = guard.guard(labels.to(torch.uint8))
    return dict(labels_d=lab_d, targets_d=tg_d, weights_d=None if weights is None else dev(weights))


def _bars(c, ref):
    return (LOSS_TOL * (c.w_overlap * max(1.0, abs(ref['overlap'])) + c.w_focal * max(1.0, abs(ref['focal']))),
            GRAD_TOL * (c.w_overlap * ref['doverlap'].abs().max().item() + c.w_focal * ref['dfocal'].abs().max().item()))


def _check(c, ref, invalid, out, what, want_counts=None):
    loss, terms, counts, dl = out
    lb, gb = _bars(c, ref)
    dl_c = dl.cpu()
    e_loss = abs(loss.item() - ref['loss'])
    e_grad = (dl_c.double() - ref['dloss']).abs().max().item()
    t = terms.cpu().tolist()
    print(f'{what}: |loss err| {e_loss:.3e} (bound {lb:.3e})  max|dlogits err| {e_grad:.3e} (bound {gb:.3e})  '
          f'terms err {abs(t[0] - ref["overlap"]):.3e} {abs(t[1] - ref["focal"]):.3e}')
    assert torch.isfinite(dl_c).all(), what
    assert (dl_c[invalid[:, None].expand_as(dl_c)] == 0).all(), what
    assert e_loss <= lb and e_grad <= gb, (what, e_loss, lb, e_grad, gb)
    assert abs(t[0] - ref['overlap']) <= LOSS_TOL * max(1.0, abs(ref['overlap'])), (what, t, ref['overlap'])
    assert abs(t[1] - ref['focal']) <= LOSS_TOL * max(1.0, abs(ref['focal'])), (what, t, ref['focal'])
    if want_counts is not None:
        assert counts.cpu().tolist() == want_counts, what


# ---------------------------------------------------------------- against the float64 restatement
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_soft_criterion_matches_the_float64_restatement(shape, case):
    logits, labels, weights, e, ignore = _case(shape, case)
    C = shape[1]
    lg_d, src = dev(logits), _source(labels, weights)
    for reduce in ('columns', 'image'):
        for name, c in _criteria(C, reduce, ignore, e):
            out = _run(c, lg_d, **src)
            ref = _reference((name, shape, reduce, case), c, logits, labels, weights)
            _check(c, ref, ~SR.valid(c, C, labels, weights), out, f'{name} {shape} {reduce} {case}',
                   SR.counts(c, logits, labels, weights))
    if case == 'smooth-all':                                # a batch without a valid pixel
        for _, c in _criteria(C, 'columns', ignore, e)[-2:]:
            loss, terms, counts, dl = _run(c, lg_d, **src)
            assert terms.cpu().tolist() == [1.0, 0.0] and loss.item() == c.w_overlap and not dl.any() and counts.cpu().tolist() == [0] * 5


# ---------------------------------------------------------------- smoothing 0 and 0 / 1 weights: the masked criterion
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_hard_labels_with_01_weights_reduce_to_the_masked_criterion(shape):
    logits, painted, ignored = _inputs(shape, 'random')
    w01 = (~ignored).float()
    lg_d, lab_d, w_d = dev(logits), guard.guard(painted.to(torch.uint8)), dev(w01)
    for reduce in ('columns', 'image'):
        for (name, c), (_, plain) in zip(_criteria(shape[1], reduce, 255), _criteria(shape[1], reduce)):
            B, C, H, W = shape
            ws = guard.alloc_bytes(_lib.load().bdn_criterion_masked_workspace_bytes(B, C, H, W, REDUCE[reduce]))
            m = [guard.full((1,), NAN), guard.full((2,), NAN), guard.full((5,), -1, dtype=torch.int32), guard.full(shape, NAN)]
            alpha_d = dev(torch.tensor(c.class_alpha[:C])) if c.class_alpha is not None else None
            _lib.call('bdn_criterion_masked', lg_d.data_ptr(), lab_d.data_ptr(), 255, c.w_overlap, c.alpha, c.beta, c.eps, REDUCE[reduce],
                      c.w_focal, c.gamma, _lib.ptr(alpha_d), int(c.size_average), ws.data_ptr(), m[0].data_ptr(), m[1].data_ptr(),
                      m[2].data_ptr(), m[3].data_ptr(), B, C, H, W, st())
            ref = _reference((name, shape, reduce, 'weights01'), plain, logits, painted, w01)
            lb, gb = _bars(c, ref)
            for what, out in (('weights 0/1', _run(plain, lg_d, labels_d=lab_d, weights_d=w_d)), ('ignore label', _run(c, lg_d, labels_d=lab_d))):
                assert abs(out[0].item() - m[0].item()) <= lb, (name, reduce, what)
                for k in (0, 1):
                    assert abs(out[1][k].item() - m[1][k].item()) <= LOSS_TOL * max(1.0, abs(m[1][k].item())), (name, reduce, what)
                assert (out[3].double() - m[3].double()).abs().max().item() <= gb, (name, reduce, what)
                assert torch.equal(out[2], m[2]), (name, reduce, what)
                print(f'{name} {shape} {reduce} {what}: bit-equal to bdn_criterion_masked: loss {torch.equal(out[0], m[0])} '
                      f'terms {torch.equal(out[1], m[1])} dlogits {torch.equal(out[3], m[3])}')


# ---------------------------------------------------------------- the two sources are one function
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_smoothed_labels_and_the_same_float_targets_agree(shape):
    logits, labels, _ = _inputs(shape, 'none')
    B, C, H, W = shape
    hi, lo = SR.smoothed_pair(E, C)
    one_hot = (labels[:, None] == torch.arange(C).view(1, C, 1, 1))
    q = torch.where(one_hot, torch.tensor(hi), torch.tensor(lo)).contiguous()
    assert q.dtype == torch.float32
    weights = _weights(shape)
    lg_d, lab_d, q_d, w_d = dev(logits), guard.guard(labels.to(torch.uint8)), dev(q), dev(weights)
    for reduce in ('columns', 'image'):
        for (name, c), (_, plain) in zip(_criteria(C, reduce, None, E), _criteria(C, reduce)):
            for wd, wc, tag in ((None, None, 'smooth-none'), (w_d, weights, 'smooth+weights')):
                a = _run(c, lg_d, labels_d=lab_d, weights_d=wd)
                b = _run(plain, lg_d, targets_d=q_d, weights_d=wd)
                ref = _reference((name, shape, reduce, tag), c, logits, labels, wc)
                lb, gb = _bars(c, ref)
                assert abs(a[0].item() - b[0].item()) <= lb and (a[3].double() - b[3].double()).abs().max().item() <= gb, (name, reduce, tag)
                for k in (0, 1):
                    assert abs(a[1][k].item() - b[1][k].item()) <= LOSS_TOL * max(1.0, abs(a[1][k].item())), (name, reduce, tag)
                assert torch.equal(a[2], b[2]), (name, reduce, tag)
                print(f'{name} {shape} {reduce} {tag}: the two sources bit-equal: loss {torch.equal(a[0], b[0])} dlogits {torch.equal(a[3], b[3])}')


# ---------------------------------------------------------------- what an invalid pixel holds reaches no output
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@guarded
def test_invalid_pixels_change_no_bit(shape):
    logits, labels, _ = _inputs(shape, 'none')
    C = shape[1]
    weights = _weights(shape)
    invalid = ~(weights > 0)
    sel = invalid[:, None].expand_as(logits)
    bad = logits.clone()
    bad[sel] = torch.tensor(POISON).repeat(logits.numel() // len(POISON) + 1)[:int(sel.sum())]
    q = _targets(shape)
    bad_q = q.clone()
    bad_q[sel] = NAN
    painted = torch.where(invalid, torch.full_like(labels, 255), labels)       # the same pixels, as an ignore label
    first, lg_bad, w_d = dev(logits), dev(bad), dev(weights)
    lab_d, pnt_d, q_d, bad_q_d = guard.guard(labels.to(torch.uint8)), guard.guard(painted.to(torch.uint8)), dev(q), dev(bad_q)
    for reduce in ('columns', 'image'):
        smooth, masked, plain = (dict(_criteria(C, reduce, ig, e)) for ig, e in ((None, E), (255, E), (None, 0.0)))
        for name in THREE:
            runs = ((smooth[name], dict(labels_d=lab_d, weights_d=w_d), dict(labels_d=lab_d, weights_d=w_d)),
                    (masked[name], dict(labels_d=pnt_d), dict(labels_d=pnt_d)),
                    (plain[name], dict(targets_d=q_d, weights_d=w_d), dict(targets_d=bad_q_d, weights_d=w_d)))
            for c, clean_src, bad_src in runs:
                a, b = _run(c, first, **clean_src), _run(c, lg_bad, **bad_src)
                torch.cuda.synchronize()
                for x, y, what in zip(a, b, ('loss', 'terms', 'counts', 'dlogits')):
                    assert torch.isfinite(y.float()).all() and torch.equal(x, y), (what, name, reduce)
                assert not b[3][sel.cuda()].any()


# ---------------------------------------------------------------- targets that are exactly 0: selected out, never multiplied
@pytest.mark.parametrize('shape', [(3, 2, 90, 77), (1, 8, 16, 300)], ids=str)
@guarded
def test_zero_targets_at_very_negative_logits(shape):
    B, C, H, W = shape
    r = np.random.default_rng(41)
    q = _targets(shape).clone()
    zero = torch.from_numpy(r.random(shape) < 0.4)
    zero[:, 0] &= ~zero[:, 1:].all(1)                       # every pixel keeps a class
    q[zero] = 0.0
    logits = _inputs(shape, 'none')[0].clone()
    logits[zero] = -100.0
    lg_d, q_d = dev(logits), dev(q)
    for reduce in ('columns', 'image'):
        for name, c in _criteria(C, reduce):
            out = _run(c, lg_d, targets_d=q_d)
            ref = _reference((name, shape, reduce, 'zero targets'), c, logits, q, None)
            _check(c, ref, torch.zeros(B, H, W, dtype=torch.bool), out, f'{name} {shape} {reduce} zero targets',
                   SR.counts(c, logits, q))
            assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()


# ---------------------------------------------------------------- determinism and optional outputs
@pytest.mark.parametrize('shape', [(3, 2, 90, 77), (1, 8, 16, 300)], ids=str)
@guarded
def test_soft_is_deterministic_and_outputs_are_optional(shape):
    logits, labels, _ = _inputs(shape, 'random')
    C = shape[1]
    lg_d = dev(logits)
    hard = dict(labels_d=guard.guard(labels.to(torch.uint8)), weights_d=dev(_weights(shape)))
    soft = dict(targets_d=dev(_targets(shape)), weights_d=hard['weights_d'])
    for reduce in ('columns', 'image'):
        for crit, src in ((dict(_criteria(C, reduce, 255, E)), hard), (dict(_criteria(C, reduce)), soft)):
            for name in THREE:
                c = crit[name]
                a, b, z = _run(c, lg_d, **src), _run(c, lg_d, **src), _run(c, lg_d, ws_fill=0, **src)     # (a, b: a workspace born as NaN)
                torch.cuda.synchronize()
                for x, y, y0, what in zip(a, b, z, ('loss', 'terms', 'counts', 'dlogits')):
                    assert torch.equal(x, y) and torch.equal(x, y0), (what, name, reduce)
                loss, terms, counts, dl = _run(c, lg_d, want_dl=False, **src)                        # validation: no gradient pass
                assert dl is None and torch.equal(loss, a[0]) and torch.equal(counts, a[2]) and torch.equal(terms, a[1])
                loss, terms, counts, dl = _run(c, lg_d, want_counts=False, want_terms=False, **src)
                assert counts is None and terms is None and torch.equal(loss, a[0]) and torch.equal(dl, a[3])
                loss, terms, counts, dl = _run(c, lg_d, want_dl=False, want_counts=False, want_terms=False, **src)
                assert (terms, counts, dl) == (None, None, None) and torch.equal(loss, a[0])


# ---------------------------------------------------------------- refusals: BDN_E_ARG before any launch, outputs untouched
@guarded
def test_refusals_leave_the_outputs_untouched():
    shape = (2, 3, 1, 5)
    B, C, H, W = shape
    logits, labels, _ = _inputs(shape, 'none')
    lg, lab, q, w = dev(logits), guard.guard(labels.to(torch.uint8)), dev(_targets(shape)), dev(_weights(shape))
    ws = guard.alloc_bytes(_lib.load().bdn_criterion_soft_workspace_bytes(B, C, H, W, 0) + 16)
    loss, terms, dl = guard.full((2,), NAN), guard.full((3,), NAN), guard.full((B * C * H * W + 1,), NAN)
    counts = guard.full((6,), -1, dtype=torch.int32)
    good = dict(logits=lg.data_ptr(), labels=lab.data_ptr(), targets=None, weights=w.data_ptr(), ignore=-1, smoothing=0.0, w_o=1.0, w_f=1.0,
                gamma=2.0, ws=ws.data_ptr(), loss=loss.data_ptr(), terms=terms.data_ptr(), counts=counts.data_ptr(), dl=dl.data_ptr())
    tg = dict(labels=None, targets=q.data_ptr())
    cases = [dict(labels=None), dict(targets=q.data_ptr()), dict(smoothing=-0.1), dict(smoothing=1.0), dict(smoothing=NAN),
             dict(tg, smoothing=0.1), dict(ignore=-2), dict(ignore=256), dict(tg, ignore=255), dict(w_o=0.0, w_f=0.0), dict(ws=None),
             dict(loss=None), dict(logits=None), dict(ws=ws.data_ptr() + 8), dict(logits=lg.data_ptr() + 2), dict(weights=w.data_ptr() + 2),
             dict(tg, targets=q.data_ptr() + 2), dict(loss=loss.data_ptr() + 2), dict(terms=terms.data_ptr() + 2),
             dict(counts=counts.data_ptr() + 2), dict(dl=dl.data_ptr() + 2)]
    for kw in cases:
        a = dict(good, **kw)
        with pytest.raises(RuntimeError, match=r'bdn_criterion_soft failed \(rc=-1\)'):
            _lib.call('bdn_criterion_soft', a['logits'], a['labels'], a['targets'], a['weights'], a['ignore'], a['smoothing'], a['w_o'], 0.5, 0.5,
                      1e-7, 0, a['w_f'], a['gamma'], None, 1, a['ws'], a['loss'], a['terms'], a['counts'], a['dl'], B, C, H, W, st())
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(terms).all() and torch.isnan(dl).all() and (counts == -1).all()
    assert (ws == 0xFF).all()
