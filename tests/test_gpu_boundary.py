"""-m gpu: bdn_boundary_loss (include/bidate_hip.h; Criterion(w_boundary=)) through the C ABI on guard-banded buffers, with a workspace of
exactly the queried size (0xFF-filled: NaN-born).

phi comes from integers and one correctly rounded sqrtf: it is compared EXACTLY with tests/edt_ref.phi_ref, and dlogits must be exactly 0 at
ignored pixels.  Term and gradient are compared with the float64 restatement tests/edt_ref.boundary_loss_ref under the bars of
tests/test_gpu_lovasz.py, this project's record for a float32 softmax term:

    |term - T64|          <= 5e-6 max(1, |T64|)
    max|dlogits - dT64|   <= 3e-4 weight max|dT64|

Every case prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import Criterion
from gpu_util import dev, st
from tests import edt_ref as ER
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 5, 7), (2, 3, 33, 65), (3, 2, 128, 128)]
TERM_TOL, GRAD_TOL = 5e-6, 3e-4
NAN = float('nan')
POISON = [1e30, float('inf'), -float('inf'), NAN]


@functools.lru_cache(maxsize=None)
def _inputs(shape, ignore_frac, seed=0, kind='blocks'):
    """float32 logits (inf / NaN at the ignored pixels), uint8 labels [B,H,W] (255 = ignored), shared: never modified.  Labels come in
    8 x 8 blocks, so the distances reach tens of pixels; image 0 of 'degenerate' lacks class 1 and its image 1 is all class 1."""
    B, C, H, W = shape
    r = np.random.default_rng(seed + H)
    logits = (3.0 * r.standard_normal(shape)).astype(np.float32)
    k = 8 if min(H, W) >= 16 else 2                        # (2 x 2 blocks on the smallest shape, so that it has contours too)
    small = r.integers(0, C, (B, (H + k - 1) // k, (W + k - 1) // k))
    labels = np.repeat(np.repeat(small, k, axis=1), k, axis=2)[:, :H, :W].astype(np.uint8)
    if kind == 'degenerate':
        labels[0][labels[0] == 1] = 0
        labels[1][:] = 1
    if kind == 'no_valid':
        labels[:] = 255
    if ignore_frac:
        m = r.random((B, H, W)) < ignore_frac
        labels[m] = 255
    ign = labels == 255
    idx = np.nonzero(np.broadcast_to(ign[:, None], shape))
    logits[idx] = np.array(POISON, np.float32)[np.arange(idx[0].size) % 4]
    return torch.from_numpy(logits), torch.from_numpy(labels)


def _run(lg_d, lb_d, ignore, classes='foreground', max_dist=None, weight=1.0, accumulate=0, loss=None, dl=None, want_dl=True, want_phi=True,
         ws=None):
    B, C, H, W = lg_d.shape
    if ws is None:
        ws = guard.alloc_bytes(_lib.load().bdn_boundary_workspace_bytes(B, C, H, W), label='boundary workspace')
    loss = guard.full((1,), NAN) if loss is None else loss
    term = guard.full((1,), NAN)
    if dl is None and want_dl:
        dl = guard.full(tuple(lg_d.shape), NAN)
    phi = guard.full((C, B * H * W), NAN) if want_phi else None
    _lib.call('bdn_boundary_loss', lg_d.data_ptr(), lb_d.data_ptr(), -1 if ignore is None else ignore, int(classes == 'all'), max_dist or 0.0,
              weight, accumulate, ws.data_ptr(), loss.data_ptr(), term.data_ptr(), _lib.ptr(dl), _lib.ptr(phi), B, C, H, W, st())
    return loss, term, dl, phi


def _check(shape, logits, labels, ignore, classes, max_dist, out, what, weight=1.0):
    loss, term, dl, phi = out
    B, C, H, W = shape
    t64, g64, phi_ref = ER.boundary_loss_ref(logits.numpy(), labels.numpy(), ignore, classes == 'all', max_dist)
    assert np.array_equal(phi.cpu().numpy().reshape(C, B, H, W), phi_ref), (what, 'phi differs')
    e_term, tb = abs(term.item() - t64), TERM_TOL * max(1.0, abs(t64))
    gmax = float(np.abs(g64).max())
    e_grad = float(np.abs(dl.cpu().double().numpy() - weight * g64).max())
    print(f'{what}: |term err| {e_term:.3e} (bound {tb:.3e}; term {t64:.6f}; max|phi| {np.abs(phi_ref).max():.2f})  max|dlogits err| {e_grad:.3e} '
          f'(bound {GRAD_TOL * weight * gmax:.3e})')
    assert e_term <= tb, (what, term.item(), t64)
    assert e_grad <= GRAD_TOL * weight * gmax, (what, e_grad, gmax)
    assert loss.item() == np.float32(weight) * np.float32(term.item()), (what, 'loss != weight * term')
    ign = (labels == 255) if ignore is not None else torch.zeros_like(labels, dtype=torch.bool)
    assert (dl.cpu()[ign[:, None].expand(shape)] == 0).all(), (what, 'gradient not exactly 0 at ignored pixels')
    assert torch.isfinite(dl).all() and torch.isfinite(term).all()


@pytest.mark.parametrize('ignore_frac', [0.0, 0.3])
@pytest.mark.parametrize('max_dist', [None, 3])
@pytest.mark.parametrize('classes', ['foreground', 'all'])
@pytest.mark.parametrize('shape', SHAPES)
@guarded
def test_boundary_loss_against_float64(shape, classes, max_dist, ignore_frac):
    logits, labels = _inputs(shape, ignore_frac)
    ignore = 255 if ignore_frac else None
    out = _run(dev(logits), dev(labels, torch.uint8), ignore, classes, max_dist, weight=0.5)
    _check(shape, logits, labels, ignore, classes, max_dist, out, f'{shape} {classes} max_dist={max_dist} ignore={ignore_frac}', weight=0.5)
    assert out[3].any() and out[2].any() and out[1].item() != 0.0


@pytest.mark.parametrize('classes', ['foreground', 'all'])
@guarded
def test_degenerate_images(classes):
    """An image where class 1 is absent and one it fills: phi of that class is 0 over the image."""
    shape = (2, 2, 33, 65)
    for frac in (0.0, 0.3):
        logits, labels = _inputs(shape, frac, kind='degenerate')
        ignore = 255 if frac else None
        out = _run(dev(logits), dev(labels, torch.uint8), ignore, classes)
        _check(shape, logits, labels, ignore, classes, None, out, f'degenerate {classes} ignore={frac}')
        assert not out[3].view(2, 2, -1)[1].any()           # class 1: absent from image 0, everywhere in image 1
        assert out[1].item() == 0.0 and not out[2].any()


@guarded
def test_batch_without_a_valid_pixel():
    shape = (2, 2, 5, 7)
    logits, labels = _inputs(shape, 0.0, kind='no_valid')
    loss, term, dl, phi = _run(dev(logits), dev(labels, torch.uint8), 255, 'all')
    assert term.item() == 0.0 and loss.item() == 0.0 and not dl.any() and not phi.any()


@pytest.mark.parametrize('shape', [(2, 3, 33, 65), (3, 2, 128, 128)])
@guarded
def test_same_bits_from_any_workspace_and_without_optional_outputs(shape):
    logits, labels = _inputs(shape, 0.3)
    lg_d, lb_d = dev(logits), dev(labels, torch.uint8)
    nbytes = _lib.load().bdn_boundary_workspace_bytes(*shape)
    outs = []
    for fill in (0xFF, 0x00, 0x5A):
        ws = guard.alloc_bytes(nbytes, label='boundary workspace').fill_(fill)
        outs.append(_run(lg_d, lb_d, 255, 'all', ws=ws))
    for o in outs[1:]:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(o, outs[0]))
    lean = _run(lg_d, lb_d, 255, 'all', want_dl=False, want_phi=False)
    assert torch.equal(lean[0], outs[0][0]) and torch.equal(lean[1], outs[0][1]) and lean[2] is None


@guarded
def test_accumulate_adds_one_rounded_product():
    shape = (2, 3, 33, 65)
    logits, labels = _inputs(shape, 0.3)
    lg_d, lb_d = dev(logits), dev(labels, torch.uint8)
    w = 0.37
    alone = _run(lg_d, lb_d, 255, 'all', weight=w)
    base_loss = guard.full((1,), 1.25)
    base_dl = guard.guard(torch.from_numpy(np.random.default_rng(2).standard_normal(shape).astype(np.float32)))
    keep = base_dl.clone()
    acc = _run(lg_d, lb_d, 255, 'all', weight=w, accumulate=1, loss=base_loss, dl=base_dl)
    assert acc[0].item() == np.float32(1.25) + np.float32(w) * np.float32(alone[1].item())
    assert torch.equal(acc[2], keep + alone[2])             # ignored pixels: + 0, untouched
    ign = (labels == 255)[:, None].expand(shape)
    assert torch.equal(acc[2].cpu()[ign], keep.cpu()[ign])


BASES = [dict(w_overlap=1.0, w_focal=0.5, gamma=2.0), dict(w_overlap=1.0, w_focal=0.5, gamma=2.0, ignore_index=255),
         dict(w_overlap=1.0, w_focal=0.5, gamma=2.0, ignore_index=255, topk=0.25), dict(w_overlap=0.0, w_focal=1.0, ignore_index=255, w_lovasz=0.5),
         dict(w_overlap=0.0, w_focal=0.0, ignore_index=255, w_lovasz=1.0)]


@pytest.mark.parametrize('base', range(len(BASES) + 1))
def test_composition_through_the_criterion(base):
    """Behind bdn_criterion, _masked, _topk, after bdn_lovasz_softmax, after the Lovasz term alone, and alone (base 5): loss == base +
    weight * term to one float32 rounding, dlogits == base + the term's own float32 gradient, exactly."""
    shape = (2, 2, 33, 65)
    kw = BASES[base] if base < len(BASES) else None
    masked = kw is None or 'ignore_index' in kw
    logits, labels = _inputs(shape, 0.3 if masked else 0.0)
    lg_d, lb_d = logits.cuda(), labels.cuda()
    w = 0.25
    bnd = dict(w_boundary=w, boundary_classes='all', boundary_max_dist=5)
    if kw is None:
        c = Criterion(w_overlap=0.0, ignore_index=255, **bnd)
        loss, terms, counts, dl = c.evaluate(lg_d, lb_d)
        ref = Criterion(ignore_index=255).evaluate(lg_d, lb_d, want_grad=False)
        assert torch.equal(counts, ref[2]) and terms.numel() == 3 and terms[0].item() == 0.0 and terms[1].item() == 0.0
        base_loss, base_dl, base_terms = torch.zeros((), device='cuda'), torch.zeros_like(dl), terms[:2]
    else:
        c = Criterion(**kw, **bnd)
        loss, terms, counts, dl = c.evaluate(lg_d, lb_d)
        base_loss, base_terms, base_counts, base_dl = Criterion(**kw).evaluate(lg_d, lb_d)
        assert torch.equal(counts, base_counts) and terms.numel() == base_terms.numel() + 1
    assert torch.equal(terms[:-1], base_terms)
    phi = torch.empty(2 * 2 * 33 * 65, dtype=torch.float32, device='cuda')
    alone = Criterion(w_overlap=0.0, ignore_index=255 if masked else None, **bnd).evaluate(lg_d, lb_d, phi=phi)
    assert terms[-1].item() == alone[1][-1].item()
    assert loss.item() == (base_loss.cpu() + torch.tensor(np.float32(w)) * alone[1][-1].cpu()).item()
    assert torch.equal(dl, base_dl + alone[3])
    t64, g64, phi_ref = ER.boundary_loss_ref(logits.numpy(), labels.numpy(), 255 if masked else None, True, 5)
    assert np.array_equal(phi.cpu().numpy().reshape(2, 2, 33, 65), phi_ref)
    assert abs(terms[-1].item() - t64) <= TERM_TOL * max(1.0, abs(t64))


def test_weight_is_read_per_call():
    shape = (2, 2, 33, 65)
    logits, labels = _inputs(shape, 0.0)
    lg_d, lb_d = logits.cuda(), labels.cuda()
    c = Criterion(w_focal=1.0, gamma=0.0, w_boundary=0.1)
    out = c.buffers(shape, lg_d.device)
    a = [t.clone() if t is not None else None for t in c.evaluate(lg_d, lb_d, out=out)]
    c.w_boundary = 0.3
    b = c.evaluate(lg_d, lb_d, out=out)
    fresh = Criterion(w_focal=1.0, gamma=0.0, w_boundary=0.3).evaluate(lg_d, lb_d)
    assert torch.equal(b[0], fresh[0]) and torch.equal(b[3], fresh[3]) and torch.equal(b[1], fresh[1])
    assert not torch.equal(a[0], b[0]) and a[1][-1].item() == b[1][-1].item()
