"""Float64 twin of bdn_sam_perturb / bdn_sam_restore (include/bidate_hip.h) over a list of tensors, pinned against torch autograd in
tests/test_sam_cpu.py.

SAM (Foret et al., ICLR 2021, eq. 2 with p = 2): e = rho * g / ||g||.  ASAM (Kwon et al., ICML 2021, eq. 6 with T_w = |w|):
e = rho * T_w^2 g / ||T_w g||.  One formula with t = 1 or |w|:

    e = rho * t^2 * g / (||t * g|| + eps),

the norm over every element of every tensor that is not frozen.  A frozen tensor has no perturbation and is not in the norm.  The update
that follows takes the gradient at w + e and applies it at w: restore() gives w back as the saved tensors themselves -- a copy, because
(w + e) - e is not w in floating point.  Importable without a device."""
import math

import torch

EPS32 = 2.0 ** -24          # half an ulp of float32, relative


def norm(params, grads, adaptive=False, frozen=()):
    """||t * g|| in float64 over the tensors whose index is not in `frozen`."""
    s = 0.0
    for i, (w, g) in enumerate(zip(params, grads)):
        if i in frozen:
            continue
        x = g.double() * (w.double().abs() if adaptive else 1.0)
        s += float((x * x).sum())
    return math.sqrt(s)


def perturb(params, grads, rho, adaptive=False, eps=1e-12, frozen=()):
    """(perturbed, e, saved, norm): float64 lists over the tensors.  saved[i] is params[i] itself (not a copy); a frozen tensor has
    e = 0 and perturbed[i] = params[i] in float64."""
    nrm = norm(params, grads, adaptive, frozen)
    scale = rho / (nrm + eps)
    out, es = [], []
    for i, (w, g) in enumerate(zip(params, grads)):
        w64 = w.double()
        if i in frozen:
            e = torch.zeros_like(w64)
        else:
            t2 = w64 * w64 if adaptive else 1.0
            e = scale * t2 * g.double()
        es.append(e)
        out.append(w64 + e)
    return out, es, list(params), nrm


def restore(saved):
    """The parameters after the restore: the saved tensors, bit for bit."""
    return [s.clone() for s in saved]


def check_perturb(params, grads, got_params, got_norm, rho, adaptive, eps=1e-12, frozen=(), what=''):
    """The kernel's float32 results against the twin, with the bounds of its arithmetic: the reported norm is one rounding of a double sum,
    |norm - ref| <= 2^-23 ref; an element carries six float32 roundings in e (norm, norm + eps, the quotient, two products by t, the
    product by g) and one in the sum, |w' - (w + e)| <= 2^-24 (8 |e| + |w + e|), with one rounding to spare.  Frozen tensors keep
    their bits.  Prints nothing; asserts."""
    ref, es, _, nrm = perturb(params, grads, rho, adaptive, eps, frozen)
    assert abs(float(got_norm) - nrm) <= 2.0 ** -23 * nrm, f'{what}: norm {float(got_norm)!r} against {nrm!r}'
    for i, (w, r, e, got) in enumerate(zip(params, ref, es, got_params)):
        if i in frozen:
            assert torch.equal(got.view(torch.int32), w.view(torch.int32)), f'{what}: frozen tensor {i} changed'
            continue
        err = (got.double() - r).abs()
        tol = EPS32 * (8.0 * e.abs() + r.abs())
        bad = err > tol
        assert not bool(bad.any()), f'{what}: tensor {i}: worst error / bound {float((err / tol.clamp_min(1e-300)).max()):.2f}'
    return nrm
