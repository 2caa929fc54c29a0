"""float64 restatement of the fused step's update rules (torch 2.10 _single_tensor_sgd / _single_tensor_adam, include/bidate_hip.h
bdn_sgd_momentum_step / bdn_adam_step), shared by tests/test_optim_cpu.py (which pins it against CPU torch.optim) and
tests/test_gpu_optim.py (which holds the HIP kernels to it).

Every rule returns the new parameters and state AND a magnitude for each output: the same expression evaluated on the absolute values of
its inputs (every subtraction turned into an addition).  A float32 evaluation of the expression, in any order and with or without fused
multiply-adds, differs from the exact value by a small multiple of float32's epsilon times that magnitude; for the parameters the magnitude
is at least max(|p|, |dp|).  ULPS is that multiple: the longest chain (Nesterov SGD with weight decay, Adam's m / (sqrt(v)/sqrt(bc2) + eps))
rounds fewer than eight times per element.
"""
import math

import torch

EPS32 = float(torch.finfo(torch.float32).eps)
ULPS = 8


def sgd(p, g, buf, lr, grad_scale=1.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=True):
    """-> (p, buf, |p|-magnitude, |buf|-magnitude); buf may be None when momentum == 0."""
    p, g = p.double(), g.double() * grad_scale
    gm = g.abs()
    if weight_decay:
        g, gm = g + weight_decay * p, gm + weight_decay * p.abs()
    bm = None
    if momentum:
        if first:
            buf, bm = g.clone(), gm.clone()
        else:
            buf, bm = momentum * buf.double() + (1 - dampening) * g, momentum * buf.double().abs() + (1 - dampening) * gm
        if nesterov:
            g, gm = g + momentum * buf, gm + momentum * bm
        else:
            g, gm = buf, bm
    return p - lr * g, buf, p.abs() + lr * gm, bm


def adam(p, g, m, v, step, lr, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
    """-> (p, m, v, |p|-magnitude, |m|-magnitude, |v|-magnitude); step is 1-based (after the increment)."""
    b1, b2 = betas
    p, g, m, v = p.double(), g.double() * grad_scale, m.double(), v.double()
    gm = g.abs()
    pm = p.abs()
    if weight_decay:
        if decoupled:
            p, pm = p * (1 - lr * weight_decay), pm * (1 - lr * weight_decay)
        else:
            g, gm = g + weight_decay * p, gm + weight_decay * p.abs()
    m_new = m + (1 - b1) * (g - m)
    mm = b1 * m.abs() + (1 - b1) * gm
    v_new = b2 * v + (1 - b2) * g * g
    vm = b2 * v.abs() + (1 - b2) * gm * gm
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    den = v_new.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m_new / den, m_new, v_new, pm + (lr / bc1) * mm / den, mm, vm


def check(got, ref, mag, what, ulps=ULPS):
    """Every element of float32 `got` within ulps * EPS32 * mag of float64 `ref` (plus the float32 subnormal floor)."""
    got = got.detach().double().cpu()
    ref, mag = ref.double().cpu(), mag.double().cpu()
    err = (got - ref).abs()
    tol = ulps * EPS32 * mag + 1e-38
    bad = err > tol
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {got.numel()} elements off; worst error / bound '
                                 f'{float((err / tol).max()):.2f} at {int((err / tol).argmax())}')
