"""float64 restatement of the fused step's gradient clipping and accumulation (torch.nn.utils.clip_grad_norm_, include/bidate_hip.h
bdn_grad_norm / bdn_grad_accumulate), shared by tests/test_grad_clip_cpu.py (which pins it against CPU torch) and the GPU tests.

The norm is over the COUNTED elements only: with a segment table [(start, stop, group id)] in elements, the segments whose id is FROZEN
are left out, as torch leaves out a parameter without a gradient.  The coefficient is torch's formula evaluated in float32 from the
float32 norm, since that is what torch computes on float32 gradients: clamp(max_norm / (norm + 1e-6), max = 1.0), where torch evaluates
a Python float divided by a tensor as reciprocal(tensor) * float (Tensor.__rtruediv__): two float32 roundings, not one.
"""
import numpy as np
import torch

from fabric_amd.optim import FROZEN

EPS32 = float(torch.finfo(torch.float32).eps)


def counted(g, segs=None):
    """The counted elements of the flat gradient `g` as one float64 tensor (segs None: all of it)."""
    g = g.detach().double().cpu().reshape(-1)
    if segs is None:
        return g
    keep = [g[a:b] for a, b, gid in segs if gid != FROZEN]
    return torch.cat(keep) if keep else g[:0]


def norm(g, segs=None, grad_scale=1.0):
    """grad_scale * sqrt(sum g^2) over the counted elements, in float64 (a Python float)."""
    v = counted(g, segs)
    return float(grad_scale) * float(torch.sqrt((v * v).sum()))


def coef32(norm32, max_norm):
    """torch's clip coefficient in float32 arithmetic from a float32 norm: min(max_norm / (norm + 1e-6), 1) with the quotient formed as
    torch forms it, (1 / (norm + 1e-6)) * max_norm; NaN kept (np.float32)."""
    with np.errstate(all='ignore'):
        c = (np.float32(1.0) / (np.float32(norm32) + np.float32(1e-6))) * np.float32(max_norm)
    return c if np.isnan(c) or c <= np.float32(1.0) else np.float32(1.0)


def clipped(grads, max_norm):
    """clip_grad_norm_ restated in float64 on a list of gradient tensors: (total norm, [scaled gradients]); the coefficient in float64."""
    gs = [g.double() for g in grads]
    total = float(torch.sqrt(sum((g * g).sum() for g in gs)))
    c = min(max_norm / (total + 1e-6), 1.0)
    return total, [g * c for g in gs]


def accumulated(gs):
    """The accumulator's fixed order in float32: acc = g1; acc += g (2..K-1); result = gK + acc.  One micro-batch: g1 itself."""
    gs = [g.float() for g in gs]
    if len(gs) == 1:
        return gs[0].clone()
    acc = gs[0].clone()
    for g in gs[1:-1]:
        acc = acc + g
    return gs[-1] + acc
