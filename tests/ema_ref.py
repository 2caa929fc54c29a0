"""float64 restatement of the averaging rule of the fused step (include/bidate_hip.h bdn_ema_update: torch's lerp element formula, as
torch.optim.swa_utils.AveragedModel applies it through torch._foreach_lerp_), shared by tests/test_ema_cpu.py (which pins it against CPU
AveragedModel) and tests/test_gpu_ema.py / tests/test_gpu_step_ema.py (which hold the HIP kernels and the step to it).

As in tests/optim_ref.py the rule returns the value AND a magnitude: the same expression on the absolute values of its inputs with every
subtraction turned into an addition.  A float32 evaluation, in any order and with or without fused multiply-adds, differs from the exact
value by a small multiple of float32's epsilon times that magnitude.  ULPS is that multiple: the longest chain (subtract, 1 - w, multiply,
subtract) rounds four times; the rest is headroom for contraction differences.  The weight is the float32 the kernel receives, widened
to double.
"""
import numpy as np
import torch

from tests.optim_ref import EPS32, check as _check

ULPS = 6


def weight32(w):
    """The double `w` as the kernels see it: rounded to float32, widened back."""
    return float(np.float32(w))


def lerp(avg, p, w):
    """-> (avg', |avg'|-magnitude) of avg' = lerp(avg, p, w): w < 0.5: avg + w (p - avg), otherwise p - (p - avg)(1 - w)."""
    w = weight32(w)
    a, q = avg.double(), p.double()
    if w < 0.5:
        return a + w * (q - a), a.abs() + w * (q.abs() + a.abs())
    return q - (q - a) * (1.0 - w), q.abs() + (1.0 - w) * (q.abs() + a.abs())


def ema_weight(decay):
    return 1.0 - decay


def swa_weight(n_averaged):
    return 1.0 / (n_averaged + 1)


def check(got, ref, mag, what, ulps=ULPS):
    _check(got, ref, mag, what, ulps=ulps)
