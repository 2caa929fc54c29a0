"""No GPU: the restatement of clipping and accumulation (tests/grad_clip_ref.py) against CPU torch, the float32 coefficient formula bit
for bit, the argument validation of the new entry points (errors are returned before anything touches a device), and the TrainStep /
fabric_amd.optim argument errors that need no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.optim import FROZEN, check_accumulate, check_max_grad_norm
from tests import grad_clip_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['bdn_sgd_step_grouped_ex', 'bdn_sgd_momentum_step_grouped_ex', 'bdn_adam_step_grouped_ex', 'bdn_grad_accumulate', 'bdn_grad_norm']
_hf = ctypes.POINTER(ctypes.c_float)
_CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'const uint32_t*': ctypes.c_void_p, 'const int32_t*': ctypes.c_void_p,
           'void*': ctypes.c_void_p, 'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
           'long long': ctypes.c_int64}


# ---------------------------------------------------------------- the restatement against CPU torch
@pytest.mark.parametrize('max_norm', [0.05, 1.0, 1e6])
def test_restatement_matches_cpu_clip_grad_norm(max_norm):
    """float64 clones of parameters of odd sizes, one of them without a gradient: norm and scaled gradients to 1e-12 relative."""
    gen = torch.Generator().manual_seed(7)
    shapes = [(3, 5), (17,), (4, 4, 3), (1,), (129,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    grads = [torch.randn(s, generator=gen, dtype=torch.float64) * (0.1 + i) for i, s in enumerate(shapes)]
    for i, (p, g) in enumerate(zip(ps, grads)):
        p.grad = None if i == 2 else g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    have = [g for i, g in enumerate(grads) if i != 2]
    rn, rg = G.clipped(have, max_norm)
    assert abs(float(total) - rn) <= 1e-12 * rn
    for p, r in zip([p for i, p in enumerate(ps) if i != 2], rg):
        assert float((p.grad - r).abs().max()) <= 1e-12 * float(r.abs().max())
    assert ps[2].grad is None
    # the flat form with a segment table: the frozen segment (NaN-filled) is left out
    flat, segs, off = [], [], 0
    for i, g in enumerate(grads):
        v = g.reshape(-1) if i != 2 else torch.full((g.numel(),), float('nan'), dtype=torch.float64)
        flat.append(v)
        segs.append((off, off + v.numel(), FROZEN if i == 2 else i % 2))
        off += v.numel()
    assert abs(G.norm(torch.cat(flat), segs) - rn) <= 1e-12 * rn
    assert abs(G.norm(torch.cat(flat), segs, 0.25) - 0.25 * rn) <= 1e-12 * rn
    assert math.isnan(G.norm(torch.cat(flat)))


@pytest.mark.parametrize('norm', [0.0, 1e-30, 3.7e-7, 0.999999, 1.0, 1.0000001, 2.5, 123456.78, 3e38, float('inf'), float('nan')])
@pytest.mark.parametrize('max_norm', [1e-3, 1.0, 7.25, float('inf')])
def test_float32_coefficient_formula_is_torchs_bit_for_bit(norm, max_norm):
    n32 = torch.tensor(norm, dtype=torch.float32)
    want = torch.clamp(max_norm / (n32 + 1e-6), max=1.0)
    got = G.coef32(np.float32(norm), max_norm)
    assert got.dtype == np.float32
    if math.isnan(float(want)):
        assert math.isnan(float(got))
    else:
        assert np.float32(want.item()).tobytes() == got.tobytes(), (float(want), float(got))
    if math.isnan(norm):
        assert math.isnan(float(got)), 'a NaN norm must give a NaN coefficient'
    elif max_norm == float('inf') and math.isfinite(norm):
        assert float(got) == 1.0


def test_accumulation_order_is_the_documented_one():
    gen = torch.Generator().manual_seed(3)
    gs = [torch.randn(1000, generator=gen) * 10.0 ** (3 * i) for i in range(4)]
    assert torch.equal(G.accumulated(gs[:1]), gs[0])
    assert torch.equal(G.accumulated(gs[:2]), gs[1] + gs[0])
    assert torch.equal(G.accumulated(gs[:3]), gs[2] + (gs[0] + gs[1]))
    assert torch.equal(G.accumulated(gs), gs[3] + ((gs[0] + gs[1]) + gs[2]))
    assert not torch.equal(G.accumulated(gs), ((gs[3] + gs[2]) + gs[1]) + gs[0]), 'the data does not tell the orders apart'


# ---------------------------------------------------------------- the C ABI
@pytest.mark.parametrize('name', NEW)
def test_header_declaration_matches_signature_row(name):
    """Host float arrays of the new signatures are POINTER(c_float) rows (tests/guard.py takes every c_void_p for a device pointer)."""
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())) for p in m.group(1).split(',')]
    want = [_hf if p.rsplit(' ', 1)[1] in ('lr', 'weight_decay') else _CTYPES[p.rsplit(' ', 1)[0].strip()] for p in params]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and want == list(args), (params, args)
    assert args[-1] is ctypes.c_void_p and params[-1] == 'void* stream', 'the stream stays the last argument'
    assert _lib.SIGNATURES['bdn_grad_norm_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_size_t])


def test_workspace_bytes_is_a_function_of_n_alone():
    lib = _lib.load()
    w = lib.bdn_grad_norm_workspace_bytes
    assert w(0) == 16 and w(4) == 16 and w(16384) == 16 and w(16384 * 2) == 16 and w(16384 * 2 + 4) == 32
    assert w(13_401_156) == (math.ceil(13_401_156 / 16384) * 8 + 15) // 16 * 16


def test_argument_errors_return_before_touching_a_device():
    lib = _lib.load()
    err = lambda: lib.bdn_last_error()                     # noqa: E731
    acc = lib.bdn_grad_accumulate
    assert acc(None, 16, 4, 0, None) != 0 and b'null' in err()
    assert acc(16, None, 4, 1, None) != 0 and b'null' in err()
    assert acc(16, 20, 4, 0, None) != 0 and b'aligned' in err()
    assert acc(24, 16, 4, 0, None) != 0 and b'aligned' in err()
    assert acc(16, 16, 4, 2, None) != 0 and b'add' in err()
    assert acc(16, 32, 0, 1, None) == 0                                        # n == 0 launches nothing
    norm = lib.bdn_grad_norm
    ok = (16, 16, 16, 1, 1.0, 1.0, 16, 16, 16, None)

    def bad(i, v):
        a = list(ok)
        a[i] = v
        return norm(*a)
    assert bad(0, None) != 0 and b'null' in err()
    assert bad(6, None) != 0 and b'null' in err()
    assert bad(7, None) != 0 and b'null' in err()
    assert bad(1, None) != 0 and b'null' in err()                              # a table is announced (n_seg = 1) but not given
    assert bad(2, None) != 0 and b'null' in err()
    assert bad(0, 24) != 0 and b'aligned' in err()
    assert bad(6, 20) != 0 and b'aligned' in err()
    assert bad(7, 18) != 0 and b'aligned' in err()
    assert bad(1, 18) != 0 and b'aligned' in err()
    assert bad(8, 18) != 0 and b'multiple of 4' in err()
    assert bad(3, -1) != 0 and b'segments' in err()
    assert bad(3, 257) != 0 and b'segments' in err()
    assert bad(5, -1.0) != 0 and b'max_norm' in err()
    assert bad(5, float('nan')) != 0 and b'max_norm' in err()
    one, wd, nine = _lib.floats([1e-3]), _lib.floats([0.0]), _lib.floats([1e-3] * 9)
    sgd, sgdm, adam = lib.bdn_sgd_step_grouped_ex, lib.bdn_sgd_momentum_step_grouped_ex, lib.bdn_adam_step_grouped_ex
    assert sgd(16, 16, 16, 16, 1, 1, one, 1.0, None, 16, None) != 0 and b'dev_scale' in err()
    assert sgd(16, 16, 16, 16, 1, 1, one, 1.0, 18, 16, None) != 0 and b'aligned' in err()
    assert sgd(None, 16, 16, 16, 1, 1, one, 1.0, 16, 16, None) != 0 and b'null' in err()
    assert sgd(16, 24, 16, 16, 1, 1, one, 1.0, 16, 16, None) != 0 and b'aligned' in err()
    assert sgd(16, 16, 16, 16, 1, 9, nine, 1.0, 16, 16, None) != 0 and b'9 groups' in err()
    assert sgd(16, 16, 16, 16, 0, 1, one, 1.0, 16, 16, None) != 0 and b'segments' in err()
    assert sgd(16, 16, 16, 16, 257, 1, one, 1.0, 16, 16, None) != 0 and b'segments' in err()
    assert sgd(16, 16, 16, 16, 1, 1, one, 1.0, 16, 18, None) != 0 and b'multiple of 4' in err()
    assert sgd(16, 16, 16, 16, 1, 1, one, 1.0, 16, 0, None) == 0
    mt = (0.9, 0.0, 0, 1)
    assert sgdm(16, 16, 32, 16, 16, 1, 1, one, wd, 1.0, None, *mt, 16, None) != 0 and b'dev_scale' in err()
    assert sgdm(16, 16, 32, 16, 16, 1, 9, nine, nine, 1.0, 16, *mt, 16, None) != 0 and b'9 groups' in err()
    assert sgdm(16, 16, None, 16, 16, 1, 1, one, wd, 1.0, 16, *mt, 16, None) != 0 and b'momentum_buf' in err()
    assert sgdm(16, 16, 36, 16, 16, 1, 1, one, wd, 1.0, 16, *mt, 16, None) != 0 and b'aligned' in err()
    assert sgdm(16, 16, 32, 16, 16, 1, 1, one, wd, 1.0, 16, 0.9, 0.1, 1, 1, 16, None) != 0 and b'nesterov' in err()
    assert sgdm(16, 16, 32, 16, 16, 1, 1, one, wd, 1.0, 16, *mt, 18, None) != 0 and b'multiple of 4' in err()
    assert sgdm(16, 16, 32, 16, 16, 300, 1, one, wd, 1.0, 16, *mt, 16, None) != 0 and b'segments' in err()
    at = (0.9, 0.999, 1e-8, 0, 1)
    assert adam(16, 16, 16, 16, 16, 16, 1, 1, one, wd, 1.0, None, *at, 16, None) != 0 and b'dev_scale' in err()
    assert adam(16, 16, 16, 16, 16, 16, 1, 1, one, wd, 1.0, 17, *at, 16, None) != 0 and b'aligned' in err()
    assert adam(16, 16, None, 16, 16, 16, 1, 1, one, wd, 1.0, 16, *at, 16, None) != 0 and b'null' in err()
    assert adam(16, 16, 16, 20, 16, 16, 1, 1, one, wd, 1.0, 16, *at, 16, None) != 0 and b'aligned' in err()
    assert adam(16, 16, 16, 16, 16, 16, 1, 9, nine, nine, 1.0, 16, *at, 16, None) != 0 and b'9 groups' in err()
    assert adam(16, 16, 16, 16, 16, 16, -1, 1, one, wd, 1.0, 16, *at, 16, None) != 0 and b'segments' in err()
    assert adam(16, 16, 16, 16, 16, 16, 1, 1, one, wd, 1.0, 16, 0.9, 0.999, 1e-8, 0, 0, 16, None) != 0 and b'step' in err()
    assert adam(16, 16, 16, 16, 16, 16, 1, 1, one, wd, 1.0, 16, *at, 18, None) != 0 and b'multiple of 4' in err()
    assert adam(16, 16, 16, 16, 16, 16, 1, 1, one, wd, 1.0, 16, *at, 0, None) == 0


# ---------------------------------------------------------------- Python-side argument errors
def test_accumulate_and_max_grad_norm_are_validated_without_a_device():
    for k in (0, -1, 2.0, 1.5, '2', None, True):
        with pytest.raises(ValueError, match='accumulate'):
            check_accumulate(k)
    assert check_accumulate(1) == 1 and check_accumulate(7) == 7
    for x in (0, 0.0, -1.0, float('nan'), float('-inf'), '1', True):
        with pytest.raises(ValueError, match='max_grad_norm'):
            check_max_grad_norm(x)
    assert check_max_grad_norm(None) is None and check_max_grad_norm(2) == 2.0 and check_max_grad_norm(float('inf')) == float('inf')
    from fabric_amd.train_step import TrainStep
    model = torch.nn.Linear(2, 2)                            # on the CPU: the argument errors come before the device is looked at
    for kw in (dict(accumulate=0), dict(accumulate=2.0), dict(max_grad_norm=0.0), dict(max_grad_norm=-3.0), dict(max_grad_norm=float('nan'))):
        with pytest.raises(ValueError):
            TrainStep(model, **kw)
    with pytest.raises(RuntimeError, match='ROCm device'):
        TrainStep(model, accumulate=2, max_grad_norm=1.0)
