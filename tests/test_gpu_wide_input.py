"""-m gpu: the entry points in front of and around the first layer at 17 to 64 bands (padded to Cpad = 32, 48, 64 channels), on
guard-banded buffers.  Every other test of them runs at Cpad = 16.

  bdn_pack_input        bf16, fp32 and the bf16x3 split form: real channels = the float32 image rounded once to the stored type (split
                        form: hi and lo as tests/forced_ref.hi_lo defines them), padded channels exact zeros, date 1 first
  bdn_gather_tiles(_sym)  bit-equal to indexing the scene on the host, padded channels exact zeros
  refusals              bdn_conv3x3_wgrad_bnbwd(_supported) above 16 padded channels and bdn_conv3x3_dgrad_first above 16 real ones return
                        BDN_E_SHAPE (-2) before any launch: the NaN-filled outputs and the 0xFF-filled scratch are left as they were
(C, Cpad) = (17, 32), (33, 48), (50, 64), (64, 64): one channel into a new 16-channel granule, a ragged last 16-byte unit in bf16 (33,
50: not multiples of 8) and in fp32 (not multiples of 4), and no padding at all.
"""
import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X2, BDN_BF16X3
from fabric_amd.utils import inference as inf
from fabric_amd.utils.dataloaders import _apply_symmetry
from tests import forced_ref as R
from tests import guard
from tests.guard import guarded
from tests.gpu_util import DT, st

pytestmark = pytest.mark.gpu
PAIRS = [(17, 32), (33, 48), (50, 64), (64, 64)]
NAN = float('nan')
E_SHAPE = r'rc=-2\)'


def _images(B, C, H, W, seed):
    """Two float32 image batches whose values need all 24 significand bits (so that bf16 rounds and the lo half is not zero)."""
    r = np.random.default_rng(seed)
    return tuple(torch.from_numpy((r.standard_normal((B, C, H, W)) * r.choice([1e-3, 1.0, 300.0], (1, C, 1, 1))).astype(np.float32))
                 for _ in range(2))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------- bdn_pack_input
@pytest.mark.parametrize('shape', [(2, 9, 21), (3, 16, 16)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('C,Cpad', PAIRS)
@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
@guarded
def test_pack_input(prec, C, Cpad, shape):
    B, H, W = shape
    dt, td = DT[prec]
    x1, x2 = _images(B, C, H, W, C + H)
    g1, g2 = guard.guard(x1), guard.guard(x2)
    out = guard.full((2 * B, H, W, Cpad), NAN, dtype=td)
    _lib.call('bdn_pack_input', dt, g1.data_ptr(), g2.data_ptr(), out.data_ptr(), B, C, H, W, Cpad, st())
    torch.cuda.synchronize()
    got = out.cpu()
    want = torch.cat([x1, x2]).permute(0, 2, 3, 1).to(td)                 # one rounding of the float32 value; date 1 first
    assert torch.equal(_bits(got[..., :C]), _bits(want))
    assert Cpad == C or bool((_bits(got[..., C:]) == 0).all())            # exact (positive) zeros
    assert not torch.equal(got[:B, ..., :C], got[B:, ..., :C])


@pytest.mark.parametrize('shape', [(2, 9, 21), (3, 16, 16)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('C,Cpad', PAIRS)
@guarded
def test_pack_input_split_form(C, Cpad, shape):
    """BDN_BF16X3: [2B, H, W, 2 Cpad] bf16 = hi | lo, hi = bf16(x), lo = bf16(x - hi)."""
    B, H, W = shape
    x1, x2 = _images(B, C, H, W, C + W)
    g1, g2 = guard.guard(x1), guard.guard(x2)
    out = guard.full((2 * B, H, W, 2 * Cpad), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_pack_input', BDN_BF16X3, g1.data_ptr(), g2.data_ptr(), out.data_ptr(), B, C, H, W, Cpad, st())
    torch.cuda.synchronize()
    got = out.cpu()
    hi, lo = R.hi_lo(torch.cat([x1, x2]).permute(0, 2, 3, 1))
    assert torch.equal(_bits(got[..., :C]), _bits(hi.to(torch.bfloat16)))
    assert torch.equal(got[..., Cpad:Cpad + C].float() + 0.0, lo + 0.0)   # + 0.0: the sign of a zero lo half is not compared
    assert bool((lo != 0).any())
    for pad in (got[..., C:Cpad], got[..., Cpad + C:]):
        assert pad.numel() == 0 or bool((_bits(pad) == 0).all())


# ---------------------------------------------------------------- bdn_gather_tiles / bdn_gather_tiles_sym
def _scene(C, h, w, seed):
    r = np.random.default_rng(seed)
    return r.standard_normal((C, h, w)).astype(np.float32), r.standard_normal((C, h, w)).astype(np.float32)


@pytest.mark.parametrize('C,Cpad', PAIRS)
@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
@guarded
def test_gather_tiles(prec, C, Cpad):
    """Plain and symmetric gather of 8 tiles of 16 x 16 (both far corners among them) from a 37 x 53 scene of C bands."""
    h, w, p, n = 37, 53, 16, 8
    dt, td = DT[prec]
    d1, d2 = _scene(C, h, w, C)
    r = np.random.default_rng(C + 1)
    o = np.stack([r.integers(0, h - p + 1, n), r.integers(0, w - p + 1, n)], 1).astype(np.int32)
    o[0], o[1] = (0, 0), (h - p, w - p)
    table = np.concatenate([o, (np.arange(n) % 8)[:, None]], 1).astype(np.int32)
    g1, g2 = guard.guard(torch.from_numpy(d1)), guard.guard(torch.from_numpy(d2))
    go, gt = guard.guard(torch.from_numpy(o)), guard.guard(torch.from_numpy(table))
    plain = guard.full((2 * n, p, p, Cpad), NAN, dtype=td)
    sym = guard.full((2 * n, p, p, Cpad), NAN, dtype=td)
    _lib.call('bdn_gather_tiles', dt, g1.data_ptr(), g2.data_ptr(), go.data_ptr(), plain.data_ptr(), n, C, h, w, p, Cpad, st())
    _lib.call('bdn_gather_tiles_sym', dt, g1.data_ptr(), g2.data_ptr(), gt.data_ptr(), sym.data_ptr(), n, C, h, w, p, Cpad, st())
    torch.cuda.synchronize()
    ref_plain = np.stack([d[:, y:y + p, x:x + p].transpose(1, 2, 0) for d in (d1, d2) for y, x in o])
    ref_sym = np.stack([np.ascontiguousarray(_apply_symmetry(d[:, y:y + p, x:x + p], inf.symmetry_bits(s)).transpose(1, 2, 0))
                        for d in (d1, d2) for y, x, s in table])
    for name, got, ref in (('plain', plain, ref_plain), ('sym', sym, ref_sym)):
        got = got.cpu()
        assert torch.equal(_bits(got[..., :C]), _bits(torch.from_numpy(np.ascontiguousarray(ref)).to(td))), name
        assert Cpad == C or bool((_bits(got[..., C:]) == 0).all()), name


# ---------------------------------------------------------------- refusals: an error code before any launch, outputs untouched
def _untouched(*tensors):
    """Every byte still 0xFF (guard.empty) or every value still NaN (guard.full(NaN))."""
    for t in tensors:
        if t.dtype == torch.uint8:
            assert bool((t == guard.FILL).all())
        else:
            assert bool(torch.isnan(t.float()).all())


@pytest.mark.parametrize('C0', [32, 48, 64])
@pytest.mark.parametrize('dtype', [BDN_BF16, BDN_BF16X3, BDN_BF16X2], ids=['bf16', 'bf16x3', 'bf16x2'])
@guarded
def test_fused_first_weight_gradient_refuses_wide_inputs(dtype, C0):
    """bdn_conv3x3_wgrad_bnbwd is the 16-padded-channel kernel: above that the query answers 0 (the engine then takes bn_bwd + the
    generic GEMM) and the entry point returns BDN_E_SHAPE with nothing launched."""
    lib = _lib.load()
    N, H, W, Cout, ipg = 4, 29, 45, 64, 2
    assert lib.bdn_conv3x3_wgrad_bnbwd_supported(dtype, N, H, W, Cout, 16, ipg) == 1          # the shape itself is taken at 16
    assert lib.bdn_conv3x3_wgrad_bnbwd_supported(dtype, N, H, W, Cout, C0, ipg) == 0
    assert lib.bdn_conv3x3_wgrad_bnbwd_kernels(dtype, N, H, W, Cout, C0, ipg) == b''
    bf = dtype == BDN_BF16
    td = torch.bfloat16 if bf else torch.float32
    dA, z = guard.zeros(N, H, W, Cout, dtype=td), guard.zeros(N, H, W, Cout, dtype=td)
    bn, sums = guard.zeros(N // ipg, 4, Cout), guard.zeros(N // ipg, 2, Cout)
    xin = guard.zeros(N, H, W, C0 if bf else 2 * C0, dtype=torch.bfloat16)
    part = guard.alloc_bytes(lib.bdn_wgrad_workspace_bytes(N, H, W, Cout, C0, ipg))
    for creal in (C0, 13):                                   # refused for the padded width, whatever the real one
        dw = guard.full((Cout, creal, 3, 3), NAN)
        with pytest.raises(RuntimeError, match=E_SHAPE):
            _lib.call('bdn_conv3x3_wgrad_bnbwd', dtype, dA.data_ptr(), Cout, z.data_ptr(), bn.data_ptr(), sums.data_ptr(), ipg, Cout,
                      xin.data_ptr(), C0, part.data_ptr(), dw.data_ptr(), creal, N, H, W, st())
        torch.cuda.synchronize()
        _untouched(dw, part)


@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
@pytest.mark.parametrize('form', ['batch', 'plain'])
@guarded
def test_input_gradient_refuses_17_bands(prec, form):
    """bdn_conv3x3_dgrad_first writes at most 16 input channels: Cin_real = 17 returns BDN_E_SHAPE with nothing launched (16 is taken:
    tests/test_gpu_input_grad.py runs up to 13, the boundary itself is asked here)."""
    dt, td = DT[prec]
    B, H, W, C = 2, 9, 21, 64
    dA, z = guard.zeros(2 * B, H, W, C, dtype=td), guard.zeros(2 * B, H, W, C, dtype=td)
    bn, sums = guard.zeros(2, 4, C), guard.zeros(2, 2, C)
    for cr, ok in ((17, False), (16, True)):
        w = guard.zeros(C, cr, 3, 3)
        dx1, dx2 = guard.full((B, cr, H, W), NAN), guard.full((B, cr, H, W), NAN)
        args = (dt, dA.data_ptr(), C, z.data_ptr() if form == 'batch' else None, bn.data_ptr() if form == 'batch' else None,
                sums.data_ptr() if form == 'batch' else None, B, w.data_ptr(), cr, dx1.data_ptr(), dx2.data_ptr(), B, H, W, st())
        if ok:
            _lib.call('bdn_conv3x3_dgrad_first', *args)
            torch.cuda.synchronize()
            assert bool((dx1 == 0).all()) and bool((dx2 == 0).all())          # the gradient of a zero dz: written in full
        else:
            with pytest.raises(RuntimeError, match=E_SHAPE):
                _lib.call('bdn_conv3x3_dgrad_first', *args)
            torch.cuda.synchronize()
            _untouched(dx1, dx2)
