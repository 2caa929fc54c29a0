"""-m gpu kernel tests of the date-fusion mode (BDN_FUSE_PRODUCT / BDN_FUSE_ABSDIFF) through the C ABI, on guard-banded buffers.

Every entry point that takes the mode is run in fp32 and bf16 (the [hi | lo] split form in fp32, the only type it has) on
C = 64 and 512, maps 2x2 (encoder level 5: nothing to pool behind it), 5x7 (odd: a trailing row and column go unpooled) and 16x16,
B = 1 and 3.  The reference (tests/fusion_ref.py) is handed the kernel's own rounded activations -- tests/gpu_util.bnrelu_ref for the
training kernels, the activations bdn_conv3x3_eval stores for the eval convolutions -- so the comparison is the one the product tests of
tests/test_gpu_kernels.py / tests/test_gpu_eval.py make, with their bounds: 1e-6 (fp32) and 8e-3 (bf16: one output rounding) of the
result's magnitude for the streaming kernels, 2e-5 / 1e-2 for the convolution epilogues, 2e-5 for the BatchNorm-backward partial sums.
Sign and routing of the backward are exact, mode 0 through the new entry points gives the bits of the old entry points, and two identical
dates give f = 0 and dA = the pooling gradient exactly.
"""
import itertools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd._lib import BDN_F32, FUSE_ABSDIFF, FUSE_PRODUCT, IN_PLAIN
from oracle import bidate_oracle as O
from tests import fusion_ref as R
from tests import guard
from tests.gpu_util import DT, assert_close, assert_masked, bn_table, bnrelu_ref, dev, from_nhwc, pack_w, preact, rnd, st, to_nhwc
from tests.guard import guarded

pytestmark = pytest.mark.gpu
PRECS = ['fp32', 'bf16']
TOL = {'fp32': 1e-6, 'bf16': 8e-3}                 # tests/test_gpu_kernels.py: test_fuse_product, test_enc_skip_bwd
CONV_TOL = {'fp32': 2e-5, 'bf16': 1e-2}            # tests/test_gpu_eval.py
SHAPES = [(B, H, W, C) for C, (H, W), B in itertools.product((64, 512), ((2, 2), (5, 7), (16, 16)), (1, 3))]
MODES = {'product': FUSE_PRODUCT, 'absdiff': FUSE_ABSDIFF}


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def _inputs(prec, shape, same=False):
    """z [2B,C,H,W] rounded to the storage type, its BatchNorm table, and a = the rounded activations the kernels form from them.
    same=True: both date halves of z identical and the two BatchNorm rows equal."""
    B, H, W, C = shape
    z = rnd(prec, _rand((2 * B, C, H, W), 43))
    bn = bn_table(2, C, 44)
    if same:
        z[B:] = z[:B]
        bn[1] = bn[0]
    return z, bn, bnrelu_ref(prec, z, bn, B)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', SHAPES)
@guarded
def test_fuse_dates(prec, shape):
    B, H, W, C = shape
    dt, td = DT[prec]
    z, bn, a = _inputs(prec, shape)
    z_d, bn_d = to_nhwc(prec, z), dev(bn)
    got = {}
    for name, mode in MODES.items():
        got[name] = guard.empty(B, H, W, C, dtype=td)
        _lib.call('bdn_fuse_dates', dt, mode, z_d.data_ptr(), bn_d.data_ptr(), got[name].data_ptr(), B, H, W, C, st())
    old = guard.empty(B, H, W, C, dtype=td)
    _lib.call('bdn_fuse_product', dt, z_d.data_ptr(), bn_d.data_ptr(), old.data_ptr(), B, H, W, C, st())
    torch.cuda.synchronize()
    for name in MODES:
        assert_close(name, from_nhwc(got[name]), R.fuse_ref(a, B, name).float(), TOL[prec])
    assert torch.equal(got['product'], old)
    assert bool((got['absdiff'].float() >= 0).all()) and not torch.equal(got['absdiff'], old)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', SHAPES)
@guarded
def test_fuse_dates_pool(prec, shape):
    """Fusion + MaxPool2d(2) in one pass: the skip against the reference and bit for bit against bdn_fuse_dates, the pooled maps bit
    for bit against bdn_bnrelu_pool (the mode does not reach them); mode 0 = bdn_product_pool's bits."""
    B, H, W, C = shape
    dt, td = DT[prec]
    z, bn, a = _inputs(prec, shape)
    z_d, bn_d = to_nhwc(prec, z), dev(bn)
    p_ref = guard.empty(2 * B, H // 2, W // 2, C, dtype=td)
    _lib.call('bdn_bnrelu_pool', dt, z_d.data_ptr(), bn_d.data_ptr(), B, p_ref.data_ptr(), 2 * B, H, W, C, st())
    f_old, p_old = guard.empty(B, H, W, C, dtype=td), guard.empty_like(p_ref)
    _lib.call('bdn_product_pool', dt, z_d.data_ptr(), bn_d.data_ptr(), f_old.data_ptr(), p_old.data_ptr(), B, H, W, C, st())
    for name, mode in MODES.items():
        f, p, f1 = guard.full((B, H, W, C), 3.0, dtype=td), guard.full_like(p_ref, 3.0), guard.empty(B, H, W, C, dtype=td)
        _lib.call('bdn_fuse_dates_pool', dt, mode, z_d.data_ptr(), bn_d.data_ptr(), f.data_ptr(), p.data_ptr(), B, H, W, C, st())
        _lib.call('bdn_fuse_dates', dt, mode, z_d.data_ptr(), bn_d.data_ptr(), f1.data_ptr(), B, H, W, C, st())
        torch.cuda.synchronize()
        f_want, p_want = R.fuse_pool_ref(a, B, name)
        assert_close(f'{name} skip', from_nhwc(f), f_want.float(), TOL[prec])
        assert_close(f'{name} pooled', from_nhwc(p), p_want.float(), TOL[prec])
        assert torch.equal(f, f1) and torch.equal(p, p_ref)
        if name == 'product':
            assert torch.equal(f, f_old) and torch.equal(p, p_old)


@pytest.mark.parametrize('shape', SHAPES)
@guarded
def test_fuse_dates_pool_split(shape):
    """bf16x3 form (float32 z): both outputs leave as [hi | lo] bf16 operands -- bdn_split_pack of the float32 kernel's outputs bit for
    bit, the skip inside a wider operand whose foreign channels stay untouched; mode 0 = bdn_product_pool_split's bits."""
    B, H, W, C = shape
    z, bn, a = _inputs('fp32', shape)
    z_d, bn_d = to_nhwc('fp32', z), dev(bn)
    Ct = C + 64                                                    # [f | 64 channels of another producer], hi then lo
    for name, mode in MODES.items():
        f, p = guard.empty(B, H, W, C), guard.empty(2 * B, H // 2, W // 2, C)
        _lib.call('bdn_fuse_dates_pool', BDN_F32, mode, z_d.data_ptr(), bn_d.data_ptr(), f.data_ptr(), p.data_ptr(), B, H, W, C, st())
        f_ref = guard.empty(B, H, W, 2 * C, dtype=torch.bfloat16)
        p_ref = guard.empty(2 * B, H // 2, W // 2, 2 * C, dtype=torch.bfloat16)
        _lib.call('bdn_split_pack', f.data_ptr(), C, None, 0, IN_PLAIN, None, B, f_ref.data_ptr(), B, H, W, st())
        _lib.call('bdn_split_pack', p.data_ptr(), C, None, 0, IN_PLAIN, None, B, p_ref.data_ptr(), 2 * B, H // 2, W // 2, st())
        f_got = guard.empty(B, H, W, 2 * Ct, dtype=torch.bfloat16)
        p_got = guard.empty_like(p_ref)
        _lib.call('bdn_fuse_dates_pool_split', mode, z_d.data_ptr(), bn_d.data_ptr(), f_got.data_ptr(), 2 * Ct, Ct, p_got.data_ptr(),
                  B, H, W, C, st())
        torch.cuda.synchronize()
        assert torch.equal(f_got[..., :C], f_ref[..., :C]) and torch.equal(f_got[..., Ct:Ct + C], f_ref[..., C:])
        guard.assert_foreign_untouched(f_got, [(0, C), (Ct, C)], 'split skip operand')
        assert torch.equal(p_got, p_ref)
        hi, lo = R.split_hi_lo(R.fuse_ref(a, B, name).float())         # ... and the split of the reference itself, to float32 rounding
        assert_close(f'{name} hi + lo', from_nhwc(f_got[..., :C]) + from_nhwc(f_got[..., Ct:Ct + C]), hi + lo, TOL['fp32'])
        if name == 'product':
            f_old, p_old = guard.empty_like(f_got), guard.empty_like(p_got)
            _lib.call('bdn_product_pool_split', z_d.data_ptr(), bn_d.data_ptr(), f_old.data_ptr(), 2 * Ct, Ct, p_old.data_ptr(), B, H, W, C, st())
            torch.cuda.synchronize()
            assert torch.equal(f_old.view(torch.int16), f_got.view(torch.int16)) and torch.equal(p_old, p_got)   # bits: the foreign channels hold NaN


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('pooled', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
@guarded
def test_enc_skip_bwd_fusion(prec, shape, pooled):
    """Encoder-skip backward under 'absdiff', with and without dP, with and without bs_partial.  Without dP the output is the fusion part
    alone: every element is exactly +dF, -dF or 0, date 2 is the exact negation of date 1, and the sign is sign(a1 - a2) wherever the two
    rounded activations differ (at equal activations, both-dead ReLUs included, exactly 0).  Mode 0 = bdn_enc_skip_bwd's bits."""
    B, H, W, C = shape
    dt, td = DT[prec]
    z, bn, a = _inputs(prec, shape)
    extra = 32
    dF = rnd(prec, _rand((B, C + extra, H, W), 53))
    dP = rnd(prec, _rand((2 * B, C, H // 2, W // 2), 54)) if pooled else None
    dF_d, z_d, bn_d = to_nhwc(prec, dF), to_nhwc(prec, z), dev(bn)
    dF_d[..., C:] = float('nan')                                   # the foreign channels ([dF | dU]): a read of them poisons the result
    dP_d = to_nhwc(prec, dP) if pooled else None
    rows = _lib.load().bdn_enc_skip_bwd_rows(dt, B, H, W, C)

    def run(entry, head, part):
        out = guard.empty(2 * B, H, W, C, dtype=td)
        _lib.call(entry, dt, *head, dF_d.data_ptr(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), dP_d.data_ptr() if pooled else None,
                  out.data_ptr(), part.data_ptr() if part is not None else None, B, H, W, C, st())
        return out
    part = guard.full((2, rows, 2, C), float('nan'))
    out_bs = run('bdn_enc_skip_bwd_fusion', (FUSE_ABSDIFF,), part)
    out = run('bdn_enc_skip_bwd_fusion', (FUSE_ABSDIFF,), None)
    part0, part_old = guard.full_like(part, float('nan')), guard.full_like(part, float('nan'))
    new0, old0 = run('bdn_enc_skip_bwd_fusion', (FUSE_PRODUCT,), part0), run('bdn_enc_skip_bwd', (), part_old)
    torch.cuda.synchronize()
    assert torch.equal(new0, old0) and torch.equal(part0, part_old)
    got = from_nhwc(out)
    fus, pool = R.enc_skip_bwd_ref(a, dF[:, :C], dP, B, 'absdiff')
    assert_close('enc_skip_bwd absdiff', got, (fus + pool).float(), TOL[prec])
    if not pooled:
        g1, g2, d = got[:B], got[B:], dF[:, :C]
        assert torch.equal(g2, -g1)
        assert bool(((g1 == d) | (g1 == -d) | (g1 == 0)).all())
        s = torch.sign(a[:B] - a[B:])
        assert torch.equal(g1, d * s)
        assert bool((s == 0).any()) and bool((s > 0).any()) and bool((s < 0).any())       # ties (dead ReLUs) and both signs are present
    # with the statistics the stored gradient is g (masked), and the sums are formed on the stored, rounded values
    assert_masked('enc_skip_bwd absdiff', from_nhwc(out_bs), got, preact(z, bn, B))
    g = from_nhwc(out_bs).double()
    for dte in range(2):
        sl = slice(dte * B, (dte + 1) * B)
        sums = part[dte].double().sum(0).cpu()
        assert_close(f'sum g (date {dte})', sums[0].float(), g[sl].sum((0, 2, 3)).float(), 2e-5, abs_floor=1e-4)
        assert_close(f'sum g*z (date {dte})', sums[1].float(), (g[sl] * z[sl].double()).sum((0, 2, 3)).float(), 2e-5, abs_floor=1e-4)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', [(3, 5, 7, 64), (1, 16, 16, 512), (3, 2, 2, 512)])
@guarded
def test_identical_dates_give_zero_skip_and_the_pool_gradient(prec, shape):
    B, H, W, C = shape
    dt, td = DT[prec]
    z, bn, a = _inputs(prec, shape, same=True)
    z_d, bn_d = to_nhwc(prec, z), dev(bn)
    f, f2, p = guard.full((B, H, W, C), 3.0, dtype=td), guard.full((B, H, W, C), 3.0, dtype=td), guard.empty(2 * B, H // 2, W // 2, C, dtype=td)
    _lib.call('bdn_fuse_dates', dt, FUSE_ABSDIFF, z_d.data_ptr(), bn_d.data_ptr(), f.data_ptr(), B, H, W, C, st())
    _lib.call('bdn_fuse_dates_pool', dt, FUSE_ABSDIFF, z_d.data_ptr(), bn_d.data_ptr(), f2.data_ptr(), p.data_ptr(), B, H, W, C, st())
    dF = rnd(prec, _rand((B, C, H, W), 53))
    dP = rnd(prec, _rand((2 * B, C, H // 2, W // 2), 54))
    dF_d, dP_d = to_nhwc(prec, dF), to_nhwc(prec, dP)
    out = guard.empty(2 * B, H, W, C, dtype=td)
    _lib.call('bdn_enc_skip_bwd_fusion', dt, FUSE_ABSDIFF, dF_d.data_ptr(), C, z_d.data_ptr(), bn_d.data_ptr(), dP_d.data_ptr(),
              out.data_ptr(), None, B, H, W, C, st())
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((f2 == 0).all())
    _, pool = R.enc_skip_bwd_ref(a, dF, dP, B, 'absdiff')
    assert torch.equal(from_nhwc(out).double(), pool) and bool(pool.any())
    if prec == 'fp32':
        fs, ps = guard.full((B, H, W, 2 * C), 3.0, dtype=torch.bfloat16), guard.empty(2 * B, H // 2, W // 2, 2 * C, dtype=torch.bfloat16)
        _lib.call('bdn_fuse_dates_pool_split', FUSE_ABSDIFF, z_d.data_ptr(), bn_d.data_ptr(), fs.data_ptr(), 2 * C, C, ps.data_ptr(),
                  B, H, W, C, st())
        torch.cuda.synchronize()
        assert bool((fs == 0).all())


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', SHAPES)
@guarded
def test_conv3x3_eval_fusion(prec, shape):
    """The eval convolutions with a fused second date: the paired form and the per-date form (mul = date 1's stored activation) under
    'absdiff' against |a_d2 - a_d1| of the activations bdn_conv3x3_eval itself stores, bit-equal to each other; mode 0 = the bits of
    bdn_conv3x3_eval / bdn_conv3x3_eval_pair; identical dates give exactly 0."""
    B, H, W, C = shape
    dt, td = DT[prec]
    x = rnd(prec, _rand((2 * B, C, H, W), 1))
    w = _rand((C, C, 3, 3), 3, (2.0 / (9 * C)) ** 0.5)
    sc, sh = _rand((C,), 5).abs() + 0.5, _rand((C,), 6, 0.3)
    wf, _ = pack_w(prec, w, C)
    dx, dsc, dsh = to_nhwc(prec, x), dev(sc), dev(sh)
    common = (wf.data_ptr(), dsc.data_ptr(), dsh.data_ptr())
    act = guard.empty(2 * B, H, W, C, dtype=td)                     # the kernel's own rounded activations, both dates
    _lib.call('bdn_conv3x3_eval', dt, dx.data_ptr(), C, None, 0, *common, act.data_ptr(), None, None, 2 * B, H, W, C, st())
    pool = guard.empty(2 * B, H // 2, W // 2, C, dtype=td)
    res = {}
    for name, mode in MODES.items():
        f_pair, f_mul, p_pair = guard.full((B, H, W, C), float('nan'), dtype=td), guard.full((B, H, W, C), float('nan'), dtype=td), guard.empty_like(pool)
        _lib.call('bdn_conv3x3_eval_pair_fusion', dt, mode, dx.data_ptr(), C, *common, f_pair.data_ptr(), p_pair.data_ptr(), B, H, W, C, st())
        _lib.call('bdn_conv3x3_eval_fusion', dt, mode, dx[B:].data_ptr(), C, None, 0, *common, f_mul.data_ptr(), act[:B].data_ptr(),
                  pool[B:].data_ptr(), B, H, W, C, st())
        res[name] = (f_pair, f_mul, p_pair)
    o_pair, o_mul, o_pool = guard.empty(B, H, W, C, dtype=td), guard.empty(B, H, W, C, dtype=td), guard.empty_like(pool)
    _lib.call('bdn_conv3x3_eval_pair', dt, dx.data_ptr(), C, *common, o_pair.data_ptr(), o_pool.data_ptr(), B, H, W, C, st())
    _lib.call('bdn_conv3x3_eval', dt, dx[B:].data_ptr(), C, None, 0, *common, o_mul.data_ptr(), act[:B].data_ptr(), None, B, H, W, C, st())
    torch.cuda.synchronize()
    a = from_nhwc(act)
    for name in MODES:
        f_pair, f_mul, p_pair = res[name]
        want = rnd(prec, R.fuse_ref(a, B, name).float())
        assert_close(f'{name} paired', from_nhwc(f_pair), want, CONV_TOL[prec], 1e-6)
        assert_close(f'{name} per date', from_nhwc(f_mul), want, CONV_TOL[prec], 1e-6)
        assert torch.equal(f_pair, f_mul)
        assert torch.equal(from_nhwc(p_pair), O.maxpool2(a)) and torch.equal(pool[B:], p_pair[B:])
    assert torch.equal(res['product'][0], o_pair) and torch.equal(res['product'][1], o_mul) and torch.equal(res['product'][2], o_pool)
    # identical dates
    dx[B:] = dx[:B]
    f0 = guard.full((B, H, W, C), float('nan'), dtype=td)
    _lib.call('bdn_conv3x3_eval_pair_fusion', dt, FUSE_ABSDIFF, dx.data_ptr(), C, *common, f0.data_ptr(), None, B, H, W, C, st())
    torch.cuda.synchronize()
    assert bool((f0 == 0).all())
