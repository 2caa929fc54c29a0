"""CPU tests of tests/illcond.py: the generators produce what they promise, the plain references agree with torch on the CPU, and for
every cap tests/test_gpu_conditioning.py applies, the reference alone stays inside it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fabric_amd.criterion import Criterion
from oracle import bidate_oracle as O
from tests import criterion_ref as CR
from tests import illcond as IC

torch.set_num_threads(8)
TOL_S = {'fp32': 5e-5, 'bf16': 2e-3}          # the statistics bars of test_conv3x3_forward_stats_finalize


# ---------------------------------------------------------------- offsets
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', [(2, 16, 16, 64, 64, 1), (4, 8, 8, 128, 128, 2), (2, 13, 15, 64, 64, 2)])
def test_offset_case_reaches_every_ratio_and_the_references_stay_inside_the_caps(prec, case):
    N, H, W, Cin, Cout, ipg = case
    x, w, b, z64 = IC.offset_conv_case(prec, N, Cin, Cout, (H, W), seed=1)
    assert torch.equal(x, IC.rnd(prec, x)) and torch.equal(w, IC.rnd(prec, w))
    assert x.mean() > 0.9                                                     # the constant positive plane
    nominal = IC.channel_ratios(Cout)
    gamma, beta = torch.rand(Cout, generator=torch.Generator().manual_seed(1)) + 0.5, torch.linspace(-0.3, 0.3, Cout)
    rm0, rv0 = torch.linspace(-0.2, 0.2, Cout), torch.linspace(0.5, 1.5, Cout)
    groups = [z64[g * ipg:(g + 1) * ipg] for g in range(N // ipg)]
    ys32, rm32, rv32 = IC.bn_torch32(groups, gamma, beta, rm0, rv0)
    means, variances = [], []
    for g, zg in enumerate(groups):
        ratio = IC.achieved_ratio(zg)
        assert torch.isinf(ratio[Cout - 2]) and torch.equal(zg[:, Cout - 2], torch.full_like(zg[:, 0], 100.25))
        assert (zg[:, Cout - 1] == 0).all()
        for r in IC.RATIOS:                                                   # every regime is reached, to within the sampling noise
            got = ratio[:Cout - 2][torch.from_numpy(nominal[:Cout - 2] == r)]
            assert len(got) >= 10 and ((got - r).abs() <= 0.25 * r + 0.5).all(), (r, got)
        y64, mean, var = IC.bn_train64(zg, gamma, beta)
        means.append(mean); variances.append(var)
        live = slice(0, Cout - 2)
        # the float32 reference on this data: the quantity 8 x of which is the cap inside the required range
        inside = (ratio <= IC.REQUIRED_RATIO)
        e_ref = IC.output_error(ys32[g], y64)[live]
        assert e_ref[inside[live]].max() < 2e-6, e_ref[inside[live]].max()          # (beyond: float32 holds z itself to 6e-8 x ratio of its std)
        # the one-pass contract restated in float32 meets the existing bar inside the required range ...
        rows = max(1, ipg * H * W // 256)
        tab, var_c = IC.onepass_contract(zg, rows, gamma, beta)
        e_c = IC.affine_error(zg, tab[2], tab[3], y64)
        assert inside[live].sum() >= 20 and e_c[inside].max() <= max(TOL_S['fp32'], 8 * e_ref[inside[live]].max().item())
        # ... and degrades beyond it as (mean / std)^2: the limit of the one-pass statistic
        far = ratio[live] > 128
        assert torch.isfinite(tab).all() and (var_c >= 0).all() and e_c[live][far].max() > 10 * e_c[inside].max()
        assert (tab[1] <= np.float32(1.0 / np.sqrt(1e-5)) * (1 + 2.0 ** -23)).all()
    rm64, rv64 = IC.running64(means, variances, ipg * H * W, rm0, rv0)
    assert ((rm32.double() - rm64).abs() <= 1e-6 * rm64.abs().max()).all()
    assert ((rv32.double() - rv64).abs() <= 1e-6 * rv64.abs() + 1e-9).all()


def test_tile_sums_restate_the_contract():
    r = np.random.default_rng(0)
    v = r.standard_normal((700, 5)).astype(np.float32) + 3
    part = IC.tile_sums_f32(v, 3)
    assert part.shape == (3, 2, 5) and part.dtype == np.float32
    np.testing.assert_allclose(part[:, 0].astype(np.float64).sum(0), v.astype(np.float64).sum(0), rtol=1e-5)
    np.testing.assert_allclose(part[:, 1].astype(np.float64).sum(0), (v.astype(np.float64) ** 2).sum(0), rtol=1e-5)
    tab, var = IC.finalize_contract(part, 700, torch.ones(5), torch.zeros(5))
    np.testing.assert_allclose(var.numpy(), v.astype(np.float64).var(0), rtol=1e-3)
    const = np.full((512, 2), 100.25, np.float32)
    tab, var = IC.finalize_contract(IC.tile_sums_f32(const, 2), 512, torch.ones(2), torch.zeros(2))
    assert (var >= 0).all() and (tab[0] == 100.25).all() and torch.isfinite(tab).all()


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_offset_map_backward_references(prec):
    N, C, H, W, ipg = 4, 64, 16, 16, 2
    z = IC.offset_map(prec, N, C, H, W, seed=3)
    assert torch.equal(z, IC.rnd(prec, z))
    gamma = torch.rand(C, generator=torch.Generator().manual_seed(2)) + 0.5
    gamma[::7] *= -1
    beta = torch.linspace(-0.3, 0.3, C)
    dA = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(3))
    dz64, dg64, db64 = IC.bn_relu_backward(z, dA, gamma, beta, ipg)
    dz32, dg32, db32 = IC.bn_relu_backward(z, dA, gamma, beta, ipg, torch.float32)
    ratio = torch.stack([IC.achieved_ratio(z[g * ipg:(g + 1) * ipg].double()) for g in range(N // ipg)]).amax(0)
    inside = ratio <= IC.REQUIRED_RATIO
    assert inside.sum() >= 20 and (ratio > 128).sum() >= 10
    e = IC.per_channel_error(dz32, dz64)
    assert e[inside].max() < 1e-4                       # the float32 reference itself meets test_bn_bwd's bar inside the required range
    # the documented contract on the true table reproduces autograd in float64 (mask taken from the float64 pre-activation)
    bn = IC.true_table(z, ipg, gamma, beta)
    pre = torch.cat([IC.bn_train64(z[g * ipg:(g + 1) * ipg].double(), gamma, beta)[0] for g in range(N // ipg)])
    dzc, dgc, dbc, _ = IC.bn_bwd_contract64(z, dA.double() * (pre > 0), bn, ipg)
    assert IC.per_channel_error(dzc, dz64)[inside].max() < 1e-5
    assert (dbc - db64).abs().max() <= 1e-9 * db64.abs().max()


# ---------------------------------------------------------------- planted grids
@pytest.mark.parametrize('shape', [(4, 64, 16, 16, 2), (4, 64, 11, 45, 2), (2, 64, 5, 5, 1), (4, 128, 9, 7, 2)])
@pytest.mark.parametrize('neg', [False, True])
def test_planted_data_is_exact_and_holds_the_promised_shares(shape, neg):
    N, C, H, W, ipg = shape
    bn = IC.planted_table(N // ipg, C, seed=5, neg_zero_shift=neg)
    z = IC.planted_map(N, C, H, W, bn, ipg, seed=6, neg_zero=neg)
    assert set(z.unique().tolist()) <= set(IC.Z_GRID)
    for t in (z, bn):
        assert torch.equal(t.to(torch.bfloat16).float(), t)                       # exact in bf16
    pre = IC.planted_preact(z, bn, ipg)
    pre64 = z.double() * 1 * torch.repeat_interleave(bn[:, 2].double(), ipg, 0)[:, :, None, None] + torch.repeat_interleave(bn[:, 3].double(), ipg, 0)[:, :, None, None]
    assert torch.equal(pre.double(), pre64) and torch.equal(pre.to(torch.bfloat16).float(), pre)
    a = torch.relu(pre)
    assert IC.zero_share(pre) >= 0.15, IC.zero_share(pre)
    assert IC.positive_tie_share(a) >= 0.5, IC.positive_tie_share(a)
    assert (a > 0).double().mean() >= 0.4, (a > 0).double().mean()           # what stays in a comparison under [a > 0]
    if neg:
        assert (torch.signbit(z) & (z == 0)).any() and (torch.signbit(bn[:, 3]) & (bn[:, 3] == 0)).any()
    else:
        assert not (torch.signbit(z) & (z == 0)).any()


@pytest.mark.parametrize('shape', [(4, 64, 16, 16, 2), (4, 64, 11, 45, 2), (2, 64, 5, 5, 1)])
def test_first_maximum_references_agree_with_torch_on_the_cpu(shape):
    N, C, H, W, ipg = shape
    bn = IC.planted_table(N // ipg, C, seed=5)
    a = torch.relu(IC.planted_preact(IC.planted_map(N, C, H, W, bn, ipg, seed=6), bn, ipg))
    dP = IC.grid_values((N, C, H // 2, W // 2), 7)
    vals, _ = IC.maxpool_first(a)
    assert torch.equal(vals, F.max_pool2d(a, 2)) and torch.equal(vals, O.maxpool2(a))
    ar = a.clone().double().requires_grad_(True)
    (F.max_pool2d(ar, 2) * dP.double()).sum().backward()
    assert torch.equal(IC.unpool_first(a, dP.double()), ar.grad)
    # the whole contract of bdn_enc_skip_bwd, on [a > 0] (test_enc_skip_bwd's comparison): autograd of relu(a2 a1) + maxpool
    B = N // 2
    dF = IC.grid_values((B, C, H, W), 8)
    ar = a.clone().double().requires_grad_(True)
    ((torch.relu(ar[B:] * ar[:B]) * dF.double()).sum() + (F.max_pool2d(ar, 2) * dP.double()).sum()).backward()
    live = a > 0
    ref = IC.enc_skip_bwd_ref(a, dF, dP, B)
    assert torch.equal(ref[live], ar.grad[live])
    assert torch.equal(ref.float().double(), ref) and torch.equal(ref.to(torch.bfloat16).double(), ref)      # exact in both storage types


# ---------------------------------------------------------------- argmax ties
@pytest.mark.parametrize('shape', [(3, 2, 24, 20), (3, 3, 24, 20), (2, 3, 16, 300)])
def test_tied_logits(shape):
    lg = IC.tied_logits(shape, 9)
    assert set(lg.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0}
    assert IC.max_tie_share(lg) >= 0.3, IC.max_tie_share(lg)
    zero_max = (lg.amax(1, keepdim=True) == 0) & (lg == 0)
    mixed = (zero_max & torch.signbit(lg)).any(1) & (zero_max & ~torch.signbit(lg)).any(1)
    assert mixed.any()                                                        # +0.0 against -0.0 at the maximum
    assert ((lg == lg[:, :1]).all(1)).double().mean() >= 0.15                 # all classes equal
    first = IC.first_argmax(lg)
    assert torch.equal(first, lg.argmax(1))
    m = lg.amax(1)
    for k in range(shape[1]):                                                 # it is the FIRST maximum
        sel = first == k
        assert (lg[:, k][sel] == m[sel]).all() and all((lg[:, j][sel] < m[sel]).all() for j in range(k))


# ---------------------------------------------------------------- loss extremes
def test_loss_generators():
    shape = (3, 2, 24, 20)
    s = IC.saturated_logits(shape, 1)
    p = torch.softmax(s, 1)
    assert (p.amax(1) == 1).double().mean() > 0.7 and torch.isfinite(s).all()               # the winning class rounds to 1 in float32
    q = IC.quarter_grid_logits(shape, 2)
    assert torch.equal((q + 8192.0) - 8192.0, q) and q.abs().max() <= 4
    assert (IC.degenerate_labels(shape, 2, 'zeros') == 0).all() and (IC.degenerate_labels(shape, 2, 'ones') == 1).all()
    col = IC.degenerate_labels(shape, 2, 'columns')
    assert (col[:, :, 0::3] == 0).all() and (col[:, :, 1::3] == 1).all() and 0 < col[:, :, 2::3].double().mean() < 1
    img = IC.degenerate_labels(shape, 2, 'image')
    assert (img[0] == 1).all() and 0 < img[1:].double().mean() < 1
    v = IC.void_labels(shape, 2, 3)
    assert 0.05 < (v >= 2).double().mean() < 0.15 and set(v.unique().tolist()) == {0, 1, 2, 7, 255}
    assert all((v == k).double().mean() > 0.02 for k in (2, 7, 255))


@pytest.mark.parametrize('shape', [(3, 2, 24, 20), (2, 3, 16, 300)])
def test_void_restatement_equals_the_oracle_on_valid_labels_and_obeys_the_rule(shape):
    B, C, H, W = shape
    lg = IC.quarter_grid_logits(shape, 4).double()
    lab = IC.mixed_labels(shape, C, 5).long()
    alpha = [0.25, 0.75] if C == 2 else [0.1, 0.5, 0.9]
    for true in (lab, lab[:, None]):
        assert torch.equal(CR.overlap_void(lg, true, 0.1, 0.9, 1e-7), O.tversky_loss(lg, true, 0.1, 0.9, 1e-7))
        assert abs(CR.overlap_void(lg, true, 0.5, 0.5, 0.5e-7) - O.dice_loss(lg, true)) < 1e-14
        assert abs(CR.overlap_void(lg, true, 1.0, 1.0, 1e-7) - O.jaccard_loss(lg, true)) < 1e-14
    for gamma, a, sa in ((0.0, None, True), (2.0, alpha, False), (0.5, alpha, True)):
        assert torch.equal(CR.focal_void(lg, lab, gamma, a, sa), O.focal_loss(lg, lab, gamma, a, sa))
    # the rule for labels >= ncls
    void = IC.void_labels(shape, C, 5)
    is_void = void >= C
    assert all((void == k).any() for k in (C, 7, 255))
    c = Criterion(1.0, 0.1, 0.9, 1e-7, 'columns', w_focal=2.0, gamma=2.0, class_alpha=alpha, size_average=True)
    ref = CR.reference(c, lg, void)
    assert (ref['dfocal'].permute(0, 2, 3, 1)[is_void] == 0).all()                       # focal gradient exactly 0 there
    kept = torch.where(is_void, torch.zeros_like(void), void).long()
    lo = lg.clone().requires_grad_(True)
    per_pixel = F.nll_loss(torch.log_softmax(lo, 1), kept, reduction='none')              # gamma 0, no alpha: focal = masked CE / all pixels
    c0 = Criterion(0.0, w_focal=1.0, gamma=0.0)
    assert abs(CR.reference(c0, lg, void)['loss'] - (per_pixel * ~is_void).sum().item() / is_void.numel()) < 1e-12
    p = torch.softmax(lg, 1)
    tp1 = (p[:, 1] * (void == 1)).sum((0, 1))
    fp1 = (p[:, 1] * (void != 1)).sum((0, 1))                                            # a void pixel adds to FP of every class
    fn1 = ((1 - p[:, 1]) * (void == 1)).sum((0, 1))
    tp0, fp0, fn0 = (p[:, 0] * (void == 0)).sum((0, 1)), (p[:, 0] * (void != 0)).sum((0, 1)), ((1 - p[:, 0]) * (void == 0)).sum((0, 1))
    if C == 2:
        want = 1 - torch.stack([tp0 / (tp0 + 0.1 * fp0 + 0.9 * fn0 + 1e-7), tp1 / (tp1 + 0.1 * fp1 + 0.9 * fn1 + 1e-7)]).mean()
        assert abs(ref['overlap'] - want.item()) < 1e-12
    assert IC.argmax_counts(lg, void)[3] == int((IC.first_argmax(lg) == void.long()).sum()) < int((~is_void).sum())
    assert CR.counts(lg, void) == IC.argmax_counts(lg, void)


# ---------------------------------------------------------------- bf16 edges
def test_bf16_edge_values_cover_every_class_and_round_to_nearest_even():
    v, kind = IC.bf16_edge_values(20000, seed=1)
    assert torch.isfinite(v).all() and v.abs().max() < 2.0 ** 101
    bits = v.view(torch.int32)
    low, man_odd = bits & 0xffff, ((bits >> 16) & 1).bool()
    assert all((kind == k).sum() > 1000 for k in range(8))
    assert (low[kind == 0] == 0x8000).all() and not man_odd[kind == 0].any()
    assert (low[kind == 1] == 0x8000).all() and man_odd[kind == 1].all()
    assert (low[kind == 2] == 0x7fff).all() and (low[kind == 3] == 0x8001).all()
    sub = v[kind == 6]
    assert (sub != 0).all() and (sub.abs() < 2.0 ** -126).all()
    zero = v[kind == 7]
    assert (zero == 0).all() and torch.signbit(zero).any() and (~torch.signbit(zero)).any()
    hi = v.to(torch.bfloat16)
    hb = IC.bits16(hi).int() & 0xffff
    trunc = (bits >> 16) & 0xffff
    assert torch.equal(hb[kind == 0], trunc[kind == 0])                      # tie above an even mantissa: down
    assert torch.equal(hb[kind == 1], trunc[kind == 1] + 1)                  # above an odd one: up
    assert torch.equal(hb[kind == 2], trunc[kind == 2]) and torch.equal(hb[kind == 3], trunc[kind == 3] + 1)
    carry = kind == 4
    assert (((hb[carry] >> 7) & 0xff) == ((trunc[carry] >> 7) & 0xff) + 1).all() and ((hb[carry] & 0x7f) == 0).all()      # next binade
    hi2, lo2 = IC.split_ref(v)
    assert torch.equal(hi2, hi)
    normal = v.abs() >= 2.0 ** -100
    rec = hi2.float().double() + lo2.float().double()
    assert ((rec - v.double()).abs()[normal] <= 2.0 ** -16 * v.double().abs()[normal]).all()
    assert torch.equal(IC.bits16(hi[kind == 7]), (bits[kind == 7] >> 16).to(torch.int16))      # the sign of a zero survives
    v2, k2 = IC.bf16_edge_values(5000, seed=1, subnormals=False)
    assert (k2 != 6).all() and ((v2 == 0) | (v2.abs() >= 2.0 ** -101)).all()
