"""-m gpu: every row of tests/launch_cases.py -- one per kernel instantiation BiDateNet launches -- against a float64 reference.

The shape of a launch picks its instantiation, and several instantiations of the benchmarked step are only reached at shapes the other
kernel tests never use.  Each test here first asks the library which instantiation the row's shape selects (it must be the row's), fills
every output with NaN, launches, and compares element by element with torch's float64 convolution (conv2d / conv2d_input /
conv2d_weight on the CPU) of the same rounded inputs.  Nothing in the reference calls the library.

Element-wise bars:
  bf16 outputs      |got - ref| <= 2^-8 |ref| + TAU max|ref|   (one rounding of the output; TAU covers float32 summation order)
  float32 outputs   |got - ref| <= 2e-5 max|ref|               (the existing fp32 bar)
  bf16x3 / bf16x2   |got - ref| <= 1e-4 max|ref|               (the existing bar of the split-product kernels)
LAUNCH_SHAPES_REPORT=<file> appends each row's worst error (in units of its bar) to that file.

Wide rows (launch_cases.WIDE_ROWS, r.creal set): the first layer of a model of creal bands padded to C0 = 32, 48 or 64 channels.  The
filter holds creal channels and is packed with Cin = creal, Cin_pad = C0 and no data-gradient image, through bdn_pack_weights AND through
the one-record bdn_pack_weights_multi descriptor the engine uses (bit-equal; bf16 / fp32: equal to the rounded filter with zero columns);
the operand's padded channels are exact zeros; the reference convolves the creal channels; a weight gradient lands in a guard-banded
buffer of exactly Cout * creal * 9 floats.  They are held to the same bars as their 16-band and 64-channel neighbours.
"""
import json
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X3, BDN_F32, IN_BNRELU, IN_PLAIN
from tests import launch_cases as lc
from tests.gpu_util import assert_masked, bn_table, bnrelu_ref, dev, frag_to_dense, from_nhwc, pack_w, preact, rnd, st, to_nhwc
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu
TAU = 2e-3
F32_TOL, X3_TOL = 2e-5, 1e-4
NAN = float('nan')


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def _report(name, worst):
    path = os.environ.get('LAUNCH_SHAPES_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps({'check': name, 'worst_over_bar': worst}) + '\n')


def check(name, got, ref, kind, rel=2.0 ** -8, tol=None):
    """Element-wise comparison with the bar of the output kind ('bf16', 'fp32', 'x3'); returns the worst |err| / bar (<= 1 passes)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f'{name}: non-finite values (an output element was not written)'
    m = ref.abs().max().item()
    if kind == 'bf16':
        bar = rel * ref.abs() + (tol if tol is not None else TAU) * m
    else:
        bar = torch.full_like(ref, (tol if tol is not None else (F32_TOL if kind == 'fp32' else X3_TOL)) * m)
    bar = bar + 1e-30
    ratio = ((got - ref).abs() / bar).max().item()
    _report(name, ratio)
    assert ratio <= 1.0, f'{name}: worst |err| = {ratio:.3f} x the bar (max|ref| {m:.3e})'
    return ratio


def _rid(r):
    return lc.row_id(r)


def _rows(*ops):
    return [r for r in lc.ALL_ROWS if r.op in ops]


def _assert_variant(r):
    assert lc.instantiation(r) == r.inst, f'{_rid(r)} selects {lc.instantiation(r)}'


def _padded(x_nchw, C0):
    """[N, creal, H, W] -> [N, C0, H, W]: the padded channels are exact zeros."""
    return F.pad(x_nchw, (0, 0, 0, 0, 0, C0 - x_nchw.shape[1]))


def _assert_zero_padding(r, t_nhwc, halves=1):
    """The padded channels of a wide row's device operand ([.., halves * C0]: the split operand has a hi and a lo half) are exact zeros."""
    for h in range(halves):
        pad = t_nhwc[..., h * r.C0 + r.creal:(h + 1) * r.C0]
        assert pad.numel() == 0 or bool((pad == 0).all()), f'{_rid(r)}: padded operand channels are not zero'


def pack_first(prec, w, C0):
    """Forward filter image of a first layer: w [Cout, creal, 3, 3] packed with Cin = creal, Cin_pad = C0 and wd = NULL, through
    bdn_pack_weights and through a one-record bdn_pack_weights_multi descriptor (the engine's form: its irregular branch whenever
    creal < C0 or C0 is no multiple of 64, its LDS tile kernel at creal = C0 = 64 in bf16).  The two images must be equal bit for bit and
    written in full; bf16 / fp32: also equal to the rounded filter with zero columns above creal.  Returns the descriptor form's image."""
    Cout, creal = w.shape[:2]
    x3 = prec in ('bf16x3', 'bf16x2')
    dt = BDN_BF16X3 if x3 else (BDN_BF16 if prec == 'bf16' else BDN_F32)
    td = torch.float32 if prec == 'fp32' else torch.bfloat16
    wdev = dev(w)
    one, multi = (guard.empty(Cout, 9, (3 if x3 else 1) * C0, dtype=td) for _ in range(2))
    _lib.call('bdn_pack_weights', dt, wdev.data_ptr(), one.data_ptr(), None, Cout, creal, C0, st())
    desc = guard.guard(torch.frombuffer(bytearray(struct.pack('<QQQiiii', wdev.data_ptr(), multi.data_ptr(), 0, Cout, creal, C0, 0)),
                                        dtype=torch.uint8))
    _lib.call('bdn_pack_weights_multi', dt, desc.data_ptr(), 1, st())
    torch.cuda.synchronize()
    assert torch.isfinite(multi.float()).all() and torch.isfinite(one.float()).all(), f'pack {prec} {creal}->{C0}: image not written in full'
    assert torch.equal(one.view(torch.uint8), multi.view(torch.uint8)), f'pack {prec} {creal}->{C0}: the two packers differ'
    if not x3:
        dense = frag_to_dense(prec, multi, Cout, C0)                     # [Cout][9][C0]
        want = _padded(rnd(prec, w), C0).reshape(Cout, C0, 9).permute(0, 2, 1)
        assert torch.equal(dense, want), f'pack {prec} {creal}->{C0}: image is not the rounded filter with zero columns'
    return multi


def _grp(t, G):
    """[N, ...] -> list of per-group slices."""
    n = t.shape[0] // G
    return [t[g * n:(g + 1) * n] for g in range(G)]


def _bn_from(z, G, seed):
    """BatchNorm table whose statistics are those of z itself (so ReLU masks are mixed)."""
    bn = bn_table(G, z.shape[1], seed)
    for g, zg in enumerate(_grp(z.double(), G)):
        mean, var = zg.mean((0, 2, 3)), zg.var((0, 2, 3), unbiased=False)
        inv = 1 / torch.sqrt(var + 1e-5)
        gamma = bn[g, 2].double() / bn[g, 1].double()
        bn[g, 0], bn[g, 1] = mean.float(), inv.float()
        bn[g, 2] = (gamma * inv).float()
        bn[g, 3] = (0.1 - mean * gamma * inv).float()
    return bn


def _finalize_and_check(name, stats, nt, z64, G, ipg, H, W, Cout, fp32):
    """bdn_bn_finalize on the launch's partials: mean / invstd / scale / shift, running buffers, num_batches_tracked against float64."""
    lib = _lib.load()
    gamma, beta = _rand((Cout,), 6).abs() + 0.5, _rand((Cout,), 7, 0.3)
    rm0, rv0 = _rand((Cout,), 8, 0.2), _rand((Cout,), 9).abs() + 0.5
    drm, drv, dg, db = dev(rm0), dev(rv0), dev(gamma), dev(beta)
    nbt = guard.zeros(1, dtype=torch.int64)
    bn = guard.full((G, 4, Cout), NAN)
    fws = guard.empty(lib.bdn_bn_finalize_workspace_bytes(nt, G, Cout) // 8, dtype=torch.float64)
    _lib.call('bdn_bn_finalize', stats.data_ptr(), nt, G, Cout, ipg * H * W, dg.data_ptr(), db.data_ptr(),
              1e-5, 0.1, drm.data_ptr(), drv.data_ptr(), nbt.data_ptr(), bn.data_ptr(), fws.data_ptr(), st())
    torch.cuda.synchronize()
    bn = bn.cpu()
    tol = 5e-5 if fp32 else 2e-3            # bf16: the statistics come from the float32 accumulators, the reference from the exact sums
    rm, rv = rm0.double(), rv0.double()
    n = ipg * H * W
    for g, zg in enumerate(_grp(z64, G)):
        mean, var = zg.mean((0, 2, 3)), zg.var((0, 2, 3), unbiased=False)
        inv = 1 / torch.sqrt(var + 1e-5)
        check(f'{name} mean g{g}', bn[g, 0], mean, 'fp32', tol=tol)
        check(f'{name} invstd g{g}', bn[g, 1], inv, 'fp32', tol=tol)
        check(f'{name} scale g{g}', bn[g, 2], gamma.double() * inv, 'fp32', tol=tol)
        check(f'{name} shift g{g}', bn[g, 3], beta.double() - mean * gamma.double() * inv, 'fp32', tol=tol)
        rm = 0.9 * rm + 0.1 * mean
        rv = 0.9 * rv + 0.1 * var * n / max(n - 1, 1)
    check(f'{name} running_mean', drm, rm, 'fp32', tol=tol)
    check(f'{name} running_var', drv, rv, 'fp32', tol=tol)
    assert int(nbt.item()) == G


# ------------------------------------------------------------------ forward + statistics (+ finalize)
def forward_case(r):
    """Inputs and float64 reference of a 'fwd' row (host tensors only)."""
    N, H, W, C0, C1, Cout, ipg, p = r.N, r.H, r.W, r.C0, r.C1, r.Cout, r.ipg, r.prec
    G = N // ipg
    cr = r.creal or C0                                   # wide rows: the filter and the reference on the real channels only
    x0 = rnd(p, _rand((N, cr, H, W), 1))
    x1 = rnd(p, _rand((N, C1, H, W), 2)) if C1 else None
    w = rnd(p, _rand((Cout, cr + C1, 3, 3), 3, (2.0 / (9 * (cr + C1))) ** 0.5))
    b = _rand((Cout,), 4, 0.1)
    bn_in = bn_table(G, C0, 5) if r.bnrelu else None
    a0 = bnrelu_ref(p, x0, bn_in, ipg) if r.bnrelu else x0
    a = torch.cat([a0, x1], 1) if C1 else a0
    ref = F.conv2d(a.double(), w.double(), b.double(), padding=1)
    return SimpleNamespace(x0=_padded(x0, C0), x1=x1, w=w, b=b, bn_in=bn_in, ref=ref)


def forward_launch(r, c, d0, d1, out, stats, N=None, ipg=None):
    """bdn_conv3x3 of a 'fwd' row on device operands (N / ipg: those of the launch when they are not the row's)."""
    N, ipg = (r.N if N is None else N), (r.ipg if ipg is None else ipg)
    wf = pack_first(r.prec, c.w, r.C0) if r.creal else pack_w(r.prec, c.w, r.C0 + r.C1)[0]
    dbn, db = (dev(c.bn_in) if r.bnrelu else None), dev(c.b)
    _lib.call('bdn_conv3x3', lc.DTYPE[r.prec], d0.data_ptr(), r.C0, d1.data_ptr() if r.C1 else None, r.C1,
              IN_BNRELU if r.bnrelu else IN_PLAIN, dbn.data_ptr() if r.bnrelu else None, ipg, wf.data_ptr(), db.data_ptr(), out.data_ptr(),
              stats.data_ptr(), N, r.H, r.W, r.Cout, st())
    torch.cuda.synchronize()


def forward_compare(r, c, out, stats, finalize=True):
    """Output and tile partials of a 'fwd' launch at the row's N against the float64 reference (+ bdn_bn_finalize on the partials)."""
    G, p, nt = r.N // r.ipg, r.prec, stats.shape[0]
    check(f'{_rid(r)} out', from_nhwc(out), c.ref, p)
    # per-group totals of the tile partials (every row written: NaN-filled) against the exact sums
    s = stats.cpu().double().reshape(G, nt // G, 2, r.Cout).sum(1)
    for g, zg in enumerate(_grp(c.ref, G)):
        check(f'{_rid(r)} sum g{g}', s[g, 0], zg.sum((0, 2, 3)), 'fp32', tol=1e-5 if p == 'fp32' else 1e-4)
        check(f'{_rid(r)} sumsq g{g}', s[g, 1], (zg * zg).sum((0, 2, 3)), 'fp32', tol=1e-5 if p == 'fp32' else 1e-4)
    if finalize:
        _finalize_and_check(_rid(r), stats, nt, c.ref, G, r.ipg, r.H, r.W, r.Cout, p == 'fp32')


@pytest.mark.parametrize('r', _rows('fwd'), ids=_rid)
@guarded
def test_forward_and_statistics(r):
    _assert_variant(r)
    p = r.prec
    td = torch.bfloat16 if p == 'bf16' else torch.float32
    c = forward_case(r)
    d0, d1 = to_nhwc(p, c.x0), (to_nhwc(p, c.x1) if r.C1 else None)
    if r.creal:
        _assert_zero_padding(r, d0)
    out = guard.full((r.N, r.H, r.W, r.Cout), NAN, dtype=td)
    nt = _lib.load().bdn_conv3x3_num_mtiles(r.N, r.H, r.W, r.Cout, r.ipg)
    stats = guard.full((nt, 2, r.Cout), NAN)
    forward_launch(r, c, d0, d1, out, stats)
    forward_compare(r, c, out, stats)


# ------------------------------------------------------------------ data gradient: plain, with fused statistics, BatchNorm backward on load
def _dgrad_setup(r, seed=11):
    p = r.prec
    dz = rnd(p, _rand((r.N, r.C0, r.H, r.W), seed))
    w = rnd(p, _rand((r.C0, r.Cout, 3, 3), seed + 1, 0.05))          # the layer: Cout -> C0 channels; its data gradient C0 -> Cout
    return dz, w


def dgrad_case(r):
    """Inputs and float64 reference of a 'dgrad' row."""
    dz, w = _dgrad_setup(r)
    ref = torch.nn.grad.conv2d_input((r.N, r.Cout, r.H, r.W), w.double(), dz.double(), padding=1)
    return SimpleNamespace(dz=dz, w=w, ref=ref)


def dgrad_launch(r, c, ddz, out, N=None, ipg=None):
    N, ipg = (r.N if N is None else N), (r.ipg if ipg is None else ipg)
    _, wd = pack_w(r.prec, c.w, r.Cout)
    _lib.call('bdn_conv3x3', lc.DTYPE[r.prec], ddz.data_ptr(), r.C0, None, 0, IN_PLAIN, None, ipg, wd.data_ptr(), None, out.data_ptr(), None,
              N, r.H, r.W, r.Cout, st())
    torch.cuda.synchronize()


def dgrad_compare(r, c, out):
    check(f'{_rid(r)} dA', from_nhwc(out), c.ref, r.prec)


@pytest.mark.parametrize('r', _rows('dgrad'), ids=_rid)
@guarded
def test_data_gradient(r):
    _assert_variant(r)
    p = r.prec
    td = torch.bfloat16 if p == 'bf16' else torch.float32
    c = dgrad_case(r)
    out = guard.full((r.N, r.H, r.W, r.Cout), NAN, dtype=td)
    dgrad_launch(r, c, to_nhwc(p, c.dz), out)
    dgrad_compare(r, c, out)


def _bs_reference(g_stored, zprev, G):
    """Per-group float64 sums of the STORED masked gradient g and of g * z: the fused epilogues reduce the values they store (bf16: rounded),
    and the stored values themselves are held against float64 by assert_masked + the plain data gradient."""
    g = g_stored.double()
    return [(gg.sum((0, 2, 3)), (gg * zz.double()).sum((0, 2, 3))) for gg, zz in zip(_grp(g, G), _grp(zprev, G))]


def _check_bs(name, part, nt, refs, G, Cout):
    s = part.cpu().double().reshape(G, nt // G, 2, Cout).sum(1)
    for g, (s0, s1) in enumerate(refs):
        check(f'{name} sum g g{g}', s[g, 0], s0, 'fp32', tol=1e-5)
        check(f'{name} sum g*z g{g}', s[g, 1], s1, 'fp32', tol=1e-5)


def dgrad_bs_case(r):
    """Inputs and float64 reference of a 'dgrad_bs' row."""
    G = r.N // r.ipg
    dz, w = _dgrad_setup(r, 51)
    ref = torch.nn.grad.conv2d_input((r.N, r.Cout, r.H, r.W), w.double(), dz.double(), padding=1)
    zprev = rnd(r.prec, _rand((r.N, r.Cout, r.H, r.W), 53))
    bnp = _bn_from(zprev, G, 54)
    return SimpleNamespace(dz=dz, w=w, ref=ref, zprev=zprev, bnp=bnp)


def dgrad_bs_launch(r, c, ddz, zp_d, plain, dA, part, N=None, ipg=None):
    """The plain data gradient into `plain`, bdn_conv3x3_dgrad_bs into dA / part."""
    N, ipg = (r.N if N is None else N), (r.ipg if ipg is None else ipg)
    dt = lc.DTYPE[r.prec]
    _, wd = pack_w(r.prec, c.w, r.Cout)
    bnp_d = dev(c.bnp)
    _lib.call('bdn_conv3x3', dt, ddz.data_ptr(), r.C0, None, 0, IN_PLAIN, None, ipg, wd.data_ptr(), None, plain.data_ptr(), None,
              N, r.H, r.W, r.Cout, st())
    _lib.call('bdn_conv3x3_dgrad_bs', dt, ddz.data_ptr(), r.C0, wd.data_ptr(), dA.data_ptr(), zp_d.data_ptr(), bnp_d.data_ptr(), ipg,
              part.data_ptr(), N, r.H, r.W, r.Cout, st())
    torch.cuda.synchronize()


def dgrad_bs_compare(r, c, plain, dA, part):
    G = r.N // r.ipg
    check(f'{_rid(r)} dA', from_nhwc(plain), c.ref, r.prec)
    assert_masked(_rid(r), from_nhwc(dA), from_nhwc(plain), preact(c.zprev, c.bnp, r.ipg))
    _check_bs(_rid(r), part, part.shape[0], _bs_reference(from_nhwc(dA), c.zprev, G), G, r.Cout)


@pytest.mark.parametrize('r', _rows('dgrad_bs'), ids=_rid)
@guarded
def test_data_gradient_with_fused_statistics(r):
    _assert_variant(r)
    p = r.prec
    td = torch.bfloat16 if p == 'bf16' else torch.float32
    c = dgrad_bs_case(r)
    ddz, zp_d = to_nhwc(p, c.dz), to_nhwc(p, c.zprev)
    plain = guard.full((r.N, r.H, r.W, r.Cout), NAN, dtype=td)
    nt = _lib.load().bdn_conv3x3_num_mtiles(r.N, r.H, r.W, r.Cout, r.ipg)
    part = guard.full((nt, 2, r.Cout), NAN)
    dA = guard.full_like(plain, NAN)
    dgrad_bs_launch(r, c, ddz, zp_d, plain, dA, part)
    dgrad_bs_compare(r, c, plain, dA, part)


def dgrad_bb_case(r):
    """Inputs and the independent float64 computation of a 'dgrad_bb' row: the BatchNorm backward dz = scale (g - s0/M - xhat s1/M) with the
    sums of g in float64, then conv2d_input of bf16(dz)."""
    N, H, W, C0, Cout, ipg = r.N, r.H, r.W, r.C0, r.Cout, r.ipg
    G, M = N // ipg, ipg * H * W
    z = rnd('bf16', _rand((N, C0, H, W), 62))
    bn = _bn_from(z, G, 63)
    pre = preact(z, bn, ipg)
    dA = rnd('bf16', _rand((N, C0, H, W), 61)) * (pre > 1e-4)          # g: masked, and zero at the switching point whichever way it rounds
    w = rnd('bf16', _rand((C0, Cout, 3, 3), 64, 0.05))
    dz64 = torch.empty(N, C0, H, W, dtype=torch.float64)
    sums64 = torch.empty(G, 2, C0, dtype=torch.float64)
    for g in range(G):
        sl = slice(g * ipg, (g + 1) * ipg)
        mean, inv, scale = (bn[g, i].double()[None, :, None, None] for i in range(3))
        gg, xhat = dA[sl].double(), (z[sl].double() - mean) * inv
        s0, s1 = gg.sum((0, 2, 3)), (gg * xhat).sum((0, 2, 3))
        sums64[g, 0], sums64[g, 1] = s0, s1
        dz64[sl] = scale * (gg - s0[None, :, None, None] / M - xhat * s1[None, :, None, None] / M)
    ref = torch.nn.grad.conv2d_input((N, Cout, H, W), w.double(), dz64.to(torch.bfloat16).double(), padding=1)
    zprev = rnd('bf16', _rand((N, Cout, H, W), 65))
    bnp = _bn_from(zprev, G, 66)
    return SimpleNamespace(z=z, bn=bn, dA=dA, w=w, dz64=dz64, sums64=sums64, ref=ref, zprev=zprev, bnp=bnp)


def dgrad_bb_launch(r, c, wd, dA_d, z_d, bn_d, sums, zp_d, out, dz, outm, part, N=None, ipg=None):
    """bdn_conv3x3_dgrad_bb without (out, dz) and with (outm, part) the producing layer's statistics; `sums` is an input.  out = None or
    outm = None leaves that launch out."""
    N, ipg = (r.N if N is None else N), (r.ipg if ipg is None else ipg)
    C0 = r.C0
    if out is not None:
        _lib.call('bdn_conv3x3_dgrad_bb', BDN_BF16, dA_d.data_ptr(), C0, z_d.data_ptr(), bn_d.data_ptr(), sums.data_ptr(), ipg, wd.data_ptr(),
                  out.data_ptr(), None, None, None, dz.data_ptr(), N, r.H, r.W, r.Cout, st())
    if outm is not None:
        bnp_d = dev(c.bnp)
        _lib.call('bdn_conv3x3_dgrad_bb', BDN_BF16, dA_d.data_ptr(), C0, z_d.data_ptr(), bn_d.data_ptr(), sums.data_ptr(), ipg, wd.data_ptr(),
                  outm.data_ptr(), zp_d.data_ptr(), bnp_d.data_ptr(), part.data_ptr(), None, N, r.H, r.W, r.Cout, st())
    torch.cuda.synchronize()


def dgrad_bb_compare(r, c, out, dz, outm, part):
    name, G = _rid(r), r.N // r.ipg
    check(f'{name} dz', from_nhwc(dz), c.dz64, 'bf16')
    check(f'{name} dA_prev', from_nhwc(out), c.ref, 'bf16')
    assert_masked(name, from_nhwc(outm), from_nhwc(out), preact(c.zprev, c.bnp, r.ipg))
    _check_bs(name, part, part.shape[0], _bs_reference(from_nhwc(outm), c.zprev, G), G, r.Cout)


@pytest.mark.parametrize('r', _rows('dgrad_bb'), ids=_rid)
@guarded
def test_data_gradient_with_bn_backward_on_load(r):
    """bdn_conv3x3_dgrad_bb against an independent float64 computation: the BatchNorm backward dz = scale (g - s0/M - xhat s1/M) with the
    sums of g in float64, then conv2d_input of bf16(dz); and against the two-kernel path (bdn_bn_bwd + the plain data gradient)."""
    _assert_variant(r)
    lib = _lib.load()
    N, H, W, C0, Cout, ipg = r.N, r.H, r.W, r.C0, r.Cout, r.ipg
    G = N // ipg
    c = dgrad_bb_case(r)
    _, wd = pack_w('bf16', c.w, Cout)
    dA_d, z_d, bn_d = to_nhwc('bf16', c.dA), to_nhwc('bf16', c.z), dev(c.bn)
    # two-kernel path: its sums feed the fused kernel
    ws = guard.empty(lib.bdn_bn_bwd_workspace_bytes(BDN_BF16, N, H, W, C0, ipg) // 4)
    sums = guard.full((G, 2, C0), NAN)
    dg, db = guard.empty(C0), guard.empty(C0)
    dz_two = guard.full((N, H, W, C0), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_bn_bwd', BDN_BF16, dA_d.data_ptr(), C0, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C0,
              ws.data_ptr(), sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dz_two.data_ptr(), st())
    out_two = guard.full((N, H, W, Cout), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_conv3x3', BDN_BF16, dz_two.data_ptr(), C0, None, 0, IN_PLAIN, None, ipg, wd.data_ptr(), None, out_two.data_ptr(), None,
              N, H, W, Cout, st())
    # fused: without and with the producing layer's statistics
    zp_d = to_nhwc('bf16', c.zprev)
    nt = lib.bdn_conv3x3_num_mtiles(N, H, W, Cout, ipg)
    part = guard.full((nt, 2, Cout), NAN)
    out = guard.full((N, H, W, Cout), NAN, dtype=torch.bfloat16)
    dz = guard.full((N, H, W, C0), NAN, dtype=torch.bfloat16)
    outm = guard.full_like(out, NAN)
    dgrad_bb_launch(r, c, wd, dA_d, z_d, bn_d, sums, zp_d, out, dz, outm, part)
    name = _rid(r)
    check(f'{name} sums', sums.cpu(), c.sums64, 'fp32', tol=1e-5)
    dgrad_bb_compare(r, c, out, dz, outm, part)
    # the two-kernel path: dz equal or one bf16 step apart, the data gradient within the kernel bar of each other
    assert (dz.float() - dz_two.float()).abs().max() <= 2.0 ** -7 * dz_two.float().abs().max()
    assert (dz == dz_two).float().mean().item() > 0.9
    check(f'{name} dA_prev vs two-kernel path', from_nhwc(out), from_nhwc(out_two), 'bf16', rel=2.0 ** -7)


# ------------------------------------------------------------------ bf16x3 / bf16x2: split operand, float32 operand
def _split(x_nchw, ipg, mode=IN_PLAIN, bn=None):
    N, C, H, W = x_nchw.shape
    sp = guard.full((N, H, W, 2 * C), NAN, dtype=torch.bfloat16)
    xd, bd = to_nhwc('fp32', x_nchw), (dev(bn) if bn is not None else None)
    _lib.call('bdn_split_pack', xd.data_ptr(), C, None, 0, mode, bd.data_ptr() if bn is not None else None, ipg, sp.data_ptr(), N, H, W, st())
    torch.cuda.synchronize()
    return sp


def _x3_weights(w):
    Cout, Cin = w.shape[:2]
    wf = guard.empty(Cout, 9, 3 * Cin, dtype=torch.bfloat16)
    wd = dev(w)
    _lib.call('bdn_pack_weights', BDN_BF16X3, wd.data_ptr(), wf.data_ptr(), None, Cout, Cin, Cin, st())
    torch.cuda.synchronize()
    return wf


@pytest.mark.parametrize('r', _rows('x3', 'x3src'), ids=_rid)
@guarded
def test_split_product_convolution(r):
    """bf16x3 (three terms: the float32 product to ~2^-16) and bf16x2 (a_hi w_hi + a_lo w_hi = a times the filter rounded to bf16) on the
    split operand (bdn_conv3x3) and on the float32 operand (bdn_conv3x3_x3src, BatchNorm+ReLU on load), with statistics."""
    _assert_variant(r)
    N, H, W, C0, Cout, ipg = r.N, r.H, r.W, r.C0, r.Cout, r.ipg
    c = x3_case(r)
    nt = _lib.load().bdn_conv3x3_num_mtiles_ex(lc.DTYPE[r.prec], N, H, W, C0, Cout, ipg)
    out = guard.full((N, H, W, Cout), NAN)
    stats = guard.full((nt, 2, Cout), NAN) if r.stats else None
    sp_out = guard.full((N, H, W, 2 * C0), NAN, dtype=torch.bfloat16) if r.op == 'x3src' and r.stats else None
    xin = _split(c.x, ipg) if r.op == 'x3' else to_nhwc('fp32', c.x)
    if r.creal:
        _assert_zero_padding(r, xin, halves=2)
    x3_launch(r, c, xin, out, stats, sp_out)
    x3_compare(r, c, out, stats, sp_out)


def x3_case(r):
    """Inputs and float64 reference of an 'x3' / 'x3src' row."""
    N, H, W, C0, Cout, ipg = r.N, r.H, r.W, r.C0, r.Cout, r.ipg
    G = N // ipg
    cr = r.creal or C0
    x = _rand((N, cr, H, W), 311)
    w = _rand((Cout, cr, 3, 3), 312, (2.0 / (9 * cr)) ** 0.5)
    b = _rand((Cout,), 313, 0.1)
    bn = bn_table(G, C0, 314) if r.bnrelu else None
    a = bnrelu_ref('fp32', x, bn, ipg) if r.bnrelu else x
    wr = w if r.prec == 'bf16x3' else w.to(torch.bfloat16).float()
    ref = F.conv2d(a.double(), wr.double(), b.double(), padding=1)
    return SimpleNamespace(x=_padded(x, C0), w=w, b=b, bn=bn, a=a, ref=ref)


def x3_launch(r, c, xin, out, stats, sp_out, N=None, ipg=None):
    """'x3': bdn_conv3x3 on the split operand `xin`; 'x3src': bdn_conv3x3_x3src on the float32 operand `xin`."""
    N, ipg = (r.N if N is None else N), (r.ipg if ipg is None else ipg)
    dt, C0 = lc.DTYPE[r.prec], r.C0
    wf = pack_first(r.prec, c.w, C0) if r.creal else _x3_weights(c.w)
    db = dev(c.b)
    if r.op == 'x3':
        _lib.call('bdn_conv3x3', dt, xin.data_ptr(), C0, None, 0, IN_PLAIN, None, ipg, wf.data_ptr(), db.data_ptr(), out.data_ptr(),
                  stats.data_ptr(), N, r.H, r.W, r.Cout, st())
    else:
        dbn = dev(c.bn) if r.bnrelu else None
        _lib.call('bdn_conv3x3_x3src', dt, xin.data_ptr(), C0, IN_BNRELU if r.bnrelu else IN_PLAIN,
                  dbn.data_ptr() if r.bnrelu else None, ipg, wf.data_ptr(), db.data_ptr(), out.data_ptr(),
                  stats.data_ptr() if r.stats else None, sp_out.data_ptr() if r.stats else None, N, r.H, r.W, r.Cout, st())
    torch.cuda.synchronize()


def x3_compare(r, c, out, stats, sp_out):
    G, C0, Cout = r.N // r.ipg, r.C0, r.Cout
    check(f'{_rid(r)} out', from_nhwc(out), c.ref, 'x3')
    if r.stats:
        nt = stats.shape[0]
        s = stats.cpu().double().reshape(G, nt // G, 2, Cout).sum(1)
        for g, zg in enumerate(_grp(c.ref, G)):
            check(f'{_rid(r)} sum g{g}', s[g, 0], zg.sum((0, 2, 3)), 'x3')
            check(f'{_rid(r)} sumsq g{g}', s[g, 1], (zg * zg).sum((0, 2, 3)), 'x3')
    if sp_out is not None:                      # the split operand left for the weight gradient: hi + lo reproduces relu(bn(x))
        rec = (sp_out[..., :C0].float() + sp_out[..., C0:].float()).cpu().permute(0, 3, 1, 2)
        check(f'{_rid(r)} split operand', rec, c.a.double(), 'x3', tol=2e-5)


# ------------------------------------------------------------------ eval epilogue
def _eval_inputs(r, seed):
    p = r.prec
    cr = r.creal or r.C0
    x0 = rnd(p, _rand((r.N * (2 if r.op == 'eval_pair' else 1), cr, r.H, r.W), seed))
    x1 = rnd(p, _rand((r.N, r.C1, r.H, r.W), seed + 1)) if r.C1 else None
    w = rnd(p, _rand((r.Cout, cr + r.C1, 3, 3), seed + 2, (2.0 / (9 * (cr + r.C1))) ** 0.5))
    sc, sh = _rand((r.Cout,), seed + 3).abs() + 0.5, _rand((r.Cout,), seed + 4, 0.3)
    a = torch.cat([x0, x1], 1) if r.C1 else x0
    act = torch.relu(F.conv2d(a.double(), w.double(), None, padding=1) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None])
    return _padded(x0, r.C0), x1, w, sc, sh, act


def _pool64(t):
    return F.max_pool2d(t, 2)


@pytest.mark.parametrize('r', _rows('eval', 'eval_pair', 'eval_cls'), ids=_rid)
@guarded
def test_eval_stage(r):
    """Eval-mode launches (conv -> folded BatchNorm -> ReLU in the epilogue): the stored activation / date product / pooled maps / logits."""
    _assert_variant(r)
    p = r.prec
    c = eval_case(r)
    d0, d1 = to_nhwc(p, c.x0), (to_nhwc(p, c.x1) if r.C1 else None)
    if r.creal:
        _assert_zero_padding(r, d0)
    outs = eval_outputs(r, r.N)
    eval_launch(r, c, d0, d1, outs)
    eval_compare(r, c, outs)


EVAL_NCLS = 2


def eval_case(r):
    """Inputs and float64 reference of an 'eval' / 'eval_pair' / 'eval_cls' row (host tensors; the filter image is packed at the launch)."""
    x0, x1, w, sc, sh, act = _eval_inputs(r, 401)
    c = SimpleNamespace(x0=x0, x1=x1, w=w, sc=sc, sh=sh, act=act)
    if r.op == 'eval_cls':
        c.cw, c.cb = _rand((EVAL_NCLS, r.Cout), 409, 0.2), _rand((EVAL_NCLS,), 410, 0.1)
    return c


def eval_outputs(r, N, born=False):
    """The NaN-filled outputs of an eval launch of N images (eval_pair: N pairs), by name (born: left as allocated, every byte 0xFF)."""
    td = torch.bfloat16 if r.prec == 'bf16' else torch.float32
    H, W, Cout = r.H, r.W, r.Cout

    def nan(shape, dtype=torch.float32):
        return guard.empty(shape, dtype=dtype) if born else guard.full(shape, NAN, dtype=dtype)
    if r.op == 'eval':
        return {'out': nan((N, H, W, Cout), td), 'pool': nan((N, H // 2, W // 2, Cout), td)}
    if r.op == 'eval_pair':
        return {'f': nan((N, H, W, Cout), td), 'pool': nan((2 * N, H // 2, W // 2, Cout), td)}
    return {'a_out': nan((N, H, W, Cout), td), 'logits': nan((N, EVAL_NCLS, H, W)), 'mask': guard.full((N, H, W), 255, dtype=torch.uint8)}


def eval_launch(r, c, d0, d1, o, N=None):
    N = r.N if N is None else N
    dt, H, W, Cout = lc.DTYPE[r.prec], r.H, r.W, r.Cout
    wf = pack_first(r.prec, c.w, r.C0) if r.creal else pack_w(r.prec, c.w, r.C0 + r.C1)[0]
    dsc, dsh = dev(c.sc), dev(c.sh)
    if r.op == 'eval':
        _lib.call('bdn_conv3x3_eval', dt, d0.data_ptr(), r.C0, d1.data_ptr() if r.C1 else None, r.C1, wf.data_ptr(),
                  dsc.data_ptr(), dsh.data_ptr(), o['out'].data_ptr(), None, o['pool'].data_ptr(), N, H, W, Cout, st())
    elif r.op == 'eval_pair':
        _lib.call('bdn_conv3x3_eval_pair', dt, d0.data_ptr(), r.C0, wf.data_ptr(), dsc.data_ptr(), dsh.data_ptr(), o['f'].data_ptr(),
                  o['pool'].data_ptr(), N, H, W, Cout, st())
    else:
        dcw, dcb = dev(c.cw), dev(c.cb)
        _lib.call('bdn_conv3x3_eval_cls', dt, d0.data_ptr(), r.C0, wf.data_ptr(), dsc.data_ptr(), dsh.data_ptr(), o['a_out'].data_ptr(),
                  dcw.data_ptr(), dcb.data_ptr(), EVAL_NCLS, o['logits'].data_ptr(), o['mask'].data_ptr(), None, 0, 0, N, H, W, Cout, st())
    torch.cuda.synchronize()


def eval_compare(r, c, o):
    p, name, act = r.prec, _rid(r), c.act
    if r.op == 'eval':
        check(f'{name} activation', from_nhwc(o['out']), act, p)
        check(f'{name} pooled', from_nhwc(o['pool']), _pool64(act), p)
    elif r.op == 'eval_pair':
        B = r.N
        # the product of two rounded activations, rounded again: two bf16 roundings in the chain
        check(f'{name} date product', from_nhwc(o['f']), act[:B] * act[B:], p, rel=2.0 ** -7)
        check(f'{name} pooled', from_nhwc(o['pool']), _pool64(act), p)
    else:
        logits = o['logits']
        a_dev = from_nhwc(o['a_out'])
        check(f'{name} activation', a_dev, act, p)
        lref = torch.einsum('nchw,kc->nkhw', a_dev.double(), c.cw.double()) + c.cb.double()[None, :, None, None]
        check(f'{name} logits (of the stored activation)', logits.cpu(), lref, 'fp32', tol=1e-5)
        assert torch.equal(o['mask'].cpu(), (logits[:, 1] > logits[:, 0]).to(torch.uint8).cpu())


# ------------------------------------------------------------------ weight gradient at the production plan
@pytest.mark.parametrize('r', _rows('wgrad'), ids=_rid)
@guarded
def test_weight_gradient(r):
    _assert_variant(r)
    assert lc.reduce_lanes(r) == r.lanes
    run_weight_gradient(r)


def weight_gradient_case(r):
    """Inputs and float64 reference of a 'wgrad' row."""
    N, H, W, C0, C1, Cout, ipg, p = r.N, r.H, r.W, r.C0, r.C1, r.Cout, r.ipg, r.prec
    G = N // ipg
    sp = 'fp32' if p in ('bf16x3', 'bf16x2') else p
    cr = r.creal or C0                                   # wide rows: the gradient of the creal real filter channels
    x0 = rnd(sp, _rand((N, cr, H, W), 21))
    x1 = rnd(sp, _rand((N, C1, H, W), 22)) if C1 else None
    dz = rnd(sp, _rand((N, Cout, H, W), 23))
    bn_in = bn_table(G, C0, 24) if r.bnrelu else None
    a0 = bnrelu_ref(sp, x0, bn_in, ipg) if r.bnrelu else x0
    a = torch.cat([a0, x1], 1) if C1 else a0
    dzr = dz.to(torch.bfloat16).float() if p == 'bf16x2' else dz          # two terms: dz_hi x [a_hi | a_lo]
    ref = torch.nn.grad.conv2d_weight(a.double(), (Cout, cr + C1, 3, 3), dzr.double(), padding=1)
    return SimpleNamespace(x0=_padded(x0, C0), x1=x1, dz=dz, bn_in=bn_in, ref=ref)


def weight_gradient_launch(r, bn_in, ddz, d0, d1, part, dw, flags=3, N=None, ipg=None):
    """bdn_conv3x3_wgrad_ex of a 'wgrad' row on device operands (bf16x3 / bf16x2: ddz and d0 are the split operands of bdn_split_pack)."""
    N, ipg = (r.N if N is None else N), (r.ipg if ipg is None else ipg)
    C0, C1, Cout, dt = r.C0, r.C1, r.Cout, lc.DTYPE[r.prec]
    if r.prec in ('bf16x3', 'bf16x2'):
        assert not r.bnrelu and not C1
        _lib.call('bdn_conv3x3_wgrad_ex', dt, ddz.data_ptr(), Cout, d0.data_ptr(), C0, None, 0, IN_PLAIN, None, ipg,
                  part.data_ptr(), dw.data_ptr(), r.creal or C0, N, r.H, r.W, flags, st())
    else:
        dbn = dev(bn_in) if r.bnrelu else None
        _lib.call('bdn_conv3x3_wgrad_ex', dt, ddz.data_ptr(), Cout, d0.data_ptr(), C0, d1.data_ptr() if C1 else None, C1,
                  IN_BNRELU if r.bnrelu else IN_PLAIN, dbn.data_ptr() if r.bnrelu else None, ipg, part.data_ptr(), dw.data_ptr(), r.creal or C0 + C1,
                  N, r.H, r.W, flags, st())
    torch.cuda.synchronize()


def run_weight_gradient(r, flags=3):
    """The body of test_weight_gradient at plan flags `flags` (tests/test_gpu_bounds.py runs it at other plans and kernels)."""
    lib = _lib.load()
    N, H, W, C0, C1, Cout, ipg, p = r.N, r.H, r.W, r.C0, r.C1, r.Cout, r.ipg, r.prec
    x3 = p in ('bf16x3', 'bf16x2')
    c = weight_gradient_case(r)
    nb = lib.bdn_wgrad_workspace_bytes_ex(lc.DTYPE[p], N, H, W, Cout, C0, C1, ipg, IN_BNRELU if r.bnrelu else IN_PLAIN, flags)
    assert flags != 3 or nb <= lib.bdn_wgrad_workspace_bytes(N, H, W, Cout, C0 + C1, ipg)
    part = guard.empty(nb // 4)
    dw = guard.full((Cout, r.creal or C0 + C1, 3, 3), NAN)          # wide rows: exactly Cout * creal * 9 floats between the guards
    if x3:
        ddz, d0, d1 = _split(c.dz, ipg), _split(c.x0, ipg), None
    else:
        ddz, d0, d1 = to_nhwc(p, c.dz), to_nhwc(p, c.x0), (to_nhwc(p, c.x1) if C1 else None)
    if r.creal:
        _assert_zero_padding(r, d0, halves=2 if x3 else 1)
    weight_gradient_launch(r, c.bn_in, ddz, d0, d1, part, dw, flags)
    check(f'{_rid(r)} dW', dw, c.ref, 'x3' if x3 else 'fp32')


FIRST_LDA, FIRST_CREAL = 80, 13


def first_layer_case(r):
    """Inputs, partial rows and float64 reference of a 'wgrad_bnbwd' row: dz = scale (g - s0/M - xhat s1/M) from the float64 sums (bf16:
    rounded to bf16 like the kernel's staging; bf16x2: dz rounded, x in full), then conv2d_weight."""
    N, H, W, C0, Cout, ipg, p = r.N, r.H, r.W, r.C0, r.Cout, r.ipg, r.prec
    G, M, Creal, ldA = N // ipg, ipg * H * W, FIRST_CREAL, FIRST_LDA
    sp = 'fp32' if p != 'bf16' else 'bf16'
    dA_full = rnd(sp, _rand((N, ldA, H, W), 301))
    z = rnd(sp, _rand((N, Cout, H, W), 302))
    x = rnd(sp, _rand((N, C0, H, W), 303))
    x[:, Creal:] = 0
    bn = _bn_from(z, G, 304)
    gm = dA_full[:, :Cout].double() * (preact(z, bn, ipg) > 0)
    # partial rows the way the producers leave them (sum g, sum g z), four per group
    rows = 4
    part = torch.zeros(G * rows, 2, Cout)
    for g in range(G):
        for q in range(rows):
            sl, hs = slice(g * ipg, (g + 1) * ipg), slice(q * H // rows, (q + 1) * H // rows)
            part[g * rows + q, 0] = gm[sl, :, hs].sum((0, 2, 3)).float()
            part[g * rows + q, 1] = (gm[sl, :, hs] * z[sl, :, hs].double()).sum((0, 2, 3)).float()
    dz64 = torch.empty(N, Cout, H, W, dtype=torch.float64)
    for g in range(G):
        sl = slice(g * ipg, (g + 1) * ipg)
        mean, inv, scale = (bn[g, i].double()[None, :, None, None] for i in range(3))
        pg = part[g * rows:(g + 1) * rows].double().sum(0)
        s0 = pg[0]
        s1 = (pg[1] - bn[g, 0].double() * pg[0]) * bn[g, 1].double()
        xhat = (z[sl].double() - mean) * inv
        dz64[sl] = scale * (gm[sl] - s0[None, :, None, None] / M - xhat * s1[None, :, None, None] / M)
    dzr = dz64 if p == 'bf16x3' else dz64.to(torch.bfloat16).double()
    ref = torch.nn.grad.conv2d_weight(x[:, :Creal].double(), (Cout, Creal, 3, 3), dzr, padding=1)
    return SimpleNamespace(dA_full=dA_full, z=z, x=x, bn=bn, part=part, rows=rows, ref=ref)


def first_layer_launch(r, dA_d, z_d, bn_d, sums, xin, wpart, dw, N=None, ipg=None, ldA=FIRST_LDA):
    """bdn_conv3x3_wgrad_bnbwd on device operands; dA_d [N,H,W,ldA] carries the layer's gradient in its first Cout channels."""
    N, ipg = (r.N if N is None else N), (r.ipg if ipg is None else ipg)
    _lib.call('bdn_conv3x3_wgrad_bnbwd', lc.DTYPE[r.prec], dA_d.data_ptr(), ldA, z_d.data_ptr(), bn_d.data_ptr(),
              sums.data_ptr(), ipg, r.Cout, xin.data_ptr(), r.C0, wpart.data_ptr(), dw.data_ptr(), FIRST_CREAL, N, r.H, r.W, st())
    torch.cuda.synchronize()


@pytest.mark.parametrize('r', _rows('wgrad_bnbwd'), ids=_rid)
@guarded
def test_first_layer_weight_gradient(r):
    """bdn_bn_bwd_finalize + bdn_conv3x3_wgrad_bnbwd (256-block plan, 16 split lanes) against float64: dz = scale (g - s0/M - xhat s1/M)
    from the float64 sums (bf16: rounded to bf16 like the kernel's staging; bf16x2: dz rounded, x in full), then conv2d_weight."""
    _assert_variant(r)
    assert lc.reduce_lanes(r) == r.lanes
    lib = _lib.load()
    N, H, W, C0, Cout, ipg, p = r.N, r.H, r.W, r.C0, r.Cout, r.ipg, r.prec
    G, Creal = N // ipg, FIRST_CREAL
    x3 = p != 'bf16'
    sp = 'fp32' if x3 else 'bf16'
    c = first_layer_case(r)
    sums = guard.full((G, 2, Cout), NAN)
    dg, db = guard.empty(Cout), guard.empty(Cout)
    bn_d, part_d = dev(c.bn), dev(c.part)
    _lib.call('bdn_bn_bwd_finalize', bn_d.data_ptr(), G, Cout, part_d.data_ptr(), c.rows, 1, sums.data_ptr(), dg.data_ptr(), db.data_ptr(),
              None, st())
    xin = _split(c.x, ipg) if x3 else to_nhwc('bf16', c.x)
    wsz = max(lib.bdn_wgrad_workspace_bytes(N, H, W, Cout, C0, ipg), lib.bdn_wgrad_workspace_bytes_ex(lc.DTYPE[p], N, H, W, Cout, C0, 0, ipg, IN_PLAIN, 3))
    wpart = guard.empty(wsz // 4)
    dw = guard.full((Cout, Creal, 3, 3), NAN)
    dA_d, z_d = to_nhwc(sp, c.dA_full), to_nhwc(sp, c.z)
    dA_d[..., Cout:] = NAN                               # the foreign channels of the wider dA: a read of them poisons the result
    first_layer_launch(r, dA_d, z_d, bn_d, sums, xin, wpart, dw)
    check(f'{_rid(r)} dW', dw, c.ref, 'x3' if x3 else 'fp32', tol=2e-4 if x3 else 1e-4)


# ------------------------------------------------------------------ statistics reductions on synthetic partials
@pytest.mark.parametrize('case', lc.STATS_CASES, ids=lambda c: f'rows{c[0]}-G{c[1]}')
@guarded
def test_bn_finalize_reduction(case):
    """bdn_bn_finalize: one launch up to 512 rows per group, reduce_rows_kernel + bn_finalize_kernel above (RS capped at 64)."""
    rpg, G = case
    C, count = 192, 64 * rpg
    lib = _lib.load()
    r = np.random.default_rng(rpg + G)
    mu = r.uniform(-1, 1, (G, 1, C))
    s0 = (mu * 64 + r.standard_normal((G, rpg, C)) * 8).astype(np.float32)
    s1 = ((mu ** 2 + r.uniform(0.5, 2.0, (G, 1, C))) * 64 * r.uniform(0.9, 1.1, (G, rpg, C))).astype(np.float32)
    part = torch.from_numpy(np.stack([s0, s1], 2).reshape(G * rpg, 2, C))
    gamma, beta = _rand((C,), 6).abs() + 0.5, _rand((C,), 7, 0.3)
    rm0, rv0 = _rand((C,), 8, 0.2), _rand((C,), 9).abs() + 0.5
    drm, drv, dgam, dbet, part_d = dev(rm0), dev(rv0), dev(gamma), dev(beta), dev(part)
    nbt = guard.full((1,), 5, dtype=torch.int64)
    bn = guard.full((G, 4, C), NAN)
    fws = guard.full((lib.bdn_bn_finalize_workspace_bytes(G * rpg, G, C) // 8,), NAN, dtype=torch.float64)
    _lib.call('bdn_bn_finalize', part_d.data_ptr(), G * rpg, G, C, count, dgam.data_ptr(), dbet.data_ptr(), 1e-5, 0.1,
              drm.data_ptr(), drv.data_ptr(), nbt.data_ptr(), bn.data_ptr(), fws.data_ptr(), st())
    torch.cuda.synchronize()
    S = part.double().reshape(G, rpg, 2, C).sum(1)
    rm, rv = rm0.double(), rv0.double()
    for g in range(G):
        mean = S[g, 0] / count
        var = S[g, 1] / count - mean * mean
        inv = 1 / torch.sqrt(var + 1e-5)
        check(f'finalize rows{rpg} G{G} mean g{g}', bn[g, 0], mean, 'fp32', tol=1e-6)
        check(f'finalize rows{rpg} G{G} invstd g{g}', bn[g, 1], inv, 'fp32', tol=1e-5)
        check(f'finalize rows{rpg} G{G} scale g{g}', bn[g, 2], gamma.double() * inv, 'fp32', tol=1e-5)
        check(f'finalize rows{rpg} G{G} shift g{g}', bn[g, 3], beta.double() - mean * gamma.double() * inv, 'fp32', tol=1e-5)
        rm = 0.9 * rm + 0.1 * mean
        rv = 0.9 * rv + 0.1 * var * count / (count - 1)
    check(f'finalize rows{rpg} G{G} running_mean', drm, rm, 'fp32', tol=1e-6)
    check(f'finalize rows{rpg} G{G} running_var', drv, rv, 'fp32', tol=1e-6)
    assert int(nbt.item()) == 5 + G


@pytest.mark.parametrize('case', lc.STATS_CASES, ids=lambda c: f'rows{c[0]}-G{c[1]}')
@guarded
def test_bn_bwd_finalize_reduction(case):
    """bdn_bn_bwd_finalize with its scratch (the two-stage row plan above 512 rows per group): sums of g and g xhat (from the raw moment
    sum g z), dgamma and dbeta accumulated over the groups, against float64."""
    rpg, G = case
    C = 256                     # (the entry point takes C dividing 1024)
    lib = _lib.load()
    bn = bn_table(G, C, rpg)
    r = np.random.default_rng(rpg * 3 + G)
    part = torch.from_numpy(r.standard_normal((G * rpg, 2, C)).astype(np.float32) * 4)
    sums = guard.full((G, 2, C), NAN)
    dg, db = guard.full((C,), NAN), guard.full((C,), NAN)
    scratch = guard.full((lib.bdn_bn_bwd_scratch_bytes(G, C) // 8,), NAN, dtype=torch.float64)
    bn_d, part_d = dev(bn), dev(part)
    _lib.call('bdn_bn_bwd_finalize', bn_d.data_ptr(), G, C, part_d.data_ptr(), rpg, 1, sums.data_ptr(), dg.data_ptr(), db.data_ptr(),
              scratch.data_ptr(), st())
    torch.cuda.synchronize()
    S = part.double().reshape(G, rpg, 2, C).sum(1)
    ref = torch.stack([S[:, 0], (S[:, 1] - bn[:, 0].double() * S[:, 0]) * bn[:, 1].double()], 1)
    check(f'bwd finalize rows{rpg} G{G} sum g', sums[:, 0], ref[:, 0], 'fp32', tol=1e-6)
    check(f'bwd finalize rows{rpg} G{G} sum g xhat', sums[:, 1], ref[:, 1], 'fp32', tol=1e-5)
    check(f'bwd finalize rows{rpg} G{G} dbeta', db, ref[:, 0].sum(0), 'fp32', tol=1e-6)
    check(f'bwd finalize rows{rpg} G{G} dgamma', dg, ref[:, 1].sum(0), 'fp32', tol=1e-5)


# ------------------------------------------------------------------ the table is complete: record what real steps launch
def _record(monkeypatch):
    from fabric_amd import engine as engine_mod
    seen = []
    real = _lib.call

    def rec(name, *args):
        if name in lc.MFMA_ENTRY_POINTS:
            seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    monkeypatch.setattr(engine_mod, 'call', rec)
    return seen


def _instantiations(seen):
    out = set()
    for name, args in seen:
        got = lc.call_instantiations(name, args)
        assert got and all(got), (name, args)
        out.update(got)
    return out


_PRECISIONS = ['bf16', 'fp32', 'bf16x3', 'bf16x3-fast']
# (precision, bands, batch, patch side): the benchmarked step (the ids it always had), and small steps of the wide first layer
_STEP_CASES = [(p, 13, 64, 128) for p in _PRECISIONS] + [(p, c, 2, 32) for c in (17, 48) for p in _PRECISIONS]
_STEP_IDS = [p if c == 13 else f'{p}-c{c}' for p, c, _, _ in _STEP_CASES]


@pytest.mark.parametrize('precision,c,B,S', _STEP_CASES, ids=_STEP_IDS)
def test_training_step_launches_equal_the_enumeration(monkeypatch, precision, c, B, S):
    """One real forward + backward of BiDateNet(13, 2) at batch 64, 128 x 128 -- and of BiDateNet(17, 2) and BiDateNet(48, 2) at batch 2,
    32 x 32, whose first layer is padded to 32 and 48 channels and takes bn_bwd + the generic GEMM: the instantiations its MFMA launches
    run equal launch_cases.train_step_instantiations (the hand-written walk cannot drift from the engine), and every one has a row."""
    from fabric_amd import BiDateNet
    torch.manual_seed(0)
    model = BiDateNet(c, 2, precision=precision).cuda().train()
    eng = model.engine()
    if c > 16:
        assert eng.first_wgrad_dtype(2 * B, S, S, B) is None
    P = {k: v.detach() for k, v in model.state_dict(keep_vars=True).items()}
    x1, x2 = torch.randn(B, c, S, S, device='cuda'), torch.randn(B, c, S, S, device='cuda')
    seen = _record(monkeypatch)
    logits, ws = eng.forward(x1, x2, P, training=True)
    grads = {k: torch.empty_like(p) for k, p in model.named_parameters()}
    eng.backward(ws, torch.randn_like(logits) * 1e-3, P, grads)
    torch.cuda.synchronize()
    got = _instantiations(seen)
    want = lc.train_step_instantiations(precision, B, S, n_channels=c)
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert got == want, f'launched but not enumerated: {sorted(got - want)}; enumerated but not launched: {sorted(want - got)}'
    assert not got - lc.covered(), f'no row for {sorted(got - lc.covered())}'


@pytest.mark.parametrize('B,c,S', [(256, 13, 128), (64, 13, 128), (2, 17, 32), (2, 48, 32)], ids=['scene-batch', 'validation', 'c17', 'c48'])
def test_eval_forward_launches_are_covered(monkeypatch, B, c, S):
    """model.eval() forwards (the eval-shaped schedule): a scene-inference batch of 256 tiles of 128 x 128 and a validation batch of 64;
    17 and 48 bands at batch 2, 32 x 32 (the multi-chunk first layer with the eval epilogue)."""
    from fabric_amd import BiDateNet
    torch.manual_seed(0)
    model = BiDateNet(c, 2, precision='bf16').cuda().eval()
    eng = model.engine()
    P = {k: v.detach() for k, v in model.state_dict(keep_vars=True).items()}
    x1, x2 = torch.randn(B, c, S, S, device='cuda'), torch.randn(B, c, S, S, device='cuda')
    seen = _record(monkeypatch)
    eng.forward(x1, x2, P, training=False)
    torch.cuda.synchronize()
    got = _instantiations(seen)
    assert got == lc.eval_forward_instantiations('bf16', B, S, n_channels=c)
    assert not got - lc.covered(), f'no row for {sorted(got - lc.covered())}'
