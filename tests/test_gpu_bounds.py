"""-m gpu: bounds cases on guard-banded buffers (tests/guard.py) that the other parametrizations lack -- odd image counts on two-image
tiles, maps smaller than one tile, weight-gradient plans with ragged last splits at exactly the queried workspace, channel slices of
wider tensors with the foreign channels poisoned, the split producers, the 3x3x3 convolution and the loss kernels called directly.

Every case is compared with the float64 reference its sibling test uses: rows of the launch-shape table run through the bodies of
tests/test_gpu_launch_shapes.py (which ask the library which instantiation the shape selects; here any answer is accepted, the point
is where the launch reads and writes), the rest through the references of tests/test_gpu_kernels.py, tests/test_gpu_input_grad.py and
oracle/bidate_oracle.py.  The sibling bodies carry @guarded themselves, so the thin parametrized wrappers here do not.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X2, BDN_BF16X3, BDN_F32, IN_BNRELU, IN_PLAIN, WG_ROLE, WG_SIMPLE, wg_flags
from oracle import bidate_oracle as O
from tests import guard
from tests import launch_cases as lc
from tests import test_gpu_kernels as tk
from tests import test_gpu_launch_shapes as ls
from tests.guard import guarded
from tests.gpu_util import DT, assert_close, bn_table, dev, from_nhwc, rnd, st, to_nhwc
from tests.test_gpu_input_grad import _dz64, _table

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def _row(op, prec, N, H, W, C0, C1, Cout, ipg, bnrelu=False, stats=True):
    return lc.Row(op, prec, N, H, W, C0, C1, Cout, ipg, bnrelu, stats, None, None)


def _complete(r):
    """The row with the instantiation (and reduction lanes) the library itself names for its shape."""
    r = r._replace(inst=lc.instantiation(r))
    return r._replace(lanes=lc.reduce_lanes(r)) if r.op in ('wgrad', 'wgrad_bnbwd') else r


RUN = {'fwd': ls.test_forward_and_statistics, 'dgrad': ls.test_data_gradient, 'dgrad_bs': ls.test_data_gradient_with_fused_statistics,
       'dgrad_bb': ls.test_data_gradient_with_bn_backward_on_load, 'x3': ls.test_split_product_convolution,
       'x3src': ls.test_split_product_convolution, 'eval': ls.test_eval_stage, 'eval_pair': ls.test_eval_stage,
       'eval_cls': ls.test_eval_stage, 'wgrad': ls.test_weight_gradient, 'wgrad_bnbwd': ls.test_first_layer_weight_gradient}


# ------------------------------------------------------------------ odd image counts on the two-image tiles of 8 x 8 maps
def _odd_rows():
    rows = []
    for N in (3, 5):
        for hw in ((8, 8), (7, 5)):
            rows += [_row('fwd', 'bf16', N, *hw, 512, 0, 512, N, bnrelu=True), _row('fwd', 'fp32', N, *hw, 512, 0, 512, N, bnrelu=True),
                     _row('dgrad', 'bf16', N, *hw, 512, 0, 512, N), _row('dgrad_bs', 'fp32', N, *hw, 512, 0, 512, N),
                     _row('x3', 'bf16x3', N, *hw, 512, 0, 512, N), _row('x3src', 'bf16x3', N, *hw, 512, 0, 512, N, bnrelu=True),
                     _row('eval', 'bf16', N, *hw, 512, 0, 512, 1), _row('eval', 'fp32', N, *hw, 512, 0, 512, 1),
                     _row('eval_pair', 'bf16', N, *hw, 512, 0, 512, 1), _row('eval_pair', 'fp32', N, *hw, 512, 0, 512, 1),
                     _row('wgrad', 'bf16', N, *hw, 512, 0, 512, N, bnrelu=True), _row('wgrad', 'fp32', N, *hw, 512, 0, 512, N, bnrelu=True),
                     _row('wgrad', 'bf16x3', N, *hw, 512, 0, 512, N)]
    # an odd number of images per statistic group: the pair of images that would straddle two groups
    rows += [_row('fwd', 'bf16', 6, 8, 8, 512, 0, 512, 3, bnrelu=True), _row('dgrad_bs', 'fp32', 6, 8, 8, 512, 0, 512, 3),
             _row('wgrad', 'bf16', 6, 8, 8, 512, 0, 512, 3, bnrelu=True)]
    return rows


@pytest.mark.parametrize('r', _odd_rows(), ids=lc.row_id)
def test_odd_image_count_on_two_image_tiles(r):
    """N = 3 and 5 (and an odd count per statistic group) at 512 channels on 8 x 8 maps, where even counts run two images per tile: the
    date-paired eval stage keeps its two-image tiles at every B; the other dispatchers answer an odd count with one-image tiles, and
    whatever they select must stay inside its buffers."""
    r = _complete(r)
    if r.op.startswith('eval') or r.op in ('fwd', 'dgrad', 'dgrad_bs', 'x3', 'x3src'):
        assert (',8,8,2,' if r.op == 'eval_pair' else ',8,16,1,') in r.inst, r.inst
    elif r.prec == 'fp32':
        assert r.inst == 'wgrad_kernel<f32,8,16,1,false>', r.inst
    else:
        assert r.inst.startswith('wgrad7'), r.inst              # the role-split GEMM: 128-pixel chunks, no image pairing
    RUN[r.op](r)


# ------------------------------------------------------------------ maps smaller than one tile
SMALL = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 37), (37, 1), (2, 45)]


def _small_rows():
    """N = 16 in two statistic groups: a group of a 1 x 1 map then still holds 8 values, so its variance is a well-conditioned number and
    the bars of the sibling tests (which assume that) apply; with one or two values per group var + eps is eps and invstd amplifies the
    float32 rounding of the two sums by 1 / eps -- a property of the statistic, not of where a kernel reads."""
    rows = []
    N, ipg = 16, 8
    for H, W in SMALL:
        # 64-wide and 256-wide outputs
        for C0, Cout in ((64, 64), (128, 256)):
            rows += [_row('fwd', 'bf16', N, H, W, C0, 0, Cout, ipg, bnrelu=True), _row('fwd', 'fp32', N, H, W, C0, 0, Cout, ipg),
                     _row('dgrad', 'bf16', N, H, W, 128, 0, Cout, ipg), _row('dgrad_bs', 'bf16', N, H, W, C0, 0, Cout, ipg),
                     _row('wgrad', 'bf16', N, H, W, C0, 0, Cout, ipg, bnrelu=True)]
            if H > 8 or W > 8:                  # bdn_conv3x3_dgrad_bb refuses maps of 8 x 8 and below
                rows += [_row('dgrad_bb', 'bf16', N, H, W, 64, 0, Cout, ipg)]
            if H >= 2 and W >= 2:               # the pooled map of the eval stage needs one 2 x 2 window
                rows += [_row('eval', 'bf16', N, H, W, C0, 0, Cout, 1), _row('eval_pair', 'bf16', N // 2, H, W, C0, 0, Cout, 1)]
        rows += [_row('fwd', 'bf16', N, H, W, 16, 0, 64, ipg), _row('wgrad', 'fp32', N, H, W, 16, 0, 64, ipg),
                 # (the fused first-layer kernel takes one-image tiles only, which small maps get at an odd count per group)
                 _row('wgrad_bnbwd', 'bf16', 14, H, W, 16, 0, 64, 7), _row('wgrad_bnbwd', 'bf16x3', 14, H, W, 16, 0, 64, 7)]
    return rows


@pytest.mark.parametrize('r', _small_rows(), ids=lc.row_id)
def test_maps_smaller_than_one_tile(r):
    """H or W of 1 and 2: every tile is ragged on both sides, the statistics partials are guarded at exactly num_mtiles rows.  These maps
    get the 8-row tiles (8 x 8 x 2, 8 x 16) at every width: the 16 x 16 tiles start at 12 x 12, see the next test."""
    RUN[r.op](_complete(r))


# ------------------------------------------------------------------ one 16 x 16 tile, ragged on both sides
def _tile16_rows():
    rows = []
    for H, W in ((12, 12), (13, 15)):
        N, g = 4, 2
        rows += [_row('fwd', 'bf16', N, H, W, 64, 0, 64, g, bnrelu=True), _row('fwd', 'bf16', N, H, W, 128, 64, 64, g),       # single chunk, two chunks
                 _row('fwd', 'fp32', N, H, W, 64, 0, 64, g, bnrelu=True), _row('fwd', 'bf16', N, H, W, 16, 0, 64, g),
                 _row('dgrad', 'bf16', N, H, W, 128, 0, 64, g), _row('dgrad_bs', 'bf16', N, H, W, 64, 0, 64, g),
                 _row('dgrad_bs', 'bf16', N, H, W, 128, 0, 64, g), _row('dgrad_bs', 'fp32', N, H, W, 64, 0, 64, g),
                 _row('dgrad_bb', 'bf16', N, H, W, 64, 0, 64, g),
                 _row('eval', 'bf16', N, H, W, 64, 0, 64, 1), _row('eval', 'bf16', N, H, W, 128, 64, 64, 1), _row('eval', 'fp32', N, H, W, 16, 0, 64, 1),
                 _row('eval_cls', 'bf16', N, H, W, 64, 0, 64, 1), _row('eval_cls', 'fp32', N, H, W, 64, 0, 64, 1),
                 _row('eval_pair', 'bf16', N, H, W, 64, 0, 64, 1), _row('eval_pair', 'bf16', N, H, W, 128, 0, 64, 1),
                 _row('eval_pair', 'fp32', N, H, W, 128, 0, 64, 1)]
    return rows


@pytest.mark.parametrize('r', _tile16_rows(), ids=lc.row_id)
def test_maps_smaller_than_one_16x16_tile(r):
    """The dispatcher gives 64-wide outputs 16 x 16 tiles only from 12 x 12 on (below that the 8-row tiles of the test above run: the
    16 x 16 kernels cannot be reached on smaller maps), so 12 x 12 and 13 x 15 are the maps smaller than one such tile: one tile per
    image, ragged on both sides.  Every row must run a 16 x 16 x 1 instantiation -- the date-paired eval stage its 8 x 16 x 2 one."""
    r = _complete(r)
    assert (',8,16,2,' if r.op == 'eval_pair' else ',16,16,1,') in r.inst, r.inst
    RUN[r.op](r)


# ------------------------------------------------------------------ weight-gradient plans at exactly the queried workspace
PLAN_ROWS = [_row('wgrad', 'bf16', 4, 29, 45, 64, 0, 64, 2, bnrelu=True), _row('wgrad', 'bf16', 4, 29, 45, 64, 64, 128, 2),
             _row('wgrad', 'bf16', 3, 37, 53, 128, 0, 128, 3, bnrelu=True), _row('wgrad', 'bf16', 2, 9, 17, 64, 0, 64, 1),
             # 8 x 8 maps with an odd image count, both kernel families (the one-chunk-at-a-time family answers with its one-image tiles)
             _row('wgrad', 'bf16', 3, 8, 8, 512, 0, 512, 3, bnrelu=True), _row('wgrad', 'bf16', 5, 8, 8, 512, 0, 512, 5)]
X3_ROWS = [_row('wgrad', 'bf16x3', 4, 29, 45, 128, 0, 128, 2), _row('wgrad', 'bf16x2', 4, 29, 45, 64, 0, 64, 2),
           _row('wgrad', 'bf16x3', 2, 9, 17, 64, 0, 64, 1), _row('wgrad', 'fp32', 4, 29, 45, 64, 0, 64, 2, bnrelu=True)]


@pytest.mark.parametrize('blocks', [0, 7, 1], ids=lambda b: f'blocks{b}')
@pytest.mark.parametrize('kernel', [0, WG_SIMPLE, WG_ROLE], ids=['default', 'simple', 'role'])
@pytest.mark.parametrize('r', PLAN_ROWS, ids=lc.row_id)
def test_weight_gradient_plans_stay_inside_their_workspace(r, kernel, blocks):
    """bdn_conv3x3_wgrad_ex at default flags and at block targets that leave a ragged last split (7) or one split for every chunk (1),
    both kernel families; the workspace holds exactly bdn_wgrad_workspace_bytes_ex bytes, 0xFF-filled."""
    fl = wg_flags(3, kernel, blocks)
    if kernel:
        assert _lib.load().bdn_conv3x3_wgrad_variant(lc.DTYPE[r.prec], r.N, r.H, r.W, r.Cout, r.C0, r.C1, r.ipg,
                                                     IN_BNRELU if r.bnrelu else IN_PLAIN, fl) == kernel
    guarded(ls.run_weight_gradient)(r, fl)


@pytest.mark.parametrize('blocks', [0, 7], ids=lambda b: f'blocks{b}')
@pytest.mark.parametrize('r', X3_ROWS, ids=lc.row_id)
def test_split_and_float32_weight_gradient_plans(r, blocks):
    guarded(ls.run_weight_gradient)(r, wg_flags(3, 0, blocks))


# ------------------------------------------------------------------ dA as a 64-channel slice of a 128-channel tensor
def _bn_case(prec, N, H, W, ipg, off, seed, frozen=False):
    """Inputs of the BatchNorm-backward family with dA at channels [off, off + 64) of a 128-channel tensor whose other half is NaN, and
    the float64 results: g under the ReLU mask, the sums, dz, dgamma / dbeta."""
    C, G = 64, N // ipg
    dA = rnd(prec, _rand((N, H, W, C), seed))
    z = rnd(prec, _rand((N, H, W, C), seed + 1))
    tab = _table(1, C, seed + 2).repeat(G, 1, 1) if frozen else _table(G, C, seed + 2)
    t = tab.double().repeat_interleave(ipg, 0)[:, :, None, None, :]
    mean, inv, sc, sh = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    mask = torch.addcmul(sh.float().expand(N, H, W, C), z, sc.float().expand(N, H, W, C)) > 0         # one float32 FMA, as the kernels form it
    g = torch.where(mask, dA.double(), torch.zeros((), dtype=torch.float64))
    xhat = (z.double() - mean) * inv
    s0 = g.reshape(G, -1, C).sum(1)
    s1 = (g * xhat).reshape(G, -1, C).sum(1)
    s1raw = (g * z.double()).reshape(G, -1, C).sum(1)
    sums = torch.stack([s0, s1], 1)                                                       # [G][2][C]
    dz = sc * g if frozen else _dz64(dA, z, tab, sums, ipg)
    td = DT[prec][1]
    wide, _ = guard.wide_input(dA.to(td), 128, off, label=f'dA in channels [{off},{off + 64}) of 128')
    return dict(C=C, G=G, dA=dA, z=z, tab=tab, g=g, sums=sums, s1raw=s1raw, dz=dz, dgamma=s1.sum(0), dbeta=s0.sum(0),
                dA_ptr=wide.data_ptr() + off * wide.element_size(), wide=wide, z_d=guard.guard(z.to(td)), tab_d=dev(tab),
                dbias=(tab[0, 2].double() * s0.sum(0)))


def _partial_rows(c, rows, H):
    """[G * rows][2][C] partial sums (sum g, sum g z) over bands of image rows, the way the fused producers leave them."""
    G, C = c['G'], c['C']
    g, z = c['g'].reshape(G, -1, H, c['g'].shape[2], C), c['z'].double().reshape(G, -1, H, c['z'].shape[2], C)
    part = torch.zeros(G * rows, 2, C)
    for gi in range(G):
        for q in range(rows):
            hs = slice(q * H // rows, (q + 1) * H // rows)
            part[gi * rows + q, 0] = g[gi][:, hs].sum((0, 1, 2)).float()
            part[gi * rows + q, 1] = (g[gi][:, hs] * z[gi][:, hs]).sum((0, 1, 2)).float()
    return part


SLICE_SHAPES = [(4, 12, 20, 2), (2, 9, 7, 1), (3, 33, 17, 3)]


@pytest.mark.parametrize('off', [0, 64], ids=['lower64', 'upper64'])
@pytest.mark.parametrize('shape', SLICE_SHAPES, ids=lambda s: 'x'.join(map(str, s[:3])) + f'-g{s[3]}')
@pytest.mark.parametrize('prec,entry', [(p, e) for e in ('bn_bwd', 'bn_bwd_apply', 'bn_bwd_apply_split', 'bn_bwd_frozen', 'bn_bwd_apply_frozen')
                                        for p in ('fp32', 'bf16') if (p, e) != ('bf16', 'bn_bwd_apply_split')])        # the split form takes float32 only
@guarded
def test_bn_backward_reads_only_its_slice_of_dA(prec, entry, shape, off):
    """ldA = 128, the upper and the lower 64 channels, the other 64 NaN; dz, sums, dgamma, dbeta against float64 at the bars of
    test_bn_bwd (1e-4 of the magnitude; dz of bf16 storage 1e-2).  Workspaces and scratch at exactly the queried bytes."""
    N, H, W, ipg = shape
    dt, td = DT[prec]
    frozen = entry.endswith('frozen')
    c = _bn_case(prec, N, H, W, ipg, off, 900 + off + N, frozen)
    C, G = c['C'], c['G']
    lib = _lib.load()
    sums = guard.full((G, 2, C), NAN)
    dg, db, dbias = guard.full((C,), NAN), guard.full((C,), NAN), guard.full((C,), NAN)
    split = entry == 'bn_bwd_apply_split'
    dz = guard.full((N, H, W, 2 * C if split else C), NAN, dtype=torch.bfloat16 if split else td)
    rows = 3
    if 'apply' in entry:
        part = dev(_partial_rows(c, rows, H))
        scratch = guard.alloc_bytes(lib.bdn_bn_bwd_scratch_bytes(G, C), label='bn_bwd scratch')
    else:
        ws = guard.alloc_bytes(lib.bdn_bn_bwd_workspace_bytes(dt, N, H, W, C, ipg), label='bn_bwd workspace')
    if entry == 'bn_bwd':
        _lib.call('bdn_bn_bwd', dt, c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), ipg, N, H, W, C, ws.data_ptr(), sums.data_ptr(),
                  dg.data_ptr(), db.data_ptr(), dz.data_ptr(), st())
    elif entry == 'bn_bwd_frozen':
        _lib.call('bdn_bn_bwd_frozen', dt, c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), ipg, N, H, W, C, ws.data_ptr(),
                  sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dbias.data_ptr(), dz.data_ptr(), st())
    elif entry == 'bn_bwd_apply':
        _lib.call('bdn_bn_bwd_apply', dt, c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), ipg, N, H, W, C, part.data_ptr(), rows, 1,
                  sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dz.data_ptr(), scratch.data_ptr(), st())
    elif entry == 'bn_bwd_apply_split':
        _lib.call('bdn_bn_bwd_apply_split', c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), ipg, N, H, W, C, part.data_ptr(), rows, 1,
                  sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dz.data_ptr(), scratch.data_ptr(), st())
    else:
        _lib.call('bdn_bn_bwd_apply_frozen', dt, c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), ipg, N, H, W, C, part.data_ptr(),
                  rows, 1, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dbias.data_ptr(), dz.data_ptr(), scratch.data_ptr(), st())
    torch.cuda.synchronize()
    got = dz.float().cpu()
    if split:
        got = got[..., :C] + got[..., C:]
    assert_close(f'{entry} dz', got, c['dz'].float(), 1e-2 if prec == 'bf16' else 1e-4)
    assert_close(f'{entry} dbeta', db.cpu(), c['dbeta'].float(), 1e-4)
    assert_close(f'{entry} dgamma', dg.cpu(), c['dgamma'].float(), 1e-4)
    if frozen:
        assert torch.equal(sums.cpu(), torch.zeros(G, 2, C))
        assert_close(f'{entry} dbias', dbias.cpu(), c['dbias'].float(), 1e-4)
    else:
        assert_close(f'{entry} sums', sums.cpu(), c['sums'].float(), 1e-4)
    assert torch.isnan(c['wide'][..., 64 - off:128 - off]).all()          # the poison is still where it was put


@pytest.mark.parametrize('off', [0, 64], ids=['lower64', 'upper64'])
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 24, 20, 13), (1, 5, 5, 3), (3, 9, 33, 13)], ids=lambda s: 'x'.join(map(str, s)))
@guarded
def test_dgrad_first_reads_only_its_slice_of_dA(shape, prec, off):
    """bdn_conv3x3_dgrad_first with dz formed on load from a dA slice (ldA = 128); reference and bar of test_dgrad_first_matches_float64."""
    B, H, W, cr = shape
    dt, td = DT[prec]
    N = 2 * B
    c = _bn_case(prec, N, H, W, B, off, 700 + off + B)
    w = _rand((64, cr, 3, 3), 77, 0.05)
    ref = torch.nn.grad.conv2d_input((N, cr, H, W), w.double(), c['dz'].permute(0, 3, 1, 2), padding=1)
    dx1, dx2 = guard.full((B, cr, H, W), NAN), guard.full((B, cr, H, W), NAN)
    dsums, dw = dev(c['sums'].float()), dev(w)
    _lib.call('bdn_conv3x3_dgrad_first', dt, c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), dsums.data_ptr(), B,
              dw.data_ptr(), cr, dx1.data_ptr(), dx2.data_ptr(), B, H, W, st())
    torch.cuda.synchronize()
    tol = {'fp32': 2e-5, 'bf16': 1e-2}[prec]
    assert_close('dx1', dx1.cpu(), ref[:B], tol)
    assert_close('dx2', dx2.cpu(), ref[B:], tol)


@pytest.mark.parametrize('off', [0, 64], ids=['lower64', 'upper64'])
@pytest.mark.parametrize('prec', ['bf16', 'bf16x3', 'bf16x2'])
@pytest.mark.parametrize('shape', [(4, 29, 45, 2), (4, 24, 16, 2), (2, 9, 7, 1)], ids=lambda s: 'x'.join(map(str, s[:3])) + f'-g{s[3]}')
@guarded
def test_first_layer_wgrad_reads_only_its_slice_of_dA(shape, prec, off):
    """bdn_conv3x3_wgrad_bnbwd with ldA = 128 at the bars of test_first_layer_weight_gradient.  bf16x3: dz in float64 from the float64 sums.
    bf16 / bf16x2 stage bf16(dz) of a float32 dz, and one element that rounds the other way than the rounded float64 value moves dW of
    these small maps by more than that bar; so their dz is the one bdn_bn_bwd_apply / bdn_bn_bwd_apply_split store from the same slice
    (held against float64 by test_bn_backward_reads_only_its_slice_of_dA, and again here), and the reference is its float64 weight gradient."""
    N, H, W, ipg = shape
    Cout, C0, Creal = 64, 16, 13
    x3 = prec != 'bf16'
    sp = 'fp32' if x3 else 'bf16'
    lib = _lib.load()
    assert lib.bdn_conv3x3_wgrad_bnbwd_supported(lc.DTYPE[prec], N, H, W, Cout, C0, ipg) == 1
    c = _bn_case(sp, N, H, W, ipg, off, 500 + off + N)
    G = c['G']
    x = rnd(sp, _rand((N, C0, H, W), 503))
    x[:, Creal:] = 0
    # the unfused path on the same slice: sums for the fused kernel, and the stored dz
    rows = 3
    part = dev(_partial_rows(c, rows, H))
    sums, dg, db = guard.full((G, 2, Cout), NAN), guard.full((Cout,), NAN), guard.full((Cout,), NAN)
    if x3:
        dzs = guard.full((N, H, W, 2 * Cout), NAN, dtype=torch.bfloat16)
        _lib.call('bdn_bn_bwd_apply_split', c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), ipg, N, H, W, Cout, part.data_ptr(), rows, 1,
                  sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dzs.data_ptr(), None, st())
    else:
        dzs = guard.full((N, H, W, Cout), NAN, dtype=torch.bfloat16)
        _lib.call('bdn_bn_bwd_apply', BDN_BF16, c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), ipg, N, H, W, Cout, part.data_ptr(), rows, 1,
                  sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dzs.data_ptr(), None, st())
    xin = ls._split(x, ipg) if x3 else to_nhwc('bf16', x)
    wsz = max(lib.bdn_wgrad_workspace_bytes(N, H, W, Cout, C0, ipg),
              lib.bdn_wgrad_workspace_bytes_ex(lc.DTYPE[prec], N, H, W, Cout, C0, 0, ipg, IN_PLAIN, 3))
    wpart = guard.alloc_bytes(wsz, label='wgrad workspace')
    dw = guard.full((Cout, Creal, 3, 3), NAN)
    _lib.call('bdn_conv3x3_wgrad_bnbwd', lc.DTYPE[prec], c['dA_ptr'], 128, c['z_d'].data_ptr(), c['tab_d'].data_ptr(), sums.data_ptr(), ipg,
              Cout, xin.data_ptr(), C0, wpart.data_ptr(), dw.data_ptr(), Creal, N, H, W, st())
    torch.cuda.synchronize()
    assert_close('sums', sums.cpu(), c['sums'].float(), 1e-4)
    stored = dzs.float().cpu()
    assert_close('stored dz', stored[..., :Cout] + stored[..., Cout:] if x3 else stored, c['dz'].float(), 1e-4 if x3 else 1e-2)
    dzr = c['dz'] if prec == 'bf16x3' else stored[..., :Cout].double()          # bf16x2: the hi term of dz, x in full
    ref = torch.nn.grad.conv2d_weight(x[:, :Creal].double(), (Cout, Creal, 3, 3), dzr.permute(0, 3, 1, 2), padding=1)
    ls.check(f'wgrad_bnbwd {prec} dW', dw, ref, 'x3' if x3 else 'fp32', tol=2e-4 if x3 else 1e-4)


# ------------------------------------------------------------------ ldF / ldU (the sibling tests poison the foreign channels themselves)
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', [(1, 1, 1, 64, False), (2, 2, 3, 64, True), (1, 37, 2, 128, True), (3, 7, 19, 64, True)], ids=str)
def test_enc_skip_bwd_reads_only_its_slice_of_dF(prec, case):
    tk.test_enc_skip_bwd(prec, case)


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', [(1, 1, 2, 2, 4, 64), (3, 2, 1, 5, 3, 64), (1, 17, 9, 35, 19, 128), (2, 16, 16, 32, 32, 64)], ids=str)
def test_upsample2x_bwd_reads_only_its_slice_of_dU(prec, case):
    """bdn_upsample2x_bwd and, where the tiled kernel takes the shape, bdn_upsample2x_bwd_bs (ldU = C + 16, the slice at channel 16)."""
    tk.test_upsample2x_and_backward(prec, case, False)


# ------------------------------------------------------------------ the split producers write only the channels they own
@pytest.mark.parametrize('shape', [(2, 24, 20, 64, 128), (1, 7, 5, 64, 64), (3, 2, 2, 128, 256), (1, 45, 22, 64, 128)], ids=str)
@guarded
def test_split_producers_leave_foreign_channels_alone(shape):
    """bdn_product_pool_split owns channels [0, C) and [Ct, Ct + C) of the [hi | lo] operand of the decoder's [f | U] (2 Ct wide),
    bdn_upsample2x_split [C, Ct) and [Ct + C, 2 Ct): each alone into a 0xFF-filled operand leaves the other's channels bit for bit, and
    what it writes equals bdn_split_pack of the float32 producers (the reference of test_split_outputs_of_the_bf16x3_producers...)."""
    B, H, W, C, Cu = shape
    Ct = C + Cu
    h, w = H // 2, W // 2
    z_d, bn_d = to_nhwc('fp32', _rand((2 * B, C, H, W), 81)), dev(bn_table(2, C, 82))
    src, bnu = to_nhwc('fp32', _rand((B, Cu, max(h, 1), max(w, 1)), 83)), dev(bn_table(1, Cu, 84))
    hs, ws_ = src.shape[1], src.shape[2]
    f, pool = guard.full((B, H, W, C), NAN), guard.full((2 * B, h, w, C), NAN)
    _lib.call('bdn_product_pool', BDN_F32, z_d.data_ptr(), bn_d.data_ptr(), f.data_ptr(), pool.data_ptr(), B, H, W, C, st())
    U = guard.full((B, H, W, Cu), NAN)
    _lib.call('bdn_upsample2x', BDN_F32, src.data_ptr(), IN_BNRELU, bnu.data_ptr(), U.data_ptr(), B, hs, ws_, H, W, Cu, st())
    ref_cat = guard.full((B, H, W, 2 * Ct), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_split_pack', f.data_ptr(), C, U.data_ptr(), Cu, IN_PLAIN, None, B, ref_cat.data_ptr(), B, H, W, st())
    ref_pool = guard.full((2 * B, h, w, 2 * C), NAN, dtype=torch.bfloat16)
    if h and w:
        _lib.call('bdn_split_pack', pool.data_ptr(), C, None, 0, IN_PLAIN, None, B, ref_pool.data_ptr(), 2 * B, h, w, st())
    own_f = torch.zeros(2 * Ct, dtype=torch.bool)
    own_f[:C] = own_f[Ct:Ct + C] = True
    a = guard.empty(B, H, W, 2 * Ct, dtype=torch.bfloat16, label='[f | U] operand, product_pool_split alone')
    b = guard.empty(B, H, W, 2 * Ct, dtype=torch.bfloat16, label='[f | U] operand, upsample2x_split alone')
    got_pool = guard.empty(2 * B, h, w, 2 * C, dtype=torch.bfloat16)
    _lib.call('bdn_product_pool_split', z_d.data_ptr(), bn_d.data_ptr(), a.data_ptr(), 2 * Ct, Ct, got_pool.data_ptr(), B, H, W, C, st())
    _lib.call('bdn_upsample2x_split', src.data_ptr(), IN_BNRELU, bnu.data_ptr(), b.data_ptr(), 2 * Ct, C, Ct, B, hs, ws_, H, W, Cu, st())
    torch.cuda.synchronize()
    ai, bi, ri = a.view(torch.int16).cpu(), b.view(torch.int16).cpu(), ref_cat.view(torch.int16).cpu()
    assert torch.equal(ai[..., own_f], ri[..., own_f]) and torch.equal(bi[..., ~own_f], ri[..., ~own_f])
    guard.assert_foreign_untouched(a, [(0, C), (Ct, C)], 'bdn_product_pool_split')
    guard.assert_foreign_untouched(b, [(C, Cu), (Ct + C, Cu)], 'bdn_upsample2x_split')
    assert torch.equal(got_pool.view(torch.int16), ref_pool.view(torch.int16))


# ------------------------------------------------------------------ 3x3x3 convolution, called directly
def _ndhwc(x_ncdhw, cp, td):
    n, c, d, h, w = x_ncdhw.shape
    out = torch.zeros(n, d, h, w, cp, dtype=td)
    out[..., :c] = x_ncdhw.permute(0, 2, 3, 4, 1).to(td)
    return guard.guard(out)


def _split3d(x_d, c, n_img):
    n, d, h, w, _ = x_d.shape
    sp = guard.full((n, d, h, w, 2 * c), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_split_pack', x_d.data_ptr(), c, None, 0, IN_PLAIN, None, n_img, sp.data_ptr(), n * d, h, w, st())
    return sp


@pytest.mark.parametrize('prec', ['fp32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('case', [(1, 1, 8, 16, 64, 64), (2, 1, 9, 7, 13, 64), (2, 2, 5, 19, 64, 64), (3, 2, 8, 8, 64, 128), (1, 2, 1, 2, 13, 64)], ids=str)
@guarded
def test_conv3d_called_directly(prec, case):
    """bdn_conv3d (forward + statistics, data gradient) and bdn_conv3d_wgrad through the calling sequence of fabric_amd/conv3d.py at
    D = 1 and D = 2 (every slice is a depth border: the block-uniform zero masks between consecutive samples), against
    torch.nn.functional.conv3d / torch.nn.grad in float64 at the bars of tests/test_gpu_conv3d.py; the first and the last sample are
    checked on their own -- what lies before the first and behind the last is guard."""
    N, D, H, W, Cin, Cout = case
    lib = _lib.load()
    x3 = prec == 'bf16x3'
    sp_ = 'bf16' if prec == 'bf16' else 'fp32'
    dt, td = DT[sp_]
    cp = (Cin + 15) // 16 * 16
    x = rnd(sp_, _rand((N, Cin, D, H, W), 1))
    w = rnd(sp_, _rand((Cout, Cin, 3, 3, 3), 2, 0.1))
    b = _rand((Cout,), 3)
    dz = rnd(sp_, _rand((N, Cout, D, H, W), 4))
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    rdx = torch.nn.grad.conv3d_input(x.shape, w.double(), dz.double(), padding=1)
    rdw = torch.nn.grad.conv3d_weight(x.double(), w.shape, dz.double(), padding=1)
    wp = torch.zeros(Cout, cp, 3, 3, 3)
    wp[:, :Cin] = w
    xd, dzd, bd = _ndhwc(x, cp, td), _ndhwc(dz, Cout, td), dev(b)
    out = guard.full((N, D, H, W, Cout), NAN, dtype=td)
    part = guard.full((lib.bdn_conv3d_num_mtiles(N, D, H, W), 2, Cout), NAN)
    dx = guard.full((N, D, H, W, cp), NAN, dtype=td) if cp % 64 == 0 else None
    dw = guard.full((Cout, Cin, 3, 3, 3), NAN)
    if x3:
        hi = wp.to(torch.bfloat16).float()
        w3 = torch.stack([hi, hi, wp - hi], 0)
        wf = guard.empty(Cout, 9, 9 * cp, dtype=torch.bfloat16)
        fwd = dev(w3.permute(1, 3, 0, 2, 4, 5).reshape(Cout, 9 * cp, 3, 3))
        _lib.call('bdn_pack_weights', BDN_BF16, fwd.data_ptr(), wf.data_ptr(), None, Cout, 9 * cp, 9 * cp, st())
        sx, sd = _split3d(xd, cp, N * D), _split3d(dzd, Cout, N * D)
        op = guard.guard(torch.cat([sx, sx[..., :cp]], -1))
        _lib.call('bdn_conv3d', BDN_BF16X3, op.data_ptr(), 3 * cp, IN_PLAIN, None, N, wf.data_ptr(), bd.data_ptr(), out.data_ptr(), part.data_ptr(),
                  N, D, H, W, Cout, st())
        if dx is not None:
            wd = guard.empty(cp, 9, 9 * Cout, dtype=torch.bfloat16)
            back = dev(w3.flip(3, 4, 5).permute(2, 3, 0, 1, 4, 5).reshape(cp, 9 * Cout, 3, 3))
            _lib.call('bdn_pack_weights', BDN_BF16, back.data_ptr(), wd.data_ptr(), None, cp, 9 * Cout, 9 * Cout, st())
            opd = guard.guard(torch.cat([sd, sd[..., :Cout]], -1))
            _lib.call('bdn_conv3d', BDN_BF16X3, opd.data_ptr(), 3 * Cout, IN_PLAIN, None, N, wd.data_ptr(), None, dx.data_ptr(), None,
                      N, D, H, W, cp, st())
        nb = lib.bdn_wgrad_workspace_bytes_ex(BDN_BF16, N * D, H, W, 2 * Cout, 2 * cp, 0, 1, IN_PLAIN, 0) + 4 * Cout * cp * 27 * 4
        ws = guard.alloc_bytes(nb, label='conv3d_wgrad workspace')
        _lib.call('bdn_conv3d_wgrad', BDN_BF16X3, sd.data_ptr(), Cout, sx.data_ptr(), cp, ws.data_ptr(), dw.data_ptr(), Cin, N, D, H, W, st())
    else:
        wf = guard.empty(Cout, 9, 3 * cp, dtype=td)
        fwd = dev(wp.permute(0, 2, 1, 3, 4).reshape(Cout, 3 * cp, 3, 3))
        _lib.call('bdn_pack_weights', dt, fwd.data_ptr(), wf.data_ptr(), None, Cout, 3 * cp, 3 * cp, st())
        _lib.call('bdn_conv3d', dt, xd.data_ptr(), cp, IN_PLAIN, None, N, wf.data_ptr(), bd.data_ptr(), out.data_ptr(), part.data_ptr(),
                  N, D, H, W, Cout, st())
        if dx is not None:
            wd = guard.empty(cp, 9, 3 * Cout, dtype=td)
            back = dev(wp.flip(2, 3, 4).permute(1, 2, 0, 3, 4).reshape(cp, 3 * Cout, 3, 3))
            _lib.call('bdn_pack_weights', dt, back.data_ptr(), wd.data_ptr(), None, cp, 3 * Cout, 3 * Cout, st())
            _lib.call('bdn_conv3d', dt, dzd.data_ptr(), Cout, IN_PLAIN, None, N, wd.data_ptr(), None, dx.data_ptr(), None, N, D, H, W, cp, st())
        nb = lib.bdn_wgrad_workspace_bytes_ex(dt, N * D, H, W, Cout, cp, 0, 1, IN_PLAIN, 0)
        ws = guard.alloc_bytes(nb, label='conv3d_wgrad workspace')
        _lib.call('bdn_conv3d_wgrad', dt, dzd.data_ptr(), Cout, xd.data_ptr(), cp, ws.data_ptr(), dw.data_ptr(), Cin, N, D, H, W, st())
    torch.cuda.synchronize()
    tol = 1e-2 if prec == 'bf16' else (1e-4 if x3 else 2e-5)
    got = out.float().cpu().permute(0, 4, 1, 2, 3)
    assert_close('conv3d', got, ref.float(), tol)
    for n in (0, N - 1):                                    # the first and the last sample against their own magnitude
        assert_close(f'conv3d sample {n}', got[n], ref[n].float(), tol)
    s = part[:, 0].double().sum(0).cpu()
    want = ref.sum((0, 2, 3, 4))
    assert torch.isfinite(part).all()
    assert (s - want).abs().max() <= (2e-2 if prec == 'bf16' else 1e-4) * want.abs().max() + 1e-2
    if dx is not None:
        gdx = dx.float().cpu().permute(0, 4, 1, 2, 3)
        assert_close('conv3d dgrad', gdx[:, :Cin], rdx.float(), tol)
        for n in (0, N - 1):
            assert_close(f'conv3d dgrad sample {n}', gdx[n, :Cin], rdx[n].float(), tol)
    assert_close('conv3d wgrad', dw.cpu(), rdw.float(), 1e-2 if prec == 'bf16' else 1e-4)


# ------------------------------------------------------------------ loss kernels, called directly
LOSS_SHAPES = [(3, 2, 7, 5), (1, 2, 3, 3), (2, 3, 9, 13), (5, 2, 11, 7), (1, 8, 5, 6), (2, 2, 1, 1)]          # W % 4 != 0, B*H*W % 16 != 0
LOSS_TOL, GRAD_TOL = 5e-6, 3e-4                            # tests/test_gpu_losses.py: test_losses_match_oracle_on_other_shapes


def _loss_inputs(shape, seed):
    B, C, H, W = shape
    assert W % 4 and (B * H * W) % 16
    r = np.random.default_rng(seed)
    logits = torch.from_numpy((3 * r.standard_normal(shape)).astype(np.float32))
    labels = torch.from_numpy(r.integers(0, C, (B, H, W)).astype(np.int64))
    return logits, labels


def _counts(logits, labels):
    pred = logits.argmax(1)
    return [int(((pred == 1) & (labels == 1)).sum()), int(((pred == 1) & (labels != 1)).sum()),
            int(((pred != 1) & (labels == 1)).sum()), int((pred == labels).sum())]


@pytest.mark.parametrize('entry,reduce_w', [('tversky', 0), ('overlap', 0), ('overlap', 1)])      # bdn_tversky is the [B,H,W] form: no reduce_w
@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=str)
@guarded
def test_overlap_loss_kernels_called_directly(shape, entry, reduce_w):
    """bdn_tversky ([B,H,W] labels: the (0,2)-dims reduction) and bdn_overlap_loss (both reductions) on the workspace of exactly
    bdn_overlap_workspace_bytes, against oracle.tversky_loss in float64."""
    B, C, H, W = shape
    logits, labels = _loss_inputs(shape, 31)
    lo = logits.double().requires_grad_(True)
    ref = O.tversky_loss(lo, labels[:, None] if reduce_w else labels, 0.3, 0.7)
    ref.backward()
    ws = guard.alloc_bytes(_lib.load().bdn_overlap_workspace_bytes(B, C, H, W, reduce_w), label='overlap workspace')
    loss, counts, dl = guard.full((1,), NAN), guard.full((4,), -1, dtype=torch.int32), guard.full(shape, NAN)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    if entry == 'tversky':
        _lib.call('bdn_tversky', lg_d.data_ptr(), lb_d.data_ptr(), 0.3, 0.7, 1e-7, ws.data_ptr(), loss.data_ptr(), counts.data_ptr(),
                  dl.data_ptr(), B, C, H, W, st())
    else:
        _lib.call('bdn_overlap_loss', lg_d.data_ptr(), lb_d.data_ptr(), 0.3, 0.7, 1e-7, reduce_w, ws.data_ptr(), loss.data_ptr(),
                  counts.data_ptr(), dl.data_ptr(), B, C, H, W, st())
    torch.cuda.synchronize()
    assert abs(loss.item() - ref.item()) < LOSS_TOL * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    assert_close('dlogits', dl.cpu(), lo.grad.float(), GRAD_TOL)
    assert counts.cpu().tolist() == _counts(logits, labels)


@pytest.mark.parametrize('form', [dict(gamma=0.0), dict(gamma=2.0), dict(gamma=1.5, size_average=False), dict(gamma=2.0, alpha=True)],
                         ids=['g0', 'g2', 'g1.5_sum', 'g2_alpha'])
@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=str)
@guarded
def test_focal_kernel_called_directly(shape, form):
    """bdn_focal on the workspace of exactly bdn_focal_workspace_bytes, against oracle.focal_loss in float64."""
    B, C, H, W = shape
    logits, labels = _loss_inputs(shape, 37)
    alpha = torch.from_numpy(np.random.default_rng(5).uniform(0.1, 0.9, C).astype(np.float32)) if form.get('alpha') else None
    lo = logits.double().requires_grad_(True)
    ref = O.focal_loss(lo, labels, form['gamma'], alpha.double() if alpha is not None else None, form.get('size_average', True))
    ref.backward()
    ws = guard.alloc_bytes(_lib.load().bdn_focal_workspace_bytes(), label='focal workspace')
    loss, counts, dl = guard.full((1,), NAN), guard.full((4,), -1, dtype=torch.int32), guard.full(shape, NAN)
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    a_d = dev(alpha) if alpha is not None else None
    _lib.call('bdn_focal', lg_d.data_ptr(), lb_d.data_ptr(), form['gamma'], a_d.data_ptr() if a_d is not None else None,
              1 if form.get('size_average', True) else 0, ws.data_ptr(), loss.data_ptr(), counts.data_ptr(), dl.data_ptr(), B, C, H, W, st())
    torch.cuda.synchronize()
    assert abs(loss.item() - ref.item()) < LOSS_TOL * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    assert_close('dlogits', dl.cpu(), lo.grad.float(), GRAD_TOL)
    assert counts.cpu().tolist() == _counts(logits, labels)
