"""The block-uniform fast paths of conv3x3_kernel against its general path, bit for bit.

A tile whose whole halo lies inside the image stages its patch without bounds tests (single-chunk, BB and eval-mode kernels) and a full
tile copies out without them.  Neither may change a bit: every case runs its entry point twice on the same
seeded inputs, once under bdn_conv3x3_force_general(1) and once without, and every byte the launch writes -- the output, the statistics or
BatchNorm-backward partial rows, the dz by-product -- must be equal.  The default run is also held to a float64 reference at the
tolerances tests/test_gpu_kernels.py uses for the same entry point (statistics sums: float32 accumulation of at most a few hundred terms
per partial, 2e-5 of the sum of magnitudes).

Shapes: the smallest that hold every kind of tile -- 48x48 on 16x16 tiles and 24x48 on 8x16 tiles have ONE interior tile of nine, 32x32 and
16x16 none, 45x45 and 40x72 ragged ones (a tile whose halo or body crosses the edge is neither interior nor full), 8x8 two images per tile.
The 128-wide single-chunk instantiations are only dispatched from 512 tiles on, hence the 58-image cases; their float64 reference covers
the first and the last image.  (A two-image tile with its second image missing cannot be reached: N is a multiple of imgs_per_group, which
is even wherever two images share a tile.)  All buffers are guard-banded (tests/guard.py): what lies outside an image is NaN, so a border
tile wrongly taken for an interior one poisons its output instead of reading zeros.
"""
import pytest
import torch
import torch.nn.functional as F

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, IN_BNRELU, IN_PLAIN
from oracle import bidate_oracle as O
from tests.gpu_util import DT, assert_close, bn_table, bnrelu_ref, dev, from_nhwc, pack_w, preact, rnd, st, to_nhwc
from tests import guard
from tests.guard import guarded
from tests.test_gpu_kernels import TOL, _rand

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _both(launch):
    """launch() -> {name: tensor the launch wrote}; run under the forced general path, then by default; every byte equal.  Returns the default run."""
    lib = _lib.load()
    lib.bdn_conv3x3_force_general(1)
    try:
        general = launch()
        torch.cuda.synchronize()
    finally:
        lib.bdn_conv3x3_force_general(0)
    fast = launch()
    torch.cuda.synchronize()
    assert general.keys() == fast.keys()
    for name in fast:
        a, b = _bits(general[name]), _bits(fast[name])
        nbad = int((a != b).sum().item())
        assert nbad == 0, f'{name}: {nbad} bytes differ between the general and the fast path'
    return fast


def _variant(N, H, W, C0, C1, Cout, ipg, prec='bf16'):
    return _lib.load().bdn_conv3x3_variant(DT[prec][0], N, H, W, C0, C1, Cout, ipg).decode()


def _group_sums(stats, G):
    """[n_mtiles][2][Cout] partial rows -> [G][2][Cout] float64 (the tiles of a statistic group are consecutive rows)."""
    return stats.cpu().double().reshape(G, -1, 2, stats.shape[-1]).sum(1)


def _forward(prec, N, H, W, C0, C1, Cout, ipg, bnrelu, epilogue, ref_groups, c0r=None):
    """bdn_conv3x3 both ways; epilogue: 'stats' (bias + statistics partials) or 'plain' (a data-gradient launch: neither)."""
    c0r = c0r or C0
    dt, td = DT[prec]
    G = N // ipg
    x0 = rnd(prec, _rand((N, C0, H, W), 1))
    x0[:, c0r:] = 0
    x1 = rnd(prec, _rand((N, C1, H, W), 2)) if C1 else None
    w = _rand((Cout, c0r + C1, 3, 3), 3, (2.0 / (9 * (c0r + C1))) ** 0.5)
    b = _rand((Cout,), 4, 0.1) if epilogue == 'stats' else None
    bn_in = bn_table(G, C0, 5) if bnrelu else None
    wp = torch.zeros(Cout, C0 + C1, 3, 3)
    wp[:, :c0r] = w[:, :c0r]
    if C1:
        wp[:, C0:] = w[:, c0r:]
    wf, _ = pack_w(prec, wp, C0 + C1)
    d0, d1 = to_nhwc(prec, x0), (to_nhwc(prec, x1) if C1 else None)
    dbn = dev(bn_in) if bnrelu else None
    db = dev(b) if b is not None else None
    nt = _lib.load().bdn_conv3x3_num_mtiles(N, H, W, Cout, ipg)

    def launch():
        out = guard.empty(N, H, W, Cout, dtype=td)
        stats = guard.full((nt, 2, Cout), float('nan')) if epilogue == 'stats' else None
        _lib.call('bdn_conv3x3', dt, d0.data_ptr(), C0, d1.data_ptr() if C1 else None, C1, IN_BNRELU if bnrelu else IN_PLAIN,
                  dbn.data_ptr() if bnrelu else None, ipg, wf.data_ptr(), db.data_ptr() if db is not None else None, out.data_ptr(),
                  stats.data_ptr() if stats is not None else None, N, H, W, Cout, st())
        return {'out': out, 'stats': stats} if stats is not None else {'out': out}
    got = _both(launch)
    # float64 reference of the chosen statistic groups (whole images; a convolution never mixes images)
    out = from_nhwc(got['out'])
    for g in ref_groups:
        s = slice(g * ipg, (g + 1) * ipg)
        a0 = bnrelu_ref(prec, x0[s], bn_in[g:g + 1], ipg) if bnrelu else x0[s]
        a = torch.cat([a0[:, :c0r], x1[s]], 1) if C1 else a0[:, :c0r]
        z_ref = O.conv3x3(a, rnd(prec, w), b if b is not None else torch.zeros(Cout))
        assert_close(f'conv out, group {g}', out[s], z_ref, TOL[prec])
        if epilogue == 'stats':
            sums = _group_sums(got['stats'], G)[g]
            zd = z_ref.double()
            assert_close(f'sum z, group {g}', sums[0], zd.sum((0, 2, 3)), 0.0, abs_floor=2e-5 * zd.abs().sum((0, 2, 3)).max().item())
            assert_close(f'sum z^2, group {g}', sums[1], (zd * zd).sum((0, 2, 3)), 2e-5)
    return got


# ------------------------------------------------------------------ 48x48 on 16x16 tiles: one interior tile of nine
@guarded
def test_first_layer_16_to_64():
    assert _variant(2, 48, 48, 16, 0, 64, 1) == 'conv3x3_kernel<bf16,32,16,16,1,64,2,2,true,bf16,false,false,false,0,false>'
    _forward('bf16', 2, 48, 48, 16, 0, 64, 1, False, 'stats', (0, 1), c0r=13)


@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
@guarded
def test_single_chunk_forward_with_bn_on_load(prec):
    C0 = 64 if prec == 'bf16' else 32
    assert ',16,16,1,64,2,2,true,' in _variant(2, 48, 48, C0, 0, 64, 1, prec)
    _forward(prec, 2, 48, 48, C0, 0, 64, 1, True, 'stats', (0, 1))


def _bs_reference(dA, z, bn, ipg, full_ref, G):
    """What a dgrad_bs launch must leave: the stored gradient equal to the reference under the ReLU mask, and partial rows that sum to
    sum g and sum g z of the STORED (rounded, masked) gradient."""
    pre = preact(z, bn, ipg)
    on, off = pre > 1e-4, pre < -1e-4
    got = from_nhwc(dA)
    assert_close('dA where the ReLU is on', got * on, full_ref * on, TOL['bf16'])
    assert (got[off] == 0).all()
    assert on.any() and off.any()
    g = got.double().reshape(G, ipg, got.shape[1], -1)
    zz = z.double().reshape(G, ipg, got.shape[1], -1)
    return g.sum((1, 3)), (g * zz).sum((1, 3)), g.abs().sum((1, 3)).max().item(), (g * zz).abs().sum((1, 3)).max().item()


@guarded
def test_dgrad_bs_64_to_64():
    N, H, W, C, ipg = 2, 48, 48, 64, 1
    dz = rnd('bf16', _rand((N, C, H, W), 51))
    w = rnd('bf16', _rand((C, C, 3, 3), 52, 0.05))
    wf, _ = pack_w('bf16', w, C)
    z = rnd('bf16', _rand((N, C, H, W), 53))
    bn = bn_table(N // ipg, C, 7)
    dzd, zd, bnd = to_nhwc('bf16', dz), to_nhwc('bf16', z), dev(bn)
    nt = _lib.load().bdn_conv3x3_num_mtiles(N, H, W, C, ipg)

    def launch():
        dA = guard.empty(N, H, W, C, dtype=torch.bfloat16)
        part = guard.full((nt, 2, C), float('nan'))
        _lib.call('bdn_conv3x3_dgrad_bs', BDN_BF16, dzd.data_ptr(), C, wf.data_ptr(), dA.data_ptr(), zd.data_ptr(), bnd.data_ptr(), ipg,
                  part.data_ptr(), N, H, W, C, st())
        return {'dA': dA, 'partials': part}
    got = _both(launch)
    s0, s1, m0, m1 = _bs_reference(got['dA'], z, bn, ipg, F.conv2d(dz.double(), w.double(), padding=1).float(), N // ipg)
    sums = _group_sums(got['partials'], N // ipg)
    assert_close('sum g', sums[:, 0], s0, 0.0, abs_floor=2e-5 * m0)
    assert_close('sum g z', sums[:, 1], s1, 0.0, abs_floor=2e-5 * m1)


def _dgrad_bb(N, H, W, Cout, ipg, with_prev, ref_groups):
    """bdn_conv3x3_dgrad_bb (C0 = 64) both ways; float64: dz = scale (g - s0/M - xhat s1/M), dA_prev = the data gradient of the stored dz."""
    C0, G = 64, N // ipg
    lib = _lib.load()
    z = rnd('bf16', _rand((N, C0, H, W), 62))
    bn = bn_table(G, C0, 63)
    pre = preact(z, bn, ipg)
    g = rnd('bf16', _rand((N, C0, H, W), 61)) * (pre > 1e-4)
    w = rnd('bf16', _rand((C0, Cout, 3, 3), 64, 0.05))
    _, wd = pack_w('bf16', w, Cout)
    gd, zd, bnd = to_nhwc('bf16', g), to_nhwc('bf16', z), dev(bn)
    M = ipg * H * W
    gg, zz = g.double().reshape(G, ipg, C0, -1), z.double().reshape(G, ipg, C0, -1)
    sums = torch.stack([gg.sum((1, 3)), (gg * (zz - bn[:, 0].double()[:, None, :, None]) * bn[:, 1].double()[:, None, :, None]).sum((1, 3))], 1)
    sd = dev(sums.float())                                                    # [G][2][C0]: sum g, sum g xhat (bdn_bn_bwd_finalize's rows)
    zp = rnd('bf16', _rand((N, Cout, H, W), 65))
    bnp = bn_table(G, Cout, 66)
    zpd, bnpd = to_nhwc('bf16', zp), dev(bnp)
    nt = lib.bdn_conv3x3_num_mtiles(N, H, W, Cout, ipg)

    def launch():
        out = guard.empty(N, H, W, Cout, dtype=torch.bfloat16)
        dz = guard.empty(N, H, W, C0, dtype=torch.bfloat16)
        part = guard.full((nt, 2, Cout), float('nan')) if with_prev else None
        _lib.call('bdn_conv3x3_dgrad_bb', BDN_BF16, gd.data_ptr(), C0, zd.data_ptr(), bnd.data_ptr(), sd.data_ptr(), ipg, wd.data_ptr(),
                  out.data_ptr(), zpd.data_ptr() if with_prev else None, bnpd.data_ptr() if with_prev else None,
                  part.data_ptr() if with_prev else None, dz.data_ptr(), N, H, W, Cout, st())
        return {'dA_prev': out, 'dz': dz, 'partials': part} if with_prev else {'dA_prev': out, 'dz': dz}
    got = _both(launch)
    dz_dev, out = from_nhwc(got['dz']), from_nhwc(got['dA_prev'])
    for gi in ref_groups:
        s = slice(gi * ipg, (gi + 1) * ipg)
        mean, inv, scale = (bn[gi, k].double()[None, :, None, None] for k in (0, 1, 2))
        s0, s1 = (sums[gi, k].float().double()[None, :, None, None] for k in (0, 1))
        dz_ref = scale * (g[s].double() - s0 / M - (z[s].double() - mean) * inv * s1 / M)
        assert_close(f'dz, group {gi}', dz_dev[s], dz_ref.float(), 8e-3)
        full = torch.nn.grad.conv2d_input((ipg, Cout, H, W), w.double(), dz_dev[s].double(), padding=1).float()
        if with_prev:
            s0p, s1p, m0, m1 = _bs_reference(got['dA_prev'][s], zp[s], bnp[gi:gi + 1], ipg, full, 1)
            psum = _group_sums(got['partials'], G)[gi]
            assert_close('sum g', psum[0], s0p[0], 0.0, abs_floor=2e-5 * m0)
            assert_close('sum g z', psum[1], s1p[0], 0.0, abs_floor=2e-5 * m1)
        else:
            assert_close(f'dA_prev, group {gi}', out[s], full, TOL['bf16'])


@guarded
def test_dgrad_bb_64_to_64_with_predecessor():
    assert _lib.load().bdn_conv3x3_dgrad_bb_variant(2, 48, 48, 64, 1) == b'conv3x3_kernel<bf16,128,16,16,1,64,2,2,true,bf16,false,true,false,0,false>'
    _dgrad_bb(2, 48, 48, 64, 1, True, (0, 1))


# ------------------------------------------------------------------ 24x48 on 8x16 tiles: one interior tile of nine
# N = 58: 522 tiles, the 128-wide column tiles (the single-chunk <8,16,1,128,1,4,true> forms of the flagship); N = 2: the 64-wide ones
@pytest.mark.parametrize('N', [2, 58])
@pytest.mark.parametrize('epilogue', ['stats', 'plain'])
@guarded
def test_64_to_128_forward_and_data_gradient(N, epilogue):
    assert _variant(N, 24, 48, 64, 0, 128, 1) == ('conv3x3_kernel<bf16,128,8,16,1,128,1,4,true,bf16,false,false,false,0,false>' if N == 58 else
                                                  'conv3x3_kernel<bf16,128,8,16,1,64,2,2,false,bf16,false,false,false,0,false>')
    _forward('bf16', N, 24, 48, 64, 0, 128, 1, epilogue == 'stats', epilogue, (0, N - 1))


@pytest.mark.parametrize('N', [2, 58])
@guarded
def test_128_to_128_two_chunk_forward(N):
    assert (',8,16,1,128,1,4,false,' if N == 58 else ',8,16,1,64,2,2,false,') in _variant(N, 24, 48, 128, 0, 128, 1)
    _forward('bf16', N, 24, 48, 128, 0, 128, 1, True, 'stats', (0, N - 1))


@pytest.mark.parametrize('N', [2, 58])
@guarded
def test_dgrad_bb_64_to_128(N):
    assert (b',8,16,1,128,1,4,true,' if N == 58 else b',8,16,1,64,2,2,false,') in _lib.load().bdn_conv3x3_dgrad_bb_variant(N, 24, 48, 128, 1)
    _dgrad_bb(N, 24, 48, 128, 1, N == 2, (0, N - 1))


# ------------------------------------------------------------------ the 4x1 multi-chunk layout, no interior tile, ragged tiles, two images per tile
@guarded
def test_128_to_64_multi_chunk_16x16():
    assert ',16,16,1,64,4,1,false,' in _variant(2, 48, 48, 128, 0, 64, 1)
    _forward('bf16', 2, 48, 48, 128, 0, 64, 1, True, 'stats', (0, 1))


@pytest.mark.parametrize('shape', [(32, 32, 64), (16, 16, 64), (16, 16, 128),      # every tile touches the border: never interior
                                   (45, 45, 64), (40, 72, 64), (45, 45, 128), (40, 72, 128)])        # ragged: the tile next to a cut one is interior, the cut one not full
@pytest.mark.parametrize('epilogue', ['stats', 'plain'])
@guarded
def test_border_only_and_ragged_maps(shape, epilogue):
    H, W, Cout = shape
    _forward('bf16', 2, H, W, 64, 0, Cout, 1, epilogue == 'stats', epilogue, (0, 1))


@guarded
def test_two_images_per_tile():
    assert ',8,8,2,' in _variant(4, 8, 8, 64, 0, 64, 2)
    _forward('bf16', 4, 8, 8, 64, 0, 64, 2, True, 'stats', (0, 1))
    _forward('bf16', 4, 8, 8, 128, 0, 128, 2, True, 'stats', (0, 1))


# ------------------------------------------------------------------ float32 outputs (bf16x3): the accumulator pass and copy-out of today
@guarded
def test_bf16x3_float32_output():
    N, H, W, Cin, Cout, ipg = 2, 24, 48, 64, 64, 1
    X3 = _lib.BDN_BF16X3
    x, w, b = _rand((N, Cin, H, W), 311), _rand((Cout, Cin, 3, 3), 312) * 0.1, _rand((Cout,), 313)
    ref = F.conv2d(x, w, b, padding=1)
    sp = guard.empty(N, H, W, 2 * Cin, dtype=torch.bfloat16)
    xd = to_nhwc('fp32', x)
    _lib.call('bdn_split_pack', xd.data_ptr(), Cin, None, 0, IN_PLAIN, None, ipg, sp.data_ptr(), N, H, W, st())
    wf = guard.empty(Cout, 9, 3 * Cin, dtype=torch.bfloat16)
    wdev, bd = dev(w), dev(b)
    _lib.call('bdn_pack_weights', X3, wdev.data_ptr(), wf.data_ptr(), None, Cout, Cin, Cin, st())
    nt = _lib.load().bdn_conv3x3_num_mtiles_ex(X3, N, H, W, Cin, Cout, ipg)

    def launch():
        out = guard.full((N, H, W, Cout), float('nan'))
        stats = guard.full((nt, 2, Cout), float('nan'))
        _lib.call('bdn_conv3x3', X3, sp.data_ptr(), Cin, None, 0, IN_PLAIN, None, ipg, wf.data_ptr(), bd.data_ptr(), out.data_ptr(),
                  stats.data_ptr(), N, H, W, Cout, st())
        return {'out': out, 'stats': stats}
    got = _both(launch)
    assert_close('x3 fwd', from_nhwc(got['out']), ref, 1e-4)
    ssum = _group_sums(got['stats'], N // ipg)[:, 0]
    want = ref.double().reshape(N // ipg, ipg, Cout, H * W).sum((1, 3))
    assert (ssum - want).abs().max() <= 1e-4 * want.abs().max() + 1e-3


# ------------------------------------------------------------------ eval mode: its interior path obeys the same switch
@guarded
def test_eval_stage_obeys_the_switch():
    N, H, W, C = 2, 48, 48, 64
    x = rnd('bf16', _rand((N, C, H, W), 1).abs())
    w = rnd('bf16', _rand((C, C, 3, 3), 3, (2.0 / (9 * C)) ** 0.5))
    sc, sh = _rand((C,), 6).abs() + 0.5, _rand((C,), 7, 0.3)
    wf, _ = pack_w('bf16', w, C)
    xd, dsc, dsh = to_nhwc('bf16', x), dev(sc), dev(sh)

    def launch():
        out = guard.empty(N, H, W, C, dtype=torch.bfloat16)
        _lib.call('bdn_conv3x3_eval', BDN_BF16, xd.data_ptr(), C, None, 0, wf.data_ptr(), dsc.data_ptr(), dsh.data_ptr(), out.data_ptr(), None, None,
                  N, H, W, C, st())
        return {'out': out}
    got = _both(launch)
    ref = torch.relu(F.conv2d(x.double(), w.double(), padding=1) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]).float()
    assert_close('eval stage', from_nhwc(got['out']), ref, TOL['bf16'])
