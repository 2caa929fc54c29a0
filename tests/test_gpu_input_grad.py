"""-m gpu kernel tests of the input-gradient and frozen-BatchNorm entry points against float64:
bdn_conv3x3_dgrad_first (the first convolution's data gradient, written as two NCHW date tensors) with dz formed on load on batch
statistics, on running statistics (zeroed sums) and from a plain dz; bdn_bn_bwd_finalize_frozen (dgamma, dbeta, conv-bias gradient);
the frozen dz of bdn_bn_bwd_apply_frozen / bdn_bn_bwd_frozen equal to scale * g under the mask, bit for bit."""
import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X3, BDN_F32
from tests.gpu_util import assert_close, st
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu

TOL = {'fp32': 2e-5, 'bf16': 1e-2}                     # tests/test_gpu_kernels.py, as test_conv3x3_dgrad applies it
DT = {'fp32': (BDN_F32, torch.float32), 'bf16': (BDN_BF16, torch.bfloat16)}


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def _table(G, C, seed):
    """A [G][4][C] BatchNorm table {mean, invstd, scale, shift} as bdn_bn_finalize / bdn_bn_eval lay it out."""
    rng = np.random.default_rng(seed)
    mean = torch.from_numpy(rng.standard_normal((G, C)).astype(np.float32) * 0.3)
    inv = torch.from_numpy(rng.uniform(0.5, 2.0, (G, C)).astype(np.float32))
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, (C,)).astype(np.float32))
    beta = torch.from_numpy(rng.standard_normal((C,)).astype(np.float32) * 0.1)
    sc = gamma[None] * inv
    sh = beta[None] - mean * sc
    return torch.stack([mean, inv, sc, sh], 1).contiguous()


def _dz64(dA, z, tab, sums, ipg):
    """float64 dz = scale (g - s0/M - xhat s1/M), g = dA where scale z + shift > 0; dA, z [N,H,W,C] float32 CPU."""
    N, H, W, C = dA.shape
    G = N // ipg
    t = tab.double().repeat_interleave(ipg, 0)[:, :, None, None, :]          # [N,4,1,1,C]
    s = sums.double().repeat_interleave(ipg, 0)[:, :, None, None, :] / (ipg * H * W)
    mean, inv, sc, sh = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    zd, gd = z.double(), dA.double()
    mask = torch.addcmul(sh.float().expand_as(zd), zd.float(), sc.float().expand_as(zd)) > 0
    g = torch.where(mask, gd, torch.zeros_like(gd))
    return sc * (g - s[:, 0] - (zd - mean) * inv * s[:, 1])


def _run_first(prec, B, H, W, cr, form, seed=0, ldA=64):
    dt, td = DT[prec]
    N, C = 2 * B, 64
    ipg = B
    dA = _rand((N, H, W, ldA), seed).to(td).float()
    z = _rand((N, H, W, C), seed + 1).to(td).float()
    w = _rand((C, cr, 3, 3), seed + 2, 0.05)
    tab = _table(2, C, seed + 3)
    sums = _rand((2, 2, C), seed + 4, 50.0) if form == 'batch' else torch.zeros(2, 2, C)
    if form == 'plain':
        dz = dA[..., :C].double()
    else:
        dz = _dz64(dA[..., :C].contiguous(), z, tab, sums, ipg)
    ref = torch.nn.grad.conv2d_input((N, cr, H, W), w.double(), dz.permute(0, 3, 1, 2), padding=1)
    dx1 = guard.full((B, cr, H, W), float('nan'))
    dx2 = guard.full((B, cr, H, W), float('nan'))
    ddA, dz_ = guard.guard(dA.to(td)), guard.guard(z.to(td))
    ddA[..., C:] = float('nan')                          # the foreign channels of a wider dA: a read of them poisons the result
    dtab, dsums, dw = guard.guard(tab), guard.guard(sums), guard.guard(w)
    if form == 'plain':
        _lib.call('bdn_conv3x3_dgrad_first', dt, ddA.data_ptr(), ldA, None, None, None, ipg, dw.data_ptr(), cr,
                  dx1.data_ptr(), dx2.data_ptr(), B, H, W, st())
    else:
        _lib.call('bdn_conv3x3_dgrad_first', dt, ddA.data_ptr(), ldA, dz_.data_ptr(), dtab.data_ptr(), dsums.data_ptr(), ipg,
                  dw.data_ptr(), cr, dx1.data_ptr(), dx2.data_ptr(), B, H, W, st())
    torch.cuda.synchronize()
    return dx1.cpu(), dx2.cpu(), ref


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('form', ['batch', 'frozen', 'plain'])
@pytest.mark.parametrize('case', [(2, 32, 32, 3), (2, 32, 32, 13), (1, 90, 90, 13), (3, 40, 72, 13), (2, 5, 5, 3)])
@guarded
def test_dgrad_first_matches_float64(prec, form, case):
    B, H, W, cr = case
    dx1, dx2, ref = _run_first(prec, B, H, W, cr, form)
    assert_close(f'dx1[{prec},{form}]', dx1, ref[:B], TOL[prec])
    assert_close(f'dx2[{prec},{form}]', dx2, ref[B:], TOL[prec])


@guarded
def test_dgrad_first_reads_a_dA_slice():
    """dA with a leading dimension above 64 (a channel slice of a wider tensor)."""
    dx1, dx2, ref = _run_first('bf16', 2, 24, 20, 13, 'batch', seed=5, ldA=128)
    assert_close('dx1', dx1, ref[:2], TOL['bf16'])
    assert_close('dx2', dx2, ref[2:], TOL['bf16'])


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@guarded
def test_dgrad_first_full_size(prec):
    """B = 64, 128 x 128, 13 bands (the benchmark shape); the float64 reference on four images (both ends of both dates)."""
    B, H, W, cr, C = 64, 128, 128, 13, 64
    dt, td = DT[prec]
    N = 2 * B
    g = torch.Generator(device='cuda').manual_seed(0)
    ddA = guard.guard(torch.randn(N, H, W, C, device='cuda', generator=g).to(td))
    dz_ = guard.guard(torch.randn(N, H, W, C, device='cuda', generator=g).to(td))
    w = _rand((C, cr, 3, 3), 2, 0.05)
    tab, sums = _table(2, C, 3), _rand((2, 2, C), 4, 50.0)
    dx1 = guard.full((B, cr, H, W), float('nan'))
    dx2 = guard.full((B, cr, H, W), float('nan'))
    dtab, dsums, dw = guard.guard(tab), guard.guard(sums), guard.guard(w)
    _lib.call('bdn_conv3x3_dgrad_first', dt, ddA.data_ptr(), C, dz_.data_ptr(), dtab.data_ptr(), dsums.data_ptr(), B,
              dw.data_ptr(), cr, dx1.data_ptr(), dx2.data_ptr(), B, H, W, st())
    torch.cuda.synchronize()
    assert torch.isfinite(dx1).all() and torch.isfinite(dx2).all()
    for n in (0, B - 1, B, N - 1):
        dA1, z1 = ddA[n:n + 1].float().cpu(), dz_[n:n + 1].float().cpu()
        g1 = n // B
        # _dz64 divides the sums by its own M (one image); the launch's M is B images
        dz = _dz64(dA1, z1, tab[g1:g1 + 1], sums[g1:g1 + 1] / B, 1)
        ref = torch.nn.grad.conv2d_input((1, cr, H, W), w.double(), dz.permute(0, 3, 1, 2), padding=1)[0]
        got = (dx1 if n < B else dx2)[n % B].cpu()
        assert_close(f'dx[{prec}] image {n}', got, ref, TOL[prec])


# ------------------------------------------------------------------ frozen BatchNorm backward
def _eval_table(C, seed):
    rng = np.random.default_rng(seed)
    gamma = guard.guard(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
    beta = guard.guard(torch.from_numpy(rng.standard_normal(C).astype(np.float32) * 0.1))
    rm = guard.guard(torch.from_numpy(rng.standard_normal(C).astype(np.float32) * 0.3))
    rv = guard.guard(torch.from_numpy(rng.uniform(0.3, 2.0, C).astype(np.float32)))
    return gamma, beta, rm, rv


@pytest.mark.parametrize('G,C,rows', [(2, 64, 37), (1, 256, 700), (2, 512, 9)])
@guarded
def test_frozen_finalize_matches_float64(G, C, rows):
    gamma, beta, rm, rv = _eval_table(C, G + C)
    bn = guard.empty(G, 4, C)
    _lib.call('bdn_bn_eval', gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, G, C, bn.data_ptr(), st())
    part = guard.guard(_rand((G * rows, 2, C), 7))
    sums = guard.full((G, 2, C), float('nan'))
    dg, db, dbias = (guard.full((C,), float('nan')) for _ in range(3))
    scratch = guard.empty(_lib.load().bdn_bn_bwd_scratch_bytes(G, C) // 4)
    _lib.call('bdn_bn_bwd_finalize_frozen', bn.data_ptr(), G, C, part.data_ptr(), rows, 1, sums.data_ptr(), dg.data_ptr(),
              db.data_ptr(), dbias.data_ptr(), scratch.data_ptr(), st())
    torch.cuda.synchronize()
    p = part.double().cpu().reshape(G, rows, 2, C).sum(1)                       # [G][2][C]: sum g, sum g z
    inv = 1.0 / torch.sqrt(rv.double().cpu() + 1e-5)
    s1 = inv * (p[:, 1] - rm.double().cpu() * p[:, 0])
    ref_db, ref_dg = p[:, 0].sum(0), s1.sum(0)
    ref_dbias = gamma.double().cpu() * inv * ref_db
    for name, got, ref in (('dbeta', db, ref_db), ('dgamma', dg, ref_dg), ('dbias', dbias, ref_dbias)):
        assert_close(name, got.cpu(), ref, 1e-5)
    assert torch.equal(sums.cpu(), torch.zeros(G, 2, C))


@pytest.mark.parametrize('dtype,fused', [('bf16', True), ('fp32', True), ('split', True), ('bf16', False), ('fp32', False)])
@guarded
def test_frozen_dz_is_scale_times_masked_gradient(dtype, fused):
    """dz = scale * g under the ReLU mask, bit for bit, whichever frozen entry point forms it (no mean-correction terms)."""
    N, H, W, C, ipg = 4, 12, 20, 64, 2
    G = N // ipg
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    dt = {'bf16': BDN_BF16, 'fp32': BDN_F32, 'split': BDN_BF16X3}[dtype]
    gamma, beta, rm, rv = _eval_table(C, 3)
    bn = guard.empty(G, 4, C)
    _lib.call('bdn_bn_eval', gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, G, C, bn.data_ptr(), st())
    dA = guard.guard(_rand((N, H, W, C), 1).to(td))
    z = guard.guard(_rand((N, H, W, C), 2).to(td))
    sums = guard.empty(G, 2, C)
    dg, db, dbias = (guard.empty(C) for _ in range(3))
    out = guard.empty(N, H, W, 2 * C if dtype == 'split' else C, dtype=torch.bfloat16 if dtype == 'split' else td)
    lib = _lib.load()
    if fused:
        rows = 5
        part = guard.guard(_rand((G * rows, 2, C), 3))
        scratch = guard.empty(lib.bdn_bn_bwd_scratch_bytes(G, C) // 4 + 1)
        _lib.call('bdn_bn_bwd_apply_frozen', dt, dA.data_ptr(), C, z.data_ptr(), bn.data_ptr(), ipg, N, H, W, C, part.data_ptr(),
                  rows, 1, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dbias.data_ptr(), out.data_ptr(), scratch.data_ptr(), st())
    else:
        ws = guard.empty(lib.bdn_bn_bwd_workspace_bytes(dt, N, H, W, C, ipg) // 4 + 1)
        _lib.call('bdn_bn_bwd_frozen', dt, dA.data_ptr(), C, z.data_ptr(), bn.data_ptr(), ipg, N, H, W, C, ws.data_ptr(),
                  sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dbias.data_ptr(), out.data_ptr(), st())
    torch.cuda.synchronize()
    t = bn.repeat_interleave(ipg, 0)[:, :, None, None, :]
    sc, sh = t[:, 2], t[:, 3]
    zf, gf = z.float(), dA.float()
    mask = torch.addcmul(sh.expand_as(zf), zf, sc.expand_as(zf)) > 0
    ref = sc * torch.where(mask, gf, torch.zeros_like(gf))
    if dtype == 'split':
        hi = ref.to(torch.bfloat16)
        lo = (ref - hi.float()).to(torch.bfloat16)
        assert torch.equal(out[..., :C].view(torch.int16), hi.view(torch.int16))
        assert torch.equal(out[..., C:].view(torch.int16), lo.view(torch.int16))
    else:
        assert torch.equal(out.float() + 0.0, ref.to(td).float() + 0.0)      # + 0.0: the sign of a zero is not compared
    assert torch.equal(sums.cpu(), torch.zeros(G, 2, C))
    if not fused:                                                         # dbeta = sum g under the mask, dbias = scale * dbeta
        ref_db = torch.where(mask, gf, torch.zeros_like(gf)).double().sum((0, 1, 2))
        assert_close('dbeta', db.cpu(), ref_db.cpu(), 1e-5)
        assert torch.equal(dbias, bn[0, 2] * db)


# ------------------------------------------------------------------ above 16 bands: refused at the door
@pytest.mark.parametrize('prec', ['bf16', 'fp32', 'bf16x3'])
def test_input_gradient_above_16_bands_is_refused_before_any_launch(prec):
    """A 17-band model: backward(dx=...) raises ValueError naming the limit and bdn_conv3x3_dgrad_first before its first launch -- the
    NaN-filled grads and dx hold only NaN afterwards -- and so does the module when an image requires grad.  The engine is left as it
    was: the next forward + backward without dx gives logits and all 74 gradients bit-equal to those of a freshly built twin."""
    from fabric_amd import BiDateNet
    from oracle import filler
    b, c, s = 2, 17, 32
    x1, x2, _ = filler.make_inputs(b, c, s, seed=0, different_dates=True)
    x1, x2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    dl = torch.from_numpy(np.random.default_rng(1).standard_normal((b, 2, s, s)).astype(np.float32) * 1e-3).cuda()

    def build():
        model = filler.fill_module(BiDateNet(c, 2, precision=prec)).cuda().train()
        return model, model.engine(), {k: v.detach() for k, v in model.state_dict(keep_vars=True).items()}

    def step(model, eng, P):
        logits, ws = eng.forward(x1, x2, P, training=True)
        grads = {k: torch.full_like(p, float('nan')) for k, p in model.named_parameters()}
        eng.backward(ws, dl, P, grads)
        torch.cuda.synchronize()
        return logits, grads

    model, eng, P = build()
    logits, ws = eng.forward(x1, x2, P, training=True)
    grads = {k: torch.full_like(p, float('nan')) for k, p in model.named_parameters()}
    dx = (torch.full_like(x1, float('nan')), torch.full_like(x2, float('nan')))
    with pytest.raises(ValueError, match=r'limited to 16 bands.*bdn_conv3x3_dgrad_first'):
        eng.backward(ws, dl, P, grads, dx=dx)
    torch.cuda.synchronize()
    assert len(grads) == 74 and all(bool(torch.isnan(g).all()) for g in grads.values())
    assert bool(torch.isnan(dx[0]).all()) and bool(torch.isnan(dx[1]).all())
    with pytest.raises(ValueError, match='bdn_conv3x3_dgrad_first'):
        model(x1.clone().requires_grad_(True), x2)
    got_logits, got = step(model, eng, P)
    twin_logits, twin = step(*build())
    assert torch.equal(got_logits, twin_logits)
    assert set(got) == set(twin) and len(got) == 74
    for k in got:
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], twin[k]), k
