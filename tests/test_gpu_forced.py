"""-m gpu: the engine's forward and backward audited at its OWN stored values (tests/forced_ref.py; harness checked by
tests/test_forced_ref_cpu.py).

The engine is driven directly -- eng.forward(x1, x2, P, training=True | frozen=True), eng.backward(ws, dlogits, P, grads, dx=, bn_mode=) --
on oracle.filler weights and inputs (independent dates).  The workspace it leaves (every z, every table, x0 / f / pool / U outside bf16x3,
the logits) is copied to the CPU, and a float64 reference re-evaluates every stage on the engine's stored predecessors.  What the existing
whole-model bounds (0.25 / 0.8 in bf16, 2e-2 / 6e-2 in fp32 / bf16x3) allow for forward divergence is gone: a stage differs from its
reference by ONE stage's rounding, a gradient by backward rounding only, and a failure names the stage or the tensor.

Shapes (B, c, H, W): s32 (2, 3, 32, 32) level-5 map 2x2; s40x72 (3, 13, 40, 72) the 13 -> 16 band padding, non-square, maps of 8x8 and below
that folds_bn_bwd refuses beside larger ones; s90 (2, 13, 90, 90) odd maps at 45 and 11 (pad_to, floor pooling).
Wide inputs: w17 (2, 17, 32, 32), w48 (3, 48, 40, 24), w50 (2, 50, 16, 48): the first layer padded to 32, 48 and 64 channels -- the
multi-chunk / single-float-chunk forward kernels, and in backward the route the 'nodx' case does NOT take: first_wgrad_dtype is None
(bdn_conv3x3_wgrad_bnbwd refuses C0 != 16), so the first layer's BatchNorm backward is a pass of its own (bf16x3: it leaves dz split) and
its weight gradient the generic GEMM with Cin_real < C0 (asserted from the recorded calls).  No dx there: it is refused above 16 bands.
Matrix: every precision x the three shapes with 'product', batch statistics and dx; per precision 'absdiff' (s40x72), bn_mode='running'
(s32), no dx = the first_wgrad_fused path (s90), fold_bn_bwd = () (s40x72), wgrad_stream=False (s32), and Gaussian dlogits with exact zeros
(s40x72); 'base' without dx on the three wide shapes and bn_mode='running' on w17.  Everywhere else dlogits is the float64
Tversky(0.1, 0.9) gradient at the engine's own logits, cast to float32.

Asserted, forward (test_forward_stages), per stage:
  conv        every element |z_engine - z_ref| <= u*|z_ref| + c*A, u = 2^-8 (bf16 storage) / 2^-23 (float32), A = conv(|a|,|w|) + |b|,
              c = forced_ref.C_CONV = 4 x the largest measured, under the ceiling K*2^-24 of the shortest reduction (K = 9*16)
  tables      mean / invstd against float64 statistics of the float64 v = conv + bias (bounds: forced_ref._audit_table), scale / shift
              against the table's own mean / invstd within one / two float32 roundings
  x0, f, U    within one rounding of the stored type of the float64 op (U: plus the float32 tap-weight term 2^-21*n_in*max|a|)
  pool        exactly the maximum of the stored activations
  logits      within (C + 2)*2^-24*(sum|a||w| + |b|) of the float64 classifier on the stored last layer
Asserted, backward (test_backward): for EVERY parameter tensor and dx1 / dx2, the engine against forced_backward: relative L2, 1 - cosine
and |gain - 1| (gain = <engine, ref> / <ref, ref>: rounding noise is incoherent and averages out of it, a coherent scale error does not).
Bounds forced_ref.GRAD_REL / GRAD_1MCOS / GRAD_GAIN = 2 x the largest measured per setting (box-to-box and summation-order spread).  Conv
biases in front of a batch-statistics BatchNorm are exactly 0 on the device; in the reference they are below 1e-9*||dlogits|| once the
table-mean residual is taken out: the explicit BatchNorm backward leaves -gamma*invstd^2*dgamma*(mean(z) - mean) there, and the engine's
table is that of the float32 accumulators while z is stored rounded, so mean(z) is not the table's mean (raw reference value: 1.2e-7 of
||dlogits|| in fp32, 8e-4 in bf16; less the residual: 2e-15).  No other element or tensor is left out.

Measured on an MI355X, largest over the cases of a setting (the case, the stage or tensor), asserted = 4 x (c) / 2 x (gradients):
  conv c          fp32 5.16e-7 (s90, d4a) = the accumulation-order floor;  bf16x3 / bf16x3-fast 1.33e-6 (s32 running, d4a);
                  bf16 4.07e-8 (s32, e3a; there u*|z_ref| carries the bound);  ceiling 9*16*2^-24 = 8.58e-6
  other stages    as a fraction of their bound: x0 / f 0.50 (fp32), 0.996 (bf16); U 0.11 (fp32), 0.996 (bf16); pooled maps 0 (exact);
                  tables 0.996 (one float32 rounding of scale = gamma*invstd reaches its bound by construction); logits 0.03
  relative L2     fp32 5.21e-6 (base-s90, dx1);  bf16x3 1.91e-5 (absdiff, inc.conv.conv.4.bias);
                  bf16x3-fast 9.24e-3 (running, down4.mpconv.1.conv.4.weight);  bf16 1.32e-2 (absdiff, inc.conv.conv.4.bias)
  1 - cosine      fp32 1.36e-11;  bf16x3 1.81e-10;  bf16x3-fast 4.26e-5;  bf16 8.25e-5 (the same cases and tensors)
  |gain - 1|      fp32 8.43e-7 (base-s90, inc.conv.conv.4.bias);  bf16x3 4.41e-6 (running, down4.mpconv.1.conv.1.weight);
                  bf16x3-fast 5.00e-3 (running, down2.mpconv.1.conv.4.weight);  bf16 4.40e-3 (running, up2.conv.conv.4.weight)
  per case, worst relative L2 (base-s32 / base-s40x72 / base-s90 / absdiff / running / nodx / nofold / nostream / gauss):
    fp32         5.16e-6  5.12e-6  5.21e-6  5.20e-6  5.02e-6  3.26e-6  5.12e-6  5.16e-6  5.13e-6
    bf16x3       1.52e-5  1.48e-5  1.91e-5  1.91e-5  1.36e-5  1.91e-5  1.48e-5  1.52e-5  1.43e-5
    bf16x3-fast  6.47e-3  6.51e-3  6.63e-3  7.68e-3  9.24e-3  6.63e-3  6.51e-3  6.47e-3  6.60e-3
    bf16         1.10e-2  9.62e-3  1.25e-2  1.32e-2  1.19e-2  1.25e-2  1.03e-2  1.10e-2  9.57e-3
  wide inputs, same bounds (the per-stage rounding does not depend on the band count; C_CEILING is that of the shortest reduction), worst
  relative L2 (base-w17 / base-w48 / base-w50 / running-w17), then the largest 1 - cosine, |gain - 1| and conv c over the four:
    fp32         2.71e-6  2.56e-6  3.21e-6  1.44e-6    5.08e-12 (base-w50)     8.50e-7 (base-w50)     4.60e-7 (running-w17, d1a)
    bf16x3       1.61e-5  1.51e-5  1.76e-5  1.15e-5    1.54e-10 (base-w50)     3.27e-6 (running-w17)  9.39e-7 (base-w17, d4a)
    bf16x3-fast  6.16e-3  6.63e-3  6.86e-3  9.92e-3    4.86e-5 (running-w17)   2.34e-3 (running-w17)  9.39e-7 (the bf16x3 forward)
    bf16         9.16e-3  1.02e-2  1.25e-2  7.95e-3    7.75e-5 (base-w50)      2.14e-3 (base-w17)     1.55e-8 (base-w48, d4a)
  (three of these exceed the largest value of the 3- and 13-band cases above -- fp32 |gain - 1| 8.50e-7 against 8.43e-7, bf16x3-fast
  relative L2 9.92e-3 against 9.24e-3 and 1 - cosine 4.86e-5 against 4.26e-5 -- by less than a tenth of the 2 x margin; the constants in
  tests/forced_ref.py are those of the narrow cases, unchanged)
The bf16 bound (2.64e-2 / 1.65e-4 / 8.8e-3) sits under the 0.8 / 0.85 of tests/test_gpu_autograd.py by a factor of 30, fp32 (1.04e-5) under
2e-2, bf16x3 (3.8e-5) and bf16x3-fast (1.85e-2) under 6e-2, and rejects the four wiring mutations of tests/test_forced_ref_cpu.py -- the
1.02 scaling through |gain - 1| (2.0e-2 against 8.8e-3): relative L2 alone, at 2.64e-2, would have admitted it.
Two one-line mutations applied by hand to engine.py on the device (not committed): the weight gradient of e3b fed e3b's own table instead
of e3a's -> down2.mpconv.1.conv.3.weight at relative L2 1.65 in fp32 and bf16 (bf16x3 reads the split operand and no table: unchanged);
upsample2x_bwd of the second decoder stage reading the skip half of dcat instead of the upsampled half -> every tensor below it fails
in all four settings (inc.conv.conv.0.weight at relative L2 1.03).
"""
import functools

import pytest
import torch

from fabric_amd import BiDateNet
from oracle import filler
from tests import forced_ref as R

pytestmark = pytest.mark.gpu
SHAPES = {'s32': (2, 3, 32, 32), 's40x72': (3, 13, 40, 72), 's90': (2, 13, 90, 90),
          'w17': (2, 17, 32, 32), 'w48': (3, 48, 40, 24), 'w50': (2, 50, 16, 48)}          # first layer padded to 32, 48 and 64 channels
WIDE = ('w17', 'w48', 'w50')
# variant -> (shape, fusion, bn_mode, dlogits, dx, engine attributes, wgrad_stream)
VARIANTS = {
    'base-s32': ('s32', 'product', 'batch', 'tversky', True, {}, True),
    'base-s40x72': ('s40x72', 'product', 'batch', 'tversky', True, {}, True),
    'base-s90': ('s90', 'product', 'batch', 'tversky', True, {}, True),
    'absdiff': ('s40x72', 'absdiff', 'batch', 'tversky', True, {}, True),
    'running': ('s32', 'product', 'running', 'tversky', True, {}, True),
    'nodx': ('s90', 'product', 'batch', 'tversky', False, {}, True),
    'nofold': ('s40x72', 'product', 'batch', 'tversky', True, {'fold_bn_bwd': ()}, True),
    'nostream': ('s32', 'product', 'batch', 'tversky', True, {}, False),
    'gauss': ('s40x72', 'product', 'batch', 'gauss', True, {}, True),
    # above 16 bands: no input gradient (refused at the door), the first layer on bn_bwd + the generic weight-gradient GEMM
    'base-w17': ('w17', 'product', 'batch', 'tversky', False, {}, True),
    'base-w48': ('w48', 'product', 'batch', 'tversky', False, {}, True),
    'base-w50': ('w50', 'product', 'batch', 'tversky', False, {}, True),
    'running-w17': ('w17', 'product', 'running', 'tversky', False, {}, True),
}
FORWARDS = sorted({v[:3] for v in VARIANTS.values()})


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    b, c, h, w = SHAPES[shape]
    x1, x2, lbl = filler.make_inputs(b, c, h, seed=0, different_dates=True, size_w=w)
    return torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(lbl)


def _engine(prec, shape, fusion, attrs=None):
    model = filler.fill_module(BiDateNet(SHAPES[shape][1], 2, precision=prec, fusion=fusion)).cuda().train()
    eng = model.engine()
    for k, v in (attrs or {}).items():
        assert hasattr(eng, k)
        setattr(eng, k, v)
    return model, eng, {k: v.detach() for k, v in model.state_dict(keep_vars=True).items()}


def _forward(eng, P, shape, bn_mode):
    x1, x2, _ = (t.cuda() for t in _inputs(shape))
    logits, ws = eng.forward(x1, x2, P, training=True) if bn_mode == 'batch' else eng.forward(x1, x2, P, training=False, frozen=True)
    torch.cuda.synchronize()
    return x1, x2, logits, ws


def _dlogits(kind, logits, shape):
    if kind == 'tversky':
        return R.tversky_dlogits(logits.cpu(), _inputs(shape)[2])
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(logits.shape, generator=gen) * 1e-3
    g[torch.rand(logits.shape, generator=gen) < 0.3] = 0.0               # exact zeros
    return g


@functools.lru_cache(maxsize=None)
def _reference(prec, shape, fusion, bn_mode, dl_kind):
    """The engine's stored state after one forward of the DEFAULT engine, its forward audit, and the forced float64 gradients for this
    dlogits: computed once per key and shared; nobody writes into it.  Every variant of the key must reproduce the logits and the
    tables bit for bit (its forward is the same launches) before it is judged against these gradients."""
    model, eng, P = _engine(prec, shape, fusion)
    assert [(L.name, L.conv, L.bn) for L in eng.layers] == [(L['name'], L['conv'], L['bn']) for L in R.build_layers(SHAPES[shape][1])]
    x1, x2, logits, ws = _forward(eng, P, shape, bn_mode)
    st = R.state_from_workspace(eng, ws, P, x1, x2, logits, bn_mode=bn_mode)
    dl = _dlogits(dl_kind, logits, shape)
    audit, residual = {}, {}
    grads = R.forced_backward(st, dl, True, audit=audit, c_conv=R.C_CONV[prec], residual=residual)
    return dict(logits=st['logits'], bn=st['bn'], dlogits=dl, audit=audit, grads=grads, residual=residual)


@pytest.mark.parametrize('shape,fusion,bn_mode', FORWARDS)
@pytest.mark.parametrize('prec', R.PRECISIONS)
def test_forward_stages(prec, shape, fusion, bn_mode):
    audit = _reference(prec, shape, fusion, bn_mode, 'tversky')['audit']
    x3 = prec.startswith('bf16x3')
    assert len(audit) == (37 if x3 else 51), sorted(audit)
    conv = {s: a for s, a in audit.items() if a['kind'] == 'conv'}
    rest = {s: a for s, a in audit.items() if a['kind'] != 'conv'}
    c, cs = max((a['c'], s) for s, a in conv.items())
    worst = {}
    for s, a in rest.items():
        if a['ratio'] >= worst.get(a['kind'], (-1.0, ''))[0]:
            worst[a['kind']] = (a['ratio'], s)
    print(f'\n[{prec} {shape} {fusion} {bn_mode}] conv c = {c:.3e} @ {cs} (asserted {R.C_CONV[prec]:.3e}, ceiling {R.C_CEILING:.3e}); '
          + '; '.join(f'{k} {v[0]:.3f} of its bound @ {v[1]}' for k, v in sorted(worst.items())))
    assert len(conv) == 18 and sum(a['kind'] == 'table' for a in rest.values()) == 18
    assert R.C_CONV[prec] <= R.C_CEILING
    for s, a in conv.items():
        assert a['c'] <= R.C_CONV[prec], (s, a)
    for s, a in rest.items():
        assert a['ratio'] <= 1.0, (s, a)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('prec', R.PRECISIONS)
def test_backward(prec, variant, monkeypatch):
    shape, fusion, bn_mode, dl_kind, want_dx, attrs, stream = VARIANTS[variant]
    ref = _reference(prec, shape, fusion, bn_mode, dl_kind)
    model, eng, P = _engine(prec, shape, fusion, attrs)
    x1, x2, logits, ws = _forward(eng, P, shape, bn_mode)
    assert torch.equal(logits.cpu().double(), ref['logits']), 'the variant\'s forward is not the reference state\'s'
    assert all(torch.equal(ws.bn[L.name].cpu().double(), ref['bn'][L.name]) for L in eng.layers)
    b, c, h, w = SHAPES[shape]
    if variant == 'nodx' and prec != 'fp32':
        assert eng.first_wgrad_dtype(2 * b, h, w, b) is not None, 'the fused first weight gradient is not taken at this shape'
    if variant == 'nofold' and prec == 'bf16':
        by = {L.name: L for L in eng.layers}
        eng.fold_bn_bwd = ('e1b', 'd4a')
        assert eng.folds_bn_bwd(by['e1b'], h, w) and eng.folds_bn_bwd(by['d4a'], h, w), 'the default does not fold at this shape'
        eng.fold_bn_bwd = ()
    seen = []
    if shape in WIDE:
        # the opposite branch of 'nodx': the fused first-layer weight gradient refuses more than 16 padded channels, so the route audited
        # here is the BatchNorm backward as a pass of its own and bdn_conv3x3_wgrad_ex on the cp-channel operand with c real columns
        assert not want_dx and eng.cp == (c + 15) // 16 * 16 > 16
        assert eng.first_wgrad_dtype(2 * b, h, w, b) is None, 'the fused first weight gradient is taken above 16 padded channels'
        from fabric_amd import engine as engine_mod
        real = engine_mod.call
        monkeypatch.setattr(engine_mod, 'call', lambda name, *a: (seen.append((name, a)), real(name, *a))[1])
    grads = {k: torch.full_like(p, float('nan')) for k, p in model.named_parameters()}
    dx = (torch.full_like(x1, float('nan')), torch.full_like(x2, float('nan'))) if want_dx else None
    dl = ref['dlogits']
    eng.backward(ws, dl.cuda(), P, grads, dx=dx, bn_mode=bn_mode, wgrad_stream=stream)
    torch.cuda.synchronize()
    if shape in WIDE:
        names = [n for n, _ in seen]
        assert 'bdn_conv3x3_wgrad_bnbwd' not in names and 'bdn_conv3x3_dgrad_first' not in names
        # (dtype, dz, Cout, in0, C0, in1, C1, in_mode, in_bn, ipg, partial, dw, Cin_real, N, H, W, flags, stream)
        first = [a for n, a in seen if n == 'bdn_conv3x3_wgrad_ex' and a[11] == grads['inc.conv.conv.0.weight'].data_ptr()]
        assert len(first) == 1 and (first[0][4], first[0][12], first[0][13:16]) == (eng.cp, c, (2 * b, h, w)), first
        if eng.x3:     # dz of the first layer leaves its BatchNorm backward split (hi | lo): no float32 dz, no split pass
            kind, at = ('bdn_bn_bwd_apply_frozen', 6) if bn_mode == 'running' else ('bdn_bn_bwd_apply_split', 5)      # index of (N, H, W, C)
            assert [a for n, a in seen if n == kind and tuple(a[at:at + 4]) == (2 * b, h, w, 64)], 'no split BatchNorm backward at full size'
            assert not [a for n, a in seen if n == 'bdn_split_pack' and tuple(a[-4:-1]) == (2 * b, h, w)]
    got = dict(grads)
    if want_dx:
        got['dx1'], got['dx2'] = dx
    assert len(grads) == 74
    want = {k: v for k, v in ref['grads'].items() if k in got}
    assert set(want) == set(got)
    zero = R.bn_fed_conv_biases(c) if bn_mode == 'batch' else []
    cmp = R.compare(got, want, zero, ref['residual'])
    raw = max(float(want[k].norm()) for k in zero) if zero else 0.0
    live = {k: v for k, v in cmp.items() if k not in zero}
    rel, cos = max((v[0], k) for k, v in live.items()), max((1 - v[1], k) for k, v in live.items())
    gain = max((abs(v[2] - 1), k) for k, v in live.items())
    print(f'\n[{prec} {variant}] worst relative L2 {rel[0]:.3e} @ {rel[1]} (bound {R.GRAD_REL[prec]:.1e}); '
          f'worst 1 - cosine {cos[0]:.3e} @ {cos[1]} (bound {R.GRAD_1MCOS[prec]:.1e}); worst |gain - 1| {gain[0]:.3e} @ {gain[1]} '
          f'(bound {R.GRAD_GAIN[prec]:.1e}); ||dlogits|| {float(dl.norm()):.3e}; reference conv-bias '
          f'gradient {raw:.2e}, less the table-mean residual {max([cmp[k][1] for k in zero] or [0.0]):.2e}')
    for k, g in got.items():
        assert torch.isfinite(g).all(), k
    for k in zero:
        assert cmp[k][0] == 0.0 and cmp[k][1] < 1e-9 * float(dl.norm()), (k, cmp[k])
    bad = {k: tuple(f'{x:.3e}' for x in (v[0], 1 - v[1], abs(v[2] - 1))) for k, v in live.items()
           if not (v[0] <= R.GRAD_REL[prec] and 1 - v[1] <= R.GRAD_1MCOS[prec] and abs(v[2] - 1) <= R.GRAD_GAIN[prec])}
    assert not bad, f'{len(bad)} of {len(live)} tensors over the bound (relative L2, 1 - cosine, |gain - 1|): {bad}'
