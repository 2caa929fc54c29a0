"""-m gpu: the kernels on ill-conditioned VALUES (tests/illcond.py; the generators and references are pinned by tests/test_illcond_cpu.py).

The other GPU tests vary shapes and feed unit Gaussians; these keep the smallest shapes that reach each code path and vary what the
numbers are:

  A  BatchNorm statistics of maps whose per-channel |mean| / std runs from 0 to 256, and of exactly constant channels;
  B  BatchNorm backward on such maps;
  C  exact ties and exact zeros: first maximum wins (pooling, unpooling, every argmax), the ReLU mask is strict;
  D  loss kernels on saturated and shifted logits, degenerate label maps and labels >= ncls;
  E  the bf16 conversions at their rounding edges.

Bars.  Every tolerance is one this suite already uses for the same entry point, or 8 x the error of torch's float32 arithmetic on the
CPU evaluated on the same data inside the test (the reference's own rounding, times an allowance for tile-order summation), or, beyond
the required range of A / B, 4 x the error of the float32 restatement of the documented one-pass contract (tests/illcond.py).
The required range is |mean| / std <= illcond.REQUIRED_RATIO = max(4, 2 R0), R0 measured on the reference network.
Lines starting with COND carry the measured figures (pytest -s); DESIGN.md tabulates them.
"""
import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X3, IN_BNRELU, IN_PLAIN
from fabric_amd.criterion import REDUCE, Criterion
from oracle import bidate_oracle as O
from tests import criterion_ref as CR
from tests import guard
from tests import illcond as IC
from tests.guard import guarded
from tests.gpu_util import DT, assert_close, assert_masked, dev, frag_to_dense, from_nhwc, pack_w, preact, rnd, st, to_nhwc

pytestmark = pytest.mark.gpu
NAN = float('nan')
PRECS = ['fp32', 'bf16']
TOL_S = {'fp32': 5e-5, 'bf16': 2e-3, 'x3': 5e-5}        # test_conv3x3_forward_stats_finalize; bf16x3 writes float32 outputs and statistics: the float32 bar
INVSTD_CAP = float(np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5))))) * (1 + 2.0 ** -23)      # 1 / sqrt(eps), one ulp


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed)) * scale


# ================================================================= A. BatchNorm statistics under offset
def _bn_params(C):
    gamma = torch.rand(C, generator=_gen(6)) + 0.5
    beta = torch.rand(C, generator=_gen(7)) * 0.6 - 0.3
    rm0 = (torch.rand(C, generator=_gen(8)) * 0.2 + 0.1) * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    rv0 = torch.rand(C, generator=_gen(9)) + 0.5
    return gamma, beta, rm0, rv0


def _finalize(stats, nt, G, C, count, gamma, beta, rm0, rv0):
    drm, drv, dg, db = dev(rm0), dev(rv0), dev(gamma), dev(beta)
    nbt = guard.zeros(1, dtype=torch.int64)
    bn = guard.full((G, 4, C), NAN)
    fws = guard.full((max(_lib.load().bdn_bn_finalize_workspace_bytes(nt, G, C) // 8, 1),), NAN, dtype=torch.float64)
    _lib.call('bdn_bn_finalize', stats.data_ptr(), nt, G, C, count, dg.data_ptr(), db.data_ptr(), 1e-5, 0.1,
              drm.data_ptr(), drv.data_ptr(), nbt.data_ptr(), bn.data_ptr(), fws.data_ptr(), st())
    torch.cuda.synchronize()
    assert int(nbt.item()) == G
    return bn.cpu(), drm.cpu(), drv.cpu()


def _regimes(C, consts):
    """{nominal ratio: channel index tensor} of the sweep (the constant channels, when present, are the last two and are left out)."""
    nominal = IC.channel_ratios(C) if consts else np.array([IC.RATIOS[c % len(IC.RATIOS)] for c in range(C)])
    return {r: torch.from_numpy(np.nonzero(nominal == r)[0]) for r in IC.RATIOS}


def _judge_statistics(name, kind, groups, bn, rm, rv, rows, gamma, beta, rm0, rv0, consts=True):
    """The bars of A on the device's table bn [G,4,C] and running buffers for the float64 groups z64 [n,C,...]."""
    G, C = len(groups), groups[0].shape[1]
    tol = TOL_S[kind]
    count = groups[0].numel() // C
    assert torch.isfinite(bn).all() and torch.isfinite(rm).all() and torch.isfinite(rv).all(), f'{name}: non-finite statistics'
    assert (bn[:, 1] > 0).all() and (bn[:, 1] <= INVSTD_CAP).all(), f'{name}: invstd outside (0, 1/sqrt(eps)]'
    assert (rv.double() >= 0.9 ** G * rv0.double() * (1 - 1e-6)).all(), f'{name}: a negative variance reached running_var'
    ys32, rm32, rv32 = IC.bn_torch32(groups, gamma, beta, rm0, rv0)
    regimes = _regimes(C, consts)
    means, variances, inside_all = [], [], torch.ones(C, dtype=torch.bool)
    for g, zg in enumerate(groups):
        ratio = IC.achieved_ratio(zg)
        y64, mean, var = IC.bn_train64(zg, gamma, beta)
        means.append(mean); variances.append(var)
        e_dev = IC.affine_error(zg, bn[g, 2], bn[g, 3], y64)
        e_ref = IC.output_error(ys32[g], y64)
        tab, _ = IC.onepass_contract(zg, rows, gamma, beta)
        e_con = IC.affine_error(zg, tab[2], tab[3], y64)
        inside = ratio <= IC.REQUIRED_RATIO
        inside_all &= inside
        for r, ch in regimes.items():
            print(f'COND fwd {name} {kind} g{g} nominal {r:g} achieved {ratio[ch].min():.1f}..{ratio[ch].max():.1f} '
                  f'e_dev {e_dev[ch].max():.3e} e_ref {e_ref[ch].max():.3e} e_contract {e_con[ch].max():.3e}')
        bad = inside & (e_dev > torch.clamp(8 * e_ref, min=tol))
        assert not bad.any(), (f'{name} g{g}: inside the required range (ratio <= {IC.REQUIRED_RATIO:.2f}) e_dev exceeds max({tol:g}, 8 e_ref) in channels '
                               f'{bad.nonzero().flatten().tolist()}: e_dev {e_dev[bad].tolist()} e_ref {e_ref[bad].tolist()} ratio {ratio[bad].tolist()}')
        for r, ch in regimes.items():
            ch = ch[~inside[ch] & torch.isfinite(ratio[ch])]
            if len(ch):                               # beyond the required range: no worse than 4 x the documented contract in float32
                assert e_dev[ch].max() <= 4 * e_con[ch].max(), \
                    f'{name} g{g} ratio {r:g}: e_dev {e_dev[ch].max():.3e} > 4 x the one-pass contract {e_con[ch].max():.3e}'
        if consts:
            # exactly constant channels (ratio infinite: outside every error bar above).  The sum of n x 100.25 is exact in float32, so
            # the mean is; the variance is whatever s1 / n - mean^2 leaves of the rounding of the sum of squares, clamped at 0.
            assert bn[g, 0, C - 2].item() == IC.CONST_BIASES[0] and bn[g, 0, C - 1].item() == 0.0, f'{name} g{g}: mean of a constant channel'
            assert bn[g, 1, C - 1].item() == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5))))), f'{name} g{g}: invstd of the zero channel'
            assert bn[g, 3, C - 1].item() == beta[C - 1].item(), f'{name} g{g}: shift of the zero channel'
    rm64, rv64 = IC.running64(means, variances, count, rm0, rv0)
    for what, got, ref32, ref64 in (('running_mean', rm, rm32, rm64), ('running_var', rv, rv32, rv64)):
        for r, ch in regimes.items():
            ch = ch[inside_all[ch]]
            if not len(ch):
                continue
            scale = ref64[ch].abs().max()
            e_d, e_r = (got[ch].double() - ref64[ch]).abs().max() / scale, (ref32[ch].double() - ref64[ch]).abs().max() / scale
            print(f'COND fwd {name} {kind} {what} nominal {r:g} e_dev {e_d:.3e} e_ref {e_r:.3e}')
            assert e_d <= max(tol, 8 * e_r.item()), f'{name} {what} ratio {r:g}: {e_d:.3e} > max({tol:g}, 8 x {e_r:.3e})'


FWD_CASES = [(2, 16, 16, 64, 64, 1), (4, 8, 8, 128, 128, 2), (2, 13, 15, 64, 64, 2)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', FWD_CASES, ids=str)
@guarded
def test_conv_statistics_under_offset(prec, case):
    """bdn_conv3x3 (stats_partial) + bdn_bn_finalize: 16x16 tiles, two 8x8 images per tile, and ragged tiles."""
    N, H, W, Cin, Cout, ipg = case
    dt, td = DT[prec]
    G = N // ipg
    x, w, b, z64 = IC.offset_conv_case(prec, N, Cin, Cout, (H, W), seed=11)
    wf, _ = pack_w(prec, w, Cin)
    d0, db = to_nhwc(prec, x), dev(b)
    out = guard.full((N, H, W, Cout), NAN, dtype=td)
    nt = _lib.load().bdn_conv3x3_num_mtiles(N, H, W, Cout, ipg)
    stats = guard.full((nt, 2, Cout), NAN)
    _lib.call('bdn_conv3x3', dt, d0.data_ptr(), Cin, None, 0, IN_PLAIN, None, ipg, wf.data_ptr(), db.data_ptr(), out.data_ptr(),
              stats.data_ptr(), N, H, W, Cout, st())
    torch.cuda.synchronize()
    assert_close('conv out', from_nhwc(out), z64.float(), 2e-5 if prec == 'fp32' else 1e-2)
    params = _bn_params(Cout)
    bn, rm, rv = _finalize(stats, nt, G, Cout, ipg * H * W, *params)
    _judge_statistics(f'conv3x3{case}', prec, [z64[g * ipg:(g + 1) * ipg] for g in range(G)], bn, rm, rv, nt // G, *params)


@guarded
def test_x3src_statistics_under_offset():
    """bdn_conv3x3_x3src (BDN_BF16X3: float32 operand split inside the staging) + bdn_bn_finalize."""
    N, H, W, Cin, Cout, ipg = 2, 16, 16, 64, 64, 1
    G = N // ipg
    x, w, b, z64 = IC.offset_conv_case('fp32', N, Cin, Cout, (H, W), seed=12)
    xd, bd, wdev = to_nhwc('fp32', x), dev(b), dev(w)
    wf = guard.empty(Cout, 9, 3 * Cin, dtype=torch.bfloat16)
    _lib.call('bdn_pack_weights', BDN_BF16X3, wdev.data_ptr(), wf.data_ptr(), None, Cout, Cin, Cin, st())
    nt = _lib.load().bdn_conv3x3_num_mtiles_ex(BDN_BF16X3, N, H, W, Cin, Cout, ipg)
    out = guard.full((N, H, W, Cout), NAN)
    stats = guard.full((nt, 2, Cout), NAN)
    _lib.call('bdn_conv3x3_x3src', BDN_BF16X3, xd.data_ptr(), Cin, IN_PLAIN, None, ipg, wf.data_ptr(), bd.data_ptr(), out.data_ptr(),
              stats.data_ptr(), None, N, H, W, Cout, st())
    torch.cuda.synchronize()
    assert_close('x3src out', from_nhwc(out), z64.float(), 1e-4)
    params = _bn_params(Cout)
    bn, rm, rv = _finalize(stats, nt, G, Cout, ipg * H * W, *params)
    _judge_statistics('x3src', 'x3', [z64[g * ipg:(g + 1) * ipg] for g in range(G)], bn, rm, rv, nt // G, *params)


@pytest.mark.parametrize('prec', PRECS)
@guarded
def test_conv3d_statistics_under_offset(prec):
    """bdn_conv3d's statistics epilogue at the smallest case of tests/test_gpu_conv3d.py."""
    N, D, H, W, Cin, Cout = 1, 1, 16, 16, 64, 64
    dt, td = DT[prec]
    x, w, b, z64 = IC.offset_conv_case(prec, N, Cin, Cout, (D, H, W), seed=13)
    view = dev(w.permute(0, 2, 1, 3, 4).reshape(Cout, 3 * Cin, 3, 3).contiguous())          # input channel kd * Cin + c (include/bidate_hip.h)
    wf = guard.empty(Cout, 9, 3 * Cin, dtype=td)
    _lib.call('bdn_pack_weights', dt, view.data_ptr(), wf.data_ptr(), None, Cout, 3 * Cin, 3 * Cin, st())
    xd = guard.guard(x.permute(0, 2, 3, 4, 1).contiguous().to(td))
    bd = dev(b)
    out = guard.full((N, D, H, W, Cout), NAN, dtype=td)
    nt = _lib.load().bdn_conv3d_num_mtiles(N, D, H, W)
    stats = guard.full((nt, 2, Cout), NAN)
    _lib.call('bdn_conv3d', dt, xd.data_ptr(), Cin, IN_PLAIN, None, N, wf.data_ptr(), bd.data_ptr(), out.data_ptr(), stats.data_ptr(),
              N, D, H, W, Cout, st())
    torch.cuda.synchronize()
    assert_close('conv3d out', out.float().cpu().permute(0, 4, 1, 2, 3), z64.float(), 2e-5 if prec == 'fp32' else 1e-2)
    params = _bn_params(Cout)
    bn, rm, rv = _finalize(stats, nt, 1, Cout, N * D * H * W, *params)
    _judge_statistics('conv3d', prec, [z64], bn, rm, rv, nt, *params)


@guarded
def test_two_stage_finalize_under_offset():
    """bdn_bn_finalize above 512 partial rows per group (reduce_rows_kernel + bn_finalize_kernel): 513 rows, the smallest such case of
    tests/launch_cases.py STATS_CASES, 64 values per row; the rows are the contract's float32 sums of a map with the ratio sweep."""
    rpg, G, C, per = 513, 1, 192, 64
    count = rpg * per
    r = np.random.default_rng(14)
    std = r.uniform(0.5, 2.0, C)
    ratio = np.array([IC.RATIOS[c % len(IC.RATIOS)] for c in range(C)])
    v = ((ratio * std)[None] + std[None] * r.standard_normal((count, C))).astype(np.float32)
    z64 = torch.from_numpy(v.astype(np.float64)).t().reshape(1, C, count, 1)
    part = torch.from_numpy(IC.tile_sums_f32(v, rpg))
    params = _bn_params(C)
    bn, rm, rv = _finalize(dev(part), rpg, G, C, count, *params)
    _judge_statistics('finalize513', 'fp32', [z64], bn, rm, rv, rpg, *params, consts=False)
    tab, _ = IC.finalize_contract(part.numpy(), count, params[0], params[1])            # same partial rows: the table is the contract's, to rounding
    for i, row in enumerate(('mean', 'invstd', 'scale', 'shift')):
        assert_close(f'{row} vs contract', bn[0, i], tab[i], 1e-6)


# ================================================================= D. loss kernels at the extremes
LOSS_TOL, GRAD_TOL = 5e-6, 3e-4                        # tests/test_gpu_losses.py, tests/test_gpu_criterion.py
LOSS_SHAPES = [(3, 2, 24, 20), (2, 3, 16, 300)]
OVERLAPS = [('tversky', 0.1, 0.9, 1e-7), ('dice', 0.5, 0.5, 0.5e-7), ('jaccard', 1.0, 1.0, 1e-7)]
FOCALS = [(g, a, sa) for g in (0.0, 0.5, 2.0) for a in (False, True) for sa in (1, 0)]


def _class_alpha(C):
    return [0.25, 0.75] if C == 2 else [round(0.1 + 0.8 * k / (C - 1), 3) for k in range(C)]


def _outputs(shape):
    return guard.full((1,), NAN), guard.full((4,), -1, dtype=torch.int32), guard.full(tuple(shape), NAN)


def _run_losses(logits, labels):
    """Every loss entry point on one (logits, labels): {name: (criterion, loss, counts, dlogits, terms or None)} as CPU tensors."""
    B, C, H, W = logits.shape
    lib = _lib.load()
    lg_d, lb_d = dev(logits), guard.guard(labels.to(torch.uint8))
    a_d = dev(torch.tensor(_class_alpha(C)))                       # exactly ncls floats in a guarded buffer: an index >= ncls reads the guard
    out = {}
    for name, al, be, eps in OVERLAPS:
        for reduce, rw in REDUCE.items():
            if name == 'tversky' and rw == 0:                      # bdn_tversky is bdn_overlap_loss(reduce_w = 0)
                ws = guard.alloc_bytes(lib.bdn_overlap_workspace_bytes(B, C, H, W, 0))
                loss, counts, dl = _outputs(logits.shape)
                _lib.call('bdn_tversky', lg_d.data_ptr(), lb_d.data_ptr(), al, be, eps, ws.data_ptr(), loss.data_ptr(), counts.data_ptr(),
                          dl.data_ptr(), B, C, H, W, st())
                out['bdn_tversky'] = (Criterion(1.0, al, be, eps, reduce), loss, counts, dl, None)
            ws = guard.alloc_bytes(lib.bdn_overlap_workspace_bytes(B, C, H, W, rw))
            loss, counts, dl = _outputs(logits.shape)
            _lib.call('bdn_overlap_loss', lg_d.data_ptr(), lb_d.data_ptr(), al, be, eps, rw, ws.data_ptr(), loss.data_ptr(), counts.data_ptr(),
                      dl.data_ptr(), B, C, H, W, st())
            out[f'overlap {name} {reduce}'] = (Criterion(1.0, al, be, eps, reduce), loss, counts, dl, None)
    for gamma, with_alpha, sa in FOCALS:
        ws = guard.alloc_bytes(lib.bdn_focal_workspace_bytes())
        loss, counts, dl = _outputs(logits.shape)
        _lib.call('bdn_focal', lg_d.data_ptr(), lb_d.data_ptr(), gamma, a_d.data_ptr() if with_alpha else None, sa, ws.data_ptr(),
                  loss.data_ptr(), counts.data_ptr(), dl.data_ptr(), B, C, H, W, st())
        c = Criterion(0.0, w_focal=1.0, gamma=gamma, class_alpha=_class_alpha(C) if with_alpha else None, size_average=bool(sa))
        out[f'focal g{gamma} alpha{int(with_alpha)} avg{sa}'] = (c, loss, counts, dl, None)
    compound = [Criterion(2.0, 0.1, 0.9, 1e-7, 'columns', w_focal=0.25, gamma=2.0, class_alpha=_class_alpha(C)),
                Criterion(0.5, 0.5, 0.5, 0.5e-7, 'image', w_focal=3.0, gamma=0.5, class_alpha=None),
                Criterion(0.0, w_focal=2.0, gamma=2.0, class_alpha=None),                        # the compound kernels with the focal term alone
                Criterion(0.0, w_focal=2.0, gamma=2.0, class_alpha=_class_alpha(C), size_average=False)]
    for i, c in enumerate(compound):
        ws = guard.alloc_bytes(lib.bdn_criterion_workspace_bytes(B, C, H, W, REDUCE[c.reduce]))
        loss, counts, dl = _outputs(logits.shape)
        terms = guard.full((2,), NAN)
        _lib.call('bdn_criterion', lg_d.data_ptr(), lb_d.data_ptr(), c.w_overlap, c.alpha, c.beta, c.eps, REDUCE[c.reduce], c.w_focal, c.gamma,
                  a_d.data_ptr() if c.class_alpha is not None else None, int(c.size_average), ws.data_ptr(), loss.data_ptr(), terms.data_ptr(),
                  counts.data_ptr(), dl.data_ptr(), B, C, H, W, st())
        out[f'criterion {i}'] = (c, loss, counts, dl, terms)
    torch.cuda.synchronize()
    return {k: (c, loss.cpu(), counts.cpu(), dl.cpu(), None if terms is None else terms.cpu()) for k, (c, loss, counts, dl, terms) in out.items()}


def _bounds(c, ref):
    return (LOSS_TOL * (c.w_overlap * max(1.0, abs(ref['overlap'])) + c.w_focal * max(1.0, abs(ref['focal']))),
            GRAD_TOL * (c.w_overlap * ref['doverlap'].abs().max().item() + c.w_focal * ref['dfocal'].abs().max().item()))


def _check_losses(tag, logits, labels, res):
    """Every entry of _run_losses against the float64 restatement (tests/criterion_ref.py) with the suite's bars; returns the references."""
    want_counts = IC.argmax_counts(logits, labels)
    refs = {}
    for name, (c, loss, counts, dl, terms) in res.items():
        ref = refs[name] = CR.reference(c, logits, labels.long())
        lb, gb = _bounds(c, ref)
        e_l, e_g = abs(loss.item() - ref['loss']), (dl.double() - ref['dloss']).abs().max().item()
        print(f'COND loss {tag} {name}: loss {loss.item():.9g} ref {ref["loss"]:.9g} |err| {e_l:.2e} (bar {lb:.2e})  dlogits err {e_g:.2e} (bar {gb:.2e})')
        assert torch.isfinite(loss).all() and torch.isfinite(dl).all(), f'{tag} {name}: non-finite loss or gradient'
        assert e_l <= lb, f'{tag} {name}: loss {loss.item():.9g} vs {ref["loss"]:.9g}, |err| {e_l:.3e} > {lb:.3e}'
        assert e_g <= gb, f'{tag} {name}: dlogits err {e_g:.3e} > {gb:.3e}'
        assert counts.tolist() == want_counts, f'{tag} {name}: counts {counts.tolist()} != {want_counts}'
        if terms is not None:
            t = terms.tolist()
            for i, key, wgt in ((0, 'overlap', c.w_overlap), (1, 'focal', c.w_focal)):       # (the restatement does not evaluate a term of weight 0)
                assert wgt == 0 or abs(t[i] - ref[key]) <= LOSS_TOL * max(1.0, abs(ref[key])), f'{tag} {name}: {key} term {t[i]:.9g} vs {ref[key]:.9g}'
    return refs


@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=str)
@guarded
def test_losses_on_saturated_logits(shape):
    logits, labels = IC.saturated_logits(shape, 21), IC.mixed_labels(shape, shape[1], 22)
    _check_losses('saturated', logits, labels, _run_losses(logits, labels))


@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=str)
@guarded
def test_losses_are_shift_invariant(shape):
    """softmax(l) = softmax(l + 8192): loss, terms, counts and dlogits of the two calls agree within the bar (and each with float64)."""
    logits, labels = IC.quarter_grid_logits(shape, 23), IC.mixed_labels(shape, shape[1], 24)
    shifted = logits + 8192.0
    assert torch.equal(shifted - 8192.0, logits)
    a, b = _run_losses(logits, labels), _run_losses(shifted, labels)
    refs = _check_losses('grid', logits, labels, a)
    _check_losses('grid+8192', shifted, labels, b)
    for name in a:
        c, la, ca, da, ta = a[name]
        _, lb_, cb, db_, tb = b[name]
        lbar, gbar = _bounds(c, refs[name])
        assert abs(la.item() - lb_.item()) <= lbar, f'{name}: loss moves by {abs(la.item() - lb_.item()):.3e} under a shift of 8192 (bar {lbar:.3e})'
        assert (da - db_).abs().max().item() <= gbar, f'{name}: dlogits move by {(da - db_).abs().max().item():.3e} under a shift (bar {gbar:.3e})'
        assert torch.equal(ca, cb)
        if ta is not None:
            assert (ta - tb).abs().max().item() <= LOSS_TOL * max(1.0, abs(refs[name]['overlap']), abs(refs[name]['focal']))


@pytest.mark.parametrize('kind', ['zeros', 'ones', 'columns', 'image'])
@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=str)
@guarded
def test_losses_on_degenerate_labels(shape, kind):
    """All background, all positive, columns without / with only positives (the reduce_w = 0 cells), one image entirely one class."""
    logits = IC.quarter_grid_logits(shape, 25) * 0.75 + _rand(shape, 26, 0.5)
    labels = IC.degenerate_labels(shape, shape[1], kind, 27)
    _check_losses(kind, logits, labels, _run_losses(logits, labels))


@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=str)
@guarded
def test_losses_with_labels_outside_the_classes(shape):
    """10 % of the pixels labelled 255, ncls or 7 (include/bidate_hip.h, "labels outside the classes"; ncls and 7 lie inside the kernels'
    8-wide class arrays, 255 outside): no true class -- FP of every class in the
    overlap terms, focal term and focal gradient exactly 0, still counted in the size_average denominator, never a correct prediction, and
    the class weights (a guarded buffer of exactly ncls floats) are not indexed with it.  The three focal code paths (bdn_focal, the
    compound statistics pass, the compound gradient pass) agree."""
    B, C, H, W = shape
    logits = _rand(shape, 28, 3.0)
    labels = IC.void_labels(shape, C, 29)
    void = (labels >= C)[:, None].expand(B, C, H, W)
    assert 0.05 < void.double().mean() < 0.15 and all((labels == k).double().mean() > 0.02 for k in (C, 7, 255))
    res = _run_losses(logits, labels)
    for name, (c, loss, counts, dl, terms) in res.items():
        if c.w_overlap == 0:                                      # focal alone, through bdn_focal and through the compound kernels
            assert torch.isfinite(loss).all(), f'{name}: loss {loss.item()} with labels >= ncls'
            assert (dl[void] == 0).all(), f'{name}: focal gradient of a pixel labelled >= ncls is not exactly 0'
    _check_losses('void', logits, labels, res)
    # the compound kernels' focal term against bdn_focal's value on the same (gamma, alpha, size_average)
    pairs = [('criterion 2', 'focal g2.0 alpha0 avg1'), ('criterion 3', 'focal g2.0 alpha1 avg0')]
    for comp, single in pairs:
        t, v = res[comp][4][1].item(), res[single][1].item()
        assert abs(t - v) <= LOSS_TOL * max(1.0, abs(v)), f'{comp}: focal term {t:.9g} vs bdn_focal {v:.9g}'
        assert (res[comp][3] - 2.0 * res[single][3]).abs().max() <= GRAD_TOL * 2.0 * res[single][3].abs().max()
    assert res['bdn_tversky'][2].tolist()[3] == int((IC.first_argmax(logits) == labels.long()).sum())


# ================================================================= C (argmax). first maximum wins
@pytest.mark.parametrize('ncls', [2, 3])
@guarded
def test_argmax_ties(ncls):
    shape = (3, ncls, 24, 20)
    logits = IC.tied_logits(shape, 31)
    assert IC.max_tie_share(logits) >= 0.3
    lg_d = dev(logits)
    out = guard.full((3, 24, 20), 255, dtype=torch.uint8)
    _lib.call('bdn_argmax', lg_d.data_ptr(), out.data_ptr(), 3, ncls, 24, 20, st())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().long(), IC.first_argmax(logits))


@pytest.mark.parametrize('ncls', [2, 3])
@guarded
def test_blend_finalize_ties(ncls):
    """acc / wsum with wsum a power of two is exact, so the planted ties survive the division: mask = first maximum of the probabilities."""
    H, W = 24, 20
    acc = IC.tied_logits((1, ncls, H, W), 32)[0] + 2.0             # {0, 1, 2, 3}: the tie structure of the generator, non-negative
    wsum = torch.from_numpy(2.0 ** np.random.default_rng(33).integers(-2, 3, (H, W))).float()
    want_p = acc / wsum[None]
    assert IC.max_tie_share(want_p[None]) >= 0.3
    acc_d, ws_d = dev(acc), dev(wsum)
    mask = guard.full((H, W), 255, dtype=torch.uint8)
    _lib.call('bdn_blend_finalize', acc_d.data_ptr(), ws_d.data_ptr(), mask.data_ptr(), ncls, H, W, st())
    torch.cuda.synchronize()
    assert torch.equal(acc_d.cpu(), want_p)
    assert torch.equal(mask.cpu().long(), IC.first_argmax(want_p[None])[0])


@pytest.mark.parametrize('prec', PRECS)
@guarded
def test_eval_classifier_ties(prec):
    """bdn_conv3x3_eval_cls with a classifier whose two rows are equal on channels [0, 32) and differ on [32, 64), and a stage whose
    channels [32, 64) are all off in half of the pixels: there the two logits are the same sums and tie exactly; class 0 must win."""
    N, H, W, C = 2, 24, 20, 64
    dt, td = DT[prec]
    x = rnd(prec, _rand((N, C, H, W), 34))
    x[:, 0] = torch.where(torch.rand((N, H, W), generator=_gen(35)) < 0.5, -1.0, 1.0)
    w = _rand((C, C, 3, 3), 36, (2.0 / (9 * C)) ** 0.5)
    w[32:] = 0.0
    w[32:, 0, 1, 1] = torch.rand(32, generator=_gen(37)) + 0.5      # channels >= 32: relu(k x0), off wherever x0 = -1
    sc, sh = torch.ones(C), torch.zeros(C)
    sh[:32] = _rand((32,), 38, 0.3)
    cw = _rand((2, C), 39, 0.2)
    cw[1, :32] = cw[0, :32]
    cb = torch.full((2,), 0.125)
    wf, _ = pack_w(prec, w, C)
    d0, dsc, dsh, dcw, dcb = to_nhwc(prec, x), dev(sc), dev(sh), dev(cw), dev(cb)
    logits = guard.full((N, 2, H, W), NAN)
    mask = guard.full((N, H, W), 255, dtype=torch.uint8)
    _lib.call('bdn_conv3x3_eval_cls', dt, d0.data_ptr(), C, wf.data_ptr(), dsc.data_ptr(), dsh.data_ptr(), None,
              dcw.data_ptr(), dcb.data_ptr(), 2, logits.data_ptr(), mask.data_ptr(), None, 0, 0, N, H, W, C, st())
    torch.cuda.synchronize()
    lg = logits.cpu()
    tied = lg[:, 0] == lg[:, 1]
    assert torch.equal(tied, x[:, 0] < 0), 'the logits tie exactly where (and only where) the differing channels are off'
    assert tied.double().mean() >= 0.3
    assert torch.equal(mask.cpu().long(), IC.first_argmax(lg))
    assert (mask.cpu()[tied] == 0).all()


@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=str)
@guarded
def test_loss_counts_on_tied_logits(shape):
    """counts of bdn_tversky / bdn_overlap_loss / bdn_focal / bdn_criterion == torch.max(logits, 1) on the CPU (_check_losses)."""
    logits, labels = IC.tied_logits(shape, 40), IC.mixed_labels(shape, shape[1], 41)
    assert IC.max_tie_share(logits) >= 0.3
    _check_losses('tied', logits, labels, _run_losses(logits, labels))


# ================================================================= E. bf16 rounding edges
EDGE_SHAPES = [(2, 9, 7, 16), (4, 12, 20, 128)]                    # test_split_pack_is_the_exact_hi_lo_split


def _edges(N, H, W, C, seed):
    v, kind = IC.bf16_edge_values(N * C * H * W, seed)
    return v.reshape(N, C, H, W), kind.reshape(N, C, H, W)


def _nhwc_bits(t_nchw_bf16):
    return IC.bits16(t_nchw_bf16.permute(0, 2, 3, 1).contiguous())


def _assert_bits(name, got_bits, want_bits, kind_nhwc):
    """Exact int16 equality, reported per input class (illcond.bf16_edge_values) so a miss names the class that rounds differently."""
    names = ['tie-even', 'tie-odd', 'below-tie', 'above-tie', 'carry', 'random', 'subnormal', 'zero']
    bad = got_bits != want_bits
    if bad.any():
        per = {names[k]: int(bad[kind_nhwc == k].sum()) for k in range(8) if bad[kind_nhwc == k].any()}
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f'{name}: {int(bad.sum())} of {bad.numel()} bf16 bit patterns differ, by input class {per}; first at {i}: '
                             f'got {int(got_bits[tuple(i)]) & 0xffff:#06x} want {int(want_bits[tuple(i)]) & 0xffff:#06x}')


@pytest.mark.parametrize('bnrelu', [False, True])
@pytest.mark.parametrize('shape', EDGE_SHAPES, ids=str)
@guarded
def test_split_pack_at_the_rounding_edges(shape, bnrelu):
    """bdn_split_pack, plain and with BatchNorm+ReLU on load at scale 1, shift 0 (relu(fma(x, 1, 0)) = relu(x) exactly)."""
    N, H, W, C = shape
    x, kind = _edges(N, H, W, C, 51)
    a = torch.where(x > 0, x, torch.zeros_like(x)) if bnrelu else x
    hi, lo = IC.split_ref(a)
    want = torch.cat([_nhwc_bits(hi), _nhwc_bits(lo)], -1)
    bn = torch.zeros(2, 4, C); bn[:, 1:3] = 1.0
    out = guard.full((N, H, W, 2 * C), NAN, dtype=torch.bfloat16)
    xd, bn_d = to_nhwc('fp32', x), dev(bn)
    _lib.call('bdn_split_pack', xd.data_ptr(), C, None, 0, IN_BNRELU if bnrelu else IN_PLAIN, bn_d.data_ptr(), N // 2, out.data_ptr(),
              N, H, W, st())
    torch.cuda.synchronize()
    k = kind.permute(0, 2, 3, 1)
    _assert_bits('split_pack', IC.bits16(out.cpu()), want, torch.cat([k, k], -1))


@pytest.mark.parametrize('shape', EDGE_SHAPES, ids=str)
@guarded
def test_pack_input_at_the_rounding_edges(shape):
    N, H, W, C = shape
    B = N // 2
    x, kind = _edges(N, H, W, C, 52)
    a, b = dev(x[:B]), dev(x[B:])
    k = kind.permute(0, 2, 3, 1)
    out = guard.full((N, H, W, C), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_pack_input', BDN_BF16, a.data_ptr(), b.data_ptr(), out.data_ptr(), B, C, H, W, C, st())
    out3 = guard.full((N, H, W, 2 * C), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_pack_input', BDN_BF16X3, a.data_ptr(), b.data_ptr(), out3.data_ptr(), B, C, H, W, C, st())
    torch.cuda.synchronize()
    hi, lo = IC.split_ref(x)
    _assert_bits('pack_input bf16', IC.bits16(out.cpu()), _nhwc_bits(hi), k)
    _assert_bits('pack_input bf16x3', IC.bits16(out3.cpu()), torch.cat([_nhwc_bits(hi), _nhwc_bits(lo)], -1), torch.cat([k, k], -1))


@pytest.mark.parametrize('layer', [(64, 16, 32), (128, 128, 128)], ids=str)
@guarded
def test_pack_weights_at_the_rounding_edges(layer):
    Cout, Cin, Cp = layer
    v, kind = IC.bf16_edge_values(Cout * Cin * 9, 53)
    w, kind = v.reshape(Cout, Cin, 3, 3), kind.reshape(Cout, Cin, 3, 3)
    hi, lo = IC.split_ref(w)
    fwd = lambda t: t.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)                              # [co][tap][ci]
    rot = lambda t: torch.flip(t, (2, 3)).permute(1, 2, 3, 0).reshape(Cin, 9, Cout)          # [ci][tap][co], taps rotated by 180 degrees
    wdev = dev(w)
    wf = guard.full((Cout, 9, Cp), NAN, dtype=torch.bfloat16)
    wd = guard.full((Cp, 9, Cout), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_pack_weights', BDN_BF16, wdev.data_ptr(), wf.data_ptr(), wd.data_ptr(), Cout, Cin, Cp, st())
    wf3 = guard.full((Cout, 9, 3 * Cp), NAN, dtype=torch.bfloat16)
    wd3 = guard.full((Cp, 9, 3 * Cout), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_pack_weights', BDN_BF16X3, wdev.data_ptr(), wf3.data_ptr(), wd3.data_ptr(), Cout, Cin, Cp, st())
    torch.cuda.synchronize()
    bits = lambda frag, rows, cols: frag_to_dense('bf16', IC.bits16(frag.cpu()), rows, cols).to(torch.int16)
    hb, lb = IC.bits16(hi), IC.bits16(lo)
    f, d = bits(wf, Cout, Cp), bits(wd, Cp, Cout)
    _assert_bits('pack_weights bf16 forward image', f[:, :, :Cin], fwd(hb), fwd(kind))
    _assert_bits('pack_weights bf16 data-gradient image', d[:Cin], rot(hb), rot(kind))
    assert (f[:, :, Cin:] == 0).all() and (d[Cin:] == 0).all()
    f3, d3 = bits(wf3, Cout, 3 * Cp), bits(wd3, Cp, 3 * Cout)
    for j, part in enumerate((hb, hb, lb)):                                                  # [w_hi | w_hi | w_lo]
        _assert_bits(f'pack_weights bf16x3 forward image part {j}', f3[:, :, j * Cp:j * Cp + Cin], fwd(part), fwd(kind))
        _assert_bits(f'pack_weights bf16x3 data-gradient image part {j}', d3[:Cin, :, j * Cout:(j + 1) * Cout], rot(part), rot(kind))


# ================================================================= B. BatchNorm backward under offset
def _gamma_beta(C):
    gamma = torch.rand(C, generator=_gen(33)) + 0.5
    gamma[::7] *= -1
    return gamma, torch.rand(C, generator=_gen(34)) * 0.6 - 0.3


def _ratios(z, ipg):
    """Largest achieved |mean| / std per channel over the statistic groups of z [N,C,H,W]."""
    return torch.stack([IC.achieved_ratio(z[i:i + ipg].double()) for i in range(0, z.shape[0], ipg)]).amax(0)


SWITCH_BAND = 1e-4          # test_conv3x3_dgrad_with_bn_backward_on_load's band around the ReLU's switching point


def _clear_of_the_switch(name, z, bn, ipg, dA):
    """dA with the pixels within SWITCH_BAND of the ReLU's switching point zeroed, as test_conv3x3_dgrad_with_bn_backward_on_load does:
    there the kernel's float32 pre-activation (one FMA on the float32 table; good to 256 x 2^-24 x |scale| ~ 3e-5 at |mean| / std = 256)
    and the float64 statistics of the autograd reference may disagree about the mask, and one flipped pixel is an error of |scale dA|.
    The share of pixels this removes is printed and bounded: at most 1 in 1000 (the band holds 2e-4 of a unit-variance pre-activation)."""
    pre = preact(z, bn, ipg)
    keep = pre.abs() > SWITCH_BAND
    share = 1.0 - keep.double().mean().item()
    print(f'COND bwd {name}: {int((~keep).sum())} of {keep.numel()} pixels ({share:.1e}) lie within {SWITCH_BAND:g} of the switching point and carry no gradient')
    assert share <= 1e-3
    return dA * keep, pre


def _judge_backward(name, kind, ratio, got, ref64, ref32, tols):
    """got / ref64 / ref32: (dz [N,C,H,W] or None, dgamma [C], dbeta [C]).  Inside the required range every channel meets
    max(existing tolerance, 8 x the float32 reference's error); beyond it the values are finite and the curve is printed."""
    inside = ratio <= IC.REQUIRED_RATIO
    assert inside.sum() >= 8
    for what, g, r64, r32, tol in zip(('dz', 'dgamma', 'dbeta'), got, ref64, ref32, tols):
        if g is None:
            continue
        assert torch.isfinite(g).all(), f'{name} {what}: non-finite values'
        if what == 'dz':
            e_dev, e_ref = IC.per_channel_error(g, r64), IC.per_channel_error(r32, r64)
        else:                                        # per-channel scalars: against the tensor's magnitude, as assert_close measures them
            m = r64.double().abs().max()
            e_dev, e_ref = (g.double() - r64.double()).abs() / m, (r32.double() - r64.double()).abs() / m
        for r in IC.RATIOS:
            ch = torch.from_numpy(np.nonzero(np.array([IC.RATIOS[c % len(IC.RATIOS)] for c in range(len(ratio))]) == r)[0])
            print(f'COND bwd {name} {kind} {what} nominal {r:g} achieved {ratio[ch].min():.1f}..{ratio[ch].max():.1f} '
                  f'e_dev {e_dev[ch].max():.3e} e_ref {e_ref[ch].max():.3e}')
        bad = inside & (e_dev > torch.clamp(8 * e_ref, min=tol))
        assert not bad.any(), (f'{name} {what}: inside the required range e_dev exceeds max({tol:g}, 8 e_ref) in channels {bad.nonzero().flatten().tolist()}: '
                               f'e_dev {e_dev[bad].tolist()} e_ref {e_ref[bad].tolist()} ratio {ratio[bad].tolist()}')


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', [(4, 16, 16, 64, 2, 0), (2, 9, 7, 128, 1, 64)], ids=str)
@guarded
def test_bn_bwd_under_offset(prec, case):
    N, H, W, C, ipg, extra = case
    dt, td = DT[prec]
    G, ld = N // ipg, C + extra
    z = IC.offset_map(prec, N, C, H, W, seed=61)
    gamma, beta = _gamma_beta(C)
    bn = IC.true_table(z, ipg, gamma, beta)
    dA_full = rnd(prec, _rand((N, ld, H, W), 62))
    dA_full[:, extra:], _ = _clear_of_the_switch(f'bn_bwd{case} {prec}', z, bn, ipg, dA_full[:, extra:])
    gd = dA_full[:, extra:]
    ref64 = IC.bn_relu_backward(z, gd, gamma, beta, ipg)
    ref32 = IC.bn_relu_backward(z, gd, gamma, beta, ipg, torch.float32)
    dz_d = guard.full((N, H, W, C), NAN, dtype=td)
    dA_d = to_nhwc(prec, dA_full)
    dA_d[..., :extra] = NAN
    z_d, bn_d = to_nhwc(prec, z), dev(bn)
    wsb = guard.empty(_lib.load().bdn_bn_bwd_workspace_bytes(dt, N, H, W, C, ipg) // 4)
    sums, dgam, dbet = guard.empty(G, 2, C), guard.empty(C), guard.empty(C)
    es = 2 if prec == 'bf16' else 4
    _lib.call('bdn_bn_bwd', dt, dA_d.data_ptr() + extra * es, ld, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C,
              wsb.data_ptr(), sums.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dz_d.data_ptr(), st())
    torch.cuda.synchronize()
    _judge_backward(f'bn_bwd{case}', prec, _ratios(z, ipg), (from_nhwc(dz_d), dgam.cpu(), dbet.cpu()), ref64, ref32,
                    (1e-4 if prec == 'fp32' else 1e-2, 1e-4, 1e-4))                      # test_bn_bwd's bars


@pytest.mark.parametrize('prec', PRECS)
@guarded
def test_fused_bn_bwd_statistics_under_offset(prec):
    """bdn_conv3x3_dgrad_bs partials (sum g, sum g z_prev: the raw moment) -> bdn_bn_bwd_apply(raw_moment = 1) and, in float32,
    bdn_bn_bwd_apply_split; z_prev carries the ratio sweep and the table is its true statistics.  The gradient is the one the device
    stored (g, masked), so only the BatchNorm-backward arithmetic is judged."""
    N, H, W, Cz, Cout, ipg = 4, 16, 16, 128, 64, 2
    dt, td = DT[prec]
    G = N // ipg
    lib = _lib.load()
    dzin = to_nhwc(prec, rnd(prec, _rand((N, Cz, H, W), 63)))
    wf, _ = pack_w(prec, rnd(prec, _rand((Cout, Cz, 3, 3), 64, 0.05)), Cz)
    zprev = IC.offset_map(prec, N, Cout, H, W, seed=65)
    gamma, beta = _gamma_beta(Cout)
    bn = IC.true_table(zprev, ipg, gamma, beta)
    z_d, bn_d = to_nhwc(prec, zprev), dev(bn)
    nt = lib.bdn_conv3x3_num_mtiles(N, H, W, Cout, ipg)
    part = guard.full((nt, 2, Cout), NAN)
    dA = guard.full((N, H, W, Cout), NAN, dtype=td)
    _lib.call('bdn_conv3x3_dgrad_bs', dt, dzin.data_ptr(), Cz, wf.data_ptr(), dA.data_ptr(), z_d.data_ptr(), bn_d.data_ptr(),
              ipg, part.data_ptr(), N, H, W, Cout, st())
    sums, dg, db = guard.full((G, 2, Cout), NAN), guard.full((Cout,), NAN), guard.full((Cout,), NAN)
    dz = guard.full((N, H, W, Cout), NAN, dtype=td)
    _lib.call('bdn_bn_bwd_apply', dt, dA.data_ptr(), Cout, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, Cout,
              part.data_ptr(), nt // G, 1, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dz.data_ptr(), None, st())
    torch.cuda.synchronize()
    g = from_nhwc(dA)
    ref64 = IC.bn_relu_backward(zprev, g, gamma, beta, ipg)
    ref32 = IC.bn_relu_backward(zprev, g, gamma, beta, ipg, torch.float32)
    ratio = _ratios(zprev, ipg)
    tols = (2e-5 if prec == 'fp32' else 8e-3, 2e-5, 2e-5)                                # test_dgrad_with_fused_bn_bwd_stats' bars
    _judge_backward('dgrad_bs+bn_bwd_apply', prec, ratio, (from_nhwc(dz), dg.cpu(), db.cpu()), ref64, ref32, tols)
    if prec == 'fp32':
        sums2, dg2, db2 = guard.full((G, 2, Cout), NAN), guard.full((Cout,), NAN), guard.full((Cout,), NAN)
        dzs = guard.full((N, H, W, 2 * Cout), NAN, dtype=torch.bfloat16)
        _lib.call('bdn_bn_bwd_apply_split', dA.data_ptr(), Cout, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, Cout,
                  part.data_ptr(), nt // G, 1, sums2.data_ptr(), dg2.data_ptr(), db2.data_ptr(), dzs.data_ptr(), None, st())
        torch.cuda.synchronize()
        assert torch.equal(sums2, sums) and torch.equal(dg2, dg) and torch.equal(db2, db)
        hi, lo = IC.split_ref(dz.cpu())                                                  # the split of the float32 kernel's dz, bit for bit
        assert torch.equal(IC.bits16(dzs.cpu()), torch.cat([IC.bits16(hi), IC.bits16(lo)], -1))


@guarded
def test_dgrad_bb_under_offset():
    """bdn_conv3x3_dgrad_bb's stored dz (a g + b z + c: b z and c cancel at a large offset) against float64 autograd."""
    N, H, W, C0, Cout, ipg = 2, 24, 20, 64, 64, 2
    lib = _lib.load()
    G = N // ipg
    z = IC.offset_map('bf16', N, C0, H, W, seed=66)
    gamma, beta = _gamma_beta(C0)
    bn = IC.true_table(z, ipg, gamma, beta)
    dA, pre = _clear_of_the_switch('dgrad_bb', z, bn, ipg, rnd('bf16', _rand((N, C0, H, W), 67)))
    g = dA * (pre > 0)                                                                   # the masked gradient the fused producers store
    ref64 = IC.bn_relu_backward(z, g, gamma, beta, ipg)
    ref32 = IC.bn_relu_backward(z, g, gamma, beta, ipg, torch.float32)
    _, wd = pack_w('bf16', rnd('bf16', _rand((C0, Cout, 3, 3), 68, 0.05)), Cout)
    g_d, z_d, bn_d = to_nhwc('bf16', g), to_nhwc('bf16', z), dev(bn)
    ws = guard.empty(lib.bdn_bn_bwd_workspace_bytes(BDN_BF16, N, H, W, C0, ipg) // 4)
    sums, dg, db = guard.empty(G, 2, C0), guard.empty(C0), guard.empty(C0)
    dz_two = guard.empty(N, H, W, C0, dtype=torch.bfloat16)
    _lib.call('bdn_bn_bwd', BDN_BF16, g_d.data_ptr(), C0, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C0,
              ws.data_ptr(), sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dz_two.data_ptr(), st())
    out = guard.full((N, H, W, Cout), NAN, dtype=torch.bfloat16)
    dz = guard.full((N, H, W, C0), NAN, dtype=torch.bfloat16)
    _lib.call('bdn_conv3x3_dgrad_bb', BDN_BF16, g_d.data_ptr(), C0, z_d.data_ptr(), bn_d.data_ptr(), sums.data_ptr(), ipg, wd.data_ptr(),
              out.data_ptr(), None, None, None, dz.data_ptr(), N, H, W, Cout, st())
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    _judge_backward('dgrad_bb', 'bf16', _ratios(z, ipg), (from_nhwc(dz), None, None), ref64, ref32, (8e-3, None, None))      # test_conv3x3_dgrad_with_bn_backward_on_load's bar


@guarded
def test_first_layer_wgrad_bnbwd_under_offset():
    """bdn_bn_bwd_finalize + bdn_conv3x3_wgrad_bnbwd with the ratio sweep on z: the weight gradient per output channel against float64
    (dz rounded to bf16 like the kernel's staging; tests/test_gpu_launch_shapes.py test_first_layer_weight_gradient's construction and bar)."""
    N, H, W, ipg, ldA = 4, 24, 16, 2, 80
    Cout, C0, Creal = 64, 16, 13
    lib = _lib.load()
    G, M = N // ipg, ipg * H * W
    z = IC.offset_map('bf16', N, Cout, H, W, seed=69)
    gamma, beta = _gamma_beta(Cout)
    bn = IC.true_table(z, ipg, gamma, beta)
    dA_full = rnd('bf16', _rand((N, ldA, H, W), 70))
    dA_full[:, :Cout], pre = _clear_of_the_switch('wgrad_bnbwd', z, bn, ipg, dA_full[:, :Cout])
    gm = dA_full[:, :Cout].double() * (pre > 0)
    x = rnd('bf16', _rand((N, C0, H, W), 71))
    x[:, Creal:] = 0
    rows = 4
    part = torch.zeros(G * rows, 2, Cout)
    for g in range(G):
        for q in range(rows):
            sl, hs = slice(g * ipg, (g + 1) * ipg), slice(q * H // rows, (q + 1) * H // rows)
            part[g * rows + q, 0] = gm[sl, :, hs].sum((0, 2, 3)).float()
            part[g * rows + q, 1] = (gm[sl, :, hs] * z[sl, :, hs].double()).sum((0, 2, 3)).float()
    refs = []
    for dtype in (torch.float64, torch.float32):
        dzr = IC.bn_relu_backward(z, gm, gamma, beta, ipg, dtype)[0].to(torch.bfloat16).to(dtype)
        refs.append(torch.nn.grad.conv2d_weight(x[:, :Creal].to(dtype), (Cout, Creal, 3, 3), dzr, padding=1))
    sums = guard.full((G, 2, Cout), NAN)
    dg, db = guard.empty(Cout), guard.empty(Cout)
    bn_d, part_d = dev(bn), dev(part)
    _lib.call('bdn_bn_bwd_finalize', bn_d.data_ptr(), G, Cout, part_d.data_ptr(), rows, 1, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), None, st())
    wpart = guard.empty(lib.bdn_wgrad_workspace_bytes(N, H, W, Cout, C0, ipg) // 4)
    dw = guard.full((Cout, Creal, 3, 3), NAN)
    dA_d, z_d, x_d = to_nhwc('bf16', dA_full), to_nhwc('bf16', z), to_nhwc('bf16', x)
    dA_d[..., Cout:] = NAN
    _lib.call('bdn_conv3x3_wgrad_bnbwd', BDN_BF16, dA_d.data_ptr(), ldA, z_d.data_ptr(), bn_d.data_ptr(), sums.data_ptr(), ipg, Cout,
              x_d.data_ptr(), C0, wpart.data_ptr(), dw.data_ptr(), Creal, N, H, W, st())
    torch.cuda.synchronize()
    as_map = lambda t: t.reshape(1, Cout, Creal * 9, 1)                                  # per output channel = per channel of z
    _judge_backward('wgrad_bnbwd', 'bf16', _ratios(z, ipg), (as_map(dw.cpu()), None, None), (as_map(refs[0]), None, None),
                    (as_map(refs[1]), None, None), (1e-4, None, None))


# ================================================================= C. ties and exact zeros on planted grids
def _planted(prec, N, C, H, W, ipg, seed, neg=False):
    bn = IC.planted_table(N // ipg, C, seed, neg_zero_shift=neg)
    z = IC.planted_map(N, C, H, W, bn, ipg, seed + 1, neg_zero=neg)
    pre = IC.planted_preact(z, bn, ipg)
    assert IC.zero_share(pre) >= 0.15
    return z, bn, pre


def _no_negative_zero(name, t):
    """Activations are >= 0: no stored element may have its sign bit set (a -0.0 would)."""
    bits = t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    assert (bits >= 0).all(), f'{name}: {int((bits < 0).sum())} elements with the sign bit set (-0.0 or negative)'


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', [(2, 16, 16, 64), (2, 11, 45, 64), (1, 5, 5, 64)], ids=str)
@guarded
def test_unpool_routes_to_the_first_maximum(prec, case):
    """bdn_enc_skip_bwd with dP on maps where most 2x2 windows hold a tie: dA on [a > 0] equals the plain-loop reference -- every value is
    a multiple of 1/32 below 8, exact in both storage types, so float32 is compared bit for bit and bf16 with the existing bar."""
    B, H, W, C = case
    dt, td = DT[prec]
    z, bn, pre = _planted(prec, 2 * B, C, H, W, B, 81)
    a = torch.relu(pre)
    assert IC.positive_tie_share(a) >= 0.5 and (a > 0).double().mean() >= 0.4
    extra = 32
    dF = IC.grid_values((B, C + extra, H, W), 83)
    dP = IC.grid_values((2 * B, C, H // 2, W // 2), 84)
    ref = IC.enc_skip_bwd_ref(a, dF[:, :C], dP, B)
    out = guard.full((2 * B, H, W, C), NAN, dtype=td)
    dF_d, z_d, bn_d, dP_d = to_nhwc(prec, dF), to_nhwc(prec, z), dev(bn), to_nhwc(prec, dP)
    dF_d[..., C:] = NAN
    _lib.call('bdn_enc_skip_bwd', dt, dF_d.data_ptr(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), dP_d.data_ptr(), out.data_ptr(), None,
              B, H, W, C, st())
    torch.cuda.synchronize()
    got, live = from_nhwc(out).double(), a > 0
    assert torch.isfinite(got).all()
    if prec == 'fp32':
        wrong = live & (got != ref)
        assert not wrong.any(), f'{int(wrong.sum())} of {int(live.sum())} live gradients differ from first-maximum routing; first {wrong.nonzero()[0].tolist()}'
    else:
        assert_close('enc_skip_bwd', got * live, ref * live, 8e-3)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', [(4, 16, 16, 64, 2), (2, 11, 11, 128, 1)], ids=str)
@guarded
def test_pool_kernels_on_the_planted_grid(prec, shape):
    """bdn_bnrelu_pool, bdn_product_pool and (float32) bdn_product_pool_split: exact values on exact data, signed zeros included
    (z and shift hold -0.0: relu must store +0.0)."""
    N, H, W, C, ipg = shape
    dt, td = DT[prec]
    z, bn, pre = _planted(prec, N, C, H, W, ipg, 85, neg=True)
    a = torch.relu(pre) + 0.0
    want_pool = O.maxpool2(a)
    z_d, bn_d = to_nhwc(prec, z), dev(bn)
    pool = guard.full((N, H // 2, W // 2, C), NAN, dtype=td)
    _lib.call('bdn_bnrelu_pool', dt, z_d.data_ptr(), bn_d.data_ptr(), ipg, pool.data_ptr(), N, H, W, C, st())
    torch.cuda.synchronize()
    assert torch.equal(from_nhwc(pool), want_pool)
    _no_negative_zero('bnrelu_pool', pool)
    # the date pair: groups = dates
    B = N // 2
    z2, bn2, pre2 = _planted(prec, N, C, H, W, B, 87, neg=True)
    a2 = torch.relu(pre2) + 0.0
    want_f, want_p = torch.relu(a2[B:] * a2[:B]), O.maxpool2(a2)
    z2_d, bn2_d = to_nhwc(prec, z2), dev(bn2)
    f = guard.full((B, H, W, C), NAN, dtype=td)
    p = guard.full((N, H // 2, W // 2, C), NAN, dtype=td)
    _lib.call('bdn_product_pool', dt, z2_d.data_ptr(), bn2_d.data_ptr(), f.data_ptr(), p.data_ptr(), B, H, W, C, st())
    torch.cuda.synchronize()
    assert torch.equal(from_nhwc(f), want_f) and torch.equal(from_nhwc(p), want_p)
    _no_negative_zero('product_pool f', f)
    _no_negative_zero('product_pool pool', p)
    if prec == 'fp32':
        fs = guard.full((B, H, W, 2 * C), NAN, dtype=torch.bfloat16)
        ps = guard.full((N, H // 2, W // 2, 2 * C), NAN, dtype=torch.bfloat16)
        _lib.call('bdn_product_pool_split', z2_d.data_ptr(), bn2_d.data_ptr(), fs.data_ptr(), 2 * C, C, ps.data_ptr(), B, H, W, C, st())
        torch.cuda.synchronize()
        for name, got, want in (('f', fs, want_f), ('pool', ps, want_p)):                # every value is exact in bf16: hi = value, lo = +0.0
            assert torch.equal(from_nhwc(got[..., :C]), want) and (IC.bits16(got[..., C:].cpu()) == 0).all(), name
            _no_negative_zero(f'product_pool_split {name}', got)


@pytest.mark.parametrize('prec', PRECS)
@guarded
def test_eval_stage_pools_on_the_planted_grid(prec):
    """The pool output of bdn_conv3x3_eval and bdn_conv3x3_eval_pair: an identity filter makes the convolution return its planted input
    exactly, the folded table is the planted (scale, shift)."""
    B, H, W, C = 2, 16, 16, 64
    dt, td = DT[prec]
    bn = IC.planted_table(1, C, 89, neg_zero_shift=True)
    z = IC.planted_map(2 * B, C, H, W, bn, 2 * B, 90, neg_zero=True)
    a = torch.relu(IC.planted_preact(z, bn, 2 * B)) + 0.0
    assert IC.positive_tie_share(a) >= 0.5
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    wf, _ = pack_w(prec, w, C)
    x_d, dsc, dsh = to_nhwc(prec, z), dev(bn[0, 2]), dev(bn[0, 3])
    out = guard.full((2 * B, H, W, C), NAN, dtype=td)
    pool = guard.full((2 * B, H // 2, W // 2, C), NAN, dtype=td)
    _lib.call('bdn_conv3x3_eval', dt, x_d.data_ptr(), C, None, 0, wf.data_ptr(), dsc.data_ptr(), dsh.data_ptr(), out.data_ptr(), None,
              pool.data_ptr(), 2 * B, H, W, C, st())
    f = guard.full((B, H, W, C), NAN, dtype=td)
    pool2 = guard.full((2 * B, H // 2, W // 2, C), NAN, dtype=td)
    _lib.call('bdn_conv3x3_eval_pair', dt, x_d.data_ptr(), C, wf.data_ptr(), dsc.data_ptr(), dsh.data_ptr(), f.data_ptr(), pool2.data_ptr(),
              B, H, W, C, st())
    torch.cuda.synchronize()
    assert torch.equal(from_nhwc(out), a) and torch.equal(from_nhwc(pool), O.maxpool2(a))
    assert torch.equal(from_nhwc(f), a[:B] * a[B:]) and torch.equal(from_nhwc(pool2), O.maxpool2(a))
    for name, t in (('eval out', out), ('eval pool', pool), ('eval_pair f', f), ('eval_pair pool', pool2)):
        _no_negative_zero(name, t)


def _strict(name, got, full, pre):
    """The stored gradient under the STRICT mask [pre > 0]: assert_masked without an either-answer band, and exactly 0 at pre == 0."""
    assert_masked(name, got, full, pre.double(), eps=0.0)
    assert (got[pre == 0] == 0).all(), f'{name}: a gradient survives at pre-activation exactly 0'
    assert (pre == 0).double().mean() >= 0.15


def _spiked(prec, shape, pre, seed):
    """Gaussian gradient with 64.0 planted wherever the pre-activation is exactly 0: a mask that lets those pixels through moves every sum."""
    return torch.where(pre == 0, torch.full(shape, 64.0), rnd(prec, _rand(shape, seed)))


def _host_partials(g, z, ipg, rows=4):
    """Partial rows (sum g, sum g z) the way the fused producers leave them, `rows` per group (test_first_layer_wgrad_with_fused_bn_bwd)."""
    N, C, H, W = z.shape
    G = N // ipg
    part = torch.zeros(G * rows, 2, C)
    for gi in range(G):
        for q in range(rows):
            sl, hs = slice(gi * ipg, (gi + 1) * ipg), slice(q * H // rows, (q + 1) * H // rows)
            part[gi * rows + q, 0] = g[sl, :, hs].double().sum((0, 2, 3)).float()
            part[gi * rows + q, 1] = (g[sl, :, hs].double() * z[sl, :, hs].double()).sum((0, 2, 3)).float()
    return part


@pytest.mark.parametrize('prec', PRECS)
@guarded
def test_bn_bwd_masks_strictly(prec):
    """bdn_bn_bwd, bdn_bn_bwd_apply (+ _split, _frozen) where 15 % or more of the pre-activations are exactly 0 and carry a gradient of 64:
    those pixels add nothing to sum g, sum g xhat, dgamma, dbeta; in frozen mode their dz is exactly 0, in training mode it is the
    documented -scale (s0 / M + xhat s1 / M) (autograd's value: the mean-correction terms reach every pixel)."""
    N, H, W, C, ipg = 4, 16, 16, 64, 2
    dt, td = DT[prec]
    G = N // ipg
    lib = _lib.load()
    z, bn, pre = _planted(prec, N, C, H, W, ipg, 91)
    dA = _spiked(prec, (N, C, H, W), pre, 93)
    g = dA * (pre > 0)
    dz64, dg64, db64, sums64 = IC.bn_bwd_contract64(z, g, bn, ipg)
    dA_d, z_d, bn_d = to_nhwc(prec, dA), to_nhwc(prec, z), dev(bn)
    tz = 1e-4 if prec == 'fp32' else 1e-2                                                # test_bn_bwd's bars

    def check(name, dz, dgam, dbet, sums, split=False):
        torch.cuda.synchronize()
        assert_close(f'{name} dbeta', dbet.cpu(), db64.float(), 1e-4)
        assert_close(f'{name} dgamma', dgam.cpu(), dg64.float(), 1e-4)
        assert_close(f'{name} sums', sums.cpu(), sums64.float(), 1e-4)
        got = (dz[..., :C].float() + dz[..., C:].float()) if split else dz
        assert_close(f'{name} dz', from_nhwc(got), dz64.float(), tz)

    wsb = guard.empty(lib.bdn_bn_bwd_workspace_bytes(dt, N, H, W, C, ipg) // 4)
    sums, dgam, dbet = guard.full((G, 2, C), NAN), guard.full((C,), NAN), guard.full((C,), NAN)
    dz = guard.full((N, H, W, C), NAN, dtype=td)
    _lib.call('bdn_bn_bwd', dt, dA_d.data_ptr(), C, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C, wsb.data_ptr(), sums.data_ptr(),
              dgam.data_ptr(), dbet.data_ptr(), dz.data_ptr(), st())
    check('bn_bwd', dz, dgam, dbet, sums)
    rows = 4
    part_d = dev(_host_partials(g, z, ipg, rows))                                        # the producers' rows hold the strictly masked sums
    sums, dgam, dbet = guard.full((G, 2, C), NAN), guard.full((C,), NAN), guard.full((C,), NAN)
    dz = guard.full((N, H, W, C), NAN, dtype=td)
    _lib.call('bdn_bn_bwd_apply', dt, dA_d.data_ptr(), C, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C, part_d.data_ptr(), rows, 1,
              sums.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dz.data_ptr(), None, st())
    check('bn_bwd_apply', dz, dgam, dbet, sums)                                          # its dz pass masks the UNMASKED dA itself
    if prec == 'fp32':
        sums, dgam, dbet = guard.full((G, 2, C), NAN), guard.full((C,), NAN), guard.full((C,), NAN)
        dzs = guard.full((N, H, W, 2 * C), NAN, dtype=torch.bfloat16)
        _lib.call('bdn_bn_bwd_apply_split', dA_d.data_ptr(), C, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C, part_d.data_ptr(), rows, 1,
                  sums.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dzs.data_ptr(), None, st())
        check('bn_bwd_apply_split', dzs, dgam, dbet, sums, split=True)
    # frozen statistics: dz = scale g, exactly 0 under the mask
    sums, dgam, dbet, dbias = guard.full((G, 2, C), NAN), guard.full((C,), NAN), guard.full((C,), NAN), guard.full((C,), NAN)
    dz = guard.full((N, H, W, C), NAN, dtype=td)
    _lib.call('bdn_bn_bwd_apply_frozen', dt, dA_d.data_ptr(), C, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C, part_d.data_ptr(), rows, 1,
              sums.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dbias.data_ptr(), dz.data_ptr(), None, st())
    torch.cuda.synchronize()
    scale = torch.repeat_interleave(bn[:, 2], ipg, 0)[:, :, None, None]
    got = from_nhwc(dz)
    assert (got[pre <= 0] == 0).all(), 'frozen dz is not exactly 0 where the pre-activation is <= 0'
    assert torch.equal(got, rnd(prec, scale * g))
    assert_close('frozen dbeta', dbet.cpu(), db64.float(), 1e-4)
    assert_close('frozen dgamma', dgam.cpu(), dg64.float(), 1e-4)


@pytest.mark.parametrize('prec', PRECS)
@guarded
def test_fused_producers_mask_strictly(prec):
    """bdn_conv3x3_dgrad_bs, bdn_enc_skip_bwd (bs_partial), bdn_upsample2x_bwd_bs and bdn_outc_bwd (bs_partial) where 15 % or more of the
    producing layer's pre-activations are exactly 0: the stored gradient there is exactly 0 and the partial sums are those of the
    strictly masked gradient (bars: test_enc_skip_bwd / test_outc_fwd_bwd / test_upsample2x_and_backward)."""
    dt, td = DT[prec]
    lib = _lib.load()

    def sums_ok(name, part, g, zp, groups=1):
        got = part.cpu().double().reshape(groups, -1, 2, part.shape[-1]).sum(1)
        n = g.shape[0] // groups
        for k in range(groups):
            gk, zk = g[k * n:(k + 1) * n].double(), zp[k * n:(k + 1) * n].double()
            assert_close(f'{name}: sum g', got[k, 0].float(), gk.sum((0, 2, 3)).float(), 2e-5 if prec == 'fp32' else 1e-4, 1e-4)
            assert_close(f'{name}: sum g z', got[k, 1].float(), (gk * zk).sum((0, 2, 3)).float(), 2e-5 if prec == 'fp32' else 1e-4, 1e-4)

    # ---- bdn_conv3x3_dgrad_bs, (4, 8, 8, 64 -> 64, ipg 2)
    N, H, W, Cz, Cout, ipg = 4, 8, 8, 64, 64, 2
    zp, bn, pre = _planted(prec, N, Cout, H, W, ipg, 95)
    dzin = to_nhwc(prec, rnd(prec, _rand((N, Cz, H, W), 97)))
    wf, _ = pack_w(prec, rnd(prec, _rand((Cout, Cz, 3, 3), 98, 0.05)), Cz)
    z_d, bn_d = to_nhwc(prec, zp), dev(bn)
    plain = guard.full((N, H, W, Cout), NAN, dtype=td)
    _lib.call('bdn_conv3x3', dt, dzin.data_ptr(), Cz, None, 0, IN_PLAIN, None, ipg, wf.data_ptr(), None, plain.data_ptr(), None, N, H, W, Cout, st())
    nt = lib.bdn_conv3x3_num_mtiles(N, H, W, Cout, ipg)
    part = guard.full((nt, 2, Cout), NAN)
    dA = guard.full((N, H, W, Cout), NAN, dtype=td)
    _lib.call('bdn_conv3x3_dgrad_bs', dt, dzin.data_ptr(), Cz, wf.data_ptr(), dA.data_ptr(), z_d.data_ptr(), bn_d.data_ptr(), ipg,
              part.data_ptr(), N, H, W, Cout, st())
    torch.cuda.synchronize()
    _strict('dgrad_bs', from_nhwc(dA), from_nhwc(plain), pre)
    sums_ok('dgrad_bs', part, from_nhwc(plain) * (pre > 0), zp, groups=N // ipg)

    # ---- bdn_enc_skip_bwd with bs_partial, (2, 16, 16, 64)
    B, H, W, C = 2, 16, 16, 64
    z, bn, pre = _planted(prec, 2 * B, C, H, W, B, 99)
    extra = 32
    dF = rnd(prec, _rand((B, C + extra, H, W), 101))
    dP = rnd(prec, _rand((2 * B, C, H // 2, W // 2), 102))
    dF_d, z_d, bn_d, dP_d = to_nhwc(prec, dF), to_nhwc(prec, z), dev(bn), to_nhwc(prec, dP)
    dF_d[..., C:] = NAN
    rows = lib.bdn_enc_skip_bwd_rows(dt, B, H, W, C)
    part = guard.full((2, rows, 2, C), NAN)
    out, out2 = guard.full((2 * B, H, W, C), NAN, dtype=td), guard.full((2 * B, H, W, C), NAN, dtype=td)
    _lib.call('bdn_enc_skip_bwd', dt, dF_d.data_ptr(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), dP_d.data_ptr(), out.data_ptr(), part.data_ptr(), B, H, W, C, st())
    _lib.call('bdn_enc_skip_bwd', dt, dF_d.data_ptr(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), dP_d.data_ptr(), out2.data_ptr(), None, B, H, W, C, st())
    torch.cuda.synchronize()
    _strict('enc_skip_bwd', from_nhwc(out), from_nhwc(out2), pre)
    sums_ok('enc_skip_bwd', part.reshape(2 * rows, 2, C), from_nhwc(out2) * (pre > 0), z, groups=2)

    # ---- bdn_upsample2x_bwd_bs, (2, 8, 8 -> 16, 16, 64)
    B, h, w, H, W, C = 2, 8, 8, 16, 16, 64
    zp, bnp, pre = _planted(prec, B, C, h, w, B, 103)
    extra = 16
    dU_d = to_nhwc(prec, rnd(prec, _rand((B, C + extra, H, W), 105)))
    dU_d[..., :extra] = NAN
    es = 2 if prec == 'bf16' else 4
    rows = lib.bdn_upsample2x_bwd_rows(dt, B, h, w, C)
    assert rows > 0
    plain = guard.full((B, h, w, C), NAN, dtype=td)
    _lib.call('bdn_upsample2x_bwd', dt, dU_d.data_ptr() + extra * es, C + extra, plain.data_ptr(), B, h, w, H, W, C, st())
    dsrc = guard.full((B, h, w, C), NAN, dtype=td)
    part = guard.full((rows, 2, C), NAN)
    zp_d, bnp_d = to_nhwc(prec, zp), dev(bnp)
    _lib.call('bdn_upsample2x_bwd_bs', dt, dU_d.data_ptr() + extra * es, C + extra, dsrc.data_ptr(), zp_d.data_ptr(), bnp_d.data_ptr(),
              part.data_ptr(), B, h, w, H, W, C, st())
    torch.cuda.synchronize()
    _strict('upsample2x_bwd_bs', from_nhwc(dsrc), from_nhwc(plain), pre)
    sums_ok('upsample2x_bwd_bs', part, from_nhwc(plain) * (pre > 0), zp)

    # ---- bdn_outc_bwd with bs_partial, (2, 16, 16, 64, ncls 2)
    B, H, W, C, ncls = 2, 16, 16, 64, 2
    z, bn, pre = _planted(prec, B, C, H, W, B, 107)
    wc = _rand((ncls, C), 109, 0.2)
    dl = _rand((B, ncls, H, W), 110)
    z_d, bn_d, w_d, dl_d = to_nhwc(prec, z), dev(bn), dev(wc), dev(dl)
    dA = guard.full((B, H, W, C), NAN, dtype=td)
    dw, dbc = guard.full((ncls, C), NAN), guard.full((ncls,), NAN)
    rows = lib.bdn_outc_bwd_rows(dt, B, H, W, C)
    part = guard.full((rows, 2, C), NAN)
    ows = guard.full((lib.bdn_outc_bwd_workspace_bytes(dt, B, H, W, C, ncls) // 4,), NAN)
    _lib.call('bdn_outc_bwd', dt, dl_d.data_ptr(), z_d.data_ptr(), bn_d.data_ptr(), w_d.data_ptr(), dA.data_ptr(), dw.data_ptr(), dbc.data_ptr(),
              part.data_ptr(), ows.data_ptr(), B, H, W, C, ncls, st())
    torch.cuda.synchronize()
    sums_ok('outc_bwd', part, from_nhwc(dA) * (pre > 0), z)                              # the sums are over the stored dA under the strict mask
    a = torch.relu(pre).double()
    assert_close('outc_bwd dw', dw.cpu(), torch.einsum('bkhw,bchw->kc', dl.double(), a).float(), 1e-4)
