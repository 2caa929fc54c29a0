"""-m gpu: the kernels on tensors of 2 to 4 GB (and past 4 GB where an entry point has no bound) -- byte offsets past the sign bit and at
the top of their 32-bit range.  The instrument is tests/bigtensor.py; tests/test_bigtensor_cpu.py proves it and the refusals on the CPU.

test_big_twin / test_big_twin_bn_backward_on_load
    One big twin per row of tests/launch_cases.py of the ops fwd, dgrad, dgrad_bs, dgrad_bb, x3, x3src, eval, eval_pair and eval_cls, at
    both sizes: 'cross' (the widest tensor passes 2^31 bytes by at least a period) and 'top' (the largest N the entry point accepts;
    tensors of half the width cross 2^31 there).  A twin asserts that the raised N still selects the instantiation it names, launches
    into outputs born 0xFF on guard-banded buffers, requires every period of every output (tile partials included) to equal period 0 of
    its block bit for bit, and holds period 0 against the sibling's float64 reference at the sibling's bar
    (tests/test_gpu_launch_shapes.py: the same case / launch / compare functions).
    Rows without a twin of their own:
      * a row whose op, precision, modes (BatchNorm+ReLU on load, second source, statistics) and instantiation AT THE RAISED N another
        twin already runs: fwd-bf16-4x37x270-128-256-g2-bnrelu, fwd-bf16-3x37x270-128-256-g1-bnrelu, fwd-fp32-3x37x270-128-256-g1-bnrelu,
        dgrad_bs-bf16-4x37x53-256-128-g2, dgrad_bb-bf16-2x37x53-64-128-g1, eval-bf16-4x7x5-512-512-g1, eval-fp32-4x7x5-512-512-g1,
        eval_pair-bf16-4x7x5-512-512-g1 (tests/test_bigtensor_cpu.py checks that these are all);
      * rows at the BN = 64 side of the column-tile threshold (conv_plan: n_mtiles * Cout / 128 < 512): raising N moves them to BN = 128.
        The twin then names the instantiation the big shape selects -- bigtensor.twins() asks the library -- and is kept when no other
        twin runs that one: the 8 x 8-map kernels <..,128,8,8,2,128,2,2,..> of fwd / dgrad / dgrad_bs (bf16, fp32), which the table only
        has in eval form.  The BN = 64 instantiations themselves cannot meet a 2 GB tensor.
test_big_weight_gradient / test_big_first_layer_weight_gradient
    Every wgrad and wgrad_bnbwd row on integer-valued data: dW must EQUAL (N / P) x the period's integers.  wgrad: 'cross', 'top' (the
    last N of the pipelined kernels) and 'far' (the first N past 2^31 elements, where wgrad_kernel takes over on operands past 4 GB).
test_big_stage_kernel / test_big_stage_backward / test_big_bn_bwd / test_big_bn_bwd_apply / test_big_classifier
    Stage-boundary kernels without a bound of their own (64-bit addresses), past 2^31 and past 2^32 bytes, at the engine's 8 x 8 x 512 and
    64 x 64 x 64 shapes: bnrelu, bnrelu_pool, fuse_product, product_pool(_split), upsample2x(_split), split_pack, enc_skip_bwd,
    upsample2x_bwd, bn_bwd, bn_bwd_apply / _split / _frozen, outc_fwd, outc_bwd.
test_big_pack_input / test_big_dgrad_first
    The two entry points outside the table, past 2^31 and 2^32 bytes (their own bounds lie beyond the memory cap).
test_big_statistics_totals / test_big_enc_skip_sums / test_big_classifier_backward_sums / test_big_bn_bwd_frozen
    The reductions over the N x tiles rows of a big launch on integer-valued data, with equality: the fused statistics of the forward and
    bdn_bn_finalize over them; the fused partial sums of dgrad_bs, enc_skip_bwd and outc_bwd and bdn_bn_bwd_finalize over their rows;
    dw / db of outc_bwd; bdn_outc_bn_bwd_apply (bf16 / fp32 / bf16x3) and bdn_bn_bwd_frozen.  bdn_upsample2x_bwd_bs runs in
    test_big_stage_backward.

No test of this file holds more than 24 GiB of device memory (asserted from torch's peak counter); every test prints its wall time and peak memory
(BIGTENSOR_REPORT=<file> appends them as JSON lines).
"""
import functools
import gc
import json
import os
import time

import pytest
import torch

from fabric_amd import _lib
from tests import bigtensor as bt
from tests import guard
from tests import launch_cases as lc
from tests import test_gpu_input_grad as tig
from tests import test_gpu_kernels as tk
from tests import test_gpu_launch_shapes as ls
from tests.gpu_util import DT, assert_close, assert_masked, bn_table, bnrelu_ref, dev, from_nhwc, pack_w, preact, rnd, st
from tests.guard import guarded

pytestmark = pytest.mark.gpu


def measured(fn=None, cap=None):
    """Print (and report) the test's wall time and peak device memory, require the peak to stay below `cap` bytes, and hand the memory
    back before returning."""
    if fn is None:
        return functools.partial(measured, cap=cap)

    @functools.wraps(fn)
    def run(*args, **kwargs):
        torch.cuda.synchronize()
        gc.collect()                                       # a guarded session is a reference cycle: its buffers wait for the collector
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        try:
            out = fn(*args, **kwargs)
            peak = torch.cuda.max_memory_allocated()
            assert cap is None or peak <= cap, f'the test held {peak / 2 ** 30:.1f} GiB of device memory (cap {cap / 2 ** 30:.0f} GiB)'
            return out
        finally:
            torch.cuda.synchronize()
            rec = {'test': fn.__name__, 'case': _case_id(*args, **kwargs), 'seconds': round(time.perf_counter() - t0, 2),
                   'peak_GiB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
            print(json.dumps(rec))
            if os.environ.get('BIGTENSOR_REPORT'):
                with open(os.environ['BIGTENSOR_REPORT'], 'a') as f:
                    f.write(json.dumps(rec) + '\n')
            gc.collect()
            torch.cuda.empty_cache()
    return run


def _case_id(*args, **kwargs):
    vals = list(args) + list(kwargs.values())
    ids = {bt.Case: bt.twin_id, bt.WgTwin: bt.wg_twin_id, bt.Stage: bt.stage_id, bt.WbTwin: bt.wb_twin_id}
    return '-'.join(ids.get(type(v), str)(v) for v in vals)


@functools.lru_cache(maxsize=1)
def _case(maker, small):
    """The period's inputs and float64 reference: computed once for both sizes of a row, never modified."""
    return maker(small)


def _alloc(shape, dtype):
    return guard.alloc(shape, dtype)


def _nhwc(prec, t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16 if prec == 'bf16' else torch.float32)


def _born(shape, dtype=torch.float32):
    return guard.empty(shape, dtype=dtype)                 # every byte 0xFF


def _periodic_and_period0(name, t, nblocks, reps):
    bt.assert_periodic(name, t, nblocks, reps)
    return bt.period0(t, nblocks, reps)


@pytest.mark.parametrize('t', [t for t in bt.twins() if t.row.op != 'dgrad_bb'], ids=bt.twin_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_twin(t):
    r, tw = t.row, t.twin
    N, G, P = tw.N, tw.G, tw.P
    assert tw.mem_bytes <= bt.MEM_CAP
    assert lc.instantiation(bt.twin_row(r, N)) == t.inst, 'raising N changed the kernel under test'
    rs = bt.small_row(r, P)
    reps = N // (G * P)
    p, H, W, Cout = r.prec, r.H, r.W, r.Cout
    td = torch.bfloat16 if p == 'bf16' else torch.float32
    lib = _lib.load()
    both = _periodic_and_period0
    if r.op == 'fwd':
        c = _case(ls.forward_case, rs)
        d0 = bt.tile(_nhwc(p, c.x0), G, N, _alloc)
        d1 = bt.tile(_nhwc(p, c.x1), G, N, _alloc) if r.C1 else None
        out = _born((N, H, W, Cout), td)
        stats = _born((lib.bdn_conv3x3_num_mtiles(N, H, W, Cout, N // G), 2, Cout))
        ls.forward_launch(r, c, d0, d1, out, stats, N=N, ipg=N // G)
        ls.forward_compare(rs, c, both('out', out, G, reps), both('tile partials', stats, G, reps), finalize=False)
    elif r.op == 'dgrad':
        c = _case(ls.dgrad_case, rs)
        ddz = bt.tile(_nhwc(p, c.dz), G, N, _alloc)
        out = _born((N, H, W, Cout), td)
        ls.dgrad_launch(r, c, ddz, out, N=N, ipg=N // G)
        ls.dgrad_compare(rs, c, both('dA', out, G, reps))
    elif r.op == 'dgrad_bs':
        c = _case(ls.dgrad_bs_case, rs)
        ddz, zp_d = bt.tile(_nhwc(p, c.dz), G, N, _alloc), bt.tile(_nhwc(p, c.zprev), G, N, _alloc)
        plain, dA = _born((N, H, W, Cout), td), _born((N, H, W, Cout), td)
        part = _born((lib.bdn_conv3x3_num_mtiles(N, H, W, Cout, N // G), 2, Cout))
        ls.dgrad_bs_launch(r, c, ddz, zp_d, plain, dA, part, N=N, ipg=N // G)
        ls.dgrad_bs_compare(rs, c, both('plain dA', plain, G, reps), both('masked dA', dA, G, reps), both('tile partials', part, G, reps))
    elif r.op in ('x3', 'x3src'):
        c = _case(ls.x3_case, rs)
        # x3: the period's split operand comes from bdn_split_pack at the small shape, as the sibling makes it
        xin = bt.tile(ls._split(c.x, P) if r.op == 'x3' else _nhwc('fp32', c.x), G, N, _alloc)
        out = _born((N, H, W, Cout))
        nt = lib.bdn_conv3x3_num_mtiles_ex(lc.DTYPE[p], N, H, W, r.C0, Cout, N // G)
        stats = _born((nt, 2, Cout)) if r.stats else None
        sp_out = _born((N, H, W, 2 * r.C0), torch.bfloat16) if r.op == 'x3src' and r.stats else None
        ls.x3_launch(r, c, xin, out, stats, sp_out, N=N, ipg=N // G)
        ls.x3_compare(rs, c, both('out', out, G, reps), both('tile partials', stats, G, reps) if r.stats else None,
                      both('split operand', sp_out, G, reps) if sp_out is not None else None)
    else:
        c = _case(ls.eval_case, rs)
        pair = r.op == 'eval_pair'                         # N pairs: the operand and the pooled maps hold both dates, two blocks
        d0 = bt.tile(_nhwc(p, c.x0), 2 if pair else 1, 2 * N if pair else N, _alloc)
        d1 = bt.tile(_nhwc(p, c.x1), 1, N, _alloc) if r.C1 else None
        outs = ls.eval_outputs(r, N, born=True)
        ls.eval_launch(r, c, d0, d1, outs, N=N)
        small = {k: both(k, v, 2 if pair and k == 'pool' else 1, reps) for k, v in outs.items()}
        ls.eval_compare(rs, c, small)


@pytest.mark.parametrize('t', [t for t in bt.twins() if t.row.op == 'dgrad_bb'], ids=bt.twin_id)
@measured(cap=bt.MEM_CAP)
def test_big_twin_bn_backward_on_load(t):
    """bdn_conv3x3_dgrad_bb in two guarded phases (six 4 GB tensors at once would pass the memory cap): without the producing layer's
    statistics (dA_prev and the dz by-product), then with them (the masked dA_prev and its tile partials).  `sums` is an input of the
    kernel: the float64 sums of the whole group, reps periods -- the two-kernel path that forms them on the device is a reduction over
    all images and keeps the sibling's small shapes."""
    r, tw = t.row, t.twin
    N, G, P = tw.N, tw.G, tw.P
    assert tw.mem_bytes <= bt.MEM_CAP
    assert lc.instantiation(bt.twin_row(r, N)) == t.inst, 'raising N changed the kernel under test'
    rs, reps, both = bt.small_row(r, P), N // (G * P), _periodic_and_period0
    H, W, Cout, td = r.H, r.W, r.Cout, torch.bfloat16
    c = _case(ls.dgrad_bb_case, rs)
    small = {}
    for phase in ('plain', 'stats'):
        with guard.checked(globals(), f'{bt.twin_id(t)} {phase}'):
            _, wd = pack_w('bf16', c.w, Cout)
            dA_d, z_d = bt.tile(_nhwc('bf16', c.dA), G, N, _alloc), bt.tile(_nhwc('bf16', c.z), G, N, _alloc)
            sums, bn_d = dev((c.sums64 * reps).float()), dev(c.bn)
            if phase == 'plain':
                out, dz = _born((N, H, W, Cout), td), _born((N, H, W, r.C0), td)
                ls.dgrad_bb_launch(r, c, wd, dA_d, z_d, bn_d, sums, None, out, dz, None, None, N=N, ipg=N // G)
                small['out'], small['dz'] = both('dA_prev', out, G, reps), both('dz', dz, G, reps)
            else:
                zp_d = bt.tile(_nhwc('bf16', c.zprev), G, N, _alloc)
                outm = _born((N, H, W, Cout), td)
                part = _born((_lib.load().bdn_conv3x3_num_mtiles(N, H, W, Cout, N // G), 2, Cout))
                ls.dgrad_bb_launch(r, c, wd, dA_d, z_d, bn_d, sums, zp_d, None, None, outm, part, N=N, ipg=N // G)
                small['outm'], small['part'] = both('masked dA_prev', outm, G, reps), both('tile partials', part, G, reps)
        del dA_d, z_d
        out = dz = outm = part = zp_d = None
        gc.collect()                                       # the session's buffers (a reference cycle) go back before the next phase
        torch.cuda.empty_cache()
    ls.dgrad_bb_compare(rs, c, small['out'], small['dz'], small['outm'], small['part'])


# ------------------------------------------------------------------ weight gradients: integer data, equality
@functools.lru_cache(maxsize=1)
def _wg_case(small, n_images):
    return bt.wg_case(small, n_images)


@pytest.mark.parametrize('tw', bt.wg_twins(), ids=bt.wg_twin_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_weight_gradient(tw):
    """bdn_conv3x3_wgrad_ex over 2 to 4 GB operands and past 4 GB (route: integer-valued data, split operands on the LO grid): the GEMM, its
    split-K partials and their fixed-order reduction must give exactly (N / P) x the period's integers."""
    r, N, G, P = tw.row, tw.N, tw.G, tw.P
    assert tw.mem_bytes <= bt.MEM_CAP
    H, W, C0, C1, Cout, p = r.H, r.W, r.C0, r.C1, r.Cout, r.prec
    ipg, dt = N // G, lc.DTYPE[p]
    mode = ls.IN_BNRELU if r.bnrelu else ls.IN_PLAIN
    big = bt.twin_row(r, N)
    assert lc.instantiation(big) == tw.inst, f'{lc.instantiation(big)}: raising N changed the kernel under test'
    rs = r._replace(N=G * P, ipg=P)
    c = _wg_case(rs, bt.wg_choose(r, 'far').N)             # one density for the three sizes: the largest tensor's
    reps = N // (G * P)
    lib = _lib.load()
    x3 = p in ('bf16x3', 'bf16x2')
    part = guard.empty(lib.bdn_wgrad_workspace_bytes_ex(dt, N, H, W, Cout, C0, C1, ipg, mode, 3) // 4)
    dw = _born((Cout, C0 + C1, 3, 3))
    if x3:
        ddz, d0, d1 = bt.tile(ls._split(c['dz'], P), G, N, _alloc), bt.tile(ls._split(c['x0'], P), G, N, _alloc), None
        assert bool((d0[:G * P, ..., C0:] != 0).any()) and bool((ddz[:G * P, ..., Cout:] != 0).any()), 'the lo halves are all zero'
    else:
        sp = 'fp32' if p == 'fp32' else 'bf16'
        ddz, d0 = bt.tile(_nhwc(sp, c['dz']), G, N, _alloc), bt.tile(_nhwc(sp, c['x0']), G, N, _alloc)
        d1 = bt.tile(_nhwc(sp, c['x1']), G, N, _alloc) if C1 else None
    ls.weight_gradient_launch(r, c['bn'], ddz, d0, d1, part, dw, 3, N=N, ipg=ipg)
    got, want = dw.cpu().double(), c['ref'] * reps
    print(f'density {c["density"]:.2e}, sum|terms| {c["abs_sum"] * reps / c["unit"]:.3g} units of 2^24 = {2 ** 24:.3g}, '
          f'{(want != 0).float().mean().item():.2f} of dW non-zero')
    bad = got != want
    assert not bad.any(), (f'{int(bad.sum())} of {bad.numel()} filter elements differ from {reps} x the period\'s integers; the first: '
                           f'{got[bad][0].item()!r} for {want[bad][0].item()!r}')


# ------------------------------------------------------------------ stage-boundary kernels: past 2^31 and past 2^32 bytes
@functools.lru_cache(maxsize=1)
def _stage_case(kernel, prec, H, W, C, P):
    """One period per block (two statistic groups, or the two dates) and the references of tests/test_gpu_kernels.py for it."""
    from oracle import bidate_oracle as O
    sp = 'fp32' if kernel in bt.SPLIT_KERNELS else prec
    z = rnd(sp, tk._rand((2 * P, C, H, W), 41))
    one = kernel.startswith('upsample2x')                  # one table row for the whole batch
    bn = bn_table(1 if one else 2, C, 42)
    a = bnrelu_ref(sp, z, bn, 2 * P if one else P)
    ref = {}
    if one:
        ref['out'] = O.pad_to(O.upsample2x_align(a.double()), torch.zeros(2 * P, 1, 2 * H, 2 * W)).float()
    if kernel == 'bnrelu':
        ref['out'] = a
    if kernel in ('bnrelu_pool', 'product_pool', 'product_pool_split'):
        ref['pool'] = O.maxpool2(a)
    if kernel in ('fuse_product', 'product_pool', 'product_pool_split'):
        ref['f'] = torch.relu(a[P:] * a[:P])               # models/bidate_model.py:35
    if kernel == 'split_pack':
        ref['rec'] = a
    return z, bn, ref


@pytest.mark.parametrize('s', bt.stage_twins(), ids=bt.stage_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_stage_kernel(s):
    """The stage-boundary kernels with 64-bit addressing (no 4 GB bound): per-image outputs periodic bit for bit, period 0 against the
    references and bars of tests/test_gpu_kernels.py."""
    assert s.mem_bytes <= bt.MEM_CAP
    k, prec, H, W, C, P, N = s.kernel, s.prec, s.H, s.W, s.C, s.P, s.N
    z, bn, ref = _stage_case(k, prec, H, W, C, P)
    reps = N // (2 * P)
    sp = 'fp32' if k in bt.SPLIT_KERNELS else prec
    dt, td = DT[sp]
    z_d, bn_d = bt.tile(_nhwc(sp, z), 2, N, _alloc), dev(bn)
    tol = (1e-5 if k == 'upsample2x' else 1e-6) if prec == 'fp32' else 8e-3
    outs = {}
    if k == 'bnrelu':
        outs['out'] = (_born((N, H, W, C), td), 2)
        _lib.call('bdn_bnrelu', dt, z_d.data_ptr(), bn_d.data_ptr(), N // 2, outs['out'][0].data_ptr(), N, H, W, C, st())
    elif k == 'bnrelu_pool':
        outs['pool'] = (_born((N, H // 2, W // 2, C), td), 2)
        _lib.call('bdn_bnrelu_pool', dt, z_d.data_ptr(), bn_d.data_ptr(), N // 2, outs['pool'][0].data_ptr(), N, H, W, C, st())
    elif k == 'product_pool_split':                        # f and the pooled maps leave as [hi | lo] operands (ld = 2 C, lo half at C)
        outs['f'], outs['pool'] = (_born((N // 2, H, W, 2 * C), torch.bfloat16), 1), (_born((N, H // 2, W // 2, 2 * C), torch.bfloat16), 2)
        _lib.call('bdn_product_pool_split', z_d.data_ptr(), bn_d.data_ptr(), outs['f'][0].data_ptr(), 2 * C, C, outs['pool'][0].data_ptr(),
                  N // 2, H, W, C, st())
    elif k == 'upsample2x_split':
        outs['out'] = (_born((N, 2 * H, 2 * W, 2 * C), torch.bfloat16), 2)
        _lib.call('bdn_upsample2x_split', z_d.data_ptr(), ls.IN_BNRELU, bn_d.data_ptr(), outs['out'][0].data_ptr(), 2 * C, 0, C,
                  N, H, W, 2 * H, 2 * W, C, st())
    elif k == 'upsample2x':
        outs['out'] = (_born((N, 2 * H, 2 * W, C), td), 2)
        _lib.call('bdn_upsample2x', dt, z_d.data_ptr(), ls.IN_BNRELU, bn_d.data_ptr(), outs['out'][0].data_ptr(), N, H, W, 2 * H, 2 * W, C, st())
    elif k == 'fuse_product':
        outs['f'] = (_born((N // 2, H, W, C), td), 1)
        _lib.call('bdn_fuse_product', dt, z_d.data_ptr(), bn_d.data_ptr(), outs['f'][0].data_ptr(), N // 2, H, W, C, st())
    elif k == 'product_pool':
        outs['f'], outs['pool'] = (_born((N // 2, H, W, C), td), 1), (_born((N, H // 2, W // 2, C), td), 2)
        _lib.call('bdn_product_pool', dt, z_d.data_ptr(), bn_d.data_ptr(), outs['f'][0].data_ptr(), outs['pool'][0].data_ptr(),
                  N // 2, H, W, C, st())
    else:
        outs['split'] = (_born((N, H, W, 2 * C), torch.bfloat16), 2)
        _lib.call('bdn_split_pack', z_d.data_ptr(), C, None, 0, ls.IN_BNRELU, bn_d.data_ptr(), N // 2, outs['split'][0].data_ptr(), N, H, W, st())
    torch.cuda.synchronize()
    for name, (t, nblocks) in outs.items():
        small = _periodic_and_period0(f'{k} {name}', t, nblocks, reps)
        if k in bt.SPLIT_KERNELS:                          # hi + lo reproduces the float32 value (the kernel's fma against the reference's mul + add)
            rec = (small[..., :C].float() + small[..., C:].float()).cpu().permute(0, 3, 1, 2)
            assert_close(f'{k} {name}: hi+lo', rec, ref['rec' if name == 'split' else name], 2e-5)
            assert bool((small[..., C:] != 0).any()), 'the lo half is all zero'
        else:
            assert_close(f'{k} {name}', from_nhwc(small), ref[name], tol)


@functools.lru_cache(maxsize=1)
def _wb_case(small, n_images):
    return bt.wb_case(small, n_images)


@pytest.mark.parametrize('tw', bt.wb_twins(), ids=bt.wb_twin_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_first_layer_weight_gradient(tw):
    """bdn_conv3x3_wgrad_bnbwd up to the last N it supports (dA, a channel slice of a wider tensor, passes 2^32 bytes there).  Route:
    integer-valued data and zero `sums` (dz = scale g exactly; the sibling's small rows cover general sums), the split operand on the LO
    grid; dW must equal (N / P) x the period's integers."""
    r, N, G, P = tw.row, tw.N, tw.G, tw.P
    assert tw.mem_bytes <= bt.MEM_CAP
    H, W, C0, Cout, p = r.H, r.W, r.C0, r.Cout, r.prec
    ipg, dt, x3 = N // G, lc.DTYPE[p], p != 'bf16'
    assert lc.instantiation(bt.twin_row(r, N)) == r.inst and lc.reduce_lanes(bt.twin_row(r, N)) == r.lanes
    rs = r._replace(N=G * P, ipg=P)
    c = _wb_case(rs, bt.wb_choose(r, 'top').N)
    reps = N // (G * P)
    lib = _lib.load()
    sp = 'fp32' if x3 else 'bf16'
    dA_d, z_d = bt.tile(_nhwc(sp, c['dA']), G, N, _alloc), bt.tile(_nhwc(sp, c['z']), G, N, _alloc)
    dA_d[..., Cout:] = float('nan')                        # the foreign channels of the wider dA: a read of them poisons the result
    xin = bt.tile(ls._split(c['x'], P) if x3 else _nhwc('bf16', c['x']), G, N, _alloc)
    assert not x3 or bool((xin[:G * P, ..., C0:] != 0).any()), 'the lo half is all zero'
    bn_d, sums = dev(c['bn']), guard.zeros(G, 2, Cout)
    wsz = max(lib.bdn_wgrad_workspace_bytes(N, H, W, Cout, C0, ipg), lib.bdn_wgrad_workspace_bytes_ex(dt, N, H, W, Cout, C0, 0, ipg, ls.IN_PLAIN, 3))
    wpart, dw = guard.empty(wsz // 4), _born((Cout, bt.WB_CREAL, 3, 3))
    assert (bt.WB_LDA, bt.WB_CREAL) == (ls.FIRST_LDA, ls.FIRST_CREAL)
    ls.first_layer_launch(r, dA_d, z_d, bn_d, sums, xin, wpart, dw, N=N, ipg=ipg)
    got, want = dw.cpu().double(), c['ref'] * reps
    print(f'density {c["density"]:.2e}, sum|terms| {c["abs_sum"] * reps / c["unit"]:.3g} units of 2^24')
    bad = got != want
    assert not bad.any(), (f'{int(bad.sum())} of {bad.numel()} filter elements differ from {reps} x the period\'s integers; the first: '
                           f'{got[bad][0].item()!r} for {want[bad][0].item()!r}')


# ------------------------------------------------------------------ bdn_pack_input
PACK_HW = (61, 125)


def _pack_cases():
    """(precision, size, B): the packed tensor [2B,H,W,16] passes 2^31 ('cross') or 2^32 ('far') bytes by a period.  The entry point's own
    bound (2 B H W Cpad / 4 < 2^31 units: 16 to 34 GB of output beside 28 GB of input) lies beyond the memory cap of this suite.  Between
    these sizes and that bound the kernel's arithmetic does not change kind: every address is a size_t product (head.hip), and its one
    32-bit quantity, the unit index, is what the bound keeps below 2^31 for the two exact FastDiv divisions."""
    out, hw = [], PACK_HW[0] * PACK_HW[1]
    for prec, bpp in (('bf16', 32), ('fp32', 64), ('bf16x3', 64)):
        for size, edge in (('cross', bt.TWO31), ('far', bt.TWO32)):
            B = -(-(edge + 2 * hw * bpp) // (2 * hw * bpp))
            out.append((prec, size, B + B % 2))
    return out


@pytest.mark.parametrize('prec,size,B', _pack_cases(), ids=lambda v: str(v))
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_pack_input(prec, size, B):
    """bdn_pack_input (64-bit addresses, unit index below 2^31): both dates periodic bit for bit, period 0 equal to the rounded input with
    zero padding channels (the reference of tests/test_gpu_kernels.py::test_pack_input_and_weights); bf16x3: the exact hi / lo split."""
    (H, W), C, Cp, P = PACK_HW, 13, 16, 2
    assert 2 * B * H * W * (Cp // 4) < bt.TWO31 and bt.TWO32 % (P * H * W * 32) and bt.TWO32 % (P * H * W * C * 4)
    x1, x2 = tk._rand((P, C, H, W), 81), tk._rand((P, C, H, W), 82)
    a, b = bt.tile(x1, 1, B, _alloc), bt.tile(x2, 1, B, _alloc)
    x3 = prec == 'bf16x3'
    td = torch.float32 if prec == 'fp32' else torch.bfloat16
    out = _born((2 * B, H, W, 2 * Cp if x3 else Cp), td)
    _lib.call('bdn_pack_input', _lib.BDN_BF16X3 if x3 else DT[prec][0], a.data_ptr(), b.data_ptr(), out.data_ptr(), B, C, H, W, Cp, st())
    torch.cuda.synchronize()
    got = from_nhwc(_periodic_and_period0('packed input', out, 2, B // P))
    x = torch.cat([x1, x2])
    if x3:
        hi = x.to(torch.bfloat16).float()
        lo = (x - hi).to(torch.bfloat16).float()
        assert torch.equal(got[:, :C], hi) and torch.equal(got[:, Cp:Cp + C], lo) and (lo != 0).any()
        assert (got[:, C:Cp] == 0).all() and (got[:, Cp + C:] == 0).all()
    else:
        assert torch.equal(got[:, :C], rnd(prec, x)) and (got[:, C:] == 0).all()


# ------------------------------------------------------------------ bdn_bn_bwd: reduction, finalize and apply
@functools.lru_cache(maxsize=1)
def _bn_bwd_case(C, H, W, P, n_images):
    return bt.bn_bwd_case(C, H, W, P, n_images)


@pytest.mark.parametrize('s', bt.bn_bwd_twins(), ids=bt.stage_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_bn_bwd(s):
    """bdn_bn_bwd past 2^31 and 2^32 bytes (64-bit addresses, int pixel counts per group).  Route: integer-valued data -- the group sums,
    dgamma and dbeta must equal (N / P) x the period's integers; dz is periodic bit for bit and period 0 meets the float64 reference at
    the bar of tests/test_gpu_kernels.py::test_bn_bwd."""
    assert s.mem_bytes <= bt.MEM_CAP
    prec, H, W, C, P, N, extra = s.prec, s.H, s.W, s.C, s.P, s.N, bt.BN_EXTRA
    c = _bn_bwd_case(C, H, W, P, bt.stage_choose('bn_bwd', prec, H, W, C, 'far').N)
    reps, ipg = N // (2 * P), N // 2
    dt, td = DT[prec]
    dA_d, z_d = bt.tile(_nhwc(prec, c['dA']), 2, N, _alloc), bt.tile(_nhwc(prec, c['z']), 2, N, _alloc)
    dA_d[..., :extra] = float('nan')                       # the foreign channels of the wider tensor: a read of them poisons the result
    dz_d = _born((N, H, W, C), td)
    wsb = guard.empty(_lib.load().bdn_bn_bwd_workspace_bytes(dt, N, H, W, C, ipg) // 4)
    sums, dgam, dbet, bn_d = _born((2, 2, C)), _born((C,)), _born((C,)), dev(c['bn'])
    _lib.call('bdn_bn_bwd', dt, dA_d.data_ptr() + extra * dA_d.element_size(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C,
              wsb.data_ptr(), sums.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dz_d.data_ptr(), st())
    torch.cuda.synchronize()
    want = c['sums'] * reps
    assert torch.equal(sums.cpu().double(), want.float().double()) and torch.equal(want.float().double(), want), 'group sums'
    assert torch.equal(dbet.cpu(), want[:, 0].sum(0).float()) and torch.equal(dgam.cpu(), want[:, 1].sum(0).float()), 'dbeta / dgamma'
    small = _periodic_and_period0('dz', dz_d, 2, reps)
    assert_close('dz', from_nhwc(small), c['dz'].float(), 1e-4 if prec == 'fp32' else 1e-2)


# ------------------------------------------------------------------ bdn_conv3x3_dgrad_first
DF_HW = (29, 45)


def _dgrad_first_cases():
    """(precision, size, B): dA and z [2B,H,W,64] pass 2^31 ('cross') or 2^32 ('far') bytes by a period.  The entry point's own bound
    (2^31 tiles) is out of any memory's reach; its addresses are 64-bit."""
    out, hw = [], DF_HW[0] * DF_HW[1]
    for prec, bpp in (('bf16', 128), ('fp32', 256)):
        for size, edge in (('cross', bt.TWO31), ('far', bt.TWO32)):
            B = -(-(edge + 2 * hw * bpp) // (2 * hw * bpp))
            out.append((prec, size, B + B % 2))
    return out


@functools.lru_cache(maxsize=1)
def _dgrad_first_case(prec, P, cr):
    """One period per date, as tests/test_gpu_input_grad.py::_run_first builds its operands ('batch' form), and its float64 reference."""
    (H, W), C, td = DF_HW, 64, tig.DT[prec][1]
    dA = tig._rand((2 * P, H, W, C), 0).to(td).float()
    z = tig._rand((2 * P, H, W, C), 1).to(td).float()
    w = tig._rand((C, cr, 3, 3), 2, 0.05)
    tab, sums = tig._table(2, C, 3), tig._rand((2, 2, C), 4, 50.0)
    dz = tig._dz64(dA, z, tab, sums, P)
    ref = torch.nn.grad.conv2d_input((2 * P, cr, H, W), w.double(), dz.permute(0, 3, 1, 2), padding=1)
    return dA.to(td), z.to(td), w, tab, sums, ref


@pytest.mark.parametrize('prec,size,B', _dgrad_first_cases(), ids=lambda v: str(v))
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_dgrad_first(prec, size, B):
    """The first convolution's data gradient with dz formed on load: both date outputs periodic bit for bit, period 0 against the float64
    reference and bar of tests/test_gpu_input_grad.py.  `sums` is an input: the period's sums times the number of periods, so that
    sums / M is the small problem's."""
    (H, W), C, cr, P = DF_HW, 64, 13, 2
    dt = tig.DT[prec][0]
    assert bt.TWO32 % (P * H * W * C * 2) and bt.TWO32 % (P * H * W * cr * 4)
    dA, z, w, tab, sums, ref = _dgrad_first_case(prec, P, cr)
    reps = B // P
    ddA, dz_ = bt.tile(dA, 2, 2 * B, _alloc), bt.tile(z, 2, 2 * B, _alloc)
    dx1, dx2 = _born((B, cr, H, W)), _born((B, cr, H, W))
    dtab, dsums, dw = dev(tab), dev(sums * reps), dev(w)
    _lib.call('bdn_conv3x3_dgrad_first', dt, ddA.data_ptr(), C, dz_.data_ptr(), dtab.data_ptr(), dsums.data_ptr(), B,
              dw.data_ptr(), cr, dx1.data_ptr(), dx2.data_ptr(), B, H, W, st())
    torch.cuda.synchronize()
    assert_close(f'dx1[{prec}]', _periodic_and_period0('dx1', dx1, 1, reps).cpu(), ref[:P], tig.TOL[prec])
    assert_close(f'dx2[{prec}]', _periodic_and_period0('dx2', dx2, 1, reps).cpu(), ref[P:], tig.TOL[prec])


BN_APPLY = (('apply', 'bf16'), ('apply', 'fp32'), ('split', 'fp32'), ('frozen', 'bf16'), ('frozen_split', 'fp32'))


@pytest.mark.parametrize('variant,prec', BN_APPLY, ids=[f'{v}-{p}' for v, p in BN_APPLY])
@pytest.mark.parametrize('shape', bt.STAGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('size', bt.STAGE_SIZES)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_bn_bwd_apply(variant, prec, shape, size):
    """bdn_bn_bwd_apply, _apply_split and _apply_frozen (dz and the [hi | lo] split store of bn_bwd_apply_kernel) on the data of
    test_big_bn_bwd: the partial rows handed in are the period's integer sums times the number of periods, one row per group, so the
    finalized sums are exact and dz is the small problem's (frozen: sums zeroed, dz = scale g exactly)."""
    H, W, C = shape
    s = bt.stage_choose('bn_bwd', prec, H, W, C, size)
    assert s.mem_bytes <= bt.MEM_CAP
    P, N, extra = s.P, s.N, bt.BN_EXTRA
    c = _bn_bwd_case(C, H, W, P, bt.stage_choose('bn_bwd', prec, H, W, C, 'far').N)
    reps, ipg = N // (2 * P), N // 2
    dt, td = DT[prec]
    dA_d, z_d = bt.tile(_nhwc(prec, c['dA']), 2, N, _alloc), bt.tile(_nhwc(prec, c['z']), 2, N, _alloc)
    dA_d[..., :extra] = float('nan')
    split = variant in ('split', 'frozen_split')
    dz_d = _born((N, H, W, 2 * C), torch.bfloat16) if split else _born((N, H, W, C), td)
    want = c['sums'] * reps
    part = dev(want.float())                               # [G][2][C]: one partial row per group
    sums, dgam, dbet, dbias, bn_d = _born((2, 2, C)), _born((C,)), _born((C,)), _born((C,)), dev(c['bn'])
    head = (dA_d.data_ptr() + extra * dA_d.element_size(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C, part.data_ptr(), 1, 0,
            sums.data_ptr(), dgam.data_ptr(), dbet.data_ptr())
    if variant == 'apply':
        _lib.call('bdn_bn_bwd_apply', dt, *head, dz_d.data_ptr(), None, st())
    elif variant == 'split':
        _lib.call('bdn_bn_bwd_apply_split', *head, dz_d.data_ptr(), None, st())
    else:
        _lib.call('bdn_bn_bwd_apply_frozen', _lib.BDN_BF16X3 if split else dt, *head, dbias.data_ptr(), dz_d.data_ptr(), None, st())
    torch.cuda.synchronize()
    frozen = variant.startswith('frozen')
    assert torch.equal(dbet.cpu(), want[:, 0].sum(0).float()) and torch.equal(dgam.cpu(), want[:, 1].sum(0).float()), 'dbeta / dgamma'
    assert torch.equal(sums.cpu().double(), torch.zeros_like(want) if frozen else want), 'group sums'
    small = _periodic_and_period0('dz', dz_d, 2, reps)
    got = (small[..., :C].float() + small[..., C:].float()).cpu().permute(0, 3, 1, 2) if split else from_nhwc(small)
    if frozen:                                             # scale g under the mask: small integers, exact in every format
        g64 = c['dA'][:, extra:].double()
        ref = torch.cat([bn2 * g64[g * P:(g + 1) * P] * (c['z'][g * P:(g + 1) * P].double() * bn2 + bn3 > 0)
                         for g in range(2) for bn2, bn3 in [(c['bn'][g, 2].double()[None, :, None, None], c['bn'][g, 3].double()[None, :, None, None])]])
        assert torch.equal(got.double(), ref)
    else:
        assert_close('dz', got, c['dz'].float(), 1e-4 if prec == 'fp32' else 1e-2)
        assert not split or bool((small[..., C:] != 0).any()), 'the lo half is all zero'


# ------------------------------------------------------------------ enc_skip_bwd, upsample2x_bwd
@functools.lru_cache(maxsize=1)
def _stage_backward_case(kernel, prec, H, W, C, P):
    """Operands and autograd references as tests/test_gpu_kernels.py builds them (test_enc_skip_bwd, test_upsample2x_and_backward)."""
    from oracle import bidate_oracle as O
    if kernel == 'enc_skip_bwd':
        B, extra = P, bt.SKIP_EXTRA
        z = rnd(prec, tk._rand((2 * B, C, H, W), 51))
        bn = bn_table(2, C, 52)
        dF = rnd(prec, tk._rand((B, C + extra, H, W), 53))
        dP = rnd(prec, tk._rand((2 * B, C, H // 2, W // 2), 54))
        a = bnrelu_ref(prec, z, bn, B).double().requires_grad_(True)
        ((torch.relu(a[B:] * a[:B]) * dF[:, :C].double()).sum() + (O.maxpool2(a) * dP.double()).sum()).backward()
        return {'z': z, 'bn': bn, 'dF': dF, 'dP': dP, 'ref': a.grad.float(), 'live': (a.detach() > 0).float()}
    extra = bt.BN_EXTRA
    dU = rnd(prec, tk._rand((2 * P, C + extra, 2 * H, 2 * W), 47))
    a = torch.zeros(2 * P, C, H, W, dtype=torch.float64, requires_grad=True)
    O.pad_to(O.upsample2x_align(a), torch.zeros(2 * P, 1, 2 * H, 2 * W)).backward(dU[:, extra:].double())
    return {'dU': dU, 'ref': a.grad.float()}


@pytest.mark.parametrize('s', bt.stage_backward_twins(), ids=bt.stage_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_stage_backward(s):
    """bdn_enc_skip_bwd (without the fused statistics: the per-image output) and bdn_upsample2x_bwd past 2^31 and 2^32 bytes: periodic bit
    for bit, period 0 against the autograd references and bars of tests/test_gpu_kernels.py."""
    assert s.mem_bytes <= bt.MEM_CAP
    k, prec, H, W, C, P, N = s.kernel, s.prec, s.H, s.W, s.C, s.P, s.N
    c = _stage_backward_case(k, prec, H, W, C, P)
    dt, td = DT[prec]
    reps = N // (2 * P)
    if k == 'enc_skip_bwd':
        B, extra = N // 2, bt.SKIP_EXTRA
        dF_d = bt.tile(_nhwc(prec, c['dF']), 1, B, _alloc)
        dF_d[..., C:] = float('nan')                       # the foreign channels ([dF | dU]): a read of them poisons the result
        z_d, dP_d, bn_d = bt.tile(_nhwc(prec, c['z']), 2, N, _alloc), bt.tile(_nhwc(prec, c['dP']), 2, N, _alloc), dev(c['bn'])
        out = _born((N, H, W, C), td)
        _lib.call('bdn_enc_skip_bwd', dt, dF_d.data_ptr(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), dP_d.data_ptr(), out.data_ptr(), None,
                  B, H, W, C, st())
        torch.cuda.synchronize()
        got = from_nhwc(_periodic_and_period0('dA', out, 2, reps))
        # where a == 0 the reference's relu(a2 a1) has zero slope while the kernel returns dF a_other; the producer's own ReLU mask
        # multiplies both in the next step, so compare there (as the sibling does)
        assert_close('enc_skip_bwd', got * c['live'], c['ref'] * c['live'], 1e-6 if prec == 'fp32' else 8e-3)
    else:
        extra = bt.BN_EXTRA
        dU_d = bt.tile(_nhwc(prec, c['dU']), 2, N, _alloc)
        dU_d[..., :extra] = float('nan')
        dsrc = _born((N, H, W, C), td)
        _lib.call('bdn_upsample2x_bwd', dt, dU_d.data_ptr() + extra * dU_d.element_size(), C + extra, dsrc.data_ptr(), N, H, W, 2 * H, 2 * W, C, st())
        torch.cuda.synchronize()
        small = _periodic_and_period0('dsrc', dsrc, 2, reps)
        assert_close('upsample bwd', from_nhwc(small), c['ref'], 1e-5 if prec == 'fp32' else 8e-3)
        # bdn_upsample2x_bwd_bs: the same pass with the BatchNorm-backward partial sums of the upsampled layer (the tiled kernel): the stored
        # gradient is g = dsrc [scale z_prev + shift > 0]; g, and the per-tile partial rows, are periodic; period 0 as the sibling holds it
        rows = _lib.load().bdn_upsample2x_bwd_rows(dt, N, H, W, C)
        assert rows > 0 and rows % (2 * reps) == 0
        zp, bnp = rnd(prec, tk._rand((2 * P, C, H, W), 48)), bn_table(1, C, 49)
        zp_d, bnp_d = bt.tile(_nhwc(prec, zp), 2, N, _alloc), dev(bnp)
        dsrc2, part = _born((N, H, W, C), td), _born((rows, 2, C))
        _lib.call('bdn_upsample2x_bwd_bs', dt, dU_d.data_ptr() + extra * dU_d.element_size(), C + extra, dsrc2.data_ptr(), zp_d.data_ptr(),
                  bnp_d.data_ptr(), part.data_ptr(), N, H, W, 2 * H, 2 * W, C, st())
        torch.cuda.synchronize()
        g_small, part_small = _periodic_and_period0('g', dsrc2, 2, reps), _periodic_and_period0('partial rows', part, 2, reps)
        assert_masked('upsample bwd', from_nhwc(g_small), from_nhwc(small), preact(zp, bnp, 2 * P))
        g, got = from_nhwc(g_small).double(), part_small.cpu().double().sum(0)
        assert_close('upsample bwd: sum g', got[0], g.sum((0, 2, 3)), 2e-5 if prec == 'fp32' else 1e-4, 1e-4)
        assert_close('upsample bwd: sum g z', got[1], (g * zp.double()).sum((0, 2, 3)), 2e-5 if prec == 'fp32' else 1e-4, 1e-4)


# ------------------------------------------------------------------ the classifier: bdn_outc_fwd, bdn_outc_bwd
@functools.lru_cache(maxsize=1)
def _outc_case(prec, H, W, C, P, ncls=2):
    """tests/test_gpu_kernels.py::test_outc_fwd_bwd on 2 P images."""
    from oracle import bidate_oracle as O
    z = rnd(prec, tk._rand((2 * P, C, H, W), 61))
    bn = bn_table(1, C, 62)
    w, b = tk._rand((ncls, C, 1, 1), 63, 0.2), tk._rand((ncls,), 64, 0.1)
    a = bnrelu_ref(prec, z, bn, 2 * P).double().requires_grad_(True)
    ref = O.conv1x1(a, w.double(), b.double())
    dl = tk._rand((2 * P, ncls, H, W), 65)
    ref.backward(dl.double())
    return {'z': z, 'bn': bn, 'w': w, 'b': b, 'dl': dl, 'logits': ref.detach().float(), 'dA': a.grad.float()}


@pytest.mark.parametrize('s', bt.outc_twins(), ids=bt.stage_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_classifier(s):
    """bdn_outc_fwd and the data gradient of bdn_outc_bwd at the classifier's width past 2^31 and 2^32 bytes: logits and dA periodic bit for
    bit, period 0 against the references and bars of tests/test_gpu_kernels.py.  (dw, db and the fused partial sums are float32
    reductions over all pixels: held to the references at the sibling's small shapes only.)"""
    assert s.mem_bytes <= bt.MEM_CAP
    prec, H, W, C, P, N, ncls = s.prec, s.H, s.W, s.C, s.P, s.N, 2
    c = _outc_case(prec, H, W, C, P)
    dt, td = DT[prec]
    reps = N // (2 * P)
    lib = _lib.load()
    z_d, dl_d = bt.tile(_nhwc(prec, c['z']), 2, N, _alloc), bt.tile(c['dl'], 2, N, _alloc)
    bn_d, w_d, b_d = dev(c['bn']), dev(c['w']), dev(c['b'])
    logits, dA = _born((N, ncls, H, W)), _born((N, H, W, C), td)
    _lib.call('bdn_outc_fwd', dt, z_d.data_ptr(), bn_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), logits.data_ptr(), N, H, W, C, ncls, st())
    dw, db = _born((ncls, C)), _born((ncls,))
    ows = guard.empty(lib.bdn_outc_bwd_workspace_bytes(dt, N, H, W, C, ncls) // 4)
    _lib.call('bdn_outc_bwd', dt, dl_d.data_ptr(), z_d.data_ptr(), bn_d.data_ptr(), w_d.data_ptr(), dA.data_ptr(),
              dw.data_ptr(), db.data_ptr(), None, ows.data_ptr(), N, H, W, C, ncls, st())
    torch.cuda.synchronize()
    assert_close('logits', _periodic_and_period0('logits', logits, 2, reps).cpu(), c['logits'], 1e-5)
    assert_close('dA', from_nhwc(_periodic_and_period0('dA', dA, 2, reps)), c['dA'], 1e-5 if prec == 'fp32' else 8e-3)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()


# ------------------------------------------------------------------ reductions over the N x tiles rows of a big launch: integers, equality
TOTALS_ROWS = ('fwd-bf16-4x61x125-64+64-256-g2', 'fwd-bf16-4x29x45-64-64-g2-bnrelu', 'fwd-fp32-4x61x125-128-256-g2-bnrelu',
               'dgrad_bs-bf16-4x61x125-128-256-g2', 'dgrad_bs-fp32-4x29x45-64-64-g2')


@functools.lru_cache(maxsize=1)
def _int_case(maker, small):
    return maker(small)


def _group_totals(part, G):
    """Per-group float64 sums of the partial rows [rows][2][C], formed on the device (exact: integers far below 2^53)."""
    return part.double().reshape(G, part.shape[0] // G, 2, part.shape[2]).sum(1).cpu()


@pytest.mark.parametrize('t', [t for t in bt.twins() if t.twin.size == 'top' and lc.row_id(t.row) in TOTALS_ROWS], ids=bt.twin_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_statistics_totals(t):
    """The fused statistics of a big launch and the finalize kernels over its N x tiles partial rows, on integer-valued data.
    fwd: the tile partials add up to exactly (N / P) x the period's sum z and sum z^2, and bdn_bn_finalize over those rows gives the mean
    float32(S / count) exactly (its arithmetic is double) and invstd / scale / shift / running statistics of the same exact sums.
    dgrad_bs: bdn_bn_bwd_finalize (raw moments, the many-row plan) over the launch's rows gives exactly (N / P) x the period's sum g and
    sum g z, dgamma and dbeta."""
    r, tw = t.row, t.twin
    N, G, P = tw.N, tw.G, tw.P
    assert lc.instantiation(bt.twin_row(r, N)) == t.inst
    rs, reps, ipg = bt.small_row(r, P), N // (G * P), N // G
    p, H, W, Cout = r.prec, r.H, r.W, r.Cout
    td = torch.bfloat16 if p == 'bf16' else torch.float32
    lib = _lib.load()
    nt = lib.bdn_conv3x3_num_mtiles(N, H, W, Cout, ipg)
    assert nt // G > 512, 'the two-stage row plan'
    part = _born((nt, 2, Cout))
    if r.op == 'fwd':
        c = _int_case(bt.int_forward_case, rs)
        d0 = bt.tile(_nhwc(p, c.x0), G, N, _alloc)
        d1 = bt.tile(_nhwc(p, c.x1), G, N, _alloc) if r.C1 else None
        out = _born((N, H, W, Cout), td)
        ls.forward_launch(r, c, d0, d1, out, part, N=N, ipg=ipg)
        want = c.totals * reps
        assert torch.equal(_group_totals(part, G), want), 'tile partials: sum z, sum z^2'
        assert torch.equal(from_nhwc(bt.period0(out, G, reps)).double(), c.ref)
        gamma, beta = tk._rand((Cout,), 6).abs() + 0.5, tk._rand((Cout,), 7, 0.3)
        rm0, rv0 = tk._rand((Cout,), 8, 0.2), tk._rand((Cout,), 9).abs() + 0.5
        drm, drv, dg, db = dev(rm0), dev(rv0), dev(gamma), dev(beta)
        nbt, bn = guard.zeros(1, dtype=torch.int64), _born((G, 4, Cout))
        fws = guard.empty(lib.bdn_bn_finalize_workspace_bytes(nt, G, Cout) // 8, dtype=torch.float64)
        count = ipg * H * W
        _lib.call('bdn_bn_finalize', part.data_ptr(), nt, G, Cout, count, dg.data_ptr(), db.data_ptr(), 1e-5, 0.1, drm.data_ptr(),
                  drv.data_ptr(), nbt.data_ptr(), bn.data_ptr(), fws.data_ptr(), st())
        torch.cuda.synchronize()
        bn, rm, rv = bn.cpu(), rm0.double(), rv0.double()
        for g in range(G):
            mean = want[g, 0] / count
            var = want[g, 1] / count - mean * mean
            inv = 1 / torch.sqrt(var + float(torch.tensor(1e-5, dtype=torch.float32)))
            assert torch.equal(bn[g, 0], mean.float()), 'mean'
            assert torch.allclose(bn[g, 1].double(), inv, rtol=1e-6, atol=0), 'invstd'
            assert torch.allclose(bn[g, 2].double(), gamma.double() * inv, rtol=1e-6, atol=0), 'scale'
            assert torch.allclose(bn[g, 3].double(), beta.double() - mean * gamma.double() * inv, rtol=1e-5, atol=1e-6), 'shift'
            rm = 0.9 * rm + 0.1 * mean
            rv = 0.9 * rv + 0.1 * var * count / (count - 1)
        assert torch.allclose(drm.cpu().double(), rm, rtol=1e-6, atol=1e-7) and torch.allclose(drv.cpu().double(), rv, rtol=1e-6, atol=1e-7)
        assert int(nbt.item()) == G
    else:
        c = _int_case(bt.int_dgrad_bs_case, rs)
        ddz, zp_d = bt.tile(_nhwc(p, c.dz), G, N, _alloc), bt.tile(_nhwc(p, c.zprev), G, N, _alloc)
        plain, dA = _born((N, H, W, Cout), td), _born((N, H, W, Cout), td)
        ls.dgrad_bs_launch(r, c, ddz, zp_d, plain, dA, part, N=N, ipg=ipg)
        want = c.sums * reps
        assert torch.equal(_group_totals(part, G), want), 'tile partials: sum g, sum g z'
        assert torch.equal(from_nhwc(bt.period0(plain, G, reps)).double(), c.ref)
        _bwd_finalize_equals(c.bnp, part, G, Cout, want)


def _bwd_finalize_equals(bn, part, G, C, want):
    """bdn_bn_bwd_finalize (raw moments; the table has mean 0 and invstd 1) over `part` [G * rows][2][C]: sums, dgamma, dbeta == want."""
    lib = _lib.load()
    sums, dgam, dbet, bn_d = _born((G, 2, C)), _born((C,)), _born((C,)), dev(bn)
    scratch = guard.empty(lib.bdn_bn_bwd_scratch_bytes(G, C) // 8, dtype=torch.float64)
    _lib.call('bdn_bn_bwd_finalize', bn_d.data_ptr(), G, C, part.data_ptr(), part.shape[0] // G, 1, sums.data_ptr(), dgam.data_ptr(),
              dbet.data_ptr(), scratch.data_ptr(), st())
    torch.cuda.synchronize()
    assert torch.equal(want.float().double(), want), 'the expected sums are not float32 numbers'
    assert torch.equal(sums.cpu().double(), want), 'sums'
    assert torch.equal(dbet.cpu(), want[:, 0].sum(0).float()) and torch.equal(dgam.cpu(), want[:, 1].sum(0).float()), 'dbeta / dgamma'


@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
@pytest.mark.parametrize('shape', bt.STAGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_enc_skip_sums(prec, shape):
    """bdn_enc_skip_bwd with its fused statistics past 2^32 bytes on integer-valued data (no pooling: ties of equal integers would make the
    arg-max a matter of convention): the stored gradient is g, periodic bit for bit and exact in period 0; the per-date partial rows and
    bdn_bn_bwd_finalize over them give exactly (N / P) x the period's sum g and sum g z."""
    H, W, C = shape
    s = bt.stage_choose('enc_skip_bwd', prec, H, W, C, 'far')
    P, N, extra = s.P, s.N, bt.SKIP_EXTRA
    B, reps = N // 2, N // (2 * P)
    c = _enc_skip_int_case(C, H, W, P)
    dt, td = DT[prec]
    dF_d = bt.tile(_nhwc(prec, c['dF']), 1, B, _alloc)
    dF_d[..., C:] = float('nan')
    z_d, bn_d = bt.tile(_nhwc(prec, c['z']), 2, N, _alloc), dev(c['bn'])
    out = _born((N, H, W, C), td)
    rows = _lib.load().bdn_enc_skip_bwd_rows(dt, B, H, W, C)
    part = _born((2, rows, 2, C))
    _lib.call('bdn_enc_skip_bwd', dt, dF_d.data_ptr(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), None, out.data_ptr(), part.data_ptr(),
              B, H, W, C, st())
    torch.cuda.synchronize()
    assert torch.equal(from_nhwc(_periodic_and_period0('g', out, 2, reps)).double(), c['g'])
    want = c['sums'] * reps
    assert torch.equal(_group_totals(part.reshape(2 * rows, 2, C), 2), want), 'partial rows'
    _bwd_finalize_equals(c['bn'], part.reshape(2 * rows, 2, C), 2, C, want)


@functools.lru_cache(maxsize=1)
def _enc_skip_int_case(C, H, W, P):
    return bt.int_enc_skip_case(C, H, W, P)


@functools.lru_cache(maxsize=1)
def _outc_int_case(C, H, W, P, n_images):
    return bt.int_outc_case(C, H, W, P, n_images)


OUTC_APPLY = ('bf16', 'fp32', 'bf16x3')


@pytest.mark.parametrize('prec', OUTC_APPLY)
@pytest.mark.parametrize('size', bt.STAGE_SIZES)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_classifier_backward_sums(prec, size):
    """bdn_outc_bwd (dA = NULL), bdn_bn_bwd_finalize over its partial rows and bdn_outc_bn_bwd_apply past 2^31 and 2^32 bytes on
    integer-valued data: dw, db, the group sums, dgamma and dbeta equal (N / P) x the period's integers; dz (bf16x3: the [hi | lo]
    operand) is periodic bit for bit and period 0 meets float64 at the bar of tests/test_gpu_kernels.py::test_bn_bwd."""
    H, W, C, ncls = 64, 64, 64, 2
    zp = 'fp32' if prec == 'bf16x3' else prec
    s = bt.stage_choose('outc', zp, H, W, C, size)
    P, N = s.P, s.N
    reps = N // (2 * P)
    c = _outc_int_case(C, H, W, P, bt.stage_choose('outc', zp, H, W, C, 'far').N)
    dt, td = DT[zp]
    lib = _lib.load()
    z_d, dl_d = bt.tile(_nhwc(zp, c['z']), 2, N, _alloc), bt.tile(c['dl'], 2, N, _alloc)
    bn_d, w_d = dev(c['bn']), dev(c['w'])
    dw, db = _born((ncls, C)), _born((ncls,))
    part = _born((lib.bdn_outc_bwd_rows(dt, N, H, W, C), 2, C))
    ows = guard.empty(lib.bdn_outc_bwd_workspace_bytes(dt, N, H, W, C, ncls) // 4)
    _lib.call('bdn_outc_bwd', dt, dl_d.data_ptr(), z_d.data_ptr(), bn_d.data_ptr(), w_d.data_ptr(), None, dw.data_ptr(), db.data_ptr(),
              part.data_ptr(), ows.data_ptr(), N, H, W, C, ncls, st())
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu().double(), c['dw'] * reps), 'dw'
    assert torch.equal(db.cpu().double(), c['db'] * reps), 'db'
    want = c['sums'] * reps
    assert torch.equal(_group_totals(part, 1), want), 'partial rows'
    _bwd_finalize_equals(c['bn'], part, 1, C, want)
    sums = dev(want.float())
    split = prec == 'bf16x3'
    dz = _born((N, H, W, 2 * C), torch.bfloat16) if split else _born((N, H, W, C), td)
    _lib.call('bdn_outc_bn_bwd_apply', _lib.BDN_BF16X3 if split else dt, dl_d.data_ptr(), w_d.data_ptr(), z_d.data_ptr(), bn_d.data_ptr(), N,
              sums.data_ptr(), dz.data_ptr(), N, H, W, C, ncls, st())
    torch.cuda.synchronize()
    small = _periodic_and_period0('dz', dz, 2, reps)
    got = (small[..., :C].float() + small[..., C:].float()).cpu().permute(0, 3, 1, 2) if split else from_nhwc(small)
    assert_close('dz', got, c['dz'].float(), 1e-2 if prec == 'bf16' else 1e-4)


@pytest.mark.parametrize('s', bt.bn_bwd_twins(), ids=bt.stage_id)
@measured(cap=bt.MEM_CAP)
@guarded
def test_big_bn_bwd_frozen(s):
    """bdn_bn_bwd_frozen (running statistics: reduction pass, frozen finalize, dz = scale g) on the integer data of test_big_bn_bwd: dbeta,
    dgamma and the conv-bias gradient equal (N / P) x the period's integers, `sums` is zeroed, dz is periodic and exactly scale g."""
    prec, H, W, C, P, N, extra = s.prec, s.H, s.W, s.C, s.P, s.N, bt.BN_EXTRA
    c = _bn_bwd_case(C, H, W, P, bt.stage_choose('bn_bwd', prec, H, W, C, 'far').N)
    reps, ipg = N // (2 * P), N // 2
    dt, td = DT[prec]
    dA_d, z_d = bt.tile(_nhwc(prec, c['dA']), 2, N, _alloc), bt.tile(_nhwc(prec, c['z']), 2, N, _alloc)
    dA_d[..., :extra] = float('nan')
    dz_d = _born((N, H, W, C), td)
    wsb = guard.empty(_lib.load().bdn_bn_bwd_workspace_bytes(dt, N, H, W, C, ipg) // 4)
    sums, dgam, dbet, dbias, bn_d = _born((2, 2, C)), _born((C,)), _born((C,)), _born((C,)), dev(c['bn'])
    _lib.call('bdn_bn_bwd_frozen', dt, dA_d.data_ptr() + extra * dA_d.element_size(), C + extra, z_d.data_ptr(), bn_d.data_ptr(), ipg, N, H, W, C,
              wsb.data_ptr(), sums.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dbias.data_ptr(), dz_d.data_ptr(), st())
    torch.cuda.synchronize()
    want = c['sums'] * reps
    dbeta = want[:, 0].sum(0).float()
    assert torch.equal(dbet.cpu(), dbeta) and torch.equal(dgam.cpu(), want[:, 1].sum(0).float()), 'dbeta / dgamma'
    assert torch.equal(dbias.cpu(), c['bn'][0, 2] * dbeta) and not bool(sums.cpu().any()), 'dbias / zeroed sums'
    g64 = c['dA'][:, extra:].double()
    ref = torch.cat([sc * g64[g * P:(g + 1) * P] * (c['z'][g * P:(g + 1) * P].double() * sc + sh > 0) for g in range(2)
                     for sc, sh in [(c['bn'][g, 2].double()[None, :, None, None], c['bn'][g, 3].double()[None, :, None, None])]])
    assert torch.equal(from_nhwc(_periodic_and_period0('dz', dz_d, 2, reps)).double(), ref)
