"""CPU guard of the launch-shape table (tests/launch_cases.py): host-side variant queries only, no GPU.

(a) every row selects the instantiation it names; (b) every instantiation one training step of BiDateNet(c, 2) at batch 64 on
128 x 128 patches launches -- in all four numerics settings, for c = 13 and for the wide inputs 17, 32, 48 and 64 bands (first layer
padded to 32, 48, 64 channels) -- and every one an eval forward launches has a row, so a new tile configuration of the step cannot go
untested by tests/test_gpu_launch_shapes.py.
"""
import pytest

from tests import launch_cases as lc


@pytest.mark.parametrize('r', lc.ALL_ROWS, ids=lc.row_id)
def test_row_selects_its_instantiation(r):
    assert lc.instantiation(r) == r.inst
    if r.op in ('wgrad', 'wgrad_bnbwd'):
        assert lc.reduce_lanes(r) == r.lanes


def test_rows_are_distinct_and_cover_every_reduction_width():
    ids = [lc.row_id(r) for r in lc.ALL_ROWS]
    assert len(ids) == len(set(ids))
    assert {r.lanes for r in lc.ROWS if r.lanes} == {1, 2, 4, 8, 16}
    # the BatchNorm-statistics rows straddle both row plans of the reductions
    assert min(c[0] for c in lc.STATS_CASES) <= 512 < max(c[0] for c in lc.STATS_CASES)


BANDS = (13, 17, 32, 48, 64)          # 13: the ids the cases always had; the wide ones carry -c<bands>


def _band_cases(keys):
    """[(key..., n_channels)], ids: the key alone at 13 bands."""
    cases = [(*k, c) for c in BANDS for k in keys]
    return cases, ['-'.join(str(v) for v in k[:-1]) + ('' if k[-1] == 13 else f'-c{k[-1]}') for k in cases]


_STEP_CASES, _STEP_IDS = _band_cases([(p,) for p in ('bf16', 'fp32', 'bf16x3', 'bf16x3-fast')])
_EVAL_CASES, _EVAL_IDS = _band_cases([(B, p) for p in ('bf16', 'fp32') for B in (256, 64)])


def test_wide_rows_carry_their_real_channel_count():
    """Every wide row has creal <= C0 = creal rounded up to 16 (the engine's cp), each (creal, C0) pair in every op and precision it
    applies to, and no row of the 16-band table carries one."""
    assert all(r.creal is None for r in lc.ROWS)
    assert all(r.creal and r.C0 == (r.creal + 15) // 16 * 16 and not r.C1 and not r.bnrelu for r in lc.WIDE_ROWS)
    want = {(op, p) for op in ('fwd', 'eval') for p in ('bf16', 'fp32')} | {('x3', p) for p in ('bf16x3', 'bf16x2')} | \
           {('wgrad', p) for p in ('bf16', 'fp32', 'bf16x3', 'bf16x2')}
    for pair in lc.WIDE_PAIRS:
        assert {(r.op, r.prec) for r in lc.WIDE_ROWS if (r.creal, r.C0) == pair} == want, pair
    assert {(r.creal, r.C0) for r in lc.WIDE_ROWS} == {(17, 32), (33, 48), (50, 64), (64, 64)}


@pytest.mark.parametrize('precision,n_channels', _STEP_CASES, ids=_STEP_IDS)
def test_every_training_step_instantiation_has_a_row(precision, n_channels):
    step = lc.train_step_instantiations(precision, B=64, S=128, n_channels=n_channels)
    assert any(i.startswith('conv3x3_kernel<') for i in step) and any(i.startswith('wgrad') for i in step)
    missing = step - lc.covered()
    assert not missing, f'{precision}, {n_channels} bands: instantiations of the step without a row: {sorted(missing)}'
    if n_channels != 13:           # the small step tests/test_gpu_launch_shapes.py records on the device at wide inputs
        small = lc.train_step_instantiations(precision, B=2, S=32, n_channels=n_channels) - lc.covered()
        assert not small, f'{precision}, {n_channels} bands at batch 2, 32 x 32: without a row: {sorted(small)}'
        first = lc._layers(n_channels)['e1a']
        assert first.cin == (n_channels + 15) // 16 * 16 > 16
        assert lc.BiDateEngine(n_channels, 2, precision).first_wgrad_dtype(4, 32, 32, 2) is None      # bn_bwd + the generic GEMM


@pytest.mark.parametrize('B,precision,n_channels', _EVAL_CASES, ids=_EVAL_IDS)
def test_every_eval_forward_instantiation_has_a_row(precision, B, n_channels):
    ev = lc.eval_forward_instantiations(precision, B, S=128, n_channels=n_channels)
    assert all(',true,0,false>' in i for i in ev)          # the eval epilogue (EV) instantiations
    missing = ev - lc.covered()
    assert not missing, f'{precision} B={B}, {n_channels} bands: eval instantiations without a row: {sorted(missing)}'
    if n_channels != 13:
        small = lc.eval_forward_instantiations(precision, 2, S=32, n_channels=n_channels) - lc.covered()
        assert not small, f'{precision}, {n_channels} bands at batch 2, 32 x 32: without a row: {sorted(small)}'


def test_eval_variant_query():
    """bdn_conv3x3_eval_variant answers for the stage, pair and classifier entry points and refuses what they refuse."""
    from fabric_amd._lib import BDN_BF16, BDN_BF16X3, BDN_F32, EVAL_CLS, EVAL_PAIR, EVAL_STAGE
    q = lc.eval_inst
    assert q(EVAL_STAGE, BDN_BF16, 4, 61, 125, 64, 64, 256) == 'conv3x3_kernel<bf16,128,8,16,1,128,1,4,false,bf16,false,false,true,0,false>'
    assert q(EVAL_PAIR, BDN_BF16, 4, 29, 45, 64, 0, 64) == 'conv3x3_kernel<bf16,128,8,16,2,64,2,2,true,bf16,false,false,true,0,false>'
    assert q(EVAL_CLS, BDN_F32, 4, 29, 45, 64, 0, 64) == 'conv3x3_kernel<float,128,16,16,1,64,4,1,false,float,false,false,true,0,false>'
    assert q(EVAL_CLS, BDN_BF16, 4, 29, 45, 64, 0, 128) == ''       # the classifier stage has 64 channels
    assert q(EVAL_PAIR, BDN_BF16, 4, 29, 45, 32, 0, 64) == ''       # pairs need whole 128-byte chunks
    assert q(EVAL_PAIR, BDN_BF16, 4, 29, 45, 64, 64, 64) == ''      # one source
    assert q(EVAL_STAGE, BDN_BF16X3, 4, 29, 45, 64, 0, 64) == ''    # bf16 / f32 only
    assert q(7, BDN_BF16, 4, 29, 45, 64, 0, 64) == ''


@pytest.mark.parametrize('shape', [(128, 8, 8, 128, 128, 64), (512, 8, 8, 64, 64, 256), (4, 61, 125, 64, 64, 2), (8, 8, 8, 512, 512, 4),
                                   (128, 128, 128, 64, 16, 64)])
def test_generic_wgrad_workspace_covers_every_dtype(shape):
    """bdn_wgrad_workspace_bytes is documented to cover every dtype of the shape under default flags: BDN_BF16X2 included -- its
    doubled-operand plan on small maps has fewer tiles than BDN_BF16X3's and therefore more splits (it used to be left out)."""
    from fabric_amd import _lib
    lib = _lib.load()
    N, H, W, Cout, Cin, ipg = shape
    generic = lib.bdn_wgrad_workspace_bytes(N, H, W, Cout, Cin, ipg)
    for dt in lc.DTYPE.values():
        assert lib.bdn_wgrad_workspace_bytes_ex(dt, N, H, W, Cout, Cin, 0, ipg, 0, 0) <= generic, dt
