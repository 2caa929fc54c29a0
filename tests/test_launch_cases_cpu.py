"""CPU guard of the launch-shape table (tests/launch_cases.py): host-side variant queries only, no GPU.

(a) every row selects the instantiation it names; (b) every instantiation one training step of BiDateNet(13, 2) at batch 64 on
128 x 128 patches launches -- in all four numerics settings -- and every one an eval forward launches has a row, so a new tile
configuration of the step cannot go untested by tests/test_gpu_launch_shapes.py.
"""
import pytest

from tests import launch_cases as lc


@pytest.mark.parametrize('r', lc.ROWS, ids=lc.row_id)
def test_row_selects_its_instantiation(r):
    assert lc.instantiation(r) == r.inst
    if r.op in ('wgrad', 'wgrad_bnbwd'):
        assert lc.reduce_lanes(r) == r.lanes


def test_rows_are_distinct_and_cover_every_reduction_width():
    ids = [lc.row_id(r) for r in lc.ROWS]
    assert len(ids) == len(set(ids))
    assert {r.lanes for r in lc.ROWS if r.lanes} == {1, 2, 4, 8, 16}
    # the BatchNorm-statistics rows straddle both row plans of the reductions
    assert min(c[0] for c in lc.STATS_CASES) <= 512 < max(c[0] for c in lc.STATS_CASES)


@pytest.mark.parametrize('precision', ['bf16', 'fp32', 'bf16x3', 'bf16x3-fast'])
def test_every_training_step_instantiation_has_a_row(precision):
    step = lc.train_step_instantiations(precision, B=64, S=128)
    assert any(i.startswith('conv3x3_kernel<') for i in step) and any(i.startswith('wgrad') for i in step)
    missing = step - lc.covered()
    assert not missing, f'{precision}: instantiations of the step without a row: {sorted(missing)}'


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
@pytest.mark.parametrize('B', [256, 64])
def test_every_eval_forward_instantiation_has_a_row(precision, B):
    ev = lc.eval_forward_instantiations(precision, B, S=128)
    assert all(',true,0,false>' in i for i in ev)          # the eval epilogue (EV) instantiations
    missing = ev - lc.covered()
    assert not missing, f'{precision} B={B}: eval instantiations without a row: {sorted(missing)}'


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
