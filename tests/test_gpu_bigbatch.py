"""-m gpu: eval-mode BiDateNet at the largest tile batches utils/inference._check_widest admits.

BASELINE's model (13 bands, 128 x 128 tiles, weights and running statistics from oracle.filler) at 1023 (bf16), 511 (fp32) and 511
(bf16x3) tiles -- the widest tensor of the forward is a few hundred KB short of 4 GB there -- and at the largest even batch below each.
The tiles are periodic with a period P that divides the batch, so the logits must be periodic bit for bit (every byte of them is compared
on the device, tests/bigtensor.py), and period 0 must agree with the same P tiles run as a batch of P within the model-level eval bar of
tests/test_gpu_model.py (test_eval_mode_matches_reference: 2e-5 / 1e-4 / 3e-2 of the logit scale for fp32 / bf16x3 / bf16).  Each case
prints its wall time and peak device memory; the 24 GiB cap of the kernel-level twins (tests/bigtensor.py MEM_CAP) does not apply here: the
forward's workspace at these batches is 33 to 40 GiB, which is what this file is there to record.  The refusal at max + 1 is a CPU test (tests/test_bigtensor_cpu.py).
"""
import pytest
import torch

from fabric_amd import BiDateNet
from fabric_amd.utils.inference import _check_widest
from oracle import filler
from tests import bigtensor as bt
from tests.test_gpu_bigtensor import measured

pytestmark = pytest.mark.gpu

EVAL_BAR = {'fp32': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}       # tests/test_gpu_model.py, relative to the largest |logit|
CASES = [('bf16', 1023), ('bf16', 1022), ('fp32', 511), ('fp32', 510), ('bf16x3', 511), ('bf16x3', 510)]


def _period(B):
    """The smallest divisor of B above 1 (1023 = 3 x 341, 511 = 7 x 73; even batches: 2)."""
    return next(p for p in range(2, B + 1) if B % p == 0)


@pytest.mark.parametrize('prec,B', CASES, ids=[f'{p}-{b}' for p, b in CASES])
@measured
def test_eval_forward_at_the_widest_batch(prec, B):
    P, S = _period(B), 128
    model = filler.fill_module(BiDateNet(13, 2, precision=prec)).cuda().eval()
    _check_widest(model.engine(), B, S)
    x1, x2, _ = filler.make_inputs(P, 13, S, seed=0)
    x1, x2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    with torch.no_grad():
        small = model(x1, x2).clone()
        big = model(x1.repeat(B // P, 1, 1, 1), x2.repeat(B // P, 1, 1, 1))
    torch.cuda.synchronize()
    assert big.shape == (B, 2, S, S) and small.shape == (P, 2, S, S)
    bt.assert_periodic(f'{prec} logits at batch {B}', big.contiguous(), 1, B // P)
    scale = small.abs().max().item()
    d = (big[:P] - small).abs().max().item()
    print(f'\n[{prec} batch {B}, period {P}] max|dlogit| vs the batch of {P} = {d:.3e} of scale {scale:.1f}')
    assert torch.isfinite(big).all() and d <= EVAL_BAR[prec] * scale
