"""CPU tests of the input-gradient and frozen-BatchNorm entry points: every argument check fails with the library's message before
anything is launched (no GPU needed)."""
import pytest

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X3, BDN_F32


def _fails(match, name, *args):
    with pytest.raises(RuntimeError, match=match):
        _lib.call(name, *args)


def test_dgrad_first_rejects_bad_arguments():
    f = 'bdn_conv3x3_dgrad_first'
    # dtype, dA, ldA, z, bn, sums, ipg, w, Cin_real, dx1, dx2, B, H, W, stream
    _fails('null pointer', f, BDN_BF16, None, 64, None, None, None, 1, 1, 3, 1, 1, 1, 8, 8, None)
    _fails('null pointer', f, BDN_BF16, 1, 64, None, None, None, 1, None, 3, 1, 1, 1, 8, 8, None)
    _fails('null pointer', f, BDN_BF16, 1, 64, None, None, None, 1, 1, 3, None, 1, 1, 8, 8, None)
    _fails('null pointer', f, BDN_F32, 1, 64, 1, None, 1, 1, 1, 3, 1, 1, 1, 8, 8, None)         # z without a table
    _fails('bad dtype', f, BDN_BF16X3, 1, 64, None, None, None, 1, 1, 3, 1, 1, 1, 8, 8, None)
    _fails('bad shape', f, BDN_BF16, 1, 64, None, None, None, 1, 1, 17, 1, 1, 1, 8, 8, None)    # more than 16 input channels
    _fails('bad shape', f, BDN_BF16, 1, 64, None, None, None, 1, 1, 0, 1, 1, 1, 8, 8, None)
    _fails('bad shape', f, BDN_BF16, 1, 60, None, None, None, 1, 1, 3, 1, 1, 1, 8, 8, None)     # ldA < 64
    _fails('bad shape', f, BDN_BF16, 1, 68, None, None, None, 1, 1, 3, 1, 1, 1, 8, 8, None)     # ldA not a whole 16-byte unit
    _fails('bad shape', f, BDN_F32, 1, 64, None, None, None, 1, 1, 3, 1, 1, 0, 8, 8, None)      # B = 0
    _fails('bad shape', f, BDN_F32, 1, 64, None, None, None, 1, 1, 3, 1, 1, 2, 0, 8, None)
    _fails('must divide', f, BDN_F32, 1, 64, 1, 1, 1, 3, 1, 3, 1, 1, 2, 8, 8, None)           # 3 images per group of 2B = 4


def test_frozen_batchnorm_backward_rejects_bad_arguments():
    f = 'bdn_bn_bwd_finalize_frozen'
    # bn, G, C, partial, rows, raw, sums, dgamma, dbeta, dbias, scratch, stream
    _fails('null pointer', f, None, 2, 64, 1, 4, 1, 1, 1, 1, 1, 1, None)
    _fails('null pointer', f, 1, 2, 64, 1, 4, 1, 1, 1, None, 1, 1, None)                 # dbias is scale * dbeta: dbeta is needed
    _fails('bad shape', f, 1, 2, 60, 1, 4, 1, 1, 1, 1, 1, 1, None)
    _fails('bad shape', f, 1, 0, 64, 1, 4, 1, 1, 1, 1, 1, 1, None)
    _fails('bad shape', f, 1, 2, 64, 1, 0, 1, 1, 1, 1, 1, 1, None)
    f = 'bdn_bn_bwd_apply_frozen'
    # dtype, dA, ldA, z, bn, ipg, N, H, W, C, partial, rows, raw, sums, dgamma, dbeta, dbias, dz, scratch, stream
    ok = [BDN_BF16, 1, 64, 1, 1, 2, 4, 8, 8, 64, 1, 4, 1, 1, 1, 1, 1, 1, 1, None]
    _fails('null pointer', f, *ok[:1], None, *ok[2:])
    _fails('null pointer', f, *ok[:17], None, *ok[18:])
    _fails('bad shape', f, *ok[:5], 3, *ok[6:])                                            # 4 images, 3 per group
    _fails('bad shape', f, *ok[:2], 32, *ok[3:])                                           # ldA < C
    _fails('must divide', f, *ok[:9], 48, *ok[10:])
    _fails('bad dtype', f, 7, *ok[1:])
    f = 'bdn_bn_bwd_frozen'
    # dtype, dA, ldA, z, bn, ipg, N, H, W, C, ws, sums, dgamma, dbeta, dbias, dz, stream
    ok = [BDN_F32, 1, 64, 1, 1, 2, 4, 8, 8, 64, 1, 1, 1, 1, 1, 1, None]
    _fails('null pointer', f, *ok[:3], None, *ok[4:])
    _fails('null pointer', f, *ok[:10], None, *ok[11:])
    _fails('bad shape', f, *ok[:6], 0, *ok[7:])
    _fails('must divide', f, *ok[:9], 48, *ok[10:])
    _fails('bad dtype', f, BDN_BF16X3, *ok[1:])


def test_input_gradient_is_refused_at_the_door_above_16_bands():
    """bdn_conv3x3_dgrad_first takes at most 16 input channels, and backward() reaches it only after the whole chain is enqueued: the
    engine refuses dx before anything else (no workspace, no device tensor is touched: meta tensors and ws = None do), and the
    autograd route refuses when an image requires grad, before the forward.  16 bands pass the check."""
    import torch
    from fabric_amd import BiDateNet
    from fabric_amd.engine import INPUT_GRAD_MAX_BANDS, BiDateEngine
    assert INPUT_GRAD_MAX_BANDS == 16
    for c in (1, 13, 16):
        BiDateEngine(c, 2).check_input_grad()
    dx = (torch.empty(2, 17, 32, 32, device='meta'), torch.empty(2, 17, 32, 32, device='meta'))
    for c in (17, 32, 64):
        for prec in ('bf16', 'fp32', 'bf16x3', 'bf16x3-fast'):
            eng = BiDateEngine(c, 2, prec)
            with pytest.raises(ValueError, match=r'limited to 16 bands.*bdn_conv3x3_dgrad_first.*' + f'this model has {c}'):
                eng.backward(None, torch.empty(2, 2, 32, 32, device='meta'), {}, {}, dx=dx)
    # the module: an image that requires grad is refused before the forward (a CPU tensor would otherwise meet "no CPU path")
    x = torch.zeros(1, 17, 16, 16)
    with pytest.raises(ValueError, match='bdn_conv3x3_dgrad_first'):
        BiDateNet(17, 2)(x.clone().requires_grad_(True), x)
    with pytest.raises(ValueError, match='bdn_conv3x3_dgrad_first'):
        BiDateNet(17, 2).eval()(x, x.clone().requires_grad_(True))
    x = torch.zeros(1, 16, 16, 16)
    with pytest.raises(RuntimeError, match='no CPU path'):            # 16 bands: past the check, up to the device check
        BiDateNet(16, 2)(x.clone().requires_grad_(True), x)
    with pytest.raises(RuntimeError, match='no CPU path'):            # 17 bands without an input gradient: not refused for the width
        BiDateNet(17, 2)(torch.zeros(1, 17, 16, 16), torch.zeros(1, 17, 16, 16))
