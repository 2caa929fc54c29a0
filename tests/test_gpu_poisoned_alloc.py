"""-m gpu: every internal buffer of the library comes from torch.empty, and the allocator often hands out memory that happens to hold
zeros or the previous call's (right) values.  Here each workload runs twice from the same inputs and state: plainly, and with a new
model / engine / TrainStep / conv3d object built under poisoned_allocations() (tests/stale.py), where every floating-point buffer is
born as NaN.  The results must be finite and the same bits: a difference is a kernel or a schedule reading memory nobody wrote -- a pad
band 13 -> 16 multiplied by a zero weight, a statistics row past the tile plan, a halo.

BiDateNet(3, 2) and BiDateNet(13, 2) (pad channels 13..15 exist), B = 2 at 16 x 16 and B = 3 at 17 x 31, all four precisions."""
import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet
from fabric_amd.conv3d import DoubleConv3d, to_ndhwc
from fabric_amd.train_step import TrainStep
from fabric_amd.utils import inference as inf
from oracle import filler
from tests.stale import all_finite, clone_state, poisoned_allocations, same_bits

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
ALL_PRECS = ['fp32', 'bf16', 'bf16x3', 'bf16x3-fast']
SHAPES = [(2, 16, 16), (3, 17, 31)]
BANDS = [3, 13]
grid = lambda f: pytest.mark.parametrize('prec', ALL_PRECS)(pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))(   # noqa: E731
    pytest.mark.parametrize('bands', BANDS)(f)))
_CACHE = {}


def _filled(bands):
    if ('sd', bands) not in _CACHE:
        _CACHE['sd', bands] = {k: v.clone().to(dev) for k, v in filler.fill_module(BiDateNet(bands, 2)).state_dict().items()}
    return _CACHE['sd', bands]


def _model(prec, bands):
    with torch.device(dev):
        m = BiDateNet(bands, 2, precision=prec)
    m.load_state_dict(_filled(bands))
    return m.train()


def _inputs(bands, shape, seed=0):
    key = ('in', bands, shape, seed)
    if key not in _CACHE:
        b, h, w = shape
        x1, x2, lbl = (torch.from_numpy(v).to(dev) for v in filler.make_inputs(b, bands, h, seed=seed, size_w=w))
        dl = torch.randn(b, 2, h, w, generator=torch.Generator().manual_seed(seed + 50)).to(dev)
        _CACHE[key] = (x1, x2, lbl, dl)
    return _CACHE[key]


def twice(work, name):
    """work() plainly, then under poisoned allocations: finite, and the same bits."""
    plain = work()
    torch.cuda.synchronize()
    with poisoned_allocations():
        probe = torch.empty(4, device=dev)
        assert bool(torch.isnan(probe).all()), 'the poison is not active'
        poisoned = work()
        torch.cuda.synchronize()
    assert torch.empty.__name__ == 'empty'
    all_finite(plain, f'{name} (plain)')
    all_finite(poisoned, f'{name} (poisoned)')
    same_bits(poisoned, plain, name)
    return plain


@grid
def test_training_forward_backward(prec, shape, bands):
    x1, x2, _, dl = _inputs(bands, shape)

    def work():
        m = _model(prec, bands)
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        out = m(a, b)
        out.backward(dl)
        return {'logits': out.detach(), 'grads': {k: p.grad for k, p in m.named_parameters()}, 'dx1': a.grad, 'dx2': b.grad,
                'state': clone_state(m)}
    twice(work, f'training forward + backward [{prec}, {shape}, {bands} bands]')


@grid
def test_eval_forwards_and_eval_backward(prec, shape, bands):
    """Eval forward on both schedules, class_map on both, and an eval-mode backward."""
    x1, x2, _, dl = _inputs(bands, shape)

    def work():
        m = _model(prec, bands).eval()
        out = {}
        for fused in (True, False):
            m.engine().eval_fused = fused
            with torch.no_grad():
                out['logits', fused] = m(x1, x2).clone()
            out['cmap', fused] = m.engine().forward(x1, x2, inf._eval_params(m), training=False, class_map=True)[0].clone()
        m.engine().eval_fused = True
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        y = m(a, b)
        y.backward(dl)
        out.update(logits_graph=y.detach(), dx1=a.grad, dx2=b.grad, grads={k: p.grad for k, p in m.named_parameters()})
        return {str(k): v for k, v in out.items()}
    twice(work, f'eval forwards + eval-mode backward [{prec}, {shape}, {bands} bands]')


STEP_CONFIGS = {
    'sgd': lambda m: dict(lr=0.05),
    'adam-groups-frozen': lambda m: dict(lr=5e-3, optimizer='adam', param_groups=[
        {'params': [k for k, p in m.named_parameters() if p.dim() > 1 and not k.startswith('down3.')]},
        {'params': [k for k, p in m.named_parameters() if p.dim() == 1 and not k.startswith('down3.')], 'lr': 1e-3}]),
    'accumulate3-clip': lambda m: dict(lr=0.05, momentum=0.9, accumulate=3, max_grad_norm=1.0),
    'ema-buffers': lambda m: dict(lr=5e-3, optimizer='adamw', ema_decay=0.9, ema_buffers=True),
}


@pytest.mark.parametrize('config', list(STEP_CONFIGS))
@grid
def test_train_step_three_calls(prec, shape, bands, config):
    batches = [_inputs(bands, shape, seed)[:3] for seed in range(3)]

    def work():
        m = _model(prec, bands)
        if config == 'adam-groups-frozen':
            for k, p in m.named_parameters():
                p.requires_grad_(not k.startswith('down3.'))
        ts = TrainStep(m, **STEP_CONFIGS[config](m))
        losses = [ts.step(*b) for b in batches]
        torch.cuda.synchronize()
        return {'losses': losses, 'logits': ts.last_logits, 'counts': ts.last_counts, 'norm': ts.last_grad_norm, 'params': ts.flat_params,
                'grads': ts.flat_grads, 'opt': dict(ts.opt_state), 'avg': ts.flat_avg, 'avg_buffers': dict(ts.avg_buffers),
                'state': clone_state(m)}
    twice(work, f'TrainStep x3, {config} [{prec}, {shape}, {bands} bands]')


@pytest.mark.parametrize('bands', BANDS)
@pytest.mark.parametrize('prec', ALL_PRECS)
def test_scene_scans(prec, bands):
    """predict_scene with one lane and with two, predict_scene_blended under symmetries (0, 3): a 44 x 40 scene in 16-pixel tiles, two per
    batch (nine tiles: a partial last batch)."""
    r = np.random.default_rng(5)
    d1 = r.standard_normal((bands, 44, 40)).astype(np.float32)
    d2 = (d1 + 0.5 * r.standard_normal(d1.shape)).astype(np.float32)
    s1, s2 = torch.from_numpy(d1).to(dev), torch.from_numpy(d2).to(dev)

    def work():
        m = _model(prec, bands).eval()
        one = inf.predict_scene(m, s1, s2, patch_size=16, batch_size=2, two_streams=False)
        two = inf.predict_scene(m, s1, s2, patch_size=16, batch_size=2, two_streams=True)
        proba, mask = inf.predict_scene_blended(m, s1, s2, patch_size=16, stride=8, symmetries=(0, 3), batch_size=2, two_streams=True)
        return {'one': one, 'two': two, 'proba': proba, 'mask': mask}
    out = twice(work, f'scene scans [{prec}, {bands} bands]')
    same_bits(out['two'], out['one'], 'two lanes against one')


@pytest.mark.parametrize('shape', [(1, 3, 11, 24, 13, 64), (2, 2, 16, 16, 64, 64)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('prec', ['fp32', 'bf16', 'bf16x3'])
def test_double_conv3d(prec, shape):
    N, D, H, W, Cin, Cout = shape
    td = torch.bfloat16 if prec == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(3)
    state = {'conv.0.weight': torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (2.0 / (27 * Cin)) ** 0.5,
             'conv.3.weight': torch.randn(Cout, Cout, 3, 3, 3, generator=g) * (2.0 / (27 * Cout)) ** 0.5}
    for k in ('0', '3'):
        state[f'conv.{k}.bias'] = torch.rand(Cout, generator=g) * 0.2 - 0.1
    for k in ('1', '4'):
        state[f'conv.{k}.weight'] = torch.rand(Cout, generator=g) + 0.5
        state[f'conv.{k}.bias'] = torch.rand(Cout, generator=g) * 0.6 - 0.3
    x = torch.randn(N, Cin, D, H, W, generator=g).to(dev)
    dy = torch.randn(N, Cout, D, H, W, generator=g).to(dev)
    cp = (Cin + 15) // 16 * 16
    xd, dyd = to_ndhwc(x, cp, td), to_ndhwc(dy, Cout, td)

    def work():
        blk = DoubleConv3d(Cin, Cout, precision=prec)
        blk.load(state)
        out = blk.forward(xd)
        dx, grads = blk.backward(dyd)
        return {'out': out, 'dx': dx, 'grads': grads, 'P': {k: v.clone() for k, v in blk.P.items()}}
    twice(work, f'DoubleConv3d [{prec}, {shape}]')
