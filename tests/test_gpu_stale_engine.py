"""-m gpu: state that survives between calls of BiDateNet / BiDateEngine -- the packed filter images, the folded eval BatchNorm tables,
the pooled workspaces and their grown scratch -- against a twin (tests/stale.py): a fresh model with a fresh engine, loaded from the used
model's state right before the probe, must give the same BITS.

Every scenario has one form (run()): a warm model, a perturbation, then the probes on the used model and on its twin.  A third model,
the twin taken BEFORE the perturbation, gives the bits a model that missed the perturbation entirely would produce; mattered() asserts
that they differ, so every scenario can tell stale from fresh.

Shapes are the smallest that walk every path: BiDateNet(3, 2), B in {1, 2, 3}, maps 16x16, 16x32, 32x16, 17x31, 24x40, a 44x40 scene in
16-pixel tiles, two per batch (nine tiles: both lanes and a partial last batch)."""
import copy
import io
import pickle

import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet
from fabric_amd.train_step import TrainStep
from fabric_amd.utils import inference as inf
from oracle import filler
from tests.stale import clone_state, mattered, same_bits, twin

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
PRECS = ['fp32', 'bf16']
ALL_PRECS = ['fp32', 'bf16', 'bf16x3', 'bf16x3-fast']
A = (2, 16, 16)                                                           # the default probe shape (B, H, W)

_CACHE = {}


def _filled(seed=123):
    """One filled state dict per seed for the whole module (building and filling the 13.4 M parameters is the dominant cost)."""
    if ('sd', seed) not in _CACHE:
        _CACHE['sd', seed] = {k: v.clone().to(dev) for k, v in filler.fill_module(BiDateNet(3, 2), seed=seed).state_dict().items()}
    return _CACHE['sd', seed]


def _model(prec, seed=123):
    with torch.device(dev):
        m = BiDateNet(3, 2, precision=prec)
    m.load_state_dict(_filled(seed))
    return m.train()


def _inputs(shape=A, seed=0):
    if ('in', shape, seed) not in _CACHE:
        b, h, w = shape
        x1, x2, _ = filler.make_inputs(b, 3, h, seed=seed, size_w=w)
        g = torch.Generator().manual_seed(1000 + seed)
        _CACHE['in', shape, seed] = (torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev),
                                     torch.randn(b, 2, h, w, generator=g).to(dev))      # the last one: d(loss) / d(logits)
    return _CACHE['in', shape, seed]


def _scene():
    if 'scene' not in _CACHE:
        r = np.random.default_rng(5)
        d1 = r.standard_normal((3, 44, 40)).astype(np.float32)
        d2 = (d1 + 0.5 * r.standard_normal(d1.shape)).astype(np.float32)
        d2[:, 11:22, 13:20] += 2.0
        _CACHE['scene'] = (torch.from_numpy(d1).to(dev), torch.from_numpy(d2).to(dev))
    return _CACHE['scene']


def _twin(m):
    """twin(), with the engine's schedule switch carried over (eval_fused is a setting, not derived state)."""
    t = twin(m)
    if m._engine is not None:
        t.engine().eval_fused = m._engine.eval_fused
    return t


# ------------------------------------------------------------------ probes
def fwd_bwd(m, shape=A, seed=0):
    """A training forward and backward on fixed inputs with input gradients requested: logits, every parameter gradient, both input
    gradients."""
    x1, x2, dl = _inputs(shape, seed)
    a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    m.train()
    m.zero_grad(set_to_none=True)
    out = m(a, b)
    out.backward(dl)
    return {'logits': out.detach().clone(), 'grads': {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
            'dx1': a.grad.clone(), 'dx2': b.grad.clone()}


def probe_train(m, shape=A, seed=0):
    out = fwd_bwd(m, shape, seed)
    out['state'] = clone_state(m)                                         # running statistics and counts included
    return out


def probe_eval(m, shape=A, seed=0):
    x1, x2, _ = _inputs(shape, seed)
    m.eval()
    with torch.no_grad():
        out = m(x1, x2).clone()
    m.train()
    return out


def probe_cmap(m, shape=A, seed=0):
    x1, x2, _ = _inputs(shape, seed)
    m.eval()
    cd, _ = m.engine().forward(x1, x2, inf._eval_params(m), training=False, class_map=True)
    m.train()
    return cd.clone()


def probe_all(m, shape=A, seed=0):
    """Eval logits, class map, then the training probe (which moves the running statistics, so it goes last)."""
    return {'eval': probe_eval(m, shape, seed), 'cmap': probe_cmap(m, shape, seed), 'train': probe_train(m, shape, seed)}


def probe_scene(m):
    s1, s2 = _scene()
    m.eval()
    mask = inf.predict_scene(m, s1, s2, patch_size=16, batch_size=2, two_streams=True)
    proba, bmask = inf.predict_scene_blended(m, s1, s2, patch_size=16, stride=16, batch_size=2, two_streams=True)
    m.train()
    return {'mask': mask.clone(), 'proba': proba.clone(), 'bmask': bmask.clone()}


def run(m, perturb, name, probe=probe_all, keys=None):
    """perturb(m), then probe(m) against probe(twin(m)); the twin taken before perturb() tells what missing it would look like.
    keys: the entries of the probe's result that the perturbation must change (None: any)."""
    base = probe(_twin(m))
    perturb(m)
    tw = _twin(m)
    got, want = probe(m), probe(tw)
    same_bits(got, want, name)
    if keys is None:
        mattered(base, got, name)
    for k in keys or ():
        mattered(base[k], got[k], f'{name} [{k}]')
    return got


def _param(m, key):
    return dict(m.named_parameters())[key]


# ================================================================== packed images
@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('prec', ALL_PRECS)
def test_torch_optimizer_steps_between_forwards(prec, opt):
    """The reference loop with a plain torch.optim and NO invalidate_weights(): the version counters alone must get the images repacked."""
    m = _model(prec)
    o = torch.optim.SGD(m.parameters(), lr=0.05) if opt == 'sgd' else torch.optim.Adam(m.parameters(), lr=0.01)
    probe_all(m)

    def steps(m):
        for it in range(2):
            fwd_bwd(m, seed=it)
            o.step()
    run(m, steps, f'{opt} steps [{prec}]', keys=('eval', 'train'))


CONV_KEYS = ['inc.conv.conv.0.weight', 'up2.conv.conv.0.weight', 'up4.conv.conv.3.weight']
DIRECT_KEYS = ['outc.conv.weight', 'up2.conv.conv.1.weight', 'down1.mpconv.1.conv.0.bias']


@pytest.mark.parametrize('key', CONV_KEYS + DIRECT_KEYS)
@pytest.mark.parametrize('prec', PRECS + ['bf16x3'])
def test_in_place_change_of_one_tensor(prec, key):
    """with torch.no_grad(): p.mul_() on exactly one tensor: a packed conv weight (first, a middle decoder one, the last), or one that the
    kernels read directly (classifier, a BatchNorm gamma, a conv bias -- which only the eval forward and the running mean can see)."""
    m = _model(prec)
    probe_all(m)

    def mul(m):
        with torch.no_grad():
            _param(m, key).mul_(1.5)
    run(m, mul, f'{key} *= 1.5 [{prec}]', keys=('eval',))


@pytest.mark.parametrize('prec', PRECS)
def test_data_repointed(prec):
    """p.data = other_tensor on a packed weight, a BatchNorm gamma and a running variance (a re-assigned buffer)."""
    m = _model(prec)
    probe_all(m)

    def repoint(m):
        for key in ('down2.mpconv.1.conv.3.weight', 'up3.conv.conv.4.weight'):
            p = _param(m, key)
            p.data = p.data * 1.25
        bn = m.down3.mpconv[1].conv[1]
        bn.running_var = bn.running_var * 1.3
    run(m, repoint, f'p.data = t [{prec}]', keys=('eval', 'train'))


@pytest.mark.parametrize('assign', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_load_state_dict_of_other_weights(prec, assign):
    m = _model(prec)
    probe_all(m)
    other = {k: v.clone() for k, v in _filled(seed=7).items()}
    run(m, lambda m: m.load_state_dict(other, assign=assign), f'load_state_dict(assign={assign}) [{prec}]', keys=('eval', 'train'))


@pytest.mark.parametrize('prec', PRECS)
def test_host_round_trip_of_the_module(prec):
    """model.cpu(), one weight changed there, model.cuda(): every tensor lives somewhere else afterwards."""
    m = _model(prec)
    probe_all(m)

    def trip(m):
        m.cpu()
        with torch.no_grad():
            m.up1.conv.conv[0].weight.mul_(0.5)
        m.cuda()
    run(m, trip, f'cpu().cuda() [{prec}]', keys=('eval', 'train'))


@pytest.mark.parametrize('how', ['deepcopy', 'pickle'])
@pytest.mark.parametrize('prec', PRECS)
def test_copies_of_a_warm_model(prec, how):
    """A deepcopy / pickle round trip of a model whose engine is warm carries no engine; the copy follows its own weights, and the
    original is not disturbed by what happens to the copy."""
    m = _model(prec)
    probe_all(m)
    if how == 'deepcopy':
        c = copy.deepcopy(m)
    else:
        buf = io.BytesIO()
        pickle.dump(m, buf)
        c = pickle.loads(buf.getvalue())
    assert c._engine is None and m._engine is not None

    def mul(c):
        with torch.no_grad():
            c.down1.mpconv[1].conv[0].weight.mul_(1.5)
    got_c = run(c, mul, f'{how} [{prec}]', keys=('eval', 'train'))
    tw = _twin(m)
    got_m = probe_all(m)
    same_bits(got_m, probe_all(tw), f'the original after its {how} was used [{prec}]')
    mattered(got_m['eval'], got_c['eval'], f'{how}: copy against original [{prec}]')


@pytest.mark.parametrize('prec', PRECS)
def test_documented_contract_copy_then_invalidate(prec):
    """p.data.copy_() bumps no version counter: the documented contract is to call invalidate_weights() after it, and then the result is
    right.  (Nothing is asserted about the call without it.)"""
    m = _model(prec)
    probe_all(m)

    def copy_(m):
        for key in CONV_KEYS:
            p = _param(m, key)
            p.data.copy_(p.data * 0.75)
        m.engine().invalidate_weights()
    run(m, copy_, f'p.data.copy_() + invalidate_weights() [{prec}]', keys=('eval', 'train'))


@pytest.mark.parametrize('prec', PRECS + ['bf16x3'])
def test_optimizer_step_then_two_lane_scan(prec):
    """optimizer.step() directly followed by predict_scene / predict_scene_blended on two lanes, with no forward in between.  The version
    counters moved but the images are still marked valid; _open_lanes must notice before it forks, or lane 0 repacks on its own stream
    inside its first batch while lane 1, ordered only behind the fork, reads images that are old or being rewritten.  That race depends
    on timing: run once on the code before the fix, this test passed.  The fix (_check_packed before _weights in _open_lanes) rests on
    reading the code, not on this test having failed; there is no repetition loop here on purpose."""
    m = _model(prec)
    o = torch.optim.SGD(m.parameters(), lr=0.05)
    probe_scene(m)                                                        # both lanes and the images are warm
    fwd_bwd(m)
    run(m, lambda m: o.step(), f'step then scan [{prec}]', probe=probe_scene, keys=('proba',))


# ================================================================== eval tables
@pytest.mark.parametrize('path', ['autograd', 'trainstep'])
@pytest.mark.parametrize('prec', PRECS)
def test_eval_after_running_statistics_moved(prec, path):
    """Eval forward, training forwards that move the running statistics (no version counter moves with them), eval forward."""
    m = _model(prec)
    ts = TrainStep(m, lr=0.05) if path == 'trainstep' else None
    probe_eval(m)
    probe_cmap(m)
    lbl = (_inputs()[2][:, 0] > 1.0).to(torch.uint8)

    def train(m):
        for it in range(2):
            if ts is None:
                fwd_bwd(m, seed=it)
            else:
                ts.step(*_inputs(seed=it)[:2], lbl)
    run(m, train, f'eval, train ({path}), eval [{prec}]', probe=lambda m: {'eval': probe_eval(m), 'cmap': probe_cmap(m)}, keys=('eval',))


@pytest.mark.parametrize('prec', PRECS)
def test_eval_after_optimizer_step_on_bn_and_bias(prec):
    """An optimizer step that changes gamma, beta and the conv biases, and nothing else, between two eval forwards."""
    m = _model(prec)
    small = [p for k, p in m.named_parameters() if p.dim() == 1]
    o = torch.optim.SGD(small, lr=0.1)
    x1, x2, dl = _inputs()
    m.eval()
    m.zero_grad(set_to_none=True)
    m(x1, x2).backward(dl)                                                # eval-mode graph: the conv biases have real gradients
    m.train()
    probe_eval(m)
    run(m, lambda m: o.step(), f'eval, step on 1-d tensors, eval [{prec}]', probe=probe_eval)


@pytest.mark.parametrize('prec', ALL_PRECS)
def test_scan_train_scan(prec):
    """predict_scene, one training step, predict_scene on the same scene: the second lane's workspaces were dropped and come back, the
    per-lane table reuse starts over, the images are repacked."""
    m = _model(prec)
    o = torch.optim.SGD(m.parameters(), lr=0.05)
    probe_scene(m)

    def step(m):
        fwd_bwd(m)
        o.step()
    run(m, step, f'scan, step, scan [{prec}]', probe=probe_scene, keys=('proba',))
    assert not [k for k in m.engine()._ws if k[4] == 1]


@pytest.mark.parametrize('prec', PRECS)
def test_eval_schedule_toggled(prec):
    """eng.eval_fused switched between calls: each schedule keeps BatchNorm tables of its own (the engine's folded ones, the
    workspace's), and each must be current when its turn comes."""
    m = _model(prec)
    probe_all(m)
    for fused in (False, True, False):
        def toggle(m):
            fwd_bwd(m, seed=3)                                            # the statistics move while the other schedule's tables rest
            m.engine().eval_fused = fused
        run(m, toggle, f'eval_fused={fused} [{prec}]', probe=lambda m: {'eval': probe_eval(m), 'cmap': probe_cmap(m), 'scene': probe_scene(m)},
            keys=('eval',))


@pytest.mark.parametrize('prec', PRECS)
def test_running_statistics_overwritten_in_place(prec):
    m = _model(prec)
    probe_all(m)

    def overwrite(m):
        for bn in (m.inc.conv.conv[1], m.up4.conv.conv[4], m.down4.mpconv[1].conv[1]):
            bn.running_mean.copy_(bn.running_mean * 0.5 + 0.05)
            bn.running_var.copy_(bn.running_var * 1.5)
    run(m, overwrite, f'running_mean.copy_() [{prec}]', probe=lambda m: {'eval': probe_eval(m), 'scene': probe_scene(m), 'train': probe_train(m)},
        keys=('eval', 'scene'))


# ================================================================== workspaces and scratch
SHAPE_PAIRS = [((2, 16, 16), (2, 24, 40)), ((2, 24, 40), (2, 16, 16)), ((2, 17, 31), (2, 16, 16)), ((1, 16, 16), (2, 17, 31)),
               ((2, 16, 32), (2, 32, 16)), ((2, 32, 16), (2, 16, 32))]


@pytest.mark.parametrize('a,b', SHAPE_PAIRS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('prec', ALL_PRECS)
def test_shape_a_then_b_then_a(prec, a, b):
    """Shape A, then B, then the probes on A: scratch only ever grows and sizes are cached per call signature, so A's launches must
    not pick up anything B left (16x32 against 32x16: the same element count in another shape)."""
    m = _model(prec)
    probe_all(m, a)
    run(m, lambda m: probe_all(m, b, seed=1), f'{a}, {b}, {a} [{prec}]', probe=lambda m: probe_all(m, a), keys=('eval',))


@pytest.mark.parametrize('prec', ALL_PRECS)
def test_batch_3_then_1_then_3(prec):
    m = _model(prec)
    three, one = (3, 16, 16), (1, 16, 16)
    probe_all(m, three)
    run(m, lambda m: probe_all(m, one, seed=1), f'B=3, 1, 3 [{prec}]', probe=lambda m: probe_all(m, three), keys=('eval',))


def _graph(m, shape=A, seed=0):
    x1, x2, dl = _inputs(shape, seed)
    a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    m.train()
    return m(a, b), (a, b, *m.parameters()), dl


def _grads(out, leaves, dl, **kw):
    return {'logits': out.detach().clone(), 'g': [g.clone() for g in torch.autograd.grad(out, leaves, dl, **kw)]}


@pytest.mark.parametrize('prec', ALL_PRECS)
def test_other_forwards_between_forward_and_backward(prec):
    """A training forward of shape B, and a no_grad and an eval forward of shape A (on other inputs), between the forward and the backward
    of a shape-A graph: the graph leases its workspace, the visitors get their own.  The twin runs the graph alone."""
    m = _model(prec)
    probe_all(m)
    tw = _twin(m)
    out, leaves, dl = _graph(m)
    fwd_bwd(m, (2, 24, 40), seed=1)
    with torch.no_grad():
        visitor = m(*_inputs(seed=2)[:2]).clone()
    visitor_eval = probe_eval(m, seed=2)
    got = _grads(out, leaves, dl)
    want = _grads(*_graph(tw))
    same_bits(got, want, f'visited graph [{prec}]')
    mattered(got['logits'], visitor, f'the no_grad visitor wrote other activations [{prec}]')
    mattered(visitor, visitor_eval, f'the eval visitor wrote other activations [{prec}]')


@pytest.mark.parametrize('prec', ALL_PRECS)
def test_two_live_graphs_backward_in_reverse_order(prec):
    """Two live training graphs of one shape, the backwards taken in the opposite order to the forwards: each equals its own twin, which
    ran forward and backward one after the other."""
    m = _model(prec)
    probe_all(m)
    tw = _twin(m)
    g1, g2 = _graph(m, seed=0), _graph(m, seed=1)
    got2 = _grads(*g2)
    got1 = _grads(*g1)
    want1 = _grads(*_graph(tw, seed=0))
    want2 = _grads(*_graph(tw, seed=1))
    same_bits(got1, want1, f'first graph, second backward [{prec}]')
    same_bits(got2, want2, f'second graph, first backward [{prec}]')
    mattered(got1, got2, f'the two graphs [{prec}]')


@pytest.mark.parametrize('prec', ALL_PRECS)
def test_second_backward_through_a_retained_graph(prec):
    """retain_graph=True: a backward on another output gradient in between, then the first one again: the first one's bits."""
    m = _model(prec)
    out, leaves, dl = _graph(m)
    first = _grads(out, leaves, dl, retain_graph=True)
    other = _grads(out, leaves, dl.flip(0) * 2.0, retain_graph=True)
    again = _grads(out, leaves, dl)
    same_bits(again, first, f'second backward [{prec}]')
    mattered(first['g'], other['g'], f'the backward in between [{prec}]')


@pytest.mark.parametrize('prec', ALL_PRECS)
def test_eval_mode_backward_then_training(prec):
    """An eval-mode backward (input gradients: the forward is recomputed in the training layout on the running statistics, and in bf16x3
    its split operands are dropped afterwards), then a training forward and backward on the same workspace."""
    m = _model(prec)
    probe_all(m)
    tw = _twin(m)

    def eval_backward(m):
        x1, x2, dl = _inputs(seed=4)
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        m.eval()
        out = m(a, b)
        g = torch.autograd.grad(out, (a, b, *m.parameters()), dl)
        m.train()
        return {'logits': out.detach().clone(), 'g': [t.clone() for t in g]}
    got_e = eval_backward(m)
    tw2 = _twin(m)
    got_t = probe_all(m)
    same_bits(got_e, eval_backward(tw), f'eval-mode backward [{prec}]')
    same_bits(got_t, probe_all(tw2), f'training after an eval-mode backward [{prec}]')
    mattered(got_e['logits'], got_t['train']['logits'], f'eval-mode against training forward [{prec}]')


@pytest.mark.parametrize('prec', ['bf16x3', 'bf16x3-fast'])
def test_split_buffers_dropped_and_regrown(prec):
    """model.eval() then model.train() in bf16x3 drops the per-layer split operands; the next training step regrows them."""
    m = _model(prec)
    o = torch.optim.SGD(m.parameters(), lr=0.05)
    fwd_bwd(m)
    assert m.engine()._ws[(2, 16, 16, str(dev), 0)][0]._split

    def drop(m):
        o.step()
        m.eval()
        assert not m.engine()._ws[(2, 16, 16, str(dev), 0)][0]._split
        m.train()
    run(m, drop, f'eval(), train() [{prec}]', probe=probe_train, keys=('logits',))


@pytest.mark.parametrize('prec,other', [('bf16', 'fp32'), ('fp32', 'bf16x3'), ('bf16x3', 'bf16')])
def test_precision_changed_and_back(prec, other):
    """model.precision set to another setting and back: each setting gets an engine of its own, nothing of the old one is used."""
    m = _model(prec)
    probe_all(m)

    def there_and_back(m):
        m.precision = other
        tw = _twin(m)
        same_bits(probe_all(m, seed=1), probe_all(tw, seed=1), f'{prec} -> {other}')
        m.precision = prec
    run(m, there_and_back, f'{prec} -> {other} -> {prec}', keys=('eval',))
