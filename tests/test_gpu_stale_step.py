"""-m gpu: state that survives between calls of the fused TrainStep -- the flat parameter / gradient / optimizer / average buffers, the
detached aliases, the descriptor tables with raw device addresses, the pending accumulation -- against twin_step() (tests/stale.py): a
new TrainStep on a fresh model, built with the same arguments and given the used step's exported state, must produce the same BITS
over K further step() calls on fixed batches.

Form of every scenario (run()): a step that has stepped, a perturbation, then the probe on the used step and on its twin; the twin taken
before the perturbation gives the bits of a step that missed it, and mattered() asserts they differ."""
import pytest
import torch

from fabric_amd import BiDateNet
from fabric_amd.criterion import Criterion
from fabric_amd.train_step import TrainStep
from fabric_amd.utils import inference as inf
from oracle import filler
from tests.stale import clone_state, mattered, same_bits, twin, twin_step

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
PRECS = ['fp32', 'bf16']
A = (2, 16, 16)
K = 4
_CACHE = {}


def _filled(seed=123):
    if ('sd', seed) not in _CACHE:
        _CACHE['sd', seed] = {k: v.clone().to(dev) for k, v in filler.fill_module(BiDateNet(3, 2), seed=seed).state_dict().items()}
    return _CACHE['sd', seed]


def _model(prec, seed=123):
    with torch.device(dev):
        m = BiDateNet(3, 2, precision=prec)
    m.load_state_dict(_filled(seed))
    return m.train()


def _batch(seed=0, shape=A, ignore=False):
    """(x1, x2, labels) of filler.make_inputs; ignore: a block and a sprinkle of pixels carry the ignore label 255."""
    key = ('b', seed, shape, ignore)
    if key not in _CACHE:
        b, h, w = shape
        x1, x2, lbl = (torch.from_numpy(v) for v in filler.make_inputs(b, 3, h, seed=seed, size_w=w))
        if ignore:
            lbl[:, :3, :5] = 255
            lbl[torch.rand(lbl.shape, generator=torch.Generator().manual_seed(seed)) < 0.1] = 255
        _CACHE[key] = (x1.to(dev), x2.to(dev), lbl.to(dev))
    return _CACHE[key]


def snapshot(ts, losses=()):
    """Everything a step leaves behind, cloned.  opt_step is the update count for Adam / AdamW; torch.optim.SGD's state carries no
    count, so a momentum-SGD step that loaded a state resumes at 1 by design (fabric_amd.optim.torch_to_flat) -- the kernels only ever
    read `opt_step == 0`, and that is what is compared there."""
    torch.cuda.synchronize()
    opt_step = ts.opt_step if ts.optim.family == 'adam' else min(ts.opt_step, 1)
    c = lambda t: None if t is None else t.detach().clone()               # noqa: E731
    return {'losses': [c(v) for v in losses], 'last_logits': c(ts.last_logits), 'last_counts': c(ts.last_counts),
            'last_dlogits': c(ts.last_dlogits), 'last_grad_norm': c(ts.last_grad_norm), 'last_clip_coef': c(ts.last_clip_coef),
            'flat_params': c(ts.flat_params), 'flat_grads': c(ts.flat_grads), 'opt_state': {k: c(v) for k, v in ts.opt_state.items()},
            'opt_step': opt_step, 'flat_avg': c(ts.flat_avg), 'avg_buffers': {k: c(v) for k, v in ts.avg_buffers.items()},
            'n_averaged': ts.n_averaged, 'micro': ts.micro, 'state': clone_state(ts.model)}


def probe(ts, k=K, ignore=False, shape=A, first=10):
    """k further step() calls on fixed batches."""
    return snapshot(ts, [ts.step(*_batch(first + i, shape, ignore)) for i in range(k)])


def run(ts, perturb, name, neutral=False, **kw):
    """neutral: the perturbation is one that must NOT reach the exported state (the scenario then shows with a mattered() of its own
    what it did change)."""
    base = None if neutral else probe(twin_step(ts), **kw)
    perturb(ts)
    tw = twin_step(ts)
    got, want = probe(ts, **kw), probe(tw, **kw)
    same_bits(got, want, name)
    if not neutral:
        mattered(base, got, name)
    return got


def _warm(ts, n=2, **kw):
    for i in range(n):
        ts.step(*_batch(i, **kw))
    return ts


# ------------------------------------------------------------------ everything at once
def _everything(prec, bn, state=None):
    m = _model(prec)
    if state is not None:
        m.load_state_dict(state)
    for k, p in m.named_parameters():
        p.requires_grad_(not k.startswith('down4.'))                     # one frozen block
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    groups = [{'params': [k for k, p in named if p.dim() > 1], 'weight_decay': 1e-2},
              {'params': [k for k, p in named if p.dim() == 1], 'lr': 2e-3, 'weight_decay': 0.0}]
    return TrainStep(m, lr=5e-3, optimizer='adamw', param_groups=groups, max_grad_norm=1.0, accumulate=2, ema_decay=0.9, ema_every=2,
                     criterion=Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255), bn=bn)


@pytest.mark.parametrize('bn', ['batch', 'frozen'])
@pytest.mark.parametrize('prec', PRECS)
def test_everything_at_once_resumes_from_disk(prec, bn, tmp_path):
    """AdamW, two groups, a frozen block, clipping, accumulate=2, EMA every second update, an ignore label -- in ONE step object.  After
    four micro-steps (two updates, one averaging update: a cadence boundary) the three state dicts go through torch.save / torch.load
    into a newly built model and step; eight more micro-steps on both must agree in every quantity, bit for bit."""
    ts = _everything(prec, bn)
    first = probe(ts, 4, ignore=True, first=0)
    assert ts.opt_step == 2 and ts.n_averaged == 1 and ts.micro == 0
    torch.save(ts.model.state_dict(), tmp_path / 'model.pt')
    torch.save(ts.optimizer_state_dict(), tmp_path / 'optim.pt')
    torch.save(ts.ema_state_dict(), tmp_path / 'ema.pt')
    load = lambda f: torch.load(tmp_path / f, map_location=dev, weights_only=False)      # noqa: E731
    rs = _everything(prec, bn, state=load('model.pt'))
    rs.load_optimizer_state_dict(load('optim.pt'))
    rs.load_ema_state_dict(load('ema.pt'))
    got, want = probe(ts, 8, ignore=True), probe(rs, 8, ignore=True)
    assert got['opt_step'] == 6 and got['n_averaged'] == 3 and 0.0 < float(got['last_grad_norm']) < float('inf')
    same_bits(got, want, f'resumed from disk [{prec}, bn={bn}]')
    for k in ('flat_params', 'flat_avg', 'opt_state', 'last_logits'):
        mattered(first[k], got[k], f'{k} over the eight micro-steps [{prec}, bn={bn}]')


# ------------------------------------------------------------------ groups and tables
@pytest.mark.parametrize('prec', PRECS)
def test_block_frozen_and_released_between_steps(prec):
    """set_param_groups() freezing and later releasing a block, with clipping and averaging on: the segment table, `need`, the zeroed
    optimizer state and the average of the frozen tensors are all re-derived."""
    m = _model(prec)
    ts = _warm(TrainStep(m, lr=5e-3, optimizer='adam', max_grad_norm=1.0, ema_decay=0.9))

    def freeze(ts, on=True):
        for k, p in ts.model.named_parameters():
            if k.startswith('up1.'):
                p.requires_grad_(not on)
        ts.set_param_groups(None)
        ts.step(*_batch(5))
    got = run(ts, freeze, f'freeze up1 [{prec}]')
    assert ts._groups is not None and ts._need is not None
    run(ts, lambda ts: freeze(ts, False), f'release up1 [{prec}]')
    assert ts._groups is None


@pytest.mark.parametrize('prec', PRECS)
def test_back_to_ungrouped_then_clipped_update(prec):
    """set_param_groups(None) from explicit groups back to the ungrouped kernels, then a clipped update: the implicit one-group table of
    the clipped update is built late here, at the twin in its constructor."""
    m = _model(prec)
    named = list(m.named_parameters())
    groups = [{'params': [k for k, p in named if p.dim() > 1]}, {'params': [k for k, p in named if p.dim() == 1], 'lr': 0.01}]
    ts = _warm(TrainStep(m, lr=0.05, momentum=0.9, param_groups=groups, max_grad_norm=0.5))
    assert ts._clip_table is None

    def ungroup(ts):
        ts.set_param_groups(None)
        ts.step(*_batch(5))
    run(ts, ungroup, f'set_param_groups(None) [{prec}]')
    assert ts._groups is None and ts._clip_table is not None


@pytest.mark.parametrize('prec', PRECS)
def test_learning_rates_reassigned(prec):
    """ts.lr and ts.param_groups[i]['lr'] reassigned between steps: twin_step builds the twin with the new values."""
    m = _model(prec)
    ts = _warm(TrainStep(m, lr=0.05, momentum=0.9))

    def new_lr(ts):
        ts.lr = 0.2
    run(ts, new_lr, f'ts.lr [{prec}]')
    m = _model(prec)
    named = list(m.named_parameters())
    groups = [{'params': [k for k, p in named if p.dim() > 1]}, {'params': [k for k, p in named if p.dim() == 1], 'lr': 0.01}]
    ts = _warm(TrainStep(m, lr=0.05, optimizer='adam', param_groups=groups))

    def new_group_lr(ts):
        ts.param_groups[0]['lr'] = 0.005
        ts.param_groups[1]['lr'] = 0.1
    run(ts, new_group_lr, f"param_groups[i]['lr'] [{prec}]")


# ------------------------------------------------------------------ averaged weights
def _eval_logits(m):
    x1, x2, _ = _batch(3)
    m.eval()
    with torch.no_grad():
        out = m(x1, x2).clone()
    m.train()
    return out


@pytest.mark.parametrize('raises', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_ema_weights_entered_and_left(prec, raises):
    """Inside `with ts.ema_weights()` an eval forward equals that of a fresh model loaded from ema_state_dict(); after the block -- also
    when its body raises -- the steps equal the twin's."""
    ts = _warm(TrainStep(_model(prec), lr=5e-3, optimizer='adamw', ema_decay=0.5), 3)
    ema = {k[len('module.'):]: v for k, v in ts.ema_state_dict().items() if k.startswith('module.')}
    fresh = _model(prec)
    fresh.load_state_dict(ema)
    live = _eval_logits(ts.model)
    seen = {}

    def swap(ts):
        try:
            with ts.ema_weights():
                seen['inside'] = _eval_logits(ts.model)
                if raises:
                    raise KeyError('body')
        except KeyError:
            assert raises
        ts.step(*_batch(5))
    run(ts, swap, f'ema_weights(raises={raises}) [{prec}]')
    same_bits(seen['inside'], _eval_logits(fresh), f'eval inside ema_weights() [{prec}]')
    mattered(live, seen['inside'], f'averaged against live weights [{prec}]')


@pytest.mark.parametrize('prec', PRECS)
def test_own_state_reloaded_mid_run(prec):
    """load_optimizer_state_dict / load_ema_state_dict of the step's own output replace the storage; the steps go on unchanged."""
    ts = _warm(TrainStep(_model(prec), lr=5e-3, optimizer='adam', ema_decay=0.9, max_grad_norm=1.0), 3)

    def reload(ts):
        ts.step(*_batch(5))
        old = [t.data_ptr() for t in ts.opt_state.values()]
        ts.load_optimizer_state_dict(ts.optimizer_state_dict())
        ts.load_ema_state_dict(ts.ema_state_dict())
        assert old != [t.data_ptr() for t in ts.opt_state.values()]
    run(ts, reload, f'own state reloaded [{prec}]')


# ------------------------------------------------------------------ accumulation
@pytest.mark.parametrize('apply', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_flush_then_steps(prec, apply):
    """flush(apply=False) drops one pending micro-step (its forward still moved the running statistics); flush() applies it alone."""
    ts = _warm(TrainStep(_model(prec), lr=5e-3, optimizer='adam', accumulate=2, max_grad_norm=1.0), 2)

    def flush(ts):
        ts.step(*_batch(5))
        assert ts.micro == 1 and ts.flush(apply=apply) is apply and ts.micro == 0
    got = run(ts, flush, f'flush(apply={apply}) [{prec}]')
    assert got['opt_step'] == (4 if apply else 3)


@pytest.mark.parametrize('accumulate', [1, 2])
@pytest.mark.parametrize('prec', PRECS)
def test_other_batch_size_and_shape_between_steps(prec, accumulate):
    """B = 4, then 2, another map shape, and back.  accumulate=2: the two micro-steps of one update run at different batch sizes; the twin
    is built before them and replays just those two."""
    big = (4, 16, 16)
    ts = _warm(TrainStep(_model(prec), lr=0.05, momentum=0.9, accumulate=accumulate), 2, shape=big)
    tw = twin_step(ts)
    before = snapshot(ts)
    seq = [(5, big), (6, A)] if accumulate == 2 else [(5, A), (6, (2, 24, 40)), (7, big)]
    for s in (ts, tw):
        for seed, shape in seq:
            s.step(*_batch(seed, shape))
    got = snapshot(ts)
    same_bits(got, snapshot(tw), f'mixed shapes, accumulate={accumulate} [{prec}]')
    mattered(before['flat_params'], got['flat_params'], f'mixed shapes [{prec}]')
    tw2 = twin_step(ts)                                                   # and on from there, against a twin that never saw another shape
    same_bits(probe(ts, shape=big), probe(tw2, shape=big), f'back at B=4, accumulate={accumulate} [{prec}]')


@pytest.mark.parametrize('prec', PRECS + ['bf16x3'])
def test_inference_between_two_micro_steps(prec):
    """An eval forward, a class_map forward and a two-lane predict_scene between the two micro-steps of accumulate=2: the packed images
    are claimed to stay valid there (no update ran), and the visitors must leave the step's workspace and pending sum alone.  The twin is
    built before the first micro-step and replays the two."""
    ts = _warm(TrainStep(_model(prec), lr=0.05, momentum=0.9, accumulate=2), 2)
    tw = twin_step(ts)
    m = ts.model
    ts.step(*_batch(5))
    x1, x2, _ = _batch(3)
    m.eval()
    P = inf._eval_params(m)
    with torch.no_grad():
        mid = m(x1, x2).clone()
    cd, _ = m.engine().forward(x1, x2, P, training=False, class_map=True)
    r = torch.Generator().manual_seed(9)
    s1 = torch.randn(3, 44, 40, generator=r).to(dev)
    s2 = (s1 + 0.5 * torch.randn(3, 44, 40, generator=r).to(dev))
    mask = inf.predict_scene(m, s1, s2, patch_size=16, batch_size=2, two_streams=True).clone()
    m.train()
    ts.step(*_batch(6))
    tw.step(*_batch(5))
    # what the visitors saw is what a fresh model on the state between the micro-steps sees
    fresh = twin(tw.model).eval()
    with torch.no_grad():
        same_bits(mid, fresh(x1, x2), f'eval forward between micro-steps [{prec}]')
    same_bits(mask, inf.predict_scene(fresh, s1, s2, patch_size=16, batch_size=2, two_streams=True), f'scan between micro-steps [{prec}]')
    same_bits(cd, fresh.engine().forward(x1, x2, inf._eval_params(fresh), training=False, class_map=True)[0], f'class map [{prec}]')
    tw.step(*_batch(6))
    got = snapshot(ts)
    same_bits(got, snapshot(tw), f'update after the visit [{prec}]')
    mattered(mid, _eval_logits_of(m, x1, x2), f'the update [{prec}]')
    same_bits(probe(ts), probe(tw), f'steps after the visit [{prec}]')


def _eval_logits_of(m, x1, x2):
    m.eval()
    with torch.no_grad():
        out = m(x1, x2).clone()
    m.train()
    return out


# ------------------------------------------------------------------ the module used beside the step
@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('prec', PRECS)
def test_eager_pass_between_fused_steps(prec, mode):
    """A fused step(), an eager model(x1, x2) forward and backward on the same module, then step() again.

    After step(): p.grad is the view of flat_grads the step bound and holds the step's own (unclipped) gradient.  After the eager
    backward: autograd ADDED its gradient in place into the same view (still the view; flat_grads = step gradient + eager gradient).
    The next step() overwrites flat_grads with its own gradient -- except the biases in front of a BatchNorm, which backward never
    writes on batch statistics because they are identically zero.  A training-mode eager pass adds zeros there; an EVAL-mode one adds
    real values (scale * dbeta), which the step has to zero again or every later update applies them.  The second step() and those
    after it are held to the twin."""
    m = _model(prec)
    ts = _warm(TrainStep(m, lr=0.05, momentum=0.9), 2)
    bias = 'up2.conv.conv.0.bias'
    views = {k: p.grad.data_ptr() for k, p in m.named_parameters()}
    assert all(views[k] == ts.grads[k].data_ptr() for k in views) and not bool(ts.grads[bias].any())

    def eager(ts):
        g_step = ts.flat_grads.clone()
        x1, x2, _ = _batch(7)
        m.train(mode == 'train')
        m(x1, x2).backward(torch.ones(2, 2, 16, 16, device=dev))
        m.train()
        assert all(p.grad.data_ptr() == views[k] for k, p in m.named_parameters())
        mattered(g_step, ts.flat_grads, f'the eager {mode} backward on p.grad [{prec}]')
        assert bool(ts.grads[bias].any()) == (mode == 'eval')
    # an eval-mode pass moves no exported state (no running statistics): what it changed is flat_grads, checked above
    got = run(ts, eager, f'eager {mode} pass between steps [{prec}]', neutral=mode == 'eval')
    assert all(p.grad.data_ptr() == views[k] for k, p in m.named_parameters()) and not bool(ts.grads[bias].any())
    same_bits(got['flat_grads'], ts.flat_grads, 'p.grad is the last step\'s gradient again')


@pytest.mark.parametrize('prec', PRECS)
def test_load_state_dict_in_place_after_the_step_is_built(prec):
    """model.load_state_dict(sd) copies into the step's flat buffers: the steps follow the new weights."""
    ts = _warm(TrainStep(_model(prec), lr=0.05, momentum=0.9), 2)
    other = {k: v.clone() for k, v in _filled(seed=7).items()}
    run(ts, lambda ts: ts.model.load_state_dict(other), f'load_state_dict in place [{prec}]')


@pytest.mark.parametrize('how', ['assign', 'p.data', 'buffer', 'second step'])
@pytest.mark.parametrize('prec', PRECS)
def test_repointed_tensors_are_refused_or_followed(prec, how):
    """load_state_dict(assign=True) / p.data = t / a re-assigned buffer / a second TrainStep built on the same module (its constructor
    re-points every parameter at its own flat buffer) after the step is built: the next step() either behaves exactly as a twin built on
    the model as it now is (with the optimizer state the step has), or raises RuntimeError naming the tensor before anything is launched.
    Silently training weights the module no longer holds fails.  Today's code follows: it binds the module again."""
    m = _model(prec)
    ts = _warm(TrainStep(m, lr=0.05, momentum=0.9), 2)
    base = probe(twin_step(ts), 2)
    key = 'up3.conv.conv.0.weight'
    if how == 'assign':
        m.load_state_dict({k: v.clone() for k, v in _filled(seed=7).items()}, assign=True)
        key = 'inc.conv.conv.0.weight'                                    # the first one met
    elif how == 'p.data':
        p = dict(m.named_parameters())[key]
        p.data = p.data * 1.5
    elif how == 'buffer':
        key = 'up3.conv.conv.1.running_var'
        m.up3.conv.conv[1].running_var = m.up3.conv.conv[1].running_var * 1.5
    else:
        key = 'inc.conv.conv.0.weight'
        other = TrainStep(m, lr=0.5)
        other.step(*_batch(7))                                            # the module's weights move in the other step's buffer
        torch.cuda.synchronize()
        assert dict(m.named_parameters())[key].data_ptr() != ts.layout.view(ts.flat_params, key).data_ptr()
    tw = TrainStep(twin(m), lr=0.05, momentum=0.9)
    tw.load_optimizer_state_dict(ts.optimizer_state_dict())
    held, flat = clone_state(m), ts.flat_params.clone()
    torch.cuda.synchronize()
    try:
        got = probe(ts, 2)
    except RuntimeError as e:
        assert key in str(e), f'the refusal must name {key}: {e}'
        torch.cuda.synchronize()
        same_bits(clone_state(m), held, 'refused: the module is untouched')
        same_bits(ts.flat_params, flat, 'refused: nothing was updated')
        return
    same_bits(got, probe(tw, 2), f'{how}: against a step built on the model as it is [{prec}]')
    what = 'state' if how == 'buffer' else 'last_logits'                   # a running variance does not reach training-mode logits
    mattered(base[what], got[what], f'{how} [{prec}]')
    for k, p in m.named_parameters():                                     # the module holds what the step trains, and sees its gradients
        assert p.data_ptr() == ts.layout.view(ts.flat_params, k).data_ptr() and p.grad.data_ptr() == ts.grads[k].data_ptr(), k
    same_bits(clone_state(m), got['state'], f'{how}: the module holds the trained weights [{prec}]')


def test_module_moved_off_the_device_is_refused():
    """model.cpu() after the step is built cannot be followed: step() raises RuntimeError naming the first tensor, nothing is launched."""
    m = _model('bf16')
    ts = _warm(TrainStep(m, lr=0.05), 1)
    flat = ts.flat_params.clone()
    m.cpu()
    with pytest.raises(RuntimeError, match='inc.conv.conv.0.weight'):
        ts.step(*_batch(5))
    torch.cuda.synchronize()
    same_bits(ts.flat_params, flat, 'refused: nothing was updated')
