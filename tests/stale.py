"""Helpers of the stale-state tests (tests/test_stale_cpu.py, tests/test_gpu_stale_*.py, tests/test_gpu_poisoned_alloc.py).

The library is bit-reproducible and uses no float atomics, so the oracle for everything that survives between calls -- packed filter
images, folded eval BatchNorm tables, pooled workspaces, grown scratch, the fused step's flat buffers and descriptor tables -- is exact:
a model that has been through a call sequence must give the same BITS as a twin, a fresh model given the same state, that has run
nothing.  twin() / twin_step() build that twin, same_bits() / mattered() compare, poisoned_allocations() makes every floating-point
buffer the library allocates start as NaN so that a read of memory nobody wrote cannot hide behind a zero the allocator happened to
hand out.  Importable without a device."""
import contextlib
import copy

import torch

FLOATS = (torch.float32, torch.bfloat16, torch.float16, torch.float64)
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ------------------------------------------------------------------ twins
def clone_state(model):
    """A clone of model.state_dict() as it is now (on the model's device)."""
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def twin(model):
    """A new BiDateNet of the same channels, classes and precision with a NEW engine, loaded from a clone of model.state_dict() taken
    now; same device, same .training flag, same requires_grad flags."""
    from fabric_amd import BiDateNet
    sd = clone_state(model)
    with torch.device(next(iter(sd.values())).device):                   # built where it will live: no host-side initialisation
        t = BiDateNet(model.n_channels, model.n_classes, precision=model.precision)
    t.load_state_dict(sd)
    t.train(model.training)
    flags = {k: p.requires_grad for k, p in model.named_parameters()}
    for k, p in t.named_parameters():
        p.requires_grad_(flags[k])
    return t


def step_kwargs(ts):
    """The constructor arguments a TrainStep was built with, as far as they shape its arithmetic, with the hyperparameters it carries NOW
    (lr and per-group lr / weight_decay may have been reassigned since)."""
    o = ts.optim
    kw = dict(lr=float(ts.lr), tversky_alpha=ts.alpha, tversky_beta=ts.beta, eps=ts.eps,
              optimizer=o.kind, momentum=o.momentum, dampening=o.dampening, nesterov=o.nesterov, weight_decay=o.weight_decay,
              betas=tuple(o.betas), adam_eps=o.eps, bn=ts.bn, criterion=ts.criterion, accumulate=ts.accumulate,
              max_grad_norm=ts.max_grad_norm, ema_decay=ts.ema_decay, average=ts.average, ema_every=ts.ema_every,
              ema_start=ts.ema_start, ema_buffers=ts.ema_buffers)
    if ts.param_groups is not None and not ts._implicit_group:
        kw['param_groups'] = copy.deepcopy(ts.param_groups)
    return kw


def twin_step(ts, **kw):
    """A new TrainStep on twin(ts.model), built with the same constructor arguments (kw overrides), the same lr, param_groups and
    requires_grad flags, then given optimizer_state_dict() and, where averaging is on, ema_state_dict().  Pending micro-steps cannot
    be exported: a scenario that ends with some builds its twin BEFORE them and replays them (it says so).  The averaging cadence
    (ema_every) restarts at a load by design, so the step must stand on a cadence boundary."""
    from fabric_amd.train_step import TrainStep
    assert ts.micro == 0, 'twin_step: micro-steps are pending; build the twin before them and replay them'
    if ts.flat_avg is not None:
        assert (ts.n_averaged > 0 or ts._updates == 0) and (ts._updates - ts.ema_start) % ts.ema_every == 0, \
            'twin_step: the averaging cadence is mid-period here and a loaded state restarts it: move the twin point'
    args = step_kwargs(ts)
    args.update(kw)
    t = TrainStep(twin(ts.model), **args)
    t.load_optimizer_state_dict(ts.optimizer_state_dict())
    if ts.flat_avg is not None:
        t.load_ema_state_dict(ts.ema_state_dict())
    return t


# ------------------------------------------------------------------ bit comparison
def _bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.view(_INT_OF_SIZE[t.element_size()])


def _leaves(v, key=''):
    """(key, leaf) pairs of a tensor, a number / None, or a (nested) dict / list / tuple of them, in a fixed order."""
    if isinstance(v, dict):
        for k in v:
            yield from _leaves(v[k], f'{key}[{k!r}]' if key else str(k))
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            yield from _leaves(x, f'{key}[{i}]')
    else:
        yield key, v


def first_difference(got, want):
    """None when got and want hold the same bits, else a one-line description of the first difference: a missing or extra key, a
    shape or dtype mismatch, or the first differing key with the number of differing elements.  Tensors are compared through an integer
    view of their bytes: equal NaNs are equal, -0.0 differs from 0.0."""
    a, b = dict(_leaves(got)), dict(_leaves(want))
    missing, extra = [k for k in b if k not in a], [k for k in a if k not in b]
    if missing or extra:
        return f'keys differ: missing {missing[:3]}, unexpected {extra[:3]}'
    for k in b:
        x, y = a[k], b[k]
        if isinstance(x, torch.Tensor) != isinstance(y, torch.Tensor):
            return f'{k or "value"}: {type(x).__name__} against {type(y).__name__}'
        if not isinstance(y, torch.Tensor):
            if isinstance(y, float) and isinstance(x, float):
                x, y = torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)
            elif x != y or type(x) is not type(y):
                return f'{k or "value"}: {x!r} against {y!r}'
            else:
                continue
        if x.dtype != y.dtype or x.shape != y.shape:
            return f'{k or "tensor"}: {x.dtype} {tuple(x.shape)} against {y.dtype} {tuple(y.shape)}'
        n = int((_bits(x) != _bits(y)).sum())
        if n:
            return f'{k or "tensor"}: {n} of {y.numel()} elements differ'
    return None


def same_bits(got, want, name):
    d = first_difference(got, want)
    assert d is None, f'{name}: not the same bits -- {d}'


def mattered(before, after, name):
    """The perturbation of a scenario must change the probe's bits: a sequence that leaves them alone cannot detect staleness."""
    assert first_difference(after, before) is not None, f'{name}: the perturbation did not change a single bit (a test bug: it proves nothing)'


def all_finite(v, name):
    for k, t in _leaves(v):
        if isinstance(t, torch.Tensor) and t.dtype in FLOATS:
            assert bool(torch.isfinite(t).all()), f'{name}: {k or "tensor"} has non-finite values'


# ------------------------------------------------------------------ poisoned allocations
def _poison(t):
    """Fill a freshly allocated floating-point tensor with 0xFF bytes (NaN in f32, bf16, f16 and f64) on the current stream.  Integer
    and uint8 results are left alone on purpose: a garbage index read from an unwritten table could turn a finding into an out-of-bounds
    access."""
    if isinstance(t, torch.Tensor) and t.dtype in FLOATS and t.numel():
        if t.is_contiguous():
            t.view(-1).view(torch.uint8).fill_(0xFF)
        else:                                    # a dense permuted result of empty_like: it owns its whole storage
            torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(0xFF)
    return t


def _wrap(fn):
    def poisoned(*a, **k):
        return _poison(fn(*a, **k))
    poisoned.__wrapped__ = fn
    return poisoned


@contextlib.contextmanager
def poisoned_allocations(monkeypatch=None):
    """While active, torch.empty, torch.empty_like and Tensor.new_empty return floating-point tensors filled with 0xFF bytes.  The
    originals come back on exit, also after an exception.  With a pytest `monkeypatch` the wrappers are installed and removed through
    monkeypatch.context() instead of by hand."""
    targets = [(torch, 'empty'), (torch, 'empty_like'), (torch.Tensor, 'new_empty')]
    if monkeypatch is not None:
        with monkeypatch.context() as m:
            for obj, name in targets:
                m.setattr(obj, name, _wrap(getattr(obj, name)))
            yield
        return
    saved = []
    try:
        for obj, name in targets:
            own = name in vars(obj)
            orig = getattr(obj, name)
            saved.append((obj, name, own, orig))
            setattr(obj, name, _wrap(orig))
        yield
    finally:
        for obj, name, own, orig in reversed(saved):
            if own:
                setattr(obj, name, orig)
            else:
                with contextlib.suppress(AttributeError):
                    delattr(obj, name)
