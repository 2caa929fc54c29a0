"""-m gpu: EMA / SWA weight averaging in the fused step (fabric_amd/train_step.py: ema_decay, average, ema_every, ema_start, ema_buffers,
ema_state_dict, load_ema_state_dict, ema_weights) on BiDateNet(3, 2), B = 2, 32 x 32, bf16.

Every update against the float64 restatement tests/ema_ref.py; five updates beside a GPU torch.optim.swa_utils.AveragedModel and the state
exchange with it in both directions; no effect on training; accumulation, start and cadence; SWA against the float64 mean; frozen tensors;
the swap context against a fresh model on the averaged state; the training loop's checkpoints and --resume."""
import json

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from fabric_amd import BiDateNet
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.helpers import load_checkpoint
from oracle import filler
from tests import ema_ref as R

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
KW = dict(lr=5e-3, optimizer='adamw')
DECAY = 0.9


def _model():
    return filler.fill_module(BiDateNet(3, 2, precision='bf16')).to(dev).train()


def _inputs(seed=3):
    return tuple(torch.from_numpy(v).to(dev) for v in filler.make_inputs(2, 3, 32, seed=seed))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _stats(d, keys):
    return torch.cat([d[k].detach().flatten() for k in keys])


def test_every_update_follows_the_restatement():
    """Five AdamW steps with ema_decay = 0.9: the first averaging update is a bit-exact copy, every later one is within R.ULPS of
    lerp(previous average, current values, float32(1 - 0.9)) for the flat parameters and for the 36 running statistics; n_averaged counts."""
    model = _model()
    ts = TrainStep(model, ema_decay=DECAY, **KW)
    keys = list(ts.avg_buffers)
    assert len(keys) == 36 and all(k.endswith(('running_mean', 'running_var')) for k in keys)
    assert ts.n_averaged == 0 and _same_bits(ts.flat_avg, ts.flat_params)
    x1, x2, lbl = _inputs()
    for it in range(5):
        prev, prev_b = ts.flat_avg.clone(), _stats(ts.avg_buffers, keys)
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        live_b = _stats(ts._P, keys)
        assert ts.n_averaged == it + 1
        if it == 0:
            assert _same_bits(ts.flat_avg, ts.flat_params) and _same_bits(_stats(ts.avg_buffers, keys), live_b)
            continue
        ref, mag = R.lerp(prev, ts.flat_params, R.ema_weight(DECAY))
        R.check(ts.flat_avg, ref, mag, f'update {it} flat_avg')
        ref, mag = R.lerp(prev_b, live_b, R.ema_weight(DECAY))
        R.check(_stats(ts.avg_buffers, keys), ref, mag, f'update {it} running statistics')
        assert bool((ts.flat_avg != prev).any()) and bool((ts.flat_avg != ts.flat_params).any())


@pytest.mark.parametrize('use_buffers', [True, False])
def test_five_updates_beside_torch_averaged_model(use_buffers):
    """The same run beside AveragedModel(copy, multi_avg_fn=get_ema_multi_avg_fn(0.9), use_buffers=...) on the GPU, updated after each
    step: every float entry within 5 * 2 * R.ULPS of the last update's magnitude (five updates, two float32 evaluations of each); the
    step's state loads into the AveragedModel (strict), and the AveragedModel's state round-trips through the step bit for bit --
    num_batches_tracked excepted, which is the live count here by design."""
    model = _model()
    ts = TrainStep(model, ema_decay=DECAY, ema_buffers=use_buffers, **KW)
    twin = BiDateNet(3, 2, precision='bf16').to(dev)
    twin.load_state_dict(model.state_dict())
    am = AveragedModel(twin, multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=use_buffers)
    x1, x2, lbl = _inputs()
    prev = None
    for it in range(5):
        prev = {k: v.clone() for k, v in am.state_dict().items()}
        ts.step(x1, x2, lbl)
        am.update_parameters(model)
    torch.cuda.synchronize()
    theirs = {k: v.clone() for k, v in am.state_dict().items()}
    mine = ts.ema_state_dict()
    assert set(mine) == set(theirs) and int(mine['n_averaged']) == int(theirs['n_averaged']) == ts.n_averaged == 5
    assert mine['n_averaged'].dtype == torch.int64 and mine['n_averaged'].dim() == 0 and mine['n_averaged'].device == theirs['n_averaged'].device
    live = model.state_dict()
    n_float = 0
    for k, v in theirs.items():
        if not v.dtype.is_floating_point:
            continue
        key = k[len('module.'):]
        if not use_buffers and key not in ts.layout.slices:
            assert _same_bits(mine[k], live[key]) and _same_bits(v, live[key]), f'{k}: use_buffers=False keeps the live buffer'
            continue
        _, mag = R.lerp(prev[k], live[key], R.ema_weight(DECAY))
        R.check(mine[k], v, mag, k, ulps=5 * 2 * R.ULPS)
        n_float += 1
    assert n_float == (74 + 36 if use_buffers else 74)
    for k in live:
        if k.endswith('num_batches_tracked'):
            # the live count, never averaged (5 forwards; the shared encoder's layers see both dates: 10)
            assert int(mine['module.' + k]) == int(live[k]) and int(live[k]) in (5, 10), k
    # AveragedModel's state -> the step -> back: bit for bit
    ts.load_ema_state_dict(theirs)
    back = ts.ema_state_dict()
    for k, v in theirs.items():
        if v.dtype.is_floating_point:
            assert _same_bits(back[k], v), k
    assert int(back['n_averaged']) == 5
    # ... and the step's state -> AveragedModel
    am.load_state_dict(mine, strict=True)
    for k, v in am.state_dict().items():
        assert torch.equal(v, mine[k]), k
    # refusals
    bad = dict(theirs)
    bad.pop('module.outc.conv.bias')
    with pytest.raises(ValueError):
        ts.load_ema_state_dict(bad)
    with pytest.raises(ValueError):
        ts.load_ema_state_dict(dict(theirs, extra=torch.zeros(1)))
    with pytest.raises(ValueError):
        ts.load_ema_state_dict({**theirs, 'module.outc.conv.bias': torch.zeros(3)})
    assert _same_bits(ts.ema_state_dict()['module.outc.conv.bias'], theirs['module.outc.conv.bias'])        # nothing was written


def _run(n, **kw):
    model = _model()
    ts = TrainStep(model, **KW, **kw)
    x1, x2, lbl = _inputs()
    losses = [ts.step(x1, x2, lbl) for _ in range(n)]
    torch.cuda.synchronize()
    return model, ts, torch.stack(losses)


def test_averaging_does_not_change_training():
    """Three steps with the average on and off: parameters, optimizer state, BatchNorm buffers and losses are bit-equal, and with it off
    nothing is kept."""
    m_on, on, l_on = _run(3, ema_decay=DECAY)
    m_off, off, l_off = _run(3)
    assert off.flat_avg is None and off.avg_buffers == {} and off.n_averaged == 0 and off._avg_desc is None
    assert _same_bits(on.flat_params, off.flat_params) and _same_bits(l_on, l_off)
    assert all(_same_bits(on.opt_state[k], off.opt_state[k]) for k in on.opt_state) and on.opt_step == off.opt_step == 3
    sd_on, sd_off = m_on.state_dict(), m_off.state_dict()
    assert all(torch.equal(sd_on[k], sd_off[k]) for k in sd_on)
    with pytest.raises(RuntimeError):
        off.ema_state_dict()
    with pytest.raises(RuntimeError):
        with off.ema_weights():
            pass


def test_accumulation_averages_once_per_update():
    _, ts, _ = _run(4, ema_decay=DECAY, accumulate=2)
    assert ts.n_averaged == 2 and ts.opt_step == 2
    x1, x2, lbl = _inputs()
    ts.step(x1, x2, lbl)
    assert ts.n_averaged == 2 and ts.micro == 1
    with pytest.raises(RuntimeError):
        ts.ema_state_dict()                                                       # a micro-step is pending
    with pytest.raises(RuntimeError):
        with ts.ema_weights():
            pass
    assert ts.flush() and ts.n_averaged == 3                                      # the flushed update is averaged too


def test_start_and_cadence():
    """ema_every = 2, ema_start = 2 over six updates: updates 4 and 6 are averaged, the first of them as a copy; the others leave the
    average's bits alone."""
    model = _model()
    ts = TrainStep(model, ema_decay=DECAY, ema_every=2, ema_start=2, **KW)
    x1, x2, lbl = _inputs()
    init = ts.flat_avg.clone()
    seen = []
    for u in range(1, 7):
        prev = ts.flat_avg.clone()
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        seen.append(ts.n_averaged)
        if u < 4:
            assert _same_bits(ts.flat_avg, init)
        elif u == 4:
            assert _same_bits(ts.flat_avg, ts.flat_params)
        elif u == 5:
            assert _same_bits(ts.flat_avg, prev)
        else:
            ref, mag = R.lerp(prev, ts.flat_params, R.ema_weight(DECAY))
            R.check(ts.flat_avg, ref, mag, 'update 6')
    assert seen == [0, 0, 0, 1, 1, 2]


def test_swa_is_the_mean_of_the_snapshots():
    """average='swa': after four updates the average is the float64 mean of the four parameter snapshots within 4 * R.ULPS of the last
    update's magnitude (three lerps with weights 1/2, 1/3, 1/4 after the copy)."""
    model = _model()
    ts = TrainStep(model, average='swa', **KW)
    x1, x2, lbl = _inputs()
    snaps = []
    for _ in range(4):
        ts.step(x1, x2, lbl)
        torch.cuda.synchronize()
        snaps.append(ts.flat_params.double().cpu())
    assert ts.n_averaged == 4
    avg, mag = snaps[0], None
    for n in range(1, 4):
        avg, mag = R.lerp(avg, snaps[n], R.swa_weight(n))
    R.check(ts.flat_avg, torch.stack(snaps).mean(0), mag, 'swa', ulps=4 * R.ULPS)
    assert bool((ts.flat_avg != ts.flat_params).any())


def test_frozen_tensors_keep_their_value_as_their_average():
    model = _model()
    groups = [{'params': [k for k, _ in model.named_parameters()]}]
    for k, p in model.named_parameters():
        if k.startswith(('inc', 'down1')):
            p.requires_grad_(False)
    ts = TrainStep(model, ema_decay=0.5, param_groups=groups, **KW)
    init = ts.flat_params.clone()
    x1, x2, lbl = _inputs()
    for _ in range(3):
        ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    frozen = [k for k in ts.layout.order if k.startswith(('inc', 'down1'))]
    assert frozen and ts.n_averaged == 3
    for k in ts.layout.order:
        a, p, i = (ts.layout.view(t, k) for t in (ts.flat_avg, ts.flat_params, init))
        if k in frozen:
            assert _same_bits(a, p) and _same_bits(a, i), k
        elif a.dim() == 4:                                                        # every trainable filter moved, and its average lags
            assert bool((a != i).any()) and bool((a != p).any()), k


def test_swap_context():
    """Inside `with step.ema_weights():` eval-mode logits are those of a fresh BiDateNet loaded from ema_state_dict() (stale packed weights
    or eval tables would show); after it, also after an exception, the live weights are back bit for bit; step() inside raises; and one
    more step after it equals the same step of a run that never entered the context."""
    model, ts, _ = _run(3, ema_decay=DECAY)
    twin_model, twin, _ = _run(3, ema_decay=DECAY)
    x1, x2, lbl = _inputs()
    e1, e2, _ = _inputs(seed=11)
    sd = ts.ema_state_dict()
    fresh = load_checkpoint(sd, device=dev, precision='bf16').eval()
    model.eval()
    with torch.no_grad():
        want = fresh(e1, e2).clone()
        before = model(e1, e2).clone()
    flat = ts.flat_params.clone()
    avg = ts.flat_avg.clone()
    assert not torch.equal(want, before)
    with ts.ema_weights():
        with torch.no_grad():
            inside = model(e1, e2).clone()
        assert _same_bits(ts.flat_params, avg) and _same_bits(ts.flat_avg, flat)
        k0, p0 = next(iter(model.named_parameters()))
        assert p0.data_ptr() == ts.layout.view(ts.flat_params, k0).data_ptr()     # the parameters stay views of flat_params
        for call in (lambda: ts.step(x1, x2, lbl), ts.flush, ts.ema_state_dict, lambda: ts.load_ema_state_dict(sd),
                     ts.optimizer_state_dict):
            with pytest.raises(RuntimeError):
                call()
    assert torch.equal(inside, want)
    with torch.no_grad():
        after = model(e1, e2).clone()
    assert torch.equal(after, before) and _same_bits(ts.flat_params, flat) and _same_bits(ts.flat_avg, avg)
    with pytest.raises(KeyError):
        with ts.ema_weights():
            raise KeyError('body')
    torch.cuda.synchronize()
    assert _same_bits(ts.flat_params, flat) and _same_bits(ts.flat_avg, avg)
    with torch.no_grad():
        assert torch.equal(model(e1, e2), before)
    model.train()
    la, lb = ts.step(x1, x2, lbl), twin.step(x1, x2, lbl)
    torch.cuda.synchronize()
    assert _same_bits(la, lb) and _same_bits(ts.flat_params, twin.flat_params) and _same_bits(ts.flat_avg, twin.flat_avg)
    sa, sb = model.state_dict(), twin_model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_swap_before_the_first_average_is_a_no_op():
    model = _model()
    ts = TrainStep(model, ema_decay=DECAY, ema_start=100, **KW)
    x1, x2, lbl = _inputs()
    ts.step(x1, x2, lbl)
    flat = ts.flat_params.clone()
    with ts.ema_weights():
        assert _same_bits(ts.flat_params, flat)
        with pytest.raises(RuntimeError):
            ts.step(x1, x2, lbl)
    assert _same_bits(ts.flat_params, flat) and ts.n_averaged == 0


def test_training_loop_writes_and_resumes_the_average(tmp_path, capsys):
    """fabric_amd.train --fused_step true --optimizer adamw --ema_decay 0.9 for two epochs: the epoch record carries ema_n_averaged,
    ema_epoch_0.pt is written beside the live checkpoint and load_checkpoint reads it as a BiDateNet on the averaged weights;
    --resume from epoch 0 restores n_averaged."""
    from fabric_amd import train as T
    common = ['--synthetic', '--batch_size', '8', '--patch_size', '64', '--stride', '128', '--num_workers', '0', '--learning_rate', '0.002',
              '--fused_step', 'true', '--optimizer', 'adamw', '--ema_decay', '0.9', '--log_dir', str(tmp_path)]
    T.main(common + ['--epochs', '2'])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith('{"epoch"')]
    assert [l['epoch'] for l in lines] == [0, 1]
    per_epoch = lines[0]['ema_n_averaged']
    assert per_epoch > 0 and lines[1]['ema_n_averaged'] == 2 * per_epoch
    sd = torch.load(tmp_path / 'ema_epoch_0.pt', weights_only=True)
    assert int(sd['n_averaged']) == per_epoch and len(sd) == 1 + 128 and all(v.device.type == 'cpu' for v in sd.values())
    ema = load_checkpoint(str(tmp_path / 'ema_epoch_0.pt'))
    live = load_checkpoint(str(tmp_path / 'checkpoint_epoch_0.state_dict.pt'))
    assert isinstance(ema, BiDateNet)
    assert torch.equal(ema.state_dict()['outc.conv.weight'], sd['module.outc.conv.weight'])
    assert not torch.equal(ema.state_dict()['outc.conv.weight'], live.state_dict()['outc.conv.weight'])     # the live weights are kept apart
    T.main(common + ['--epochs', '2', '--resume', str(tmp_path / 'checkpoint_epoch_0.state_dict.pt')])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith('{"epoch"')]
    assert [l['epoch'] for l in lines] == [1] and lines[0]['ema_n_averaged'] == 2 * per_epoch
    with pytest.raises(SystemExit):
        T.main(['--synthetic', '--ema_decay', '0.9'])                             # --fused_step true only


def test_freezing_mid_run_and_a_loaded_average_that_was_running():
    """set_param_groups() with averaging on: a tensor frozen now takes its value as its average (the exchange skips it, so anything else
    would make the model inside ema_weights() differ from ema_state_dict()), the others keep their average's bits, and after one more
    step the logits inside the block are still those of a fresh model on ema_state_dict().  load_ema_state_dict() of a state whose
    n_averaged > 0 ends the ema_start delay; one with n_averaged == 0 does not."""
    model, ts, _ = _run(2, ema_decay=DECAY)
    avg = ts.flat_avg.clone()
    for k, p in model.named_parameters():
        if k.startswith('outc'):
            p.requires_grad_(False)
    ts.set_param_groups(None)
    torch.cuda.synchronize()
    for k in ts.layout.order:
        a, p, old = (ts.layout.view(t, k) for t in (ts.flat_avg, ts.flat_params, avg))
        if k.startswith('outc'):
            assert _same_bits(a, p) and not _same_bits(a, old), k
        else:
            assert _same_bits(a, old), k
    x1, x2, lbl = _inputs()
    ts.step(x1, x2, lbl)
    e1, e2, _ = _inputs(seed=11)
    fresh = load_checkpoint(ts.ema_state_dict(), device=dev, precision='bf16').eval()
    model.eval()
    with torch.no_grad(), ts.ema_weights():
        assert torch.equal(model(e1, e2), fresh(e1, e2))
    # the start delay and a loaded average
    sd = ts.ema_state_dict()
    late = TrainStep(_model(), ema_decay=DECAY, ema_start=100, ema_every=2, **KW)
    late.step(x1, x2, lbl)
    assert late.n_averaged == 0
    late.load_ema_state_dict(dict(sd, n_averaged=torch.tensor(0)))
    late.step(x1, x2, lbl)
    assert late.n_averaged == 0                                                   # no average was running: the delay holds
    late.load_ema_state_dict(sd)
    assert late.n_averaged == 3
    seen = []
    for _ in range(4):
        late.step(x1, x2, lbl)
        seen.append(late.n_averaged)
    assert seen == [3, 4, 4, 5]                                                   # every second update from the load on
