"""CPU tests of the fused step's weight averaging: the float64 restatement tests/ema_ref.py pinned against CPU
torch.optim.swa_utils.AveragedModel (EMA through get_ema_multi_avg_fn, and the default SWA average), fabric_amd.optim.check_ema, the
flat <-> AveragedModel state conversion, load_checkpoint on an AveragedModel state dict, the C ABI rows and argument checks of the three
entry points, and train.py's flags."""
import ctypes
import io
import os
import re

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from fabric_amd import BiDateNet, _lib
from fabric_amd.optim import average_weight, avg_to_torch, check_ema, is_averaged_state, torch_to_avg
from fabric_amd.parallel import FlatLayout
from fabric_amd.utils.helpers import load_checkpoint
from tests import ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement against AveragedModel
def _small():
    torch.manual_seed(7)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    with torch.no_grad():
        m[1].running_mean.normal_()
        m[1].running_var.uniform_(0.5, 2.0)
    return m


def _move(m, g):
    with torch.no_grad():
        for t in list(m.parameters()) + [b for b in m.buffers() if b.dtype.is_floating_point]:
            t.add_(torch.randn(t.shape, generator=g) * 0.3)


@pytest.mark.parametrize('decay', [0.9, 0.999, 0.3])
def test_restatement_matches_cpu_averaged_model_ema(decay):
    """Five updates of AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True): the first is a copy, every later one
    is within R.ULPS of R.lerp(previous average, current values, 1 - decay) (decay 0.3 takes lerp's w >= 0.5 branch)."""
    m = _small()
    am = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True)
    g = torch.Generator().manual_seed(1)
    for it in range(5):
        prev = {k: v.clone() for k, v in am.module.state_dict().items()}
        _move(m, g)
        am.update_parameters(m)
        for k, v in am.module.state_dict().items():
            if not v.dtype.is_floating_point:
                continue
            cur = m.state_dict()[k]
            if it == 0:
                assert torch.equal(v, cur), k
            else:
                ref, mag = R.lerp(prev[k], cur, R.ema_weight(decay))
                R.check(v, ref, mag, f'decay {decay} update {it} {k}')
    assert int(am.n_averaged) == 5


def test_restatement_matches_cpu_averaged_model_swa():
    """The default average of AveragedModel (SWA: the equal-weight running mean) against R.lerp with weight 1 / (n_averaged + 1), and
    after five updates against the float64 mean of the five snapshots."""
    m = _small()
    am = AveragedModel(m)
    g = torch.Generator().manual_seed(2)
    snaps = []
    for it in range(5):
        prev = {k: v.clone() for k, v in am.module.state_dict().items()}
        _move(m, g)
        snaps.append({k: v.double().clone() for k, v in m.named_parameters()})
        am.update_parameters(m)
        for k, p in m.named_parameters():
            v = am.module.state_dict()[k]
            if it == 0:
                assert torch.equal(v, p), k
            else:
                ref, mag = R.lerp(prev[k], p, R.swa_weight(it))
                R.check(v, ref, mag, f'swa update {it} {k}')
                assert average_weight('swa', None, it) == R.swa_weight(it)
    for k, _ in m.named_parameters():
        mean = torch.stack([s[k] for s in snaps]).mean(0)
        mag = torch.stack([s[k].abs() for s in snaps]).mean(0) * 1.5
        R.check(am.module.state_dict()[k], mean, mag, f'swa mean {k}', ulps=5 * R.ULPS)


def test_restatement_edges():
    a, p = torch.tensor([1.5, -2.0, 3e-4]), torch.tensor([0.25, 7.0, -1e3])
    assert torch.equal(R.lerp(a, p, 0.0)[0], a.double()) and torch.equal(R.lerp(a, p, 1.0)[0], p.double())
    assert R.weight32(1 - 0.9) == float(torch.tensor(1 - 0.9, dtype=torch.float32)) != 1 - 0.9
    v, mag = R.lerp(a, p, 0.25)
    assert torch.allclose(v, a.double() + R.weight32(0.25) * (p.double() - a.double())) and bool((mag >= v.abs()).all())
    v, mag = R.lerp(a, p, 0.75)
    assert torch.allclose(v, 0.25 * a.double() + 0.75 * p.double()) and bool((mag >= v.abs()).all())
    assert average_weight('ema', 0.999, 17) == 1 - 0.999


# ---------------------------------------------------------------- check_ema
def test_check_ema():
    assert check_ema() == (False, None, 'ema', 1, 0)
    assert check_ema(0.999) == (True, 0.999, 'ema', 1, 0)
    assert check_ema(0, 'ema', 4, 10) == (True, 0.0, 'ema', 4, 10)
    assert check_ema(None, 'swa', 2, 3) == (True, None, 'swa', 2, 3)
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=float('nan')), dict(ema_decay=True), dict(ema_decay='0.9'),
                dict(ema_every=0), dict(ema_every=1.5), dict(ema_every=True), dict(ema_start=-1), dict(ema_start=0.0),
                dict(average='mean'), dict(average=None), dict(ema_decay=0.9, average='swa')):
        with pytest.raises(ValueError):
            check_ema(**bad)


# ---------------------------------------------------------------- flat <-> AveragedModel state
def _layout():
    shapes = [('a.weight', (4, 3, 3, 3)), ('a.bias', (4,)), ('bn.weight', (5,)), ('bn.bias', (5,))]
    keys = ['a.weight', 'a.bias', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var', 'bn.num_batches_tracked']
    return FlatLayout(shapes, ['bn.bias', 'bn.weight', 'a.bias', 'a.weight']), keys


def test_state_conversion_round_trip():
    layout, keys = _layout()
    g = torch.Generator().manual_seed(3)
    flat = torch.randn(layout.total, generator=g)
    bufs = {'bn.running_mean': torch.randn(5, generator=g), 'bn.running_var': torch.rand(5, generator=g),
            'bn.num_batches_tracked': torch.tensor(12)}
    sd = avg_to_torch(layout, keys, flat, bufs, 9)
    assert list(sd) == ['n_averaged'] + ['module.' + k for k in keys]
    assert sd['n_averaged'].dtype == torch.int64 and sd['n_averaged'].dim() == 0 and int(sd['n_averaged']) == 9
    assert is_averaged_state(sd) and not is_averaged_state({k: v for k, v in sd.items() if k != 'n_averaged'})
    assert not is_averaged_state(dict(sd, extra=torch.zeros(1))) and not is_averaged_state({'n_averaged': torch.tensor(1)})
    for k in keys:
        want = layout.view(flat, k) if k in layout.slices else bufs[k]
        assert torch.equal(sd['module.' + k], want) and sd['module.' + k].data_ptr() != want.data_ptr()        # copies, not views
    n, vals = torch_to_avg(sd, layout, keys, bufs)
    assert n == 9 and list(vals) == keys and all(torch.equal(vals[k], sd['module.' + k]) for k in keys)
    # what AveragedModel itself writes for the same module has the same keys
    for bad in ({k: v for k, v in sd.items() if k != 'module.a.bias'},                   # missing
                dict(sd, **{'module.c.weight': torch.zeros(1)}),                         # unexpected
                dict(sd, **{'module.a.bias': torch.zeros(5)}),                           # wrong shape
                dict(sd, **{'module.bn.running_var': torch.zeros(4)}),
                {k: v for k, v in sd.items() if k != 'n_averaged'},
                dict(sd, n_averaged=torch.tensor(1.0)), dict(sd, n_averaged=torch.tensor(-1))):
        with pytest.raises(ValueError):
            torch_to_avg(bad, layout, keys, bufs)


def test_state_has_averaged_models_keys():
    m = BiDateNet(3, 2)
    theirs = AveragedModel(m, use_buffers=True).state_dict()
    assert is_averaged_state(theirs)
    assert list(theirs) == ['n_averaged'] + ['module.' + k for k in m.state_dict()]
    assert theirs['n_averaged'].dtype == torch.int64 and theirs['n_averaged'].dim() == 0


# ---------------------------------------------------------------- load_checkpoint
def test_load_checkpoint_reads_an_averaged_model_state_dict(tmp_path):
    torch.manual_seed(5)
    m = BiDateNet(3, 2)
    am = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(0.5), use_buffers=True)
    for _ in range(2):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        am.update_parameters(m)
    sd = am.state_dict()
    path = tmp_path / 'ema_epoch_3.pt'
    torch.save(sd, path)
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    for src in (sd, str(path), buf, {'state_dict': sd}):
        got = load_checkpoint(src, allow_pickle=False)
        assert isinstance(got, BiDateNet) and got.n_channels == 3 and got.n_classes == 2
        want = am.module.state_dict()
        assert list(got.state_dict()) == list(want) and all(torch.equal(got.state_dict()[k], want[k]) for k in want)
    assert not torch.equal(got.state_dict()['outc.conv.weight'], m.state_dict()['outc.conv.weight'])
    # every other input behaves as before: a DataParallel-style dict, and one with a stray unprefixed key still fails strictly
    plain = load_checkpoint({'module.' + k: v for k, v in m.state_dict().items()})
    assert torch.equal(plain.state_dict()['outc.conv.weight'], m.state_dict()['outc.conv.weight'])
    with pytest.raises(RuntimeError):
        load_checkpoint(dict(sd, n_averaged=torch.tensor(2.0)))                            # not an integer count: not an averaged state


# ---------------------------------------------------------------- the C ABI
_CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'const uint32_t*': ctypes.c_void_p, 'const int32_t*': ctypes.c_void_p,
           'const void*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}
NEW = ['bdn_ema_update', 'bdn_ema_update_multi', 'bdn_swap_segments']


@pytest.mark.parametrize('name', NEW)
def test_header_declaration_matches_signature_row(name):
    """Every pointer of the new entry points is device memory (c_void_p rows, which tests/guard.py checks); the scalars go by value."""
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())) for p in m.group(1).split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and [_CTYPES[p.rsplit(' ', 1)[0].strip()] for p in params] == list(args), (params, args)
    assert params[-1] == 'void* stream'


def test_argument_errors_return_before_touching_a_device():
    lib = _lib.load()
    err = lambda: lib.bdn_last_error()                     # noqa: E731
    ema, multi, swap = lib.bdn_ema_update, lib.bdn_ema_update_multi, lib.bdn_swap_segments
    ok = [16, 32, None, None, 0, 0.1, 0, 16, None]

    def bad(i, v, j=None, u=None):
        a = list(ok)
        a[i] = v
        if j is not None:
            a[j] = u
        return ema(*a)
    assert bad(0, None) == -1 and b'null' in err()
    assert bad(1, None) == -1 and b'null' in err()
    assert bad(0, 20) == -1 and b'aligned' in err()
    assert bad(4, 1) == -1 and b'null' in err()                                # a table is announced but not given
    assert bad(4, 257) == -1 and b'segments' in err()
    assert bad(4, -1) == -1 and b'segments' in err()
    assert bad(2, 18, 4, 1) == -1
    assert bad(7, 18) == -1 and b'multiple of 4' in err()
    for w in (-1e-3, 1.0001, float('nan'), float('inf')):
        assert bad(5, w) == -1 and b'weight' in err()
        assert multi(16, 1, 1, w, 0, None) == -1 and b'weight' in err()
    assert bad(6, 2) == -1 and b'copy' in err()
    assert bad(7, 0) == 0                                                      # n == 0 launches nothing
    assert multi(None, 1, 1, 0.5, 0, None) == -1 and b'null' in err()
    assert multi(20, 1, 1, 0.5, 0, None) == -1 and b'aligned' in err()
    assert multi(16, -1, 1, 0.5, 0, None) != 0 and multi(16, 1, -1, 0.5, 0, None) != 0 and multi(16, 65536, 1, 0.5, 0, None) != 0
    assert multi(16, 0, 8, 0.5, 0, None) == 0 and multi(16, 3, 0, 0.5, 1, None) == 0
    assert swap(16, 32, None, None, 0, 0, None) == 0
    assert swap(16, 16, None, None, 0, 16, None) == -1 and b'same' in err()
    assert swap(16, None, None, None, 0, 16, None) == -1 and b'null' in err()
    assert swap(16, 36, None, None, 0, 16, None) == -1 and b'aligned' in err()
    assert swap(16, 32, 16, None, 2, 16, None) == -1 and b'null' in err()
    assert swap(16, 32, None, None, 0, 6, None) == -1 and b'multiple of 4' in err()


# ---------------------------------------------------------------- train.py's flags
def test_train_flags_parse_and_need_the_fused_step():
    from fabric_amd import train as T
    for flags in (['--ema_decay', '0.999'], ['--swa'], ['--ema_every', '4'], ['--ema_start', '100'], ['--ema_buffers', 'false'],
                  ['--ema_decay', '0.9', '--ema_every', '2', '--ema_start', '5', '--ema_buffers', 'true']):
        with pytest.raises(SystemExit, match='--fused_step true'):
            T.main(['--synthetic'] + flags)
    # with the fused step the flags parse and reach check_ema, which refuses these before anything touches a device
    for flags, msg in ((['--swa', '--ema_decay', '0.9'], 'swa'), (['--ema_decay', '1.0'], 'ema_decay'), (['--ema_decay', '0.9', '--ema_every', '0'], 'ema_every'),
                       (['--swa', '--ema_start', '-2'], 'ema_start')):
        with pytest.raises(SystemExit, match=msg):
            T.main(['--synthetic', '--fused_step', 'true'] + flags)
    for flags in (['--ema_every', '4'], ['--ema_start', '10'], ['--ema_buffers', 'false']):      # nothing to shape without an average
        with pytest.raises(SystemExit, match='--ema_decay D or --swa'):
            T.main(['--synthetic', '--fused_step', 'true'] + flags)
    import inspect
    assert inspect.signature(T.save_if_better).parameters['ema_state'].default is None
