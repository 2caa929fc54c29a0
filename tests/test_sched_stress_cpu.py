"""The launch-perturbation harness (tests/sched_stress.py) pinned without a device, as tests/test_guarded_cpu.py pins the guard: a fake
library behind fabric_amd._lib.load(), a fake sleep and a fake device synchronisation.  A scripted sequence of _lib.call()s on three
streams shows which launches each pattern delays and on which stream, that seeds reproduce, that stream and event entry points are never
touched, that the hook is gone after an exception, and that no launch is ever dropped."""
import pytest

from fabric_amd import _lib
from tests import sched_stress as ss

CHAIN, WGRAD, COPY = 0x1000, 0x2000, 0x3000
HANDLES = {'chain': CHAIN, 'wgrad': WGRAD, 'copy': COPY}


class _FakeLib:
    """Every entry point returns 0 and is recorded."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('bdn_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return b'' if name == 'bdn_last_error' else 0
        return fn


def _args(name, stream):
    """Dummy arguments of the right count; the stream last."""
    n = len(_lib.SIGNATURES[name][1])
    return (0,) * (n - 1) + (stream,)


# one backward-like exchange: chain work, hand-off, a GEMM on the second stream, a copy, the join, more chain work
SCRIPT = [
    ('bdn_outc_bwd', CHAIN),                 # 0
    ('bdn_bn_bwd_finalize', CHAIN),          # 1
    ('bdn_event_record', None),              # hand-off chain -> wgrad (ignored)
    ('bdn_stream_wait_event', None),
    ('bdn_conv3x3_wgrad_ex', WGRAD),         # 2
    ('bdn_conv3x3', CHAIN),                  # 3
    ('bdn_upload_band', COPY),               # 4
    ('bdn_conv3x3_wgrad_ex', WGRAD),         # 5
    ('bdn_bn_bwd', CHAIN),                   # 6
    ('bdn_conv3x3_wgrad_ex', WGRAD),         # 7
    ('bdn_event_record', None),              # the join
    ('bdn_stream_wait_event', None),
    ('bdn_sgd_step', CHAIN),                 # 8
    ('bdn_conv3x3_num_mtiles', None),        # a query without a stream (never goes through call() in the product; ignored all the same)
]
N_LAUNCHES = 9


def _play():
    for name, stream in SCRIPT:
        if name == 'bdn_event_record':
            _lib.call(name, 0x77, WGRAD)
        elif name == 'bdn_stream_wait_event':
            _lib.call(name, WGRAD, 0x77)
        elif stream is None:
            _lib.call(name, *((0,) * len(_lib.SIGNATURES[name][1])))
        else:
            _lib.call(name, *_args(name, stream))


@pytest.fixture
def fake(monkeypatch):
    lib = _FakeLib()
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    monkeypatch.setattr(_lib, 'SKIP', None)
    return lib


def _run(pattern, fake, short=10, long=1000):
    slept, syncs = [], []
    h = ss.Perturb(pattern, short, long, sleep=lambda s, c: slept.append((s, c)), synchronize=lambda: syncs.append(len(fake.calls)),
                   handle_of=lambda r: HANDLES.get(r, r))
    n0 = len(fake.calls)
    with h:
        _play()
    assert _lib.SKIP is None
    assert [c[0] for c in fake.calls[n0:]] == [s[0] for s in SCRIPT], 'a launch was dropped or reordered'
    assert sum(h.launches.values()) == h.n == N_LAUNCHES
    assert h.launches == {CHAIN: 5, WGRAD: 3, COPY: 1}
    assert [(s, c) for _, _, s, c in h.log] == slept
    return h, slept, syncs


def test_none_and_sync(fake):
    h, slept, syncs = _run(ss.none(), fake)
    assert slept == [] and syncs == [] and h.log == []
    h, slept, syncs = _run(ss.sync(), fake)
    assert slept == [] and len(syncs) == N_LAUNCHES          # one synchronisation in front of every launch, none for events or queries
    # the synchronisation comes BEFORE its launch: the number of library calls made so far, per launch
    n0 = syncs[0]
    assert [s - n0 for s in syncs] == [0, 1, 4, 5, 6, 7, 8, 9, 12]


@pytest.mark.parametrize('role, idx', [('wgrad', [2, 5, 7]), ('chain', [0, 1, 3, 6, 8]), ('copy', [4]), (WGRAD, [2, 5, 7])])
def test_lag_delays_every_launch_of_its_stream_and_no_other(fake, role, idx):
    h, slept, _ = _run(ss.lag(role), fake)
    want = HANDLES.get(role, role)
    assert [i for i, _, _, _ in h.log] == idx
    assert slept == [(want, 10)] * len(idx)


@pytest.mark.parametrize('role, k, idx', [('wgrad', 0, 2), ('wgrad', 2, 7), ('chain', 0, 0), ('chain', 3, 6), ('copy', 0, 4)])
def test_stall_delays_the_kth_launch_of_its_stream_once(fake, role, k, idx):
    h, slept, _ = _run(ss.stall(role, k), fake)
    assert [(i, s, c) for i, _, s, c in h.log] == [(idx, HANDLES[role], 1000)]
    assert h.log[0][1] == [s for s in SCRIPT if s[1] is not None][idx][0]


def test_stall_beyond_the_last_launch_delays_nothing(fake):
    h, slept, _ = _run(ss.stall('wgrad', 3), fake)
    assert slept == [] and h.log == []


def test_random_is_seeded(fake):
    a = _run(ss.random(1, 0.5), fake)[0].log
    b = _run(ss.random(1, 0.5), fake)[0].log
    c = _run(ss.random(2, 0.5), fake)[0].log
    assert a == b and a != c
    assert 0 < len(a) < N_LAUNCHES and all(cy == 10 for _, _, _, cy in a)
    own = [x[1] for x in SCRIPT if x[1] is not None]          # launch index -> the stream it goes to
    assert all(s == own[i] for i, _, s, _ in a), 'slept on another stream than the launch'
    assert _run(ss.random(3, 0.0), fake)[0].log == []
    assert len(_run(ss.random(3, 1.0), fake)[0].log) == N_LAUNCHES


def test_stream_and_event_entry_points_are_ignored(fake):
    for name in _lib.SIGNATURES:
        if name.startswith(('bdn_stream_', 'bdn_event_')):
            assert not ss.takes_stream(name), name
    assert ss.takes_stream('bdn_conv3x3') and ss.takes_stream('bdn_upload_band') and ss.takes_stream('bdn_sgd_step')
    assert not ss.takes_stream('bdn_conv3x3_num_mtiles') and not ss.takes_stream('bdn_wgrad_workspace_bytes')
    slept = []
    with ss.Perturb(ss.random(0, 1.0), 10, 1000, sleep=lambda s, c: slept.append(s), handle_of=lambda r: r) as h:
        _lib.call('bdn_event_record', 0x77, WGRAD)
        _lib.call('bdn_stream_wait_event', CHAIN, 0x77)
        _lib.call('bdn_stream_destroy', WGRAD)
    assert slept == [] and h.n == 0 and h.launches == {}
    assert [c[0] for c in fake.calls[-3:]] == ['bdn_event_record', 'bdn_stream_wait_event', 'bdn_stream_destroy']


def test_head_sleeps_come_first_and_once_per_stream(fake):
    slept = []
    class _Mark:                                  # the heads run out after the sixth library call
        def query(self):
            return len(fake.calls) - n0 >= 6
    h = ss.Perturb(ss.lag('wgrad', queued=True), 10, 1000, head=500, head_roles=('chain', 'wgrad', WGRAD, 'copy'),
                   sleep=lambda s, c: slept.append((s, c, len(fake.calls))), handle_of=lambda r: HANDLES.get(r, r), mark=lambda s: _Mark())
    n0 = len(fake.calls)
    with h:
        _play()
    assert slept[:3] == [(CHAIN, 500, n0), (WGRAD, 500, n0), (COPY, 500, n0)]          # before the first library call, the duplicate role once
    assert [(s, c) for s, c, _ in slept[3:]] == [(WGRAD, 10)] * 3 and len(h.log) == 3   # then the pattern's own sleeps; the log holds only those
    assert h.queued == [True] * 4 + [False] * 5                # launches 0-3 are library calls 0, 1, 4, 5
    slept.clear()
    for pat, head in ((ss.none(queued=True), 0), (ss.none(), 500), (ss.stall('copy', 9), 500)):      # no length, or a pattern that is not queued
        with ss.Perturb(pat, 10, 1000, head=head, head_roles=('chain',), sleep=lambda s, c: slept.append(s), handle_of=HANDLES.get, mark=None) as h:
            _play()
        assert h.queued == []
    assert slept == []
    assert repr(ss.lag('wgrad', queued=True)) == "lag('wgrad') queued" and repr(ss.none(queued=True)) == 'none queued'


def test_hook_is_restored_after_an_exception(fake):
    with pytest.raises(ZeroDivisionError):
        with ss.Perturb(ss.lag('wgrad'), 10, 1000, sleep=lambda s, c: None, handle_of=HANDLES.get):
            assert _lib.SKIP is not None
            1 / 0
    assert _lib.SKIP is None
    with ss.Perturb(ss.none(), handle_of=HANDLES.get):
        with pytest.raises(RuntimeError, match='SKIP is taken'):
            with ss.Perturb(ss.none(), handle_of=HANDLES.get):
                pass
        assert _lib.SKIP is not None                     # the refused inner context left the outer hook in place
    assert _lib.SKIP is None


def test_the_hook_never_returns_a_value_that_drops_a_launch(fake):
    pats = [ss.sync(), ss.none(), ss.lag('wgrad'), ss.lag('chain'), ss.stall('wgrad', 1), ss.stall('copy', 0), ss.random(5, 0.5)]
    for pat in pats:
        h = ss.Perturb(pat, 10, 1000, sleep=lambda s, c: None, synchronize=lambda: None, handle_of=lambda r: HANDLES.get(r, r))
        with h:
            for name in _lib.SIGNATURES:
                n = len(_lib.SIGNATURES[name][1])
                for stream in (CHAIN, WGRAD, 0, None):
                    assert h._hook(name, (0,) * max(n - 1, 0) + ((stream,) if n else ())) is False, (pat, name)


def test_pattern_arguments_and_names():
    assert repr(ss.lag('wgrad')) == "lag('wgrad')" and repr(ss.stall('chain', 3)) == "stall('chain', 3)"
    assert repr(ss.random(7, 0.25)) == 'random(7, 0.25)' and repr(ss.sync()) == 'sync' and repr(ss.none()) == 'none'
    with pytest.raises(ValueError):
        ss.stall('wgrad', -1)
    with pytest.raises(ValueError):
        ss.random(0, 1.5)
