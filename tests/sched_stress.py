"""Launch-perturbation harness: the instrument this suite has for WHEN a kernel runs.

Every result of the training and inference paths is bit-reproducible (fixed-order reductions, no float atomics), and the multi-stream
schedule around the kernels (fabric_amd/engine.py backward, train_step.py, utils/inference.py, input_pipeline.py) orders every
cross-stream reader behind its writer with events.  If that is true, no change of when launches START can change a bit.  The harness
changes when they start: `Perturb(pattern)` is a context manager that installs a callable in `fabric_amd._lib.SKIP`, the hook
`_lib.call` consults before every launch (product modules import `call` by name, so the seam has to be inside it).  The callable
enqueues a sleep kernel on the launch's OWN stream (the last argument of every entry point that takes one) and returns False, so no
launch is ever dropped.  It creates no stream (new streams would shift the hardware-queue mapping fabric_amd/streams.py arranged), sets
no environment variable, and ignores bdn_stream_*, bdn_event_* and entry points without a stream argument.

Patterns (all deterministic):
  sync()            torch.cuda.synchronize() before every library launch: race-free by construction, the ground truth of every subject
  none()            the natural schedule
  lag(role)         a short sleep before every launch on that role's stream
  stall(role, k)    one long sleep before the k-th launch (0-based) on that role's stream
  random(seed, p)   a short sleep before each launch, on whatever stream, with probability p (one seeded generator per context)

queued=True on none / lag / stall / random, with Perturb(head=cycles, head_roles=(...)): one sleep of that length on each of those streams when
the context opens, before the subject enqueues anything.  At test shapes the HOST paces the launches (tens of microseconds each, as long as the kernels), every kernel starts when it
is enqueued and no queue ever forms, so a lagging stream catches up between two launches; behind a head sleep as long as the subject
takes to enqueue, the streams start on full queues and run at the device's pace, which is the regime of the full-size step (the host
runs a step ahead there) and the one the lag pattern is designed for.

A role is a name of fabric_amd/streams.py ('wgrad', 'chain', 'copy', 'copy2'), or a stream / raw handle (a scene lane, the caller's
stream).  The short and long sleep lengths come from the caller, who measures them (tests/test_gpu_sched_stress.py).

`probe=(chain, wgrad)`: the harness also watches the hand-off entry points (it never delays them) and records timing events, so that a
test can tell whether a perturbation moved the schedule at all (`Perturb.join_lag_us`, `Perturb.idle_before_launch`).

The sleep, the device synchronisation and the stream lookup are injectable so that tests/test_sched_stress_cpu.py can pin the harness
without a device.
"""
import random as _random

from fabric_amd import _lib

IGNORED = ('bdn_stream_', 'bdn_event_')          # their void* are stream / event handles: never delayed


class Pattern:
    __slots__ = ('kind', 'role', 'k', 'seed', 'p', 'queued')

    def __init__(self, kind, role=None, k=None, seed=None, p=None, queued=False):
        self.kind, self.role, self.k, self.seed, self.p, self.queued = kind, role, k, seed, p, bool(queued)

    def __repr__(self):
        q = ' queued' if self.queued else ''
        if self.kind == 'lag':
            return f'lag({self.role!r}){q}'
        if self.kind == 'stall':
            return f'stall({self.role!r}, {self.k}){q}'
        if self.kind == 'random':
            return f'random({self.seed}, {self.p}){q}'
        return self.kind + q


def sync():
    return Pattern('sync')


def none(queued=False):
    return Pattern('none', queued=queued)


def lag(role, queued=False):
    return Pattern('lag', role=role, queued=queued)


def stall(role, k, queued=False):
    if k < 0:
        raise ValueError('stall: k counts launches from 0')
    return Pattern('stall', role=role, k=int(k), queued=queued)


def random(seed, p, queued=False):
    if not 0.0 <= p <= 1.0:
        raise ValueError('random: p is a probability')
    return Pattern('random', seed=int(seed), p=float(p), queued=queued)


def takes_stream(name):
    """Is `name` a launch the harness may delay: an entry point whose last argument is a stream, and not a stream / event call."""
    args = _lib.SIGNATURES[name][1]
    return bool(args) and args[-1] is _lib._vp and not name.startswith(IGNORED)


_ext = {}


def _torch_stream(handle):
    """The torch stream object of a raw handle, cached per handle (as _lib._profiled does): never a new stream."""
    import torch
    st = _ext.get(handle)
    if st is None:
        st = _ext[handle] = torch.cuda.ExternalStream(handle) if handle else torch.cuda.default_stream()
    return st


def device_sleep(handle, cycles):
    """torch.cuda._sleep(cycles) enqueued on the stream `handle`."""
    import torch
    with torch.cuda.stream(_torch_stream(handle)):
        torch.cuda._sleep(int(cycles))


def device_mark(handle):
    """An event recorded on the stream `handle` now; .query() tells whether the stream has got past it."""
    import torch
    e = torch.cuda.Event()
    e.record(_torch_stream(handle))
    return e


def _device_sync():
    import torch
    torch.cuda.synchronize()


def role_handle(role):
    """Raw stream handle of a role: a name of fabric_amd.streams, a torch stream, or a handle (0 / None: the default stream)."""
    if isinstance(role, str):
        from fabric_amd import streams
        return streams.get(role).cuda_stream or 0
    if role is None:
        return 0
    return int(getattr(role, 'cuda_stream', role)) or 0


class Perturb:
    """with Perturb(pattern, short, long) as h: <enqueue the subject>.  `short` / `long`: sleep lengths in _sleep cycles.
    h.log: (launch index, entry point, stream handle, cycles slept before it) of every launch that was delayed;
    h.launches: {stream handle: launches seen on it} and h.trace: every launch in order, both kept under every pattern.
    h.queued: for a queued pattern, per launch, whether the head sleep of its stream was still running when the launch was enqueued (a
    host synchronisation inside the subject waits the heads out: then no queue forms and the list says so).
    Refuses to nest and to displace another SKIP hook; restores the hook on exit, also when the body raises."""

    def __init__(self, pattern, short=0, long=0, probe=None, head=0, head_roles=(), sleep=device_sleep, synchronize=_device_sync,
                 handle_of=role_handle, mark=device_mark):
        self.pattern, self.short, self.long = pattern, int(short), int(long)
        self.head, self.head_roles, self._mark_head = int(head), tuple(head_roles), mark
        self._heads = {}                         # stream handle -> event behind its head sleep
        self.queued = []                         # per launch on a stream with a head: was the head still running when it was enqueued?
        self._sleep, self._sync, self._handle_of = sleep, synchronize, handle_of
        self._probe_roles = probe
        self.log, self.launches, self.n = [], {}, 0
        self.trace = []                          # (entry point, stream handle) of every launch seen, in order
        self._target = None
        self._rng = _random.Random(pattern.seed) if pattern.kind == 'random' else None
        self._probe = None
        self.handoffs, self.joins = [], []

    # ------------------------------------------------------------------ the hook
    def __enter__(self):
        if _lib.SKIP is not None:
            raise RuntimeError('sched_stress: fabric_amd._lib.SKIP is taken (a nested Perturb, or a diagnostic tool)')
        if self.pattern.kind in ('lag', 'stall'):
            self._target = self._handle_of(self.pattern.role)
        if self._probe_roles is not None:
            self._open_probe()
        if self.head and self.pattern.queued:
            for h in dict.fromkeys(self._handle_of(r) for r in self.head_roles):      # once per stream, all before the first launch
                self._sleep(h, self.head)
                self._heads[h] = self._mark_head(h)
        _lib.SKIP = self._hook
        return self

    def __exit__(self, *exc):
        _lib.SKIP = None
        return False

    def _hook(self, name, args):
        if not takes_stream(name):
            if self._probe is not None and name.startswith('bdn_'):
                self._watch(name, args)
            return False
        h = args[-1] or 0
        k = self.launches.get(h, 0)
        self.launches[h] = k + 1
        self.trace.append((name, h))
        if h in self._heads:
            self.queued.append(not self._heads[h].query())
        kind, cycles = self.pattern.kind, 0
        if kind == 'sync':
            self._sync()
        elif kind == 'lag':
            cycles = self.short if h == self._target else 0
        elif kind == 'stall':
            cycles = self.long if h == self._target and k == self.pattern.k else 0
        elif kind == 'random':
            cycles = self.short if self._rng.random() < self.pattern.p else 0
        if cycles:
            self._sleep(h, cycles)
            self.log.append((self.n, name, h, cycles))
        self.n += 1
        return False          # never drop a launch

    # ------------------------------------------------------------------ did the perturbation move the schedule?  (engine.backward)
    def _open_probe(self):
        import torch
        chain, wgrad = (self._handle_of(r) for r in self._probe_roles)
        torch.cuda.synchronize()
        base = torch.cuda.Event(enable_timing=True)
        base.record(_torch_stream(chain))
        torch.cuda.synchronize()                  # the base precedes everything either stream runs inside the context
        self._probe = (chain, wgrad, base)

    def _mark(self, handle):
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record(_torch_stream(handle))
        return e

    def _watch(self, name, args):
        """Hand-offs of engine.backward seen from the hook, which runs BEFORE the call it is consulted for.
        chain -> wgrad: bdn_stream_wait_event(wgrad, ev).  An event on the second stream here closes that stream's work so far; one on
        the chain sits right behind the signal the wait refers to.  The second stream was idle before the launches that follow iff
        its event completed first.
        wgrad -> chain: bdn_event_record(ev, wgrad), a join.  An event on the second stream here is behind its last launch, one on
        the chain behind everything the chain enqueued before the join.  The FIRST join of a pass is the one that can be late: a pass
        that runs to the first layer joins behind that layer's weight gradient and again, with nothing in between, at its end."""
        chain, wgrad, _ = self._probe
        if name == 'bdn_stream_wait_event' and (args[0] or 0) == wgrad:
            self.handoffs.append((self.launches.get(chain, 0), self._mark(wgrad), self._mark(chain)))
        elif name == 'bdn_event_record' and (args[1] or 0) == wgrad:
            self.joins.append((self._mark(wgrad), self._mark(chain)))

    def join_lag_us(self, i=0):
        """Microseconds by which the second stream finished its last launch AFTER the chain finished everything it had enqueued before
        the i-th join (negative: the second stream was done first).  Call after a device synchronisation."""
        base = self._probe[2]
        side, chain = self.joins[i]
        return (base.elapsed_time(side) - base.elapsed_time(chain)) * 1e3

    def idle_before_launch(self):
        """[(chain launches enqueued before the hand-off, microseconds the second stream had been idle at it)] per chain -> wgrad
        hand-off, in order; negative: it was still busy, by so much, when the chain signalled."""
        base = self._probe[2]
        return [(n, (base.elapsed_time(chain) - base.elapsed_time(side)) * 1e3) for n, side, chain in self.handoffs]
