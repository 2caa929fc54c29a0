"""Guard-banded test buffers: the only instrument this suite has for WHERE a kernel reads and writes.

A guarded tensor is the middle of its own uint8 allocation, [guard | payload | guard].  Every guard byte is 0xFF: NaN as float32, bf16 and
float64, -1 as int32, 255 as uint8 -- a guard value that is read and used poisons the result, and a write into a guard is visible byte for
byte.  Each guard holds max(64 KiB, one leading-dimension slice of the tensor) bytes, rounded up to 256: one image / filter row / partial
row is the largest unit any kernel indexes by (and covers the missing second image of a two-image tile), 64 KiB exceeds the largest chunk
a kernel stages at once (the weight-gradient ring buffer is 40 KiB, one wave instruction moves 1 KiB).  These are conditions of the test,
not measurements.  Payloads start 256-byte aligned (no alignment torch would not give) and END where their last byte ends: a workspace
allocated from a size query is guarded at exactly that many bytes.  Fresh payloads (`empty`) are 0xFF as well, so a partial that is read
before it is written shows up as NaN.

`@guarded` on a test wraps fabric_amd._lib.call for the test's duration: every void* argument of every entry point (found from
_lib.SIGNATURES) other than None, the trailing stream and the documented host pointers must lie inside the payload of a guarded tensor
made during the test, and after the body every guard byte must still be 0xFF.

Everything takes device= so tests/test_guarded_cpu.py can prove the guard itself on the CPU.
"""
import ctypes
import functools
import math

import torch

from fabric_amd import _lib

GUARD_MIN = 64 * 1024
ALIGN = 256
FILL = 0xFF

# void* arguments that are HOST memory by contract (include/bidate_hip.h), by 0-based position
HOST_ARGS = {
    'bdn_sample_patches': (1, 4),                   # city_hw_host, desc_host
    'bdn_upload_band': (1,),                        # src_planes_host
    'bdn_sgd_step_grouped': (6,),                   # lr
    'bdn_sgd_momentum_step_grouped': (7, 8),        # lr, weight_decay
    'bdn_adam_step_grouped': (8, 9),                # lr, weight_decay
}
NOT_MEMORY = ('bdn_stream_', 'bdn_event_')          # their void* are stream / event handles

_REG = None          # list of _Rec while a @guarded test runs


class GuardError(AssertionError):
    pass


class _Rec:
    __slots__ = ('base', 'off', 'nbytes', 'label', 'start')

    def __init__(self, base, off, nbytes, label):
        self.base, self.off, self.nbytes, self.label = base, off, nbytes, label
        self.start = base.data_ptr() + off


def _up(n, a):
    return (n + a - 1) // a * a


def guard_bytes(shape, itemsize):
    """Bytes of each guard of a tensor of this shape: max(64 KiB, one leading-dimension slice), rounded up to 256."""
    lead = itemsize * math.prod(shape[1:]) if len(shape) else itemsize
    return _up(max(GUARD_MIN, lead), ALIGN)


def alloc(shape, dtype=torch.float32, device='cuda', label=None, guard_shape=None):
    """Guarded contiguous tensor whose payload is 0xFF bytes (guard_shape: the shape that sizes the guards, when it is not `shape`)."""
    shape = tuple(int(s) for s in shape)
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = es * math.prod(shape)
    g = guard_bytes(tuple(guard_shape) if guard_shape is not None else shape, es)
    base = torch.full((g + ALIGN + nbytes + g,), FILL, dtype=torch.uint8, device=device)
    off = g + (-(base.data_ptr() + g)) % ALIGN
    rec = _Rec(base, off, nbytes, label or f'{str(dtype).replace("torch.", "")}{list(shape)}')
    if _REG is not None:
        _REG.append(rec)
    return base[off:off + nbytes].view(dtype).view(shape)


def alloc_bytes(nbytes, device='cuda', label=None):
    """Workspace / scratch of exactly the byte count a size query returned, rounded up to 16 bytes only; uint8, 0xFF-filled."""
    return alloc((_up(int(nbytes), 16),), torch.uint8, device, label or f'workspace[{int(nbytes)} B]')


def guard(t, device='cuda', label=None):
    """Copy of `t` (any device) in a guarded allocation on `device`; what `t.cuda()` gives, strides of a dense permuted tensor included."""
    if t.is_contiguous():
        out = alloc(t.shape, t.dtype, device, label)
    else:
        out = alloc((t.numel(),), t.dtype, device, label or f'{str(t.dtype).replace("torch.", "")}{list(t.shape)}',
                    guard_shape=t.shape).as_strided(t.shape, torch.empty_like(t).stride())
    out.copy_(t)
    return out


def _shape(size):
    return tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)


def empty(*size, dtype=torch.float32, device='cuda', label=None):
    return alloc(_shape(size), dtype or torch.float32, device, label)


def full(size, fill_value, dtype=None, device='cuda', label=None):
    dtype = dtype or torch.full((), fill_value).dtype
    return alloc((size,) if isinstance(size, int) else tuple(size), dtype, device, label).fill_(fill_value)


def zeros(*size, dtype=torch.float32, device='cuda', label=None):
    return alloc(_shape(size), dtype or torch.float32, device, label).zero_()


def _like(t, dtype, device):
    return alloc(t.shape, dtype or t.dtype, device or t.device)


def empty_like(t, dtype=None, device=None):
    return _like(t, dtype, device)


def full_like(t, fill_value, dtype=None, device=None):
    return _like(t, dtype, device).fill_(fill_value)


def zeros_like(t, dtype=None, device=None):
    return _like(t, dtype, device).zero_()


def clone(t):
    return guard(t, t.device)


# ---------------------------------------------------------------- channel slices of a wider tensor
def wide_input(t, ld, off, device='cuda', label=None):
    """[..., C] tensor `t` placed at channels [off, off + C) of a guarded [..., ld] tensor whose foreign channels are 0xFF (NaN): a kernel
    that reads outside its slice and uses the value poisons its result.  Returns (wide, view of the slice)."""
    C = t.shape[-1]
    assert 0 <= off and off + C <= ld
    wide = alloc(tuple(t.shape[:-1]) + (ld,), t.dtype, device, label)
    wide[..., off:off + C].copy_(t)
    return wide, wide[..., off:off + C]


def assert_foreign_untouched(wide, owned, name='slice'):
    """Every byte of the 0xFF-filled output `wide` outside the channel ranges `owned` = [(off, C), ...] of its last dimension still holds 0xFF."""
    es = wide.element_size()
    keep = torch.ones(wide.shape[-1] * es, dtype=torch.bool, device=wide.device)
    for off, C in owned:
        keep[off * es:(off + C) * es] = False
    b = wide.contiguous().view(torch.uint8).reshape(-1, wide.shape[-1] * es)
    n = int((b[:, keep] != FILL).sum().item())
    if n:
        raise GuardError(f'{name}: {n} bytes of the foreign channels (outside {list(owned)} of {wide.shape[-1]}) were overwritten')


# ---------------------------------------------------------------- the check
def _changed(rec):
    """[(side, count, first, last)] of the guard bytes of `rec` that are no longer 0xFF; offsets relative to the payload (left: negative,
    from its first byte; right: from the first byte after it)."""
    out = []
    end = rec.off + rec.nbytes
    for side, part, origin in (('left', rec.base[:rec.off], rec.off), ('right', rec.base[end:], end)):
        bad = part != FILL
        if bool(bad.any().item()):
            idx = bad.nonzero().flatten()
            first, last = int(idx[0].item()) - (origin if side == 'left' else 0), int(idx[-1].item()) - (origin if side == 'left' else 0)
            out.append((side, int(idx.numel()), first, last))
    return out


def check_guards(records):
    """Raise GuardError naming every tensor whose guard bytes changed."""
    if not records:
        return
    # one reduction per tensor, one host round trip for all of them
    dirty = torch.stack([(r.base[:r.off] != FILL).any() | (r.base[r.off + r.nbytes:] != FILL).any() for r in records]).tolist()
    msgs = []
    for r, d in zip(records, dirty):
        if d:
            for side, n, first, last in _changed(r):
                msgs.append(f'{r.label}: {side} guard, {n} bytes changed, offsets {first:+d} .. {last:+d} relative to the payload '
                            f'{"start" if side == "left" else "end"} ({r.nbytes} payload bytes)')
    if msgs:
        raise GuardError('guard bytes overwritten:\n  ' + '\n  '.join(msgs))


def _addr(a):
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    if isinstance(a, (ctypes.Array, ctypes.Structure)):
        return ctypes.addressof(a)
    return int(a)


def check_pointers(name, args, records):
    """Every device void* of this call lies inside the payload of a guarded tensor."""
    if name.startswith(NOT_MEMORY):
        return
    argtypes = _lib.SIGNATURES[name][1]
    host = HOST_ARGS.get(name, ())
    last = len(argtypes) - 1
    for i, (ty, a) in enumerate(zip(argtypes, args)):
        if ty is not ctypes.c_void_p or i == last or i in host or a is None:
            continue
        p = _addr(a)
        if p == 0:
            continue
        if not any(r.start <= p < r.start + r.nbytes or (r.nbytes == 0 and p == r.start) for r in records):
            raise GuardError(f'{name}: argument {i} ({p:#x}) is not inside a guarded tensor of this test')


class Session:
    """What @guarded opens: the registry, and _lib.call wrapped with the pointer check."""

    def __init__(self, test_globals=None):
        self.test_globals = test_globals          # a test module that did `from fabric_amd._lib import call` holds its own binding

    def __enter__(self):
        global _REG
        assert _REG is None, 'guarded sessions do not nest'
        self.records = _REG = []
        self.calls = 0
        self.real = _lib.call

        def call(name, *args):
            check_pointers(name, args, self.records)
            self.calls += not name.startswith(NOT_MEMORY)          # stream / event handles: no kernel, nothing to guard
            return self.real(name, *args)
        self.wrapper = call
        _lib.call = call
        self.rebound = self.test_globals is not None and self.test_globals.get('call') is self.real
        if self.rebound:
            self.test_globals['call'] = call
        return self

    def __exit__(self, et, ev, tb):
        global _REG
        _REG = None
        if _lib.call is self.wrapper:
            _lib.call = self.real
        if self.rebound and self.test_globals.get('call') is self.wrapper:
            self.test_globals['call'] = self.real
        return False


class checked(Session):
    """A Session that, when its block ends without an error, synchronizes, requires every guard byte to be 0xFF still and at least one
    library call on memory.  What @guarded opens around a whole test; a test that also runs code which allocates for itself (a model,
    the engine) opens it around its direct library calls only."""

    def __init__(self, test_globals=None, name='guarded block'):
        super().__init__(test_globals)
        self.name = name

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                if any(r.base.is_cuda for r in self.records):
                    torch.cuda.synchronize()
                check_guards(self.records)
                assert self.calls > 0, f'{self.name}: made no library call'
        finally:
            super().__exit__(et, ev, tb)
        return False


def guarded(fn):
    """Test decorator: run the body on guarded buffers only (see the module docstring).  functools.wraps keeps the signature pytest reads,
    so parametrization and fixtures work unchanged."""
    @functools.wraps(fn)
    def run(*args, **kwargs):
        with checked(fn.__globals__, fn.__name__):
            return fn(*args, **kwargs)
    return run
