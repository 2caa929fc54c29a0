"""-m gpu: the averaging kernels of the fused step (include/bidate_hip.h bdn_ema_update, bdn_ema_update_multi, bdn_swap_segments) on
guard-banded buffers (tests/guard.py), against the float64 restatement tests/ema_ref.py (pinned against CPU AveragedModel in
tests/test_ema_cpu.py).

Sizes: one vector, the block's 256-vector edge, and several passes of a thread (4 * 256 * k +- 4 floats for k = 1, 16).  Segment tables:
none, 1, 3 and 256 segments, boundaries at vectors 1, 255, 256 and 257, a frozen segment first, in the middle and last, and a table that
ends before n / 4.  A vector that does not count -- frozen, or behind the table's end -- keeps its bits in both buffers even when the other
buffer holds NaN or inf there."""
import struct

import pytest
import torch

from fabric_amd import _lib
from tests import ema_ref as R
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
NAN, INF = float('nan'), float('inf')

_SIZES = [4, 1020, 1028, 4 * 256 * 16 - 4, 4 * 256 * 16 + 4]
_WEIGHTS = [0.0, 1e-3, 0.25, 0.5, 0.999, 1.0]


def _tables(n4):
    """[(name, ends, ids)] of the segment tables that fit n4 vectors; ends in float4 units, ids -1 = frozen."""
    out = [('none', [], []), ('one', [n4], [0]), ('one_frozen', [n4], [-1])]
    if n4 >= 2:
        out.append(('short', [n4 // 2], [3]))                                     # ends before n / 4: the rest is not touched
    for a, b in ((1, 255), (255, 256), (256, 257), (1, 257)):
        if b < n4:
            out += [(f'frozen_first_{a}_{b}', [a, b, n4], [-1, 0, 1]), (f'frozen_mid_{a}_{b}', [a, b, n4], [0, -1, 7]),
                    (f'frozen_last_{a}_{b}', [a, b, n4], [2, 0, -1])]
    if n4 >= 257:
        # 256 segments: one vector each up to 255, the rest in the last; every third one frozen, one id outside 0..7 (skipped like frozen)
        ids = [-1 if k % 3 == 1 else k % 8 for k in range(256)]
        ids[7] = 9
        out.append(('256_segments', list(range(1, 256)) + [n4], ids))
        out.append(('256_short', list(range(1, 256)) + [n4 - 1], ids[:255] + [0]))
    return out


def _counts(n4, ends, ids):
    """bool [4 * n4]: the elements of the vectors that count."""
    m = torch.zeros(n4, dtype=torch.bool)
    if not ends:
        m[:] = True
    lo = 0
    for e, g in zip(ends, ids):
        if 0 <= g < 8:
            m[lo:e] = True
        lo = e
    return m.repeat_interleave(4)


def _table_args(ends, ids):
    if not ends:
        return None, None, 0
    return (guard.guard(torch.tensor(ends, dtype=torch.int64).to(torch.int32), dev).data_ptr(),
            guard.guard(torch.tensor(ids, dtype=torch.int32), dev).data_ptr(), len(ends))


def _bits(t):
    return t.detach().cpu().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _pair(n, seed, counts, poison):
    """Random (avg, params) on the host; where a vector does not count, one of the two buffers holds NaN / inf."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    avg, p = torch.randn(n, generator=g), torch.randn(n, generator=g)
    avg[::7] *= 1e-3
    p[::5] *= 1e3
    if poison == 'params':
        p[~counts] = NAN
    elif poison == 'avg':
        avg[~counts] = INF
    return avg, p


@pytest.mark.parametrize('w', _WEIGHTS)
@pytest.mark.parametrize('n', _SIZES)
@guarded
def test_ema_update_matches_float64_restatement(n, w):
    """Every table: the vectors that count are within R.ULPS of the restatement (w = 0 and w = 1: avg's and the parameters' bits), the
    others keep their bits in both buffers, the parameters are never written, and a second run from the same inputs gives the same bits."""
    st = _lib.stream_ptr()
    for ti, (name, ends, ids) in enumerate(_tables(n // 4)):
        counts = _counts(n // 4, ends, ids)
        avg0, p0 = _pair(n, n * 13 + ti, counts, ('params', 'avg')[ti % 2])
        tab = _table_args(ends, ids)
        runs = []
        for _ in range(2):
            avg, p = guard.guard(avg0, dev), guard.guard(p0, dev)
            _lib.call('bdn_ema_update', avg.data_ptr(), p.data_ptr(), *tab, w, 0, n, st)
            runs.append((avg, p))
        torch.cuda.synchronize()
        avg, p = runs[0]
        what = f'n={n} w={w} table {name}'
        assert _same_bits(p, p0), f'{what}: the parameters were written'
        assert _same_bits(avg.cpu()[~counts], avg0[~counts]), f'{what}: a vector that does not count changed'
        if counts.any():
            ref, mag = R.lerp(avg0[counts], p0[counts], w)
            R.check(avg.cpu()[counts], ref, mag, what)
            if w == 0.0:
                assert _same_bits(avg.cpu()[counts], avg0[counts]), f'{what}: w = 0 must leave the average\'s bits'
            elif w == 1.0:
                assert _same_bits(avg.cpu()[counts], p0[counts]), f'{what}: w = 1 must give the parameters\' bits'
            else:
                assert bool((avg.cpu()[counts] != avg0[counts]).any()), f'{what}: nothing moved'
        assert _same_bits(runs[0][0], runs[1][0]), f'{what}: repeat run differs'


@pytest.mark.parametrize('n', _SIZES)
@guarded
def test_ema_copy_is_bit_exact(n):
    """copy = 1: avg = params bit for bit where a vector counts (NaN payloads and -0 included), whatever the weight; nothing elsewhere."""
    st = _lib.stream_ptr()
    for ti, (name, ends, ids) in enumerate(_tables(n // 4)):
        counts = _counts(n // 4, ends, ids)
        avg0, p0 = _pair(n, n * 17 + ti, counts, ('params', 'avg')[ti % 2])
        p0[counts.nonzero().flatten()[::11]] = -0.0
        if counts.any():
            i = int(counts.nonzero().flatten()[-1])
            p0.view(torch.int32)[i] = 0x7fc12345                                  # a NaN with a payload, in a vector that counts
        avg, p = guard.guard(avg0, dev), guard.guard(p0, dev)
        _lib.call('bdn_ema_update', avg.data_ptr(), p.data_ptr(), *_table_args(ends, ids), 0.25, 1, n, st)
        torch.cuda.synchronize()
        assert _same_bits(p, p0)
        assert _same_bits(avg.cpu()[counts], p0[counts]), f'n={n} table {name}: copy is not bit-exact'
        assert _same_bits(avg.cpu()[~counts], avg0[~counts]), f'n={n} table {name}: a vector that does not count changed'


@guarded
def test_bad_arguments_are_refused():
    a, b = guard.zeros(8, device=dev), guard.zeros(8, device=dev)
    desc = guard.zeros(24, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()
    for w in (-0.1, 1.5, NAN, INF):
        with pytest.raises(RuntimeError, match=r'rc=-1'):
            _lib.call('bdn_ema_update', a.data_ptr(), b.data_ptr(), None, None, 0, w, 0, 8, st)
        with pytest.raises(RuntimeError, match=r'rc=-1'):
            _lib.call('bdn_ema_update_multi', desc.data_ptr(), 0, 0, w, 0, st)
    with pytest.raises(RuntimeError, match=r'rc=-1'):
        _lib.call('bdn_ema_update', a.data_ptr(), b.data_ptr(), None, None, 0, 0.5, 2, 8, st)              # copy is 0 or 1
    with pytest.raises(RuntimeError, match=r'rc=-1'):
        _lib.call('bdn_ema_update', a.data_ptr(), b.data_ptr(), None, None, 0, 0.5, 0, 6, st)              # n is a multiple of 4
    with pytest.raises(RuntimeError, match=r'rc=-1'):
        _lib.call('bdn_ema_update', a.data_ptr() + 4, b.data_ptr(), None, None, 0, 0.5, 0, 4, st)          # 16-byte alignment
    with pytest.raises(RuntimeError, match=r'rc=-1'):
        _lib.call('bdn_ema_update', a.data_ptr(), b.data_ptr(), None, None, 257, 0.5, 0, 8, st)            # at most 256 segments
    with pytest.raises(RuntimeError, match=r'rc=-1'):
        _lib.call('bdn_swap_segments', a.data_ptr(), a.data_ptr(), None, None, 0, 8, st)
    _lib.call('bdn_ema_update', a.data_ptr(), b.data_ptr(), None, None, 0, 0.5, 0, 0, st)                  # n = 0: nothing to do
    torch.cuda.synchronize()
    assert not bool(a.any()) and not bool(b.any())


_LENS = [1, 3, 64, 512, 513]


@pytest.mark.parametrize('w,copy', [(0.25, 0), (0.999, 0), (0.0, 0), (1.0, 0), (0.25, 1)])
@guarded
def test_ema_update_multi(w, copy):
    """Five tensors of lengths 1, 3, 64, 512 and 513 in one launch, the average of the 512-element one 4 bytes off a float4 (its first
    element belongs to nobody and must keep its bits).  Each guarded allocation ends with its tensor, so a write past a length shows."""
    g = torch.Generator(device='cpu').manual_seed(int(w * 1000) + copy)
    host, devt, rec = [], [], b''
    for n in _LENS:
        a0, s0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
        off = 1 if n == 512 else 0
        a = guard.guard(torch.cat([torch.full((off,), NAN), a0]), dev)
        s = guard.guard(s0, dev)
        host.append((a0, s0, off))
        devt.append((a, s))
        rec += struct.pack('<QQii', a.data_ptr() + 4 * off, s.data_ptr(), n, 0)
    desc = guard.guard(torch.frombuffer(bytearray(rec), dtype=torch.uint8), dev)
    _lib.call('bdn_ema_update_multi', desc.data_ptr(), len(_LENS), max(_LENS), w, copy, _lib.stream_ptr())
    torch.cuda.synchronize()
    for (a0, s0, off), (a, s) in zip(host, devt):
        what = f'multi w={w} copy={copy} len={a0.numel()}'
        got = a.cpu()
        assert _same_bits(s, s0), f'{what}: the source was written'
        if off:
            assert bool(got[:off].isnan().all()), f'{what}: the element in front of the tensor was written'
        got = got[off:]
        if copy or w == 1.0:
            assert _same_bits(got, s0), what
        elif w == 0.0:
            assert _same_bits(got, a0), what
        else:
            ref, mag = R.lerp(a0, s0, w)
            R.check(got, ref, mag, what)
            assert bool((got != a0).all()), f'{what}: an element did not move'


@pytest.mark.parametrize('n', _SIZES)
@guarded
def test_swap_segments(n):
    """Applied once, a and b exchange exactly the vectors that count (the others keep their bits, NaN / inf in the other buffer or not);
    applied twice it is the identity, bit for bit."""
    st = _lib.stream_ptr()
    for ti, (name, ends, ids) in enumerate(_tables(n // 4)):
        counts = _counts(n // 4, ends, ids)
        a0, b0 = _pair(n, n * 19 + ti, counts, ('params', 'avg')[ti % 2])
        a, b = guard.guard(a0, dev), guard.guard(b0, dev)
        tab = _table_args(ends, ids)
        _lib.call('bdn_swap_segments', a.data_ptr(), b.data_ptr(), *tab, n, st)
        a1, b1 = a.clone(), b.clone()
        _lib.call('bdn_swap_segments', a.data_ptr(), b.data_ptr(), *tab, n, st)
        torch.cuda.synchronize()
        what = f'swap n={n} table {name}'
        assert _same_bits(a1, torch.where(counts, b0, a0)) and _same_bits(b1, torch.where(counts, a0, b0)), f'{what}: once'
        assert _same_bits(a, a0) and _same_bits(b, b0), f'{what}: twice is not the identity'
