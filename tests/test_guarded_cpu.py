"""The guard itself (tests/guard.py), proved on the CPU: the same helpers with device='cpu' and plain torch operations through as_strided
views that stay inside the allocation.  Nothing here is a library kernel and nothing can fault; the library call is stubbed."""
import ctypes

import pytest
import torch

from fabric_amd import _lib
from tests import guard
from tests.guard import GuardError, guarded

CPU = 'cpu'


def _session():
    """An open registry without the decorator (the checks are called by hand)."""
    return guard.Session()


def _bytes_around(t, before, after):
    """uint8 view of `t`'s payload with `before` / `after` bytes of its guards on either side (inside the allocation)."""
    flat = t.reshape(-1).view(torch.uint8)
    return flat.as_strided((before + flat.numel() + after,), (1,), flat.storage_offset() - before)


def _make(dtype=torch.float32, shape=(3, 5, 7)):
    t = guard.zeros(*shape, dtype=dtype, device=CPU)
    return t, t.numel() * t.element_size()


def test_layout_alignment_and_guard_size():
    with _session() as s:
        t = guard.full((4, 8, 8, 64), 1.5, dtype=torch.bfloat16, device=CPU)
        big = guard.empty(2, 256, 256, 64, device=CPU)                      # one image = 16 MiB > 64 KiB
        r, rb = s.records
        assert t.data_ptr() % 256 == 0 and big.data_ptr() % 256 == 0
        assert r.off >= 64 * 1024 and r.base.numel() - r.off - r.nbytes >= 64 * 1024
        assert guard.guard_bytes((4, 8, 8, 64), 2) == 64 * 1024
        assert guard.guard_bytes((2, 256, 256, 64), 4) == 256 * 256 * 64 * 4
        assert guard.guard_bytes((1000,), 4) == 64 * 1024 and guard.guard_bytes((3, 100, 333), 2) % 256 == 0
        assert rb.off >= 256 * 256 * 64 * 4
        assert bool((r.base[:r.off] == 0xFF).all()) and bool((r.base[r.off + r.nbytes:] == 0xFF).all())
        assert torch.isnan(big).all()                                        # fresh payloads are 0xFF too
        ws = guard.alloc_bytes(1000, device=CPU)
        assert ws.numel() == 1008 and ws.dtype == torch.uint8 and bool((ws == 0xFF).all())
        guard.check_guards(s.records)


@pytest.mark.parametrize('where', ['one_before', 'one_after', 'far_left', 'far_right'])
def test_guard_check_catches_a_stray_write(where):
    with _session() as s:
        t, nb = _make()
        r = s.records[0]
        left, right = r.off, r.base.numel() - r.off - nb
        v = _bytes_around(t, left, right)
        pos = {'one_before': left - 1, 'one_after': left + nb, 'far_left': 0, 'far_right': left + nb + right - 1}[where]
        v[pos] = 0
        with pytest.raises(GuardError) as e:
            guard.check_guards(s.records)
        msg = str(e.value)
        side = 'left' if 'before' in where or 'left' in where else 'right'
        rel = pos - left if side == 'left' else pos - left - nb
        assert f'{side} guard, 1 bytes changed' in msg and f'{rel:+d} .. {rel:+d}' in msg and 'float32[3, 5, 7]' in msg


def test_guard_check_reports_count_first_and_last():
    with _session() as s:
        t, nb = _make(torch.int32, (10,))
        v = _bytes_around(t, 0, 100)
        v[nb + 3] = 1
        v[nb + 40:nb + 44] = 0
        with pytest.raises(GuardError, match=r'int32\[10\]: right guard, 5 bytes changed, offsets \+3 \.\. \+43'):
            guard.check_guards(s.records)


def test_clean_buffers_pass_and_payload_writes_are_free():
    with _session() as s:
        big = guard.guard(torch.zeros(2, 4, 200, 200).permute(0, 2, 3, 1), CPU)          # permuted: guards still sized by one leading slice
        assert s.records[0].off >= 4 * 200 * 200 * 4 and big.shape == (2, 200, 200, 4)
        t, _ = _make()
        t.fill_(float('nan'))
        u = guard.guard(torch.arange(24.0).reshape(2, 3, 4).permute(0, 2, 1), CPU)       # dense, permuted: strides kept like .cuda()
        assert u.stride() == (12, 1, 4) and torch.equal(u, torch.arange(24.0).reshape(2, 3, 4).permute(0, 2, 1))
        guard.check_guards(s.records)


def test_slice_foreign_channels():
    with _session():
        x = torch.arange(2 * 3 * 64, dtype=torch.float32).reshape(2, 3, 64)
        wide, sl = guard.wide_input(x, 128, 64, device=CPU)
        assert torch.equal(sl, x) and torch.isnan(wide[..., :64]).all()                 # a read of the foreign channels gives NaN
        wout = guard.empty(2, 3, 128, dtype=torch.bfloat16, device=CPU)
        wout[..., :32].copy_(x[..., :32])
        wout[..., 64:96].copy_(x[..., 32:])
        guard.assert_foreign_untouched(wout, [(0, 32), (64, 32)])
        wout[1, 2, 96] = 0.0                                                            # first foreign channel behind the second range
        with pytest.raises(GuardError, match='2 bytes of the foreign channels'):
            guard.assert_foreign_untouched(wout, [(0, 32), (64, 32)])


@pytest.mark.parametrize('dtype,seen', [(torch.float32, 'nan'), (torch.bfloat16, 'nan'), (torch.float64, 'nan'), (torch.int32, -1), (torch.uint8, 255)])
def test_a_read_one_element_past_the_end_is_poison(dtype, seen):
    with _session():
        t = guard.zeros(6, dtype=dtype, device=CPU)
        for over in (t.as_strided((7,), (1,)), t.as_strided((7,), (1,), t.storage_offset() - 1).flip(0)):     # one past the end / one before
            got = over[-1]
            assert torch.isnan(got) if seen == 'nan' else int(got) == seen
            if seen == 'nan':
                assert torch.isnan(over.double().sum())          # a use of the value poisons the result


# ---------------------------------------------------------------- the _lib.call wrapper, on a stubbed library
@pytest.fixture
def stub(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: seen.append(name))
    return seen


def test_wrapper_rejects_an_unguarded_pointer(stub):
    with _session():
        a = guard.zeros(64, device=CPU)
        bare = torch.zeros(64)
        with pytest.raises(GuardError, match=r'bdn_sgd_step: argument 1 '):
            _lib.call('bdn_sgd_step', a.data_ptr(), bare.data_ptr(), 0.1, 1.0, 64, 0)
        with pytest.raises(GuardError, match=r'bdn_sgd_step: argument 0 '):
            _lib.call('bdn_sgd_step', a.data_ptr() + a.numel() * 4, a.data_ptr(), 0.1, 1.0, 64, 0)    # first byte after the payload
        with pytest.raises(GuardError, match=r'argument 0 '):
            _lib.call('bdn_sgd_step', a.data_ptr() - 1, a.data_ptr(), 0.1, 1.0, 64, 0)
        assert stub == []
    assert _lib.call('x') is None and stub == ['x']                  # the wrapper is gone with the session


def test_wrapper_accepts_interior_pointers_and_skips_none_stream_and_host_arguments(stub):
    with _session() as s:
        img = guard.zeros(4, 8, 8, 128, dtype=torch.bfloat16, device=CPU)
        p, g = guard.zeros(64, device=CPU), guard.zeros(64, device=CPU)
        tab = guard.zeros(4, dtype=torch.int32, device=CPU)
        # an interior slice pointer (second image, upper 64 channels); None; the trailing stream is never looked at
        _lib.call('bdn_upsample2x_bwd', 1, img[1:].data_ptr() + 64 * 2, 128, p.data_ptr(), 1, 4, 4, 8, 8, 64, 0xdeadbeef)
        _lib.call('bdn_sgd_momentum_step', p.data_ptr(), g.data_ptr(), None, 0.1, 1.0, 0.0, 0.0, 0.0, 0, 1, 64, 0xdeadbeef)
        # host arrays of the grouped rules, ctypes arrays or addresses
        lr = _lib.floats([0.1, 0.2])
        _lib.call('bdn_sgd_step_grouped', p.data_ptr(), g.data_ptr(), tab.data_ptr(), tab.data_ptr(), 4, 2, lr, 1.0, 64, 0)
        _lib.call('bdn_adam_step_grouped', p.data_ptr(), g.data_ptr(), p.data_ptr(), g.data_ptr(), tab.data_ptr(), tab.data_ptr(), 4, 2,
                  ctypes.addressof(lr), lr, 1.0, 0.9, 0.999, 1e-8, 0, 1, 64, 0)
        host = torch.zeros(16)
        _lib.call('bdn_upload_band', p.data_ptr(), host.data_ptr(), 1, 4, 4, 0, 4, 0)
        _lib.call('bdn_sample_patches', p.data_ptr(), host.data_ptr(), 1, 1, host.data_ptr(), tab.data_ptr(), 1, 1,
                  p.data_ptr(), g.data_ptr(), tab.data_ptr(), 0)
        _lib.call('bdn_event_record', 0x1234, 0x5678)                  # handles, not memory
        assert s.calls == 6 and len(stub) == 7                        # the handle-only call does not count as a library call on memory
        with pytest.raises(GuardError, match='bdn_upload_band: argument 0'):          # ... but the device side of the same call is checked
            _lib.call('bdn_upload_band', host.data_ptr(), host.data_ptr(), 1, 4, 4, 0, 4, 0)
        with pytest.raises(GuardError, match='bdn_sgd_step_grouped: argument 2'):
            _lib.call('bdn_sgd_step_grouped', p.data_ptr(), g.data_ptr(), host.data_ptr(), tab.data_ptr(), 4, 2, lr, 1.0, 64, 0)


def test_tensors_of_an_earlier_session_are_not_accepted(stub):
    with _session():
        old = guard.zeros(64, device=CPU)
    with _session():
        new = guard.zeros(64, device=CPU)
        with pytest.raises(GuardError, match='argument 1'):
            _lib.call('bdn_sgd_step', new.data_ptr(), old.data_ptr(), 0.1, 1.0, 64, 0)


# ---------------------------------------------------------------- the decorator
def test_decorator_fails_a_test_that_writes_outside(stub):
    @guarded
    def body():
        t = guard.zeros(8, device=CPU)
        _lib.call('bdn_sgd_step', t.data_ptr(), t.data_ptr(), 0.1, 1.0, 8, 0)
        t.as_strided((9,), (1,))[8] = 0.0

    with pytest.raises(GuardError, match=r'float32\[8\]: right guard, 4 bytes changed, offsets \+0 \.\. \+3'):
        body()


def test_decorator_requires_a_library_call(stub):
    @guarded
    def body():
        guard.zeros(8, device=CPU)

    with pytest.raises(AssertionError, match='no library call'):
        body()


def test_decorator_rebinds_a_module_level_call(monkeypatch):
    """A test module that did `from fabric_amd._lib import call` is checked like one that goes through _lib.call."""
    g = {'call': _lib.call}
    hit = []

    def body():
        hit.append(g['call'] is not _lib_real)
    _lib_real = _lib.call
    with guard.Session(g):
        body()
    assert hit == [True] and g['call'] is _lib_real


@pytest.mark.parametrize('n', [3, 5])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@guarded
def test_decorator_keeps_parametrization_and_fixtures(golden_dir, monkeypatch, tmp_path, stub, dtype, n):
    import os
    monkeypatch.setenv('GUARDED_CPU_PROBE', str(n))
    assert os.path.isdir(golden_dir) and tmp_path.is_dir() and os.environ['GUARDED_CPU_PROBE'] == str(n)
    assert n in (3, 5) and dtype in (torch.float32, torch.bfloat16)
    t = guard.zeros(n, dtype=dtype, device=CPU)
    _lib.call('bdn_sgd_step', t.data_ptr(), t.data_ptr(), 0.1, 1.0, n, 0)
    assert stub == ['bdn_sgd_step']


def test_decorated_signature_is_the_tests_own():
    import inspect

    @guarded
    def f(golden_dir, case, prec='bf16'):
        pass
    assert list(inspect.signature(f).parameters) == ['golden_dir', 'case', 'prec'] and f.__name__ == 'f'
