"""The stale-state helper itself (tests/stale.py), on the CPU: the poison wrapper, the bit comparison, and the twin comparison on a
small object with a deliberately stale cache."""
import pytest
import torch

from tests import stale


# ------------------------------------------------------------------ poisoned_allocations
def _all_ff(t):
    return t.numel() > 0 and bool((t.contiguous().view(-1).view(torch.uint8) == 0xFF).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_poison_fills_floating_point_results(dtype):
    with stale.poisoned_allocations():
        made = [torch.empty(3, 5, dtype=dtype), torch.empty((7,), dtype=dtype), torch.empty_like(torch.zeros(4, 2, dtype=dtype)),
                torch.zeros(2, dtype=dtype).new_empty(6), torch.zeros(2).new_empty((2, 3), dtype=dtype),
                torch.empty_like(torch.zeros(2, 3), dtype=dtype), torch.empty((), dtype=dtype)]
        alloc = lambda *s: torch.empty(*s, dtype=dtype, device='cpu')     # noqa: E731  (the engine allocates through such lambdas)
        made.append(alloc(2, 3, 4))
    for t in made:
        assert t.dtype == dtype and _all_ff(t) and bool(torch.isnan(t).all())


def test_poison_fills_a_permuted_dense_result():
    src = torch.zeros(2, 3, 4, 5).permute(0, 2, 3, 1)                     # dense, not contiguous: empty_like keeps the strides
    with stale.poisoned_allocations():
        t = torch.empty_like(src)
    assert t.stride() == src.stride() and bool(torch.isnan(t).all())


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64, torch.uint8, torch.bool])
def test_poison_leaves_integer_results_alone(dtype):
    """An integer result must come back untouched: no fill is launched on it (checked by making the fill impossible to miss: the wrapper's
    only write is _poison, which is asked directly too)."""
    z = torch.zeros(16, dtype=dtype)
    assert stale._poison(z) is z and bool((z == 0).all())
    with stale.poisoned_allocations():
        t = torch.empty(4, 4, dtype=dtype)
        u = torch.empty_like(z)
        v = z.new_empty(3)
    assert t.dtype == u.dtype == v.dtype == dtype and t.shape == (4, 4) and u.shape == (16,) and v.shape == (3,)


def test_poison_takes_zero_size_tensors():
    with stale.poisoned_allocations():
        t = torch.empty(0, 4)
        u = torch.empty_like(torch.zeros(0))
    assert t.shape == (0, 4) and u.shape == (0,)


def test_poison_restores_the_originals():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with stale.poisoned_allocations():
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
        assert torch.empty.__wrapped__ is before[0]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(KeyError):
        with stale.poisoned_allocations():
            raise KeyError('body raises')
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    assert 'new_empty' not in vars(torch.Tensor) or vars(torch.Tensor)['new_empty'] is before[2]


def test_poison_through_monkeypatch(monkeypatch):
    before = (torch.empty, torch.empty_like)
    with stale.poisoned_allocations(monkeypatch):
        assert bool(torch.isnan(torch.empty(5)).all())
    assert (torch.empty, torch.empty_like) == before
    monkeypatch.undo()
    assert (torch.empty, torch.empty_like) == before and torch.zeros(2).new_empty(3).shape == (3,)


# ------------------------------------------------------------------ same_bits / mattered
def test_same_bits_nan_and_signed_zero():
    nan = torch.tensor([float('nan'), 1.0])
    stale.same_bits(nan, nan.clone(), 'equal NaNs are equal')
    other_nan = nan.clone()
    other_nan.view(torch.int32)[0] += 1                                   # another NaN payload: other bits
    with pytest.raises(AssertionError, match='1 of 2 elements differ'):
        stale.same_bits(other_nan, nan, 'payload')
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))         # what a value comparison would let through
    with pytest.raises(AssertionError, match='1 of 1 elements differ'):
        stale.same_bits(torch.tensor([-0.0]), torch.tensor([0.0]), 'signed zero')
    for dt in (torch.bfloat16, torch.float64, torch.int64, torch.uint8, torch.bool):
        stale.same_bits(torch.ones(3, dtype=dt), torch.ones(3, dtype=dt), str(dt))
    stale.same_bits(torch.tensor(2.5), torch.tensor(2.5), '0-dim')
    with pytest.raises(AssertionError, match='float32 .* against torch.float64'):
        stale.same_bits(torch.ones(2), torch.ones(2, dtype=torch.float64), 'dtype')
    with pytest.raises(AssertionError, match=r'\(2, 1\) against'):
        stale.same_bits(torch.ones(2, 1), torch.ones(2), 'shape')


def test_same_bits_dicts_name_the_first_differing_key():
    a = {'x': torch.zeros(4), 'y': torch.arange(6.0), 'n': 3, 'z': None}
    b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
    stale.same_bits(a, b, 'equal dicts')
    b['y'][2:4] += 1
    with pytest.raises(AssertionError, match=r'seq: not the same bits -- y: 2 of 6 elements differ'):
        stale.same_bits(a, b, 'seq')
    with pytest.raises(AssertionError, match=r"missing \['w'\]"):
        stale.same_bits(a, dict(a, w=torch.zeros(1)), 'missing key')
    with pytest.raises(AssertionError, match=r"unexpected \['y'\]"):
        stale.same_bits(a, {k: v for k, v in a.items() if k != 'y'}, 'extra key')
    with pytest.raises(AssertionError, match='n: 3 against 4'):
        stale.same_bits(a, dict(a, n=4), 'host int')
    stale.same_bits({'t': (torch.ones(2), [torch.zeros(1)])}, {'t': (torch.ones(2), [torch.zeros(1)])}, 'nested')


def test_mattered():
    stale.mattered(torch.zeros(3), torch.tensor([0.0, -0.0, 0.0]), 'one sign bit')
    with pytest.raises(AssertionError, match='did not change a single bit'):
        stale.mattered({'a': torch.ones(2)}, {'a': torch.ones(2)}, 'nothing moved')


def test_all_finite():
    stale.all_finite({'a': torch.ones(2), 'i': torch.arange(3)}, 'fine')
    with pytest.raises(AssertionError, match='b has non-finite'):
        stale.all_finite({'a': torch.ones(2), 'b': torch.tensor([float('inf')])}, 'inf')


# ------------------------------------------------------------------ the twin comparison catches a stale cache
class _Scaled:
    """y = x * (2 w), with 2 w cached behind w's version counter -- and, when `forget` is set, behind nothing at all."""

    def __init__(self, w, forget):
        self.w, self.forget, self._cache, self._version = w, forget, None, None

    def state(self):
        return {'w': self.w.clone()}

    def twin(self):
        return _Scaled(self.state()['w'], self.forget)

    def __call__(self, x):
        if self._cache is None or (not self.forget and self._version != self.w._version):
            self._cache, self._version = 2 * self.w, self.w._version
        return x * self._cache


def test_twin_comparison_catches_a_stale_cache():
    x = torch.arange(4.0)
    for forget in (True, False):
        m = _Scaled(torch.full((4,), 3.0), forget)
        before = m(x)
        m.w.mul_(0.5)                                                     # the perturbation
        after, want = m(x), m.twin()(x)
        if forget:
            with pytest.raises(AssertionError, match='did not change'):   # the stale cache hides the perturbation ...
                stale.mattered(before, after, 'stale')
            with pytest.raises(AssertionError, match='4 of 4|3 of 4'):    # ... and the used object differs from its twin
                stale.same_bits(after, want, 'stale')
            m._cache = None                                               # refreshed: the same object passes
            after = m(x)
        stale.mattered(before, after, 'fresh')
        stale.same_bits(after, want, 'fresh')


def test_twin_of_a_model_is_a_fresh_model_with_the_same_state():
    from fabric_amd import BiDateNet
    m = BiDateNet(3, 2, precision='fp32').eval()
    m.inc.conv.conv[0].weight.requires_grad_(False)
    m.engine()
    t = stale.twin(m)
    assert t is not m and t._engine is None and t.precision == 'fp32' and not t.training
    stale.same_bits(dict(t.state_dict()), dict(m.state_dict()), 'state')
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(t.state_dict().values(), m.state_dict().values()))
    assert [p.requires_grad for p in t.parameters()] == [p.requires_grad for p in m.parameters()]
