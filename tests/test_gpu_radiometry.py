"""-m gpu: bdn_band_quantiles / bdn_transfer_apply / bdn_stretch_u8 (include/bidate_hip.h; fabric_amd.utils.radiometry) through the C ABI
on guard-banded buffers, with a workspace of exactly the queried size born as 0xFF, against tests/radiometry_ref.py.  Everything is bit
for bit: order, value, count, the applied raster and the stretched bytes; every entry runs twice and must give the same bits.

Shapes: as small as the kernels can still go wrong at -- one pixel, more ranks than pixels, 97 x 131 (thirteen chunks of 1024 pixels, the
last one partial), a band subset of a 13-band stack, 1024 probabilities on 7 bands (two groups of bands: 5 + 2), and one 97 x 131 stack of
bands built to take one path each: no valid pixel, one value, 8 values, keys that differ only in the last level's digit, keys that share
the top digit and split at the second, both zeros with negatives and denormals, non-finite pixels."""
import functools

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from gpu_util import dev, st
from tests import guard
from tests import radiometry_ref as RR
from tests import sched_stress as ss
from tests.guard import guarded

pytestmark = pytest.mark.gpu
EXV = 9


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _probs(nq):
    """n_q probabilities with 0 and 1 among them (from n_q = 2 on); 1024: unsorted, with repeats."""
    if nq == 1:
        return np.array([0.5])
    if nq == 2:
        return np.array([0.0, 1.0])
    if nq == 256:
        return RR.default_probs(256)
    r = np.random.default_rng(nq)
    p = np.concatenate([[1.0, 0.0, 0.5, 0.5], r.random(nq - 4)])
    r.shuffle(p)
    return p


def _quant(scene_d, bands, probs, ex_d=None, positive_only=False, stream=None):
    C, H, W = scene_d.shape
    nb, nq = len(bands), len(probs)
    bands_d = dev(torch.tensor(bands), torch.int32)
    probs_d = dev(torch.from_numpy(np.asarray(probs, np.float64)), torch.float64)
    value, order, count = guard.empty(nb, nq, dtype=torch.float64), guard.empty(nb, nq, 2), guard.empty(nb, dtype=torch.int64)
    ws = guard.alloc_bytes(_lib.load().bdn_band_quantiles_workspace_bytes(nb, nq, H, W), label='band_quantiles workspace')
    _lib.call('bdn_band_quantiles', scene_d.data_ptr(), bands_d.data_ptr(), nb, _lib.ptr(ex_d), EXV if ex_d is not None else 0,
              1 if positive_only else 0, probs_d.data_ptr(), nq, value.data_ptr(), order.data_ptr(), count.data_ptr(), ws.data_ptr(), C, H, W,
              st() if stream is None else stream)
    return value, order, count


def _check(scene, bands, probs, ex=None, positive_only=False, what=''):
    """Two runs against the twin, bit for bit.  Returns the twin's (value, order, count)."""
    scene_d = dev(torch.from_numpy(scene))
    ex_d = None if ex is None else dev(torch.from_numpy(ex), torch.uint8)
    want = RR.quantiles_ref(scene, probs, bands, ex, EXV, positive_only)
    runs = [_quant(scene_d, bands, probs, ex_d, positive_only) for _ in range(2)]
    got = [t.cpu().numpy() for t in runs[0]]
    assert np.array_equal(got[2], want[2]), (what, 'count', got[2], want[2])
    for k, name in ((1, 'order'), (0, 'value')):
        bad = _bits(got[k]) != _bits(want[k])
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (what, 'second run')
    return want


def _gamma(seed, shape):
    return np.random.default_rng(seed).gamma(2.0, 1.0, shape).astype(np.float32)


@guarded
def test_one_pixel_and_more_ranks_than_pixels():
    value, order, count = _check(np.array([[[2.5]]], np.float32), [0], _probs(256), what='1x1x1')
    assert count.tolist() == [1] and (value == 2.5).all() and (order == 2.5).all()
    x = _gamma(1, (1, 3, 5)) - np.float32(1.0)
    value, order, count = _check(x, [0], _probs(256), what='3x5')
    assert count.tolist() == [15] and value[0, 0] == x.min() and value[0, -1] == x.max() and (np.diff(value[0]) >= 0).all()


@pytest.mark.parametrize('nq', [1, 2, 256, 1024])
@guarded
def test_one_band_that_straddles_the_chunks(nq):
    x = _gamma(2, (1, 97, 131)) - np.float32(1.5)
    value, order, count = _check(x, [0], _probs(nq), what=f'97x131 n_q={nq}')
    assert count.tolist() == [97 * 131]
    if nq == 2:
        assert value[0].tolist() == [float(x.min()), float(x.max())]


@guarded
def test_a_band_subset_of_a_13_band_stack():
    x = _gamma(3, (13, 150, 130)) * np.arange(1, 14, dtype=np.float32)[:, None, None]
    value, _, _ = _check(x, [11, 0, 7, 3], _probs(256), what='13x150x130')
    assert [float(v) for v in value[:, -1]] == [float(x[b].max()) for b in (11, 0, 7, 3)]      # the rows follow the list


@guarded
def test_1024_probabilities_take_the_bands_in_groups():
    x = _gamma(4, (7, 40, 50)) - np.arange(7, dtype=np.float32)[:, None, None]
    q = _lib.load().bdn_band_quantiles_workspace_bytes
    assert q(7, 1024, 40, 50) == 5 * q(1, 1024, 40, 50)      # the condition: two groups, 5 + 2 bands
    _check(x, list(range(7)), _probs(1024), what='7 bands n_q=1024')


@functools.lru_cache(maxsize=None)
def _special():
    """One 97 x 131 stack, a path per band.  Shared: never modified."""
    h, w = 97, 131
    r = np.random.default_rng(5)
    j = np.arange(h * w, dtype=np.float32).reshape(h, w)
    b = np.empty((10, h, w), np.float32)
    b[0] = np.nan                                            # no valid pixel
    b[1] = 3.5                                               # one value
    b[2] = r.integers(0, 8, (h, w)).astype(np.float32) * np.float32(0.75) - np.float32(2.0)          # 8 values
    b[3] = np.float32(1.0) + (j % 1024) * np.float32(2.0 ** -23)       # the keys differ only in the last level's digit
    b[4] = np.float32(1.0) + j * np.float32(2.0 ** -23)      # ... in the last level's and the low bits of the second
    b[5] = r.uniform(1.0, 1.25, (h, w)).astype(np.float32)   # one top digit (sign, exponent, two mantissa bits), every second digit
    mix = np.concatenate([np.full(3000, -0.0), np.full(3000, 0.0), r.standard_normal(3000) * 1e-40, -r.gamma(2.0, 1.0, 3000),
                          r.standard_normal(h * w - 12000) * 1e-3]).astype(np.float32)
    r.shuffle(mix)
    b[6] = mix.reshape(h, w)                                 # negatives, both zeros, denormals
    b[7] = r.gamma(2.0, 1.0, (h, w)).astype(np.float32)
    k = h * w // 50
    b[7].reshape(-1)[r.choice(h * w, k, replace=False)] = r.choice([np.nan, np.inf, -np.inf], k)      # 2 % non-finite
    b[8] = -r.gamma(2.0, 1.0, (h, w)).astype(np.float32)     # nothing > 0
    b[8, 0, :5] = 0.0
    b[9] = np.inf
    ex = np.where(r.random((h, w)) < 0.05, EXV, 0).astype(np.uint8)
    assert (np.unique(RR.keys(b[3]) >> 10).size, np.unique(RR.keys(b[5]) >> 21).size) == (1, 1) and np.unique(RR.keys(b[5]) >> 10).size > 1000
    assert np.unique(RR.keys(b[6]) >> 21).size > 50 and (np.abs(b[6][b[6] != 0]) < 1.2e-38).sum() > 2000
    return b, ex


@pytest.mark.parametrize('mode', ['plain', 'exclude', 'positive_only', 'all excluded'])
@guarded
def test_bands_that_take_one_path_each(mode):
    b, ex = _special()
    ex = {'plain': None, 'exclude': ex, 'positive_only': None, 'all excluded': np.full_like(ex, EXV)}[mode]
    value, order, count = _check(b, list(range(10)), _probs(256), ex, mode == 'positive_only', what=mode)
    assert count[0] == 0 and count[9] == 0 and np.isnan(value[0]).all() and np.isnan(order[9]).all()
    if mode == 'plain':
        assert count[1] == 97 * 131 and (value[1] == 3.5).all() and np.unique(order[2]).size == 8 and count[7] == 97 * 131 - 97 * 131 // 50
        assert np.signbit(order[6]).any() and (order[6] == 0).any() and not np.isnan(value[1:9]).any()
    if mode == 'exclude':
        assert 0 < count[1] == int((ex != EXV).sum()) < 97 * 131
    if mode == 'positive_only':
        assert count[8] == 0 and np.isnan(value[8]).all() and 0 < count[6] < 97 * 131 and (order[6] > 0).all() and count[2] < 97 * 131
    if mode == 'all excluded':
        assert not count.any() and np.isnan(value).all() and np.isnan(order).all()


@guarded
def test_a_probability_outside_the_unit_interval_and_a_band_outside_the_stack():
    x = _gamma(6, (2, 9, 11))
    value, order, count = _check(x, [1, 5, -1], [0.5, 1.5, float('nan'), -0.1, 1.0], what='outside')
    assert count.tolist() == [99, 0, 0] and np.isnan(value[0, 1:4]).all() and not np.isnan(value[0, [0, 4]]).any() and np.isnan(value[1:]).all()


@guarded
def test_a_lagging_side_stream_gives_the_bits_of_the_synchronised_run():
    b, ex = _special()
    scene_d, ex_d = dev(torch.from_numpy(b)), dev(torch.from_numpy(ex), torch.uint8)
    bands, probs = list(range(10)), _probs(256)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    e0.record(); torch.cuda._sleep(4_000_000); e1.record()
    torch.cuda.synchronize()
    rate = 4_000_000 / (e0.elapsed_time(e1) * 1e3)           # _sleep cycles per microsecond
    with ss.Perturb(ss.sync()):
        e0.record()
        ref = _quant(scene_d, bands, probs, ex_d)
        e1.record()
    torch.cuda.synchronize()
    short = int(3 * e0.elapsed_time(e1) * 1e3 / 7 * rate)    # three times the mean launch of the seven
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ss.Perturb(ss.lag(side), short=short) as h, torch.cuda.stream(side):
        got = _quant(scene_d, bands, probs, ex_d, stream=side.cuda_stream)
    side.synchronize()
    assert len(h.log) == 1 and h.log[0][1] == 'bdn_band_quantiles' and h.log[0][3] == short > 0
    for a, c in zip(ref, got):
        assert torch.equal(a.view(torch.uint8), c.view(torch.uint8))


# ---------------------------------------------------------------- the transfer
def _apply(src_d, bands, S, T, mode, out_d=None, exact=None):
    C, H, W = src_d.shape
    bands_d = dev(torch.tensor(bands), torch.int32)
    s_d, t_d = dev(torch.from_numpy(np.ascontiguousarray(S, np.float32))), dev(torch.from_numpy(np.ascontiguousarray(T, np.float32)))
    ex_d = None if exact is None else dev(torch.tensor(exact), torch.uint8)
    out_d = guard.empty(C, H, W) if out_d is None else out_d
    _lib.call('bdn_transfer_apply', src_d.data_ptr(), out_d.data_ptr(), bands_d.data_ptr(), len(bands), s_d.data_ptr(), t_d.data_ptr(),
              S.shape[1], mode, _lib.ptr(ex_d), C, H, W, st())
    return out_d


def _transfer_case(K):
    """A 4-band 97 x 131 stack, bands 2 and 0 named: knots fitted on the data (K = 2: the 2 % and 98 % quantiles), pixels exactly on knots,
    below the first and at and above the last, and non-finite ones."""
    r = np.random.default_rng(K)
    src = r.gamma(2.0, 1.0, (4, 97, 131)).astype(np.float32) - np.float32(1.0)
    d1 = (np.float32(0.7) * np.sqrt(src + np.float32(1.0)) + np.float32(0.1)).astype(np.float32)
    probs = [0.02, 0.98] if K == 2 else RR.default_probs(K)
    S, T, _ = RR.fit_ref(src, d1, probs, K, [2, 0])
    for i, b in enumerate((2, 0)):
        flat = src[b].reshape(-1)
        flat[:K] = S[i]                                      # exactly on every knot
        flat[K:K + 4] = [S[i, 0] - 1, np.nextafter(S[i, 0], np.float32(-9)), np.nextafter(S[i, -1], np.float32(99)), S[i, -1] + 7]
        flat[K + 4:K + 8] = [np.nan, np.inf, -np.inf, -0.0]
    src[1, 0, :3] = [np.nan, np.inf, -0.0]
    return src, S, T


@pytest.mark.parametrize('mode', [RR.OFFSET, RR.SLOPE], ids=['offset', 'slope'])
@pytest.mark.parametrize('K', [2, 1024])
@guarded
def test_apply_is_the_twin_bit_for_bit(K, mode):
    src, S, T = _transfer_case(K)
    assert (np.diff(S, axis=1) >= 0).all() and (np.diff(T, axis=1) >= 0).all() and (K == 2 or (np.diff(S, axis=1) == 0).sum() < K // 2)
    want = RR.apply_ref(src, [2, 0], S, T, mode)
    src_d = dev(torch.from_numpy(src))
    outs = [_apply(src_d, [2, 0], S, T, mode) for _ in range(2)]
    got = outs[0].cpu().numpy()
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (K, mode, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert np.array_equal(_bits(got[[1, 3]]), _bits(src[[1, 3]])) and (got[2] != src[2]).mean() > 0.9        # un-named bands are copies
    for i, b in enumerate((2, 0)):                           # a knot below the last, apart from its neighbours, lands on its knot
        lone = np.flatnonzero((np.diff(S[i], prepend=-np.inf) > 0)[:-1] & (np.diff(S[i]) > 0))
        assert lone.size >= (K - 1) // 2 and np.array_equal(got[b].reshape(-1)[lone], T[i][lone])
    assert np.array_equal(_bits(got[2].reshape(-1)[K + 4:K + 7]), _bits(src[2].reshape(-1)[K + 4:K + 7]))    # NaN, inf keep their bits
    inplace = dev(torch.from_numpy(src))                     # out == src: un-named bands are left alone
    _apply(inplace, [2, 0], S, T, mode, out_d=inplace)
    assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(want))


@guarded
def test_apply_identity_zero_length_ends_nan_knots_and_exact_flags():
    src, S, T = _transfer_case(2)
    src_d = dev(torch.from_numpy(src))
    for mode in (RR.OFFSET, RR.SLOPE):
        for tab in (S, RR.fit_ref(src, src, None, 1024, [2, 0])[0]):           # a table matched to itself: every bit comes back
            got = _apply(src_d, [2, 0], tab, tab, mode).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(src)), mode
        s = np.array([[-0.5, -0.5, 0.5, 2.0, 2.0]] * 2, np.float32)           # zero-length end segments: SLOPE falls back to the offset
        t = np.array([[10, 10, 20, 30, 30], [-1, -1, 0, 0, 0]], np.float32)
        got = _apply(src_d, [2, 0], s, t, mode).cpu().numpy()
        want = RR.apply_ref(src, [2, 0], s, t, mode)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(want), _bits(RR.apply_ref(src, [2, 0], s, t, RR.OFFSET)))
        assert got[2][src[2] >= 2.0].min() >= 30 and (src[2] < -0.5).any()
        t_nan = T.copy()
        t_nan[1, 0] = np.nan                                 # band 0 has a NaN knot: it passes through; band 2 is mapped
        got = _apply(src_d, [2, 0], S, t_nan, mode).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(RR.apply_ref(src, [2, 0], S, t_nan, mode))) and np.array_equal(_bits(got[0]), _bits(src[0]))
        got = _apply(src_d, [2, 0], S, T, mode, exact=[1, 0]).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(RR.apply_ref(src, [2, 0], S, T, mode, exact=[1, 0]))) and np.array_equal(_bits(got[2]), _bits(src[2]))


# ---------------------------------------------------------------- the stretch
@pytest.mark.parametrize('u16', [False, True], ids=['float32', 'uint16'])
@guarded
def test_stretch_is_the_twin_byte_for_byte(u16):
    r = np.random.default_rng(8)
    x = (r.gamma(2.0, 500.0, (4, 97, 131)) * (r.random((4, 97, 131)) > 0.1))
    x = x.astype(np.uint16) if u16 else x.astype(np.float32)
    x[1] = 7                                                 # a constant band: d == c
    x[1, 0, :2] = [6, 8]
    x[2] = 0                                                 # nothing > 0: c and d are NaN
    if not u16:
        x[3, 0, :3] = [np.nan, np.inf, -np.inf]
    cd = np.empty((4, 2))
    for b in range(4):
        cd[b] = RR.quantiles_sorted(RR.valid_sorted(x[b].astype(np.float32), positive_only=True), [0.02, 0.98])[0]
    cd[1] = 7.0                                              # (the percentiles of band 1 are 7 up to the two pixels that differ)
    assert np.isnan(cd[2]).all() and cd[0, 0] < cd[0, 1]
    want = np.stack([RR.stretch_ref(x[b], *cd[b]) for b in range(4)])
    x_d = guard.guard(torch.from_numpy(x))
    cd_d = dev(torch.from_numpy(cd), torch.float64)
    outs = []
    for _ in range(2):
        out = guard.empty(4, 97, 131, dtype=torch.uint8)
        _lib.call('bdn_stretch_u8', x_d.data_ptr(), 1 if u16 else 0, cd_d.data_ptr(), out.data_ptr(), 4, 97, 131, st())
        outs.append(out)
    got = outs[0].cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert torch.equal(outs[0], outs[1])
    assert got[1, 0, :3].tolist() == [0, 255, 0] and not got[2].any() and got[0].max() == 255 and got[0].min() == 0
    if not u16:
        assert got[3, 0, :3].tolist() == [0, 255, 0]
