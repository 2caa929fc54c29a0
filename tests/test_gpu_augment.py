"""bdn_sample_patches_aug on the device against its numpy twin (tests/augment_ref.py), bit for bit wherever the specification is exact.

Shapes are the smallest at which the kernel can go wrong: S = 12 (below one 64 x 64 tile and no multiple of the 4-column noise group),
64 (exactly one tile), 70 (a ragged 2 x 2 of tiles); C = 3 and 13; eight samples over four cities, one of exactly S x S and two with
H - S or W - S below the jitter.  The sample keys are constants found by `search_keys` on the CPU; `assert_coverage` states, on the
reference's own draws and before the device is touched, what they were searched for.
"""
import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.augment import PatchAugment
from tests import augment_ref as R
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu

SEED = 0x5EED2026A06
J = 6
N = 8
EPOCH = 1
# dataset indices whose keys (EPOCH << 32 | index) give, under full_policy(S): sample k the symmetry code k; samples 0-3 erased with a
# rectangle on the top / left / bottom / right border; samples 4-7 kept, with a jitter that is clamped at the low / high row, low / high
# column.  Output of search_keys(S).
INDICES = {12: [3, 2, 5, 6, 31, 28, 50, 113],
           64: [43, 201, 7, 296, 31, 28, 50, 113],
           70: [43, 201, 7, 296, 31, 28, 50, 113]}


def shapes(S):
    return [(S, S), (S + 3, S + 40), (S + 50, S + 4), (S + 20, S + 25)]


def descriptors(S):
    """(city, row, col, sym): sample 0 in the S x S city, 1 and 2 where the city is narrower than the jitter, 4-7 on the four borders."""
    return np.array([(0, 0, 0, 0), (1, 1, 20, 1), (2, 25, 2, 2), (3, 10, 12, 3), (3, 0, 7, 4), (3, 20, 9, 5), (3, 5, 0, 6), (3, 8, 25, 7)],
                    np.int32)


def full_policy(S, **kw):
    return PatchAugment(**dict(dict(seed=SEED, jitter=J, symmetry=True, gain=0.25, bias=0.125, per_date=True, erase_p=0.5,
                                    erase_size=(max(1, S // 4), S), erase_label=255, erase_fill=-1.5), **kw))


def _wanted(k, g, H, W, S):
    if g['sym'] != k:
        return False
    if k < 4:
        return g['erased'] and (g['top'] == 0, g['left'] == 0, g['top'] + g['eh'] == S, g['left'] + g['ew'] == S)[k]
    return not g['erased'] and (g['raw_row'] < 0, g['raw_row'] > H - S, g['raw_col'] < 0, g['raw_col'] > W - S)[k - 4]


def _geometry(pol, S, index, k):
    city, row, col, sym = (int(v) for v in descriptors(S)[k])
    H, W = shapes(S)[city]
    g = R.geometry(pol, R.sample_key(EPOCH, index), row, col, sym, H, W, S)
    g['raw_row'], g['raw_col'] = row + g['dy'], col + g['dx']
    return g, H, W


def search_keys(S, pool=200000):
    """CPU only: the first dataset index per sample slot that meets _wanted (distinct indices).  How INDICES was made."""
    pol, out = full_policy(S), []
    for k in range(N):
        for index in range(pool):
            g, H, W = _geometry(pol, S, index, k)
            if index not in out and _wanted(k, g, H, W, S):
                out.append(index)
                break
        else:
            raise AssertionError(f'no index for slot {k}')
    return out


def keys_of(S):
    return np.array([R.sample_key(EPOCH, i) for i in INDICES[S]], np.uint64)


def assert_coverage(S):
    """A condition of the tests, checked on the reference's draws: an uncovered case fails here instead of passing silently."""
    pol = full_policy(S)
    gs = [_geometry(pol, S, i, k) for k, i in enumerate(INDICES[S])]
    assert len(set(INDICES[S])) == N
    assert {g['sym'] for g, _, _ in gs} == set(range(8)), 'all eight symmetry codes'
    assert any(g['raw_row'] < 0 for g, _, _ in gs) and any(g['raw_row'] > H - S for g, H, _ in gs), 'both row clamps'
    assert any(g['raw_col'] < 0 for g, _, _ in gs) and any(g['raw_col'] > W - S for g, _, W in gs), 'both column clamps'
    assert any(H - S < J or W - S < J for _, H, W in gs) and any((H, W) == (S, S) for _, H, W in gs)
    er = [g for g, _, _ in gs if g['erased']]
    assert er and len(er) < N, 'erased and kept samples'
    assert any(g['top'] == 0 for g in er) and any(g['left'] == 0 for g in er), 'rectangles on the top and left borders'
    assert any(g['top'] + g['eh'] == S for g in er) and any(g['left'] + g['ew'] == S for g in er), 'rectangles on the bottom and right borders'
    whole = full_policy(S, erase_p=1.0, erase_size=(S, S))
    for k, i in enumerate(INDICES[S]):
        g, _, _ = _geometry(whole, S, i, k)
        assert (g['erased'], g['top'], g['left'], g['eh'], g['ew']) == (1, 0, 0, S, S), 'a rectangle covering the whole patch'


@pytest.mark.parametrize('S', [12, 64, 70])
def test_committed_keys_cover_the_cases(S):
    assert_coverage(S)


# ---------------------------------------------------------------- fixtures: cities, one upload per (S, C)
def _special(r, shape):
    """float32 noise with NaN payloads (quiet and signalling, both signs), -0.0, +-inf and denormals sprinkled in."""
    x = r.standard_normal(shape).astype(np.float32)
    bits = x.view(np.uint32)
    specials = np.array([0x7fc01234, 0xffc00001, 0x7f800001, 0xff912345, 0x80000000, 0x7f800000, 0xff800000, 0x00000001], np.uint32)
    m = r.uniform(0, 1, shape) < 0.05
    bits[m] = specials[r.integers(0, len(specials), int(m.sum()))]
    return x


_CITIES = {}


def host_cities(S, C, special=False):
    key = (S, C, special)
    if key not in _CITIES:
        r = np.random.default_rng(1000 * S + 10 * C + special)
        _CITIES[key] = [{'images': _special(r, (2, C, h, w)) if special else r.standard_normal((2, C, h, w)).astype(np.float32),
                         'labels': r.integers(0, 200, (h, w)).astype(np.uint8)} for h, w in shapes(S)]
    return _CITIES[key]


class Device:
    """The guarded device side of one (S, C): cities, their table, and fresh outputs per run."""

    def __init__(self, S, C, cities):
        self.S, self.C = S, C
        self.dev = [{k: guard.guard(torch.from_numpy(v)) for k, v in c.items()} for c in cities]
        rec = np.array([[d['images'].data_ptr(), d['labels'].data_ptr(), h | (w << 32)] for d, (h, w) in zip(self.dev, shapes(S))], np.int64)
        self.table = guard.guard(torch.from_numpy(rec))
        self.hw = np.array(shapes(S), np.int32)

    def run(self, pol, keys, desc, export=True, plain=False):
        """One call on n samples -> numpy (d1, d2, labels, geom, radio); plain: bdn_sample_patches on the same descriptors."""
        S, C, n = self.S, self.C, len(desc)
        desc = np.ascontiguousarray(desc, np.int32)
        desc_dev = guard.guard(torch.from_numpy(desc))
        o1 = guard.full((n, C, S, S), float('nan'))
        o2 = guard.full_like(o1, float('nan'))
        ol = guard.full((n, S, S), 77, dtype=torch.uint8)
        if plain:
            _lib.call('bdn_sample_patches', self.table.data_ptr(), self.hw.ctypes.data, len(self.hw), C, desc.ctypes.data, desc_dev.data_ptr(),
                      n, S, o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), _lib.stream_ptr())
            torch.cuda.synchronize()
            return o1.cpu().numpy(), o2.cpu().numpy(), ol.cpu().numpy(), None, None
        keys_dev = guard.guard(torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)))
        geom = guard.full((n, 8), -7, dtype=torch.int32) if export else None
        radio = guard.full((n, 2, C, 2), float('nan')) if export else None
        _lib.call('bdn_sample_patches_aug', self.table.data_ptr(), _lib.host_int32(self.hw), len(self.hw), C, _lib.host_int32(desc),
                  desc_dev.data_ptr(), n, S, o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), keys_dev.data_ptr(), *pol.abi_args(),
                  _lib.ptr(geom), _lib.ptr(radio), _lib.stream_ptr())
        torch.cuda.synchronize()
        return (o1.cpu().numpy(), o2.cpu().numpy(), ol.cpu().numpy(), geom.cpu().numpy() if export else None,
                radio.cpu().numpy() if export else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_exact(got, ref, what):
    o1, o2, ol, geom, radio = got
    for k, r in enumerate(ref):
        assert geom[k].tolist() == r['geom'], (what, k, geom[k].tolist(), r['geom'])
        assert np.array_equal(_bits(radio[k]), _bits(r['radio'])), (what, k, 'radio')
        assert np.array_equal(ol[k], r['labels']), (what, k, 'labels')
        assert np.array_equal(_bits(o1[k]), _bits(r['x'][0])), (what, k, 'date 1')
        assert np.array_equal(_bits(o2[k]), _bits(r['x'][1])), (what, k, 'date 2')


# ---------------------------------------------------------------- every policy without noise: exact bits
@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_draws_labels_and_images_match_the_reference_bit_for_bit(S, C):
    assert_coverage(S)
    cities = host_cities(S, C)
    dev = Device(S, C, cities)
    keys, desc = keys_of(S), descriptors(S)
    policies = {
        'full': full_policy(S),
        'geometry only': PatchAugment(seed=SEED, jitter=J, symmetry=True),
        'jitter, descriptor symmetries, shared dates': full_policy(S, symmetry=False, per_date=False, erase_p=0.0),
        'gain only, labels kept': full_policy(S, jitter=0, bias=0.0, erase_label=None, erase_fill=0.0),
        'bias only': full_policy(S, gain=0.0, erase_p=0.0),
        'whole patch erased': full_policy(S, erase_p=1.0, erase_size=(S, S)),
        'one pixel erased': full_policy(S, gain=0.0, bias=0.0, erase_p=1.0, erase_size=(1, 1), erase_label=0),
    }
    for what, pol in policies.items():
        ref = R.reference_batch(pol, keys, desc, cities, S)
        _assert_exact(dev.run(pol, keys, desc), ref, what)
    full = R.reference_batch(policies['full'], keys, desc, cities, S)
    assert any(not np.array_equal(r['radio'][0], r['radio'][1]) for r in full)                          # per-date draws differ ...
    shared = R.reference_batch(policies['jitter, descriptor symmetries, shared dates'], keys, desc, cities, S)
    assert all(np.array_equal(r['radio'][0], r['radio'][1]) for r in shared)                            # ... unless shared
    assert [r['geom'][2] for r in shared] == list(range(8))
    # without the exports nothing else changes
    got = dev.run(policies['full'], keys, desc, export=False)
    for k, r in enumerate(full):
        assert np.array_equal(_bits(got[0][k]), _bits(r['x'][0])) and np.array_equal(_bits(got[1][k]), _bits(r['x'][1]))
        assert np.array_equal(got[2][k], r['labels'])


# ---------------------------------------------------------------- every stage off: the bits of bdn_sample_patches
@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_all_stages_off_gives_the_bits_of_sample_patches(S, C):
    cities = host_cities(S, C, special=True)
    dev = Device(S, C, cities)
    desc = []
    for city, (h, w) in enumerate(shapes(S)):
        desc += [(city, r, c, sym) for sym in range(8) for r, c in ((0, 0), (h - S, w - S))]
    desc = np.array(desc, np.int32)
    keys = np.array([R.sample_key(EPOCH, i) for i in range(len(desc))], np.uint64)
    off = PatchAugment(seed=SEED, symmetry=False)
    a1, a2, al, geom, radio = dev.run(off, keys, desc)
    p1, p2, pl, _, _ = dev.run(off, keys, desc, plain=True)
    assert np.array_equal(_bits(a1), _bits(p1)) and np.array_equal(_bits(a2), _bits(p2)) and np.array_equal(al, pl)
    assert np.isnan(p1).any() and (_bits(p1) == 0x80000000).any() and np.isinf(p1).any()          # the specials are in the windows
    assert np.array_equal(geom[:, :3], desc[:, 1:]) and not geom[:, 3:].any()
    assert np.array_equal(radio, np.broadcast_to(np.array([1.0, 0.0], np.float32), radio.shape))
    # geometric stages alone move bit patterns too: NaN payloads and -0.0 arrive unchanged (erase fill -0.0)
    geo = PatchAugment(seed=SEED, jitter=J, symmetry=True, erase_p=0.5, erase_size=(1, S), erase_fill=-0.0)
    ref = R.reference_batch(geo, keys[:8], desc[3::8], cities, S)
    _assert_exact(dev.run(geo, keys[:8], desc[3::8]), ref, 'geometry on special values')
    assert any(r['geom'][3] for r in ref)
    assert all((_bits(r['x'])[:, :, r['mask']] == 0x80000000).all() for r in ref if r['geom'][3])


# ---------------------------------------------------------------- the batch a sample arrives in does not matter
@pytest.mark.parametrize('S', [12, 70])
@guarded
def test_the_same_keys_in_batches_of_1_3_and_all_give_the_same_bits(S):
    C = 3
    cities = host_cities(S, C)
    dev = Device(S, C, cities)
    keys, desc = keys_of(S), descriptors(S)
    pol = full_policy(S, noise_std=0.05)
    whole = dev.run(pol, keys, desc)
    for size in (1, 3):
        parts = [dev.run(pol, keys[b:b + size], desc[b:b + size]) for b in range(0, N, size)]
        for f, name in enumerate(('date 1', 'date 2', 'labels', 'geom', 'radio')):
            joined = np.concatenate([p[f] for p in parts])
            assert joined.dtype == whole[f].dtype and np.array_equal(joined.view(np.uint8), whole[f].view(np.uint8)), (size, name)
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])                                   # and neither does its position in the batch
    perm = dev.run(pol, keys[order], desc[order])
    for f in range(5):
        assert np.array_equal(perm[f].view(np.uint8), whole[f][order].view(np.uint8))


# ---------------------------------------------------------------- noise: float64 Box-Muller of the same words
# Only z may deviate from the reference: the bar is |out - ref| <= sigma * TOL + 1 ulp(ref).  Derived expectation: |z| <= 5.8, ln, sqrt,
# sin / cos each within a few float32 ulp, so |z - z64| of order 1e-6.  TOL is the maximum of |z - z64| measured over this test's inputs
# (printed below; sigma = 1 on zero images gives out = z exactly), times 4 for unseen arguments, rounded up to a power of two; as a
# condition TOL <= 1e-4, anything larger being a wrong formula and not rounding.
TOL = 2.0 ** -18          # measured maximum 5.97e-7 (S = 64, C = 13; 3.3e-7 .. 6.0e-7 over the six cases), x 4 = 2.4e-6 <= 2^-18 = 3.8e-6


@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_noise_is_the_float64_box_muller_of_the_same_words(S, C):
    assert TOL <= 1e-4
    cities = host_cities(S, C)
    dev = Device(S, C, cities)
    keys, desc = keys_of(S), descriptors(S)
    sigma = 0.3
    for what, pol in (('full + noise', full_policy(S, noise_std=sigma)), ('noise only', PatchAugment(seed=SEED, symmetry=False, noise_std=sigma))):
        ref = R.reference_batch(pol, keys, desc, cities, S)
        o1, o2, ol, geom, radio = dev.run(pol, keys, desc)
        worst = 0.0
        for k, r in enumerate(ref):
            assert geom[k].tolist() == r['geom'] and np.array_equal(_bits(radio[k]), _bits(r['radio'])) and np.array_equal(ol[k], r['labels'])
            out = np.stack([o1[k], o2[k]])
            assert np.array_equal(_bits(out[:, :, r['mask']]), _bits(r['x'][:, :, r['mask']])), (what, k, 'erased pixels are exact')
            err = np.abs(out.astype(np.float64) - r['x64'])
            bar = float(np.float32(sigma)) * TOL + np.spacing(np.abs(r['x64']).astype(np.float32)).astype(np.float64)
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (what, k, float(err.max()), float((err / bar).max()))
        print(f'noise S={S} C={C} {what}: worst error / bar = {worst:.3f}')
    # z itself: sigma = 1 on zero images, nothing else on -> out = 0 + 1 * z = z
    zero = [{'images': np.zeros_like(c['images']), 'labels': c['labels']} for c in cities]
    zdev = Device(S, C, zero)
    pol = PatchAugment(seed=SEED, symmetry=False, noise_std=1.0)
    o1, o2, _, _, _ = zdev.run(pol, keys, desc)
    z64 = np.stack([np.stack([R.noise_z64(SEED, int(k), p, S) for p in range(2 * C)]).reshape(2, C, S, S) for k in keys])
    z = np.stack([o1, o2], 1).astype(np.float64)
    dz = float(np.abs(z - z64).max())
    print(f'noise S={S} C={C}: max |z - z64| = {dz:.3e}, max |z| = {float(np.abs(z).max()):.3f}')
    assert dz * 4 <= TOL, dz
    # the field is a function of the output coordinates: the symmetry that is drawn does not move it
    sym = PatchAugment(seed=SEED, symmetry=True, noise_std=1.0)
    s1, s2, _, g, _ = zdev.run(sym, keys, desc)
    assert len(set(g[:, 2].tolist())) == 8
    assert np.array_equal(_bits(s1), _bits(o1)) and np.array_equal(_bits(s2), _bits(o2))


# ---------------------------------------------------------------- ranks
def test_two_ranks_together_give_the_samples_of_one():
    from fabric_amd.device_loader import DevicePatchLoader
    from fabric_amd.parallel import ShardSampler
    from fabric_amd.utils.dataloaders import OneraPreloader, synthetic_onera
    data = synthetic_onera(n_cities=3, bands=3, size=(60, 52), seed=5)
    meta = [[c, i, j] for c in sorted(data) for i in range(0, 60 - 16, 11) for j in range(0, 52 - 16, 9)]
    ds = OneraPreloader('', meta, data, 16, aug=True)
    pol = PatchAugment(seed=SEED, jitter=5, gain=0.2, bias=0.1, noise_std=0.05, erase_p=0.5, erase_size=(2, 9), erase_label=255)

    def samples(rank, world, bs, epoch):
        sampler = ShardSampler(len(ds), rank, world, seed=3)
        sampler.set_epoch(epoch)
        loader = DevicePatchLoader(ds, data, bs, sampler=sampler, augment=pol, export_drawn=True)
        out = {}
        idx = list(sampler)
        k = 0
        for x1, x2, y in loader:
            geom, radio = loader.last_drawn
            for b in range(x1.shape[0]):
                out[idx[k]] = tuple(t[b].cpu().numpy().copy() for t in (x1, x2, y, geom, radio))
                k += 1
        assert k == len(idx)
        return out

    for epoch in (0, 2):
        one = samples(0, 1, 7, epoch)
        two = {**samples(0, 2, 4, epoch), **samples(1, 2, 5, epoch)}
        assert len(two) == (len(ds) // 2) * 2 and set(two) <= set(one)
        for i, parts in two.items():
            for a, b in zip(parts, one[i]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (epoch, i)
    assert any(not np.array_equal(samples(0, 1, 7, 0)[i][3], one[i][3]) for i in one)          # another epoch, other draws
