"""bdn_sample_patches_warp on the device against its numpy twin (tests/warp_ref.py): bit for bit wherever the specification is exact, which
is everything downstream of the warp record; the record's rotation / zoom entries under a measured bar.

Shapes, cities, descriptors, the augment policy and the guarded Device follow tests/test_gpu_augment.py: S = 12 (below one 64 x 64 tile), 64
(exactly one), 70 (a ragged 2 x 2 of tiles); C = 3 and 13; eight samples over four cities, one of exactly S x S.  Inputs are finite (the
interpolation does not preserve NaN or inf, by specification).  The sample keys are constants found by `search_keys` on the CPU;
`assert_coverage` states, on the reference's own draws and before the device is touched, what they were searched for.
"""
import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.augment import PatchAugment, PatchWarp
from tests import augment_ref as R
from tests import guard
from tests import warp_ref as WR
from tests.guard import guarded
from tests.test_gpu_augment import EPOCH, N, SEED, TOL, _bits, descriptors, full_policy, host_cities, shapes

pytestmark = pytest.mark.gpu

# misreg <= 1.5 keeps ulp(t) <= ulp(1 / s_min) = ulp(4 / 3); 30 degrees and a zoom in [0.75, 1.5] push the S x S city's corners out
WARP = PatchWarp(rotate=30.0, scale=(0.75, 1.5), misreg=1.5, oob_label=255)
# dataset indices whose keys (EPOCH << 32 | index) give, under full_policy(S) and WARP: sample 0 a positive angle, 1 a negative one,
# 2 a zoom below 1, 3 a zoom above 1 with every tap inside the city, 4-7 a footprint that leaves the city at the top / bottom / left /
# right.  Output of search_keys(S): the warp draws do not depend on S, and these eight meet the conditions at every S.
INDICES = {S: [0, 3, 9, 1, 4, 13, 10, 8] for S in (12, 64, 70)}


def _footprint(S, index, k):
    """What the reference draws for slot k with this dataset index: the drawn warp, the unclamped tap ranges of both dates and labels."""
    pol = full_policy(S)
    city, row, col, sym = (int(v) for v in descriptors(S)[k])
    H, W = shapes(S)[city]
    key = R.sample_key(EPOCH, index)
    g = R.geometry(pol, key, row, col, sym, H, W, S)
    rec = WR.record64(WARP, SEED, key).astype(np.float32)
    iy, ix = [], []
    for d in range(2):
        ty, tx, _, _ = WR.taps(rec[d], S, g['sym'], g['row'], g['col'], H, W)
        iy += [ty, ty + 1]
        ix += [tx, tx + 1]
    iy, ix = np.stack(iy), np.stack(ix)
    ly, lx = WR.label_taps(rec[0], S, g['sym'], g['row'], g['col'])
    outside = (ly < 0) | (ly > H - 1) | (lx < 0) | (lx > W - 1)
    ty, tx, _, _ = WR.taps(rec[0], S, g['sym'], g['row'], g['col'], H, W)
    span = 0                                                  # the largest tap extent of one 64 x 64 OUTPUT tile, rows or columns
    for a in range(0, S, 64):
        for b in range(0, S, 64):
            span = max(span, int(ty[a:a + 64, b:b + 64].max() + 1 - ty[a:a + 64, b:b + 64].min()) + 1,
                       int(tx[a:a + 64, b:b + 64].max() + 1 - tx[a:a + 64, b:b + 64].min()) + 1)
    d = WR.drawn(WARP, SEED, key)
    return dict(d, top=bool((iy < 0).any()), bottom=bool((iy > H - 1).any()), left=bool((ix < 0).any()), right=bool((ix > W - 1).any()),
                outside=outside, span=span)


def _wanted(k, f):
    inside = not (f['top'] or f['bottom'] or f['left'] or f['right'] or f['outside'].any())
    return (f['theta'] > 0, f['theta'] < 0, f['s'] < 1, f['s'] > 1 and inside, f['top'], f['bottom'], f['left'], f['right'])[k]


def search_keys(S, pool=5000):
    """CPU only: the first dataset index per sample slot that meets _wanted (distinct indices).  How INDICES was made."""
    out = []
    for k in range(N):
        for index in range(pool):
            if index not in out and _wanted(k, _footprint(S, index, k)):
                out.append(index)
                break
        else:
            raise AssertionError(f'no index for slot {k}')
    return out


def out_of_city_share(S):
    fs = [_footprint(S, i, k) for k, i in enumerate(INDICES[S])]
    return float(np.mean([f['outside'].mean() for f in fs]))


def assert_coverage(S):
    """A condition of the tests, checked on the reference's draws: an uncovered case fails here instead of passing silently."""
    fs = [_footprint(S, i, k) for k, i in enumerate(INDICES[S])]
    assert len(set(INDICES[S])) == N
    assert any(f['theta'] > 0 for f in fs) and any(f['theta'] < 0 for f in fs), 'both signs of the angle'
    assert any(f['s'] < 1 for f in fs) and any(f['s'] > 1 for f in fs), 'zoom below and above 1'
    for side in ('top', 'bottom', 'left', 'right'):
        assert any(f[side] for f in fs), f'a footprint leaving the city at the {side}'
    assert any(not (f['top'] or f['bottom'] or f['left'] or f['right'] or f['outside'].any()) for f in fs), 'a sample wholly inside'
    assert any(f['t_i'] != 0 and f['t_j'] != 0 for f in fs), 'date 2 shifted on both axes'
    # an output tile whose taps span more than 64 source rows or columns covers more than one 64 x 64 source tile.  A 12-pixel patch
    # cannot: its footprint is at most 12 * sqrt(2) / 0.75 + 2 < 25 pixels across.
    if S >= 64:
        assert any(f['span'] > 64 for f in fs), 'a footprint beyond one 64 x 64 source tile'
    share = out_of_city_share(S)
    assert 0.0 < share < 0.5, share


@pytest.mark.parametrize('S', [12, 64, 70])
def test_committed_keys_cover_the_cases(S):
    assert_coverage(S)


def keys_of(S):
    return np.array([R.sample_key(EPOCH, i) for i in INDICES[S]], np.uint64)


class Device:
    """The guarded device side of one (S, C): cities, their table, and fresh outputs per run."""

    def __init__(self, S, C, cities):
        self.S, self.C = S, C
        self.dev = [{k: guard.guard(torch.from_numpy(v)) for k, v in c.items()} for c in cities]
        rec = np.array([[d['images'].data_ptr(), d['labels'].data_ptr(), h | (w << 32)] for d, (h, w) in zip(self.dev, shapes(S))], np.int64)
        self.table = guard.guard(torch.from_numpy(rec))
        self.hw = np.array(shapes(S), np.int32)

    def _outputs(self, n):
        S, C = self.S, self.C
        o1 = guard.full((n, C, S, S), float('nan'))
        return o1, guard.full_like(o1, float('nan')), guard.full((n, S, S), 77, dtype=torch.uint8)

    def run(self, pol, warp, keys, desc, records=None, entry='warp'):
        """One call on n samples -> numpy (d1, d2, labels, geom, radio, records used).  records: float32 [n][2][6] used instead of the
        drawn ones.  entry 'aug': bdn_sample_patches_aug with `pol`; 'plain': bdn_sample_patches (the last three are then None)."""
        S, C, n = self.S, self.C, len(desc)
        desc = np.ascontiguousarray(desc, np.int32)
        desc_dev = guard.guard(torch.from_numpy(desc))
        o1, o2, ol = self._outputs(n)
        if entry == 'plain':
            _lib.call('bdn_sample_patches', self.table.data_ptr(), self.hw.ctypes.data, len(self.hw), C, desc.ctypes.data, desc_dev.data_ptr(),
                      n, S, o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), _lib.stream_ptr())
            torch.cuda.synchronize()
            return o1.cpu().numpy(), o2.cpu().numpy(), ol.cpu().numpy(), None, None, None
        keys_dev = guard.guard(torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)))
        geom = guard.full((n, 8), -7, dtype=torch.int32)
        radio = guard.full((n, 2, C, 2), float('nan'))
        args = (self.table.data_ptr(), _lib.host_int32(self.hw), len(self.hw), C, _lib.host_int32(desc), desc_dev.data_ptr(), n, S,
                o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), keys_dev.data_ptr(), *pol.abi_args(), geom.data_ptr(), radio.data_ptr())
        used = None
        if entry == 'aug':
            _lib.call('bdn_sample_patches_aug', *args, _lib.stream_ptr())
        else:
            used = guard.full((n, 2, 6), float('nan'))
            rec = None if records is None else np.ascontiguousarray(records, np.float32)
            rec_dev = None if rec is None else guard.guard(torch.from_numpy(rec))
            _lib.call('bdn_sample_patches_warp', *args, *warp.abi_args(), _lib.host_float32(rec), _lib.ptr(rec_dev), used.data_ptr(),
                      _lib.stream_ptr())
        torch.cuda.synchronize()
        return (o1.cpu().numpy(), o2.cpu().numpy(), ol.cpu().numpy(), geom.cpu().numpy(), radio.cpu().numpy(),
                None if used is None else used.cpu().numpy())


def _same(a, b, what):
    for f, name in enumerate(('date 1', 'date 2', 'labels', 'geom', 'radio')):
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), (what, name)


def _assert_exact(got, ref, what, x64_bar=None):
    o1, o2, ol, geom, radio, _ = got
    for k, r in enumerate(ref):
        assert geom[k].tolist() == r['geom'], (what, k, geom[k].tolist(), r['geom'])
        assert np.array_equal(_bits(radio[k]), _bits(r['radio'])), (what, k, 'radio')
        assert np.array_equal(ol[k], r['labels']), (what, k, 'labels')
        out = np.stack([o1[k], o2[k]])
        if x64_bar is None:
            assert np.array_equal(_bits(out), _bits(r['x'])), (what, k, 'images', int((_bits(out) != _bits(r['x'])).sum()))
        else:                                                  # noise: the bar of tests/test_gpu_augment.py; erased pixels are exact
            assert np.array_equal(_bits(out[:, :, r['mask']]), _bits(r['x'][:, :, r['mask']])), (what, k, 'erased pixels')
            err = np.abs(out.astype(np.float64) - r['x64'])
            bar = x64_bar + np.spacing(np.abs(r['x64']).astype(np.float32)).astype(np.float64)
            assert (err <= bar).all(), (what, k, float(err.max()), float((err / bar).max()))


# ---------------------------------------------------------------- override: identity records are bdn_sample_patches_aug
@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_identity_records_give_the_bits_of_sample_patches_aug(S, C):
    dev = Device(S, C, host_cities(S, C))
    keys, desc = keys_of(S), descriptors(S)
    ident = np.broadcast_to(WR.IDENTITY, (N, 2, 6))
    for what, pol in (('full + noise', full_policy(S, noise_std=0.05)), ('full', full_policy(S)), ('every stage off', PatchAugment(seed=SEED, symmetry=False))):
        got = dev.run(pol, WARP, keys, desc, records=ident)
        _same(got, dev.run(pol, None, keys, desc, entry='aug'), what)
        assert np.array_equal(_bits(got[5]), _bits(ident)), 'the records used are the records given'
    # a PatchWarp that is off draws the identity itself (theta = 0, s = 2^0, t = 0 * sgn)
    got = dev.run(full_policy(S), PatchWarp(), keys, desc)
    _same(got, dev.run(full_policy(S), None, keys, desc, entry='aug'), 'off policy, drawn records')
    assert np.array_equal(got[5], ident)                      # -0.0 == 0.0: a_ij = -sinf(0) / 1


# ---------------------------------------------------------------- override: quarter turns are symmetries
QUARTER_SYM = {0: 0, 1: 5, 2: 3, 3: 6}          # out[i][j] = W[S-1-j][i] (90), W[S-1-i][S-1-j] (180), W[j][S-1-i] (270) as codes 4 t + 2 rr + rc


@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_quarter_turn_records_give_the_bits_of_the_matching_symmetry(S, C):
    dev = Device(S, C, host_cities(S, C))
    keys, desc = keys_of(S), descriptors(S)
    desc[:, 3] = 0
    off = PatchAugment(seed=SEED, symmetry=False)
    for q, sym in QUARTER_SYM.items():
        rec = np.broadcast_to(WR.rotation_record(q), (N, 2, 6))
        want = desc.copy()
        want[:, 3] = sym
        got, plain = dev.run(off, WARP, keys, desc, records=rec), dev.run(off, None, keys, want, entry='plain')
        for f, name in enumerate(('date 1', 'date 2', 'labels')):
            assert np.array_equal(got[f].view(np.uint8), plain[f].view(np.uint8)), (q, name)


# ---------------------------------------------------------------- override: date 2 alone is translated
@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_translations_of_date_2_leave_date_1_and_the_labels_alone(S, C):
    cities = host_cities(S, C)
    dev = Device(S, C, cities)
    keys, desc = keys_of(S), descriptors(S)                   # every symmetry code, windows on the four borders, the S x S city
    off = PatchAugment(seed=SEED, symmetry=False)
    base = dev.run(off, None, keys, desc, entry='plain')
    nolabel = PatchWarp(oob_label=None)
    for t in ((3.0, -2.0), (-1.0, 0.0), (0.5, 0.0), (-1.5, 2.5), (0.25, -0.75), (float(S), -float(S))):
        rec = np.broadcast_to(WR.rotation_record(0, t), (N, 2, 6))
        got = dev.run(off, nolabel, keys, desc, records=rec)
        assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(got[2], base[2]), (t, 'date 1 and the labels')
        _assert_exact(got, WR.reference_batch(off, nolabel, rec, keys, desc, cities, S), t)
        if t[0] != int(t[0]) or t[1] != int(t[1]):
            continue
        for k, (city, row, col, sym) in enumerate(desc.tolist()):          # an integer shift: the shifted crop, replicate-clamped
            im = cities[city]['images'][1]
            H, W = im.shape[1:]
            i, j = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
            ri, cj = (S - 1 - i if sym & 2 else i), (S - 1 - j if sym & 1 else j)
            ip, jp = (cj, ri) if sym & 4 else (ri, cj)
            want = im[:, np.clip(row + ip + int(t[0]), 0, H - 1), np.clip(col + jp + int(t[1]), 0, W - 1)]
            assert np.array_equal(_bits(got[1][k]), _bits(want)), (t, k)


# ---------------------------------------------------------------- drawn records against the float64 formula
# The rotation / zoom entries come from the device library's cosf, sinf and exp2f and one division each; their documented accuracy is a
# few ulp, so a measured error above 16 ulp would be a finding, not a tolerance.  Unit: the float32 ulp of 1 / s_min = 4 / 3, the
# largest magnitude an entry can have.  RECORD_ULP is four times the largest error measured over the fixture keys (see the docstring).
RECORD_ULP = 2.24          # 4 x 0.559


@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_drawn_records_match_the_float64_formula(S):
    """Measured on an MI355X over the fixture keys (the same eight at S = 12, 64 and 70; the draws do not depend on S): the largest error
    of a rotation / zoom entry against the float64 formula is 0.559 ulp of 1 / s_min.  The bar is four times that, 2.24 ulp."""
    C = 3
    dev = Device(S, C, host_cities(S, C))
    keys, desc = keys_of(S), descriptors(S)
    used = dev.run(full_policy(S), WARP, keys, desc)[5]
    ulp = float(np.spacing(np.float32(1.0 / WARP.scale[0])))
    worst = 0.0
    for k, key in enumerate(keys):
        ref = WR.record64(WARP, SEED, int(key))
        ti, tj = WR.record_shift32(WARP, SEED, int(key))
        assert np.array_equal(_bits(used[k][:, 2]), _bits(np.array([0.0, ti], np.float32))), (k, 't_i is exact')
        assert np.array_equal(_bits(used[k][:, 5]), _bits(np.array([0.0, tj], np.float32))), (k, 't_j is exact')
        assert np.array_equal(_bits(used[k][0, [0, 1, 3, 4]]), _bits(used[k][1, [0, 1, 3, 4]])), (k, 'one rotation and zoom for both dates')
        assert used[k][0, 0] == used[k][0, 4] and used[k][0, 1] == -used[k][0, 3], (k, 'a_ii = a_jj, a_ij = -a_ji')
        worst = max(worst, float(np.abs(used[k].astype(np.float64) - ref)[:, [0, 1, 3, 4]].max()) / ulp)
    print(f'warp records S={S}: largest error {worst:.3f} ulp of 1/s_min')
    assert RECORD_ULP <= 16.0
    assert worst <= RECORD_ULP, worst


# ---------------------------------------------------------------- drawn records: the mapping is exact given the record
@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [12, 64, 70])
@guarded
def test_drawn_warps_match_the_reference_bit_for_bit_given_the_records(S, C):
    assert_coverage(S)
    cities = host_cities(S, C)
    dev = Device(S, C, cities)
    keys, desc = keys_of(S), descriptors(S)
    keep = PatchWarp(rotate=WARP.rotate, scale=WARP.scale, misreg=WARP.misreg, oob_label=None)
    cases = {
        'full, outside labels 255': (full_policy(S), WARP),
        'full, outside labels kept': (full_policy(S), keep),
        'warp only': (PatchAugment(seed=SEED, symmetry=False), WARP),
        'rotation only, descriptor symmetries': (full_policy(S, symmetry=False, gain=0.0, bias=0.0, erase_p=0.0), PatchWarp(rotate=180.0, oob_label=7)),
        'zoom only': (full_policy(S, erase_p=0.0), PatchWarp(scale=(0.125, 8.0))),
        'misregistration only': (full_policy(S), PatchWarp(misreg=64.0, oob_label=255)),
    }
    outside = 0
    for what, (pol, warp) in cases.items():
        got = dev.run(pol, warp, keys, desc)
        ref = WR.reference_batch(pol, warp, got[5], keys, desc, cities, S)
        _assert_exact(got, ref, what)
        if warp is WARP:
            outside += sum(int((got[2][k] == 255).sum()) for k in range(N))
    assert outside > 0
    # every value stage on: the noise is the float64 Box-Muller of the same words, under the bar of tests/test_gpu_augment.py
    sigma = 0.3
    pol = full_policy(S, noise_std=sigma)
    got = dev.run(pol, WARP, keys, desc)
    _assert_exact(got, WR.reference_batch(pol, WARP, got[5], keys, desc, cities, S), 'full + noise', x64_bar=float(np.float32(sigma)) * TOL)
    # the drawn records are the same whatever the value stages: the warp stream is its own
    assert np.array_equal(_bits(got[5]), _bits(dev.run(PatchAugment(seed=SEED, symmetry=False), WARP, keys, desc)[5]))


# ---------------------------------------------------------------- the batch a sample arrives in does not matter
@pytest.mark.parametrize('S', [12, 70])
@guarded
def test_the_same_keys_in_other_batches_and_twice_give_the_same_bits(S):
    C = 3
    dev = Device(S, C, host_cities(S, C))
    keys, desc = keys_of(S), descriptors(S)
    pol = full_policy(S, noise_std=0.05)
    whole = dev.run(pol, WARP, keys, desc)
    again = dev.run(pol, WARP, keys, desc)
    for f in range(6):
        assert np.array_equal(again[f].view(np.uint8), whole[f].view(np.uint8)), ('two runs', f)
    for size in (1, 3):
        parts = [dev.run(pol, WARP, keys[b:b + size], desc[b:b + size]) for b in range(0, N, size)]
        for f in range(6):
            joined = np.concatenate([p[f] for p in parts])
            assert joined.dtype == whole[f].dtype and np.array_equal(joined.view(np.uint8), whole[f].view(np.uint8)), (size, f)
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])                                   # and neither does its position in the batch
    perm = dev.run(pol, WARP, keys[order], desc[order])
    for f in range(6):
        assert np.array_equal(perm[f].view(np.uint8), whole[f][order].view(np.uint8))
