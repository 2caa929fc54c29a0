"""CPU tests of the patch warp: PatchWarp and its refusals, the argument refusals of bdn_sample_patches_warp (fake device pointers: nothing
reaches a device), header / signature agreement, the CLI flags, and the properties of the numpy twin (tests/warp_ref.py) that the GPU
tests rely on."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from fabric_amd import _lib
from fabric_amd.augment import PatchAugment, PatchWarp
from tests import augment_ref as R
from tests import warp_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DEV = 1 << 20          # a non-null, aligned stand-in for device pointers: every call below fails validation first


# ---------------------------------------------------------------- PatchWarp
def test_patch_warp_defaults_and_abi():
    p = PatchWarp()
    assert p.off and p.abi_args() == (0.0, 0.0, 0.0, 0.0, -1)
    assert (p.rotate, p.scale, p.misreg, p.oob_label) == (0.0, (1.0, 1.0), 0.0, None)
    p = PatchWarp(rotate=30, scale=(0.5, 2), misreg=0.75, oob_label=255)
    assert not p.off and p.abi_args() == (math.radians(30.0), -1.0, 1.0, 0.75, 255)
    assert PatchWarp(rotate=180, scale=(0.125, 8), misreg=64, oob_label=0).abi_args() == (math.pi, -3.0, 3.0, 64.0, 0)
    assert PatchWarp(oob_label=255).off                                       # the label byte alone warps nothing
    assert not PatchWarp(rotate=1e-3).off and not PatchWarp(scale=(1.0, 1.5)).off and not PatchWarp(misreg=0.5).off
    assert repr(p) == 'PatchWarp(rotate=30.0, scale=(0.5, 2.0), misreg=0.75, oob_label=255)'
    assert eval(repr(p)).abi_args() == p.abi_args()


@pytest.mark.parametrize('kw', [dict(rotate=-1), dict(rotate=180.5), dict(rotate=float('nan')), dict(rotate=float('inf')), dict(rotate='x'),
                                dict(scale=1.0), dict(scale=(1.0,)), dict(scale=(0.1, 1.0)), dict(scale=(1.0, 8.5)), dict(scale=(2.0, 1.0)),
                                dict(scale=(float('nan'), 1.0)), dict(scale=(0.0, 1.0)), dict(misreg=-0.5), dict(misreg=64.5),
                                dict(misreg=float('nan')), dict(oob_label=-1), dict(oob_label=256), dict(oob_label=1.0), dict(oob_label=True)])
def test_patch_warp_refuses(kw):
    with pytest.raises(ValueError, match='PatchWarp: '):
        PatchWarp(**kw)


# ---------------------------------------------------------------- the entry point
def test_header_signature_and_library_agree_on_the_new_entry():
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'int bdn_sample_patches_warp\((.*?)\);', hdr, re.S)
    assert m, 'bdn_sample_patches_warp is not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    host, hostf = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    table = {'const int32_t* city_hw_host': host, 'const int32_t* desc_host': host, 'const float* warp_host': hostf, 'int': ctypes.c_int,
             'float': ctypes.c_float, 'uint64_t': ctypes.c_uint64}
    want = []
    for p in params:
        ty = p.rsplit(' ', 1)[0]
        want.append(table.get(p) or table.get(ty) or (ctypes.c_void_p if ty.endswith('*') else None))
    assert None not in want, params
    res, args = _lib.SIGNATURES['bdn_sample_patches_warp']
    assert res is ctypes.c_int and args == want
    aug = _lib.SIGNATURES['bdn_sample_patches_aug'][1]
    assert args[:len(aug) - 1] == aug[:-1], 'the arguments of bdn_sample_patches_aug up to and including its two exports'
    assert args[len(aug) - 1:] == [ctypes.c_float] * 4 + [ctypes.c_int, hostf, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'bdn_sample_patches_warp')
    assert 'utils/dataloaders.py:148-165' in hdr[:m.start()][-5000:]                    # the reference call site it extends
    core = open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'philox_core.hpp')).read()
    assert re.search(r'PHILOX_WARP = 0x57415250u', core) and WR.WARP == 0x57415250


def test_the_warp_stream_collides_with_no_noise_stream():
    for C in range(1, 65):
        assert WR.WARP not in range(R.NOISE, R.NOISE + 2 * C) and WR.WARP not in (R.GEOMETRY, R.RADIOMETRY)
    assert WR.WARP > R.NOISE + 2 * 64


GOOD_POLICY = dict(seed=5, J=3, flags=3, gain=0.1, bias=0.1, sigma=0.1, erase_p=0.5, lo=2, hi=6, erase_label=255, erase_fill=0.0)
GOOD_WARP = dict(rotate_rad=0.5, log2_lo=-0.5, log2_hi=0.5, misreg=1.0, oob_label=255)
IDENT2 = np.ascontiguousarray(np.broadcast_to(WR.IDENTITY, (2, 2, 6)))


def _call(desc=((0, 0, 0, 0), (1, 18, 38, 7)), hw=((40, 36), (30, 50)), S=12, C=3, keys=FAKE_DEV, geom=None, radio=None, records=None,
          rec_dev=None, out=None, **kw):
    p = dict(GOOD_POLICY, **{k: v for k, v in kw.items() if k in GOOD_POLICY})
    w = dict(GOOD_WARP, **{k: v for k, v in kw.items() if k in GOOD_WARP})
    assert set(kw) <= set(p) | set(w)
    hw = np.ascontiguousarray(hw, dtype=np.int32)
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 4)
    rec = None if records is None else np.ascontiguousarray(records, np.float32)
    _lib.call('bdn_sample_patches_warp', FAKE_DEV, _lib.host_int32(hw), len(hw), C, _lib.host_int32(desc), FAKE_DEV, len(desc), S,
              FAKE_DEV, FAKE_DEV, FAKE_DEV, keys, p['seed'], p['J'], p['flags'], p['gain'], p['bias'], p['sigma'], p['erase_p'], p['lo'], p['hi'],
              p['erase_label'], p['erase_fill'], geom, radio, w['rotate_rad'], w['log2_lo'], w['log2_hi'], w['misreg'], w['oob_label'],
              _lib.host_float32(rec), rec_dev, out, None)


def _record(entry, value):
    rec = IDENT2.copy()
    rec.reshape(-1)[entry] = value
    return rec


@pytest.mark.parametrize('kw, msg', [
    (dict(rotate_rad=-0.1), 'rotate_rad'),
    (dict(rotate_rad=3.2), 'rotate_rad'),
    (dict(rotate_rad=float('nan')), 'rotate_rad'),
    (dict(log2_lo=-3.5), 'scale'),
    (dict(log2_hi=3.5), 'scale'),
    (dict(log2_lo=0.75), 'scale'),
    (dict(log2_lo=float('nan')), 'scale'),
    (dict(misreg=-1.0), 'misreg'),
    (dict(misreg=64.5), 'misreg'),
    (dict(misreg=float('inf')), 'misreg'),
    (dict(oob_label=-2), 'oob_label -2'),
    (dict(oob_label=256), 'oob_label 256'),
    (dict(records=IDENT2), 'warp_host and warp_dev go together'),
    (dict(rec_dev=FAKE_DEV), 'warp_host and warp_dev go together'),
    (dict(records=IDENT2, rec_dev=FAKE_DEV + 2), '4-byte aligned'),
    (dict(out=FAKE_DEV + 1), '4-byte aligned'),
    (dict(records=_record(0, float('nan')), rec_dev=FAKE_DEV), 'warp record 0: entry 0 is not finite'),
    (dict(records=_record(17, float('inf')), rec_dev=FAKE_DEV), 'warp record 1: entry 5 is not finite'),
    (dict(records=_record(1, 8.5), rec_dev=FAKE_DEV), 'warp record 0: entry 1 = 8.5 outside'),
    (dict(records=_record(16, -9.0), rec_dev=FAKE_DEV), 'warp record 1: entry 4 = -9 outside'),
    (dict(records=_record(8, 2.0 ** 20 + 1), rec_dev=FAKE_DEV), 'warp record 0: entry 8'),
    (dict(records=_record(23, -2.0 ** 21), rec_dev=FAKE_DEV), 'warp record 1: entry 11'),
    # and the policy checks it shares with bdn_sample_patches_aug, under its own name
    (dict(J=-1), 'jitter J=-1'),
    (dict(sigma=-0.5), 'sigma >= 0'),
    (dict(hi=13), 'hi=13 S=12'),
    (dict(keys=None), 'null pointer'),
    (dict(geom=FAKE_DEV + 2), '4-byte aligned'),
])
def test_sample_patches_warp_refuses(kw, msg):
    with pytest.raises(RuntimeError, match=f'sample_patches_warp: .*{re.escape(msg)}'):
        _call(**kw)


def test_sample_patches_warp_validates_the_descriptor_and_accepts_records_at_the_bounds():
    """A record at the validation bounds passes the record check: the call then fails later, on the descriptor."""
    rec = IDENT2.copy()
    rec[:, :, [0, 1, 3, 4]] = [8.0, -8.0, 8.0, -8.0]
    rec[:, :, [2, 5]] = [2.0 ** 20, -2.0 ** 20]
    with pytest.raises(RuntimeError, match='sample_patches_warp: descriptor 1: row 19'):
        _call(desc=((0, 0, 0, 0), (1, 19, 0, 0)), records=rec, rec_dev=FAKE_DEV, rotate_rad=math.pi, log2_lo=-3.0, log2_hi=3.0, misreg=64.0)
    with pytest.raises(RuntimeError, match='host table'):
        _lib.host_float32(np.zeros((2, 2, 6), np.float64))


# ---------------------------------------------------------------- reference properties
def _city(H, W, C=2, seed=0):
    r = np.random.default_rng(seed)
    return {'images': r.standard_normal((2, C, H, W)).astype(np.float32), 'labels': r.integers(0, 200, (H, W)).astype(np.uint8)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


OFF = PatchAugment(seed=9, symmetry=False)


@pytest.mark.parametrize('S', [5, 12])
def test_an_identity_record_returns_the_symmetry_crop(S):
    city = _city(S + 7, S + 4)
    for sym in range(8):
        for row, col in ((0, 0), (7, 4), (3, 2)):
            r = WR.reference_sample(OFF, PatchWarp(oob_label=255), WR.IDENTITY, 1, (0, row, col, sym), [city], S)
            assert np.array_equal(_bits(r['x']), _bits(R.symmetry(city['images'][:, :, row:row + S, col:col + S], sym)))
            assert np.array_equal(r['labels'], R.symmetry(city['labels'][row:row + S, col:col + S], sym)) and not r['outside'].any()


@pytest.mark.parametrize('S', [5, 12])
def test_the_four_quarter_turn_records_are_symmetry_codes(S):
    city = _city(S + 7, S + 4, seed=1)
    for q, sym in {0: 0, 1: 5, 2: 3, 3: 6}.items():
        for row, col in ((0, 0), (7, 4), (3, 2)):
            r = WR.reference_sample(OFF, PatchWarp(oob_label=255), WR.rotation_record(q), 1, (0, row, col, 0), [city], S)
            assert np.array_equal(_bits(r['x']), _bits(R.symmetry(city['images'][:, :, row:row + S, col:col + S], sym))), q
            assert np.array_equal(r['labels'], R.symmetry(city['labels'][row:row + S, col:col + S], sym)) and not r['outside'].any()
        # and they compose with the descriptor's own code as the dihedral group does: a quarter turn of a transposed window
        r = WR.reference_sample(OFF, PatchWarp(), WR.rotation_record(q), 1, (0, 2, 1, 4), [city], S)
        win = np.swapaxes(WR.reference_sample(OFF, PatchWarp(), WR.rotation_record(q), 1, (0, 2, 1, 0), [city], S)['x'], -1, -2)
        assert np.array_equal(_bits(r['x']), _bits(win))


def test_an_integer_translation_is_the_shifted_replicate_clamped_crop():
    S = 8
    city = _city(S + 5, S + 3, seed=2)
    H, W = city['labels'].shape
    for t in ((0, 0), (3, -2), (-4, 1), (S, S), (-20, 30)):
        for row, col in ((0, 0), (5, 3), (2, 1)):
            rec = WR.rotation_record(0, t)
            r = WR.reference_sample(OFF, PatchWarp(oob_label=None), rec, 1, (0, row, col, 0), [city], S)
            rows, cols = np.clip(row + t[0] + np.arange(S), 0, H - 1), np.clip(col + t[1] + np.arange(S), 0, W - 1)
            assert np.array_equal(_bits(r['x'][1]), _bits(city['images'][1][:, rows[:, None], cols[None, :]])), t
            assert np.array_equal(_bits(r['x'][0]), _bits(city['images'][0][:, row:row + S, col:col + S]))            # date 1 stays
            assert np.array_equal(r['labels'], city['labels'][row:row + S, col:col + S])                              # and so do the labels
    # labels follow date 1's record, and outside pixels become oob_label only when it is set
    both = np.array([[1, 0, 3, 0, 1, -2]] * 2, np.float32)
    kept = WR.reference_sample(OFF, PatchWarp(oob_label=None), both, 1, (0, 5, 0, 0), [city], S)
    marked = WR.reference_sample(OFF, PatchWarp(oob_label=255), both, 1, (0, 5, 0, 0), [city], S)
    assert kept['outside'].sum() == S * S - (S - 3) * (S - 2) and np.array_equal(kept['outside'], marked['outside'])
    assert (marked['labels'][marked['outside']] == 255).all()
    assert np.array_equal(marked['labels'][~marked['outside']], kept['labels'][~kept['outside']])
    assert np.array_equal(kept['labels'], city['labels'][np.clip(8 + np.arange(S), 0, H - 1)[:, None], np.clip(np.arange(S) - 2, 0, W - 1)[None, :]])


def test_a_half_pixel_shift_is_the_mean_of_two_neighbours():
    S = 6
    city = _city(S + 2, S + 2, seed=3)
    r = WR.reference_sample(OFF, PatchWarp(), WR.rotation_record(0, (0.5, 0.0)), 1, (0, 0, 1, 0), [city], S)
    im = city['images'][1]
    want = np.float32(0.5) * im[:, 0:S, 1:1 + S] + np.float32(0.5) * im[:, 1:S + 1, 1:1 + S]
    assert np.array_equal(_bits(r['x'][1]), _bits(want))


def test_every_tap_lies_in_the_city_for_records_at_the_validation_bounds():
    """The clamp, not the record, keeps addresses in range; the float -> int conversions stay far inside int32."""
    S, H, W = 70, 75, 71
    for a in (8.0, -8.0):
        for t in (2.0 ** 20, -2.0 ** 20):
            rec = np.array([a, -a, t, a, a, -t], np.float32)
            for sym in (0, 5):
                iy, ix, fy, fx = WR.taps(rec, S, sym, 3, 1, H, W)
                assert max(np.abs(iy).max(), np.abs(ix).max()) < 2 ** 21 + 16 * S
                assert ((fy >= 0) & (fy < 1) & (fx >= 0) & (fx < 1)).all()
                for v, n in ((iy, H), (iy + 1, H), (ix, W), (ix + 1, W)):
                    c = np.clip(v, 0, n - 1)
                    assert c.min() >= 0 and c.max() <= n - 1
                out = WR.gather_plane(np.arange(H * W, dtype=np.float32).reshape(H, W), rec, S, sym, 3, 1)
                assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= H * W - 1
                ly, lx = WR.label_taps(rec, S, sym, 3, 1)
                assert max(np.abs(ly).max(), np.abs(lx).max()) < 2 ** 21 + 16 * S


def test_the_record_formula_and_its_exact_half():
    warp = PatchWarp(rotate=30, scale=(0.75, 1.5), misreg=1.5)
    seen = set()
    for index in range(64):
        key = R.sample_key(1, index)
        rec, d = WR.record64(warp, 7, key), WR.drawn(warp, 7, key)
        assert abs(d['theta']) <= math.radians(30) * (1 + 1e-7) and 0.75 * (1 - 1e-7) <= d['s'] <= 1.5 * (1 + 1e-7)
        assert abs(d['t_i']) <= 1.5 and abs(d['t_j']) <= 1.5
        assert np.allclose(rec[0, [0, 1, 3, 4]], np.array([math.cos(d['theta']), -math.sin(d['theta']), math.sin(d['theta']), math.cos(d['theta'])]) / d['s'])
        assert np.array_equal(rec[0, [0, 1, 3, 4]], rec[1, [0, 1, 3, 4]]) and not rec[0, [2, 5]].any()
        ti, tj = WR.record_shift32(warp, 7, key)
        assert ti.dtype == np.float32 and abs(float(ti) - d['t_i']) <= np.spacing(np.float32(1.5)) / 2 and abs(float(tj) - rec[1, 5]) <= np.spacing(np.float32(1.5)) / 2
        seen.add((d['theta'] > 0, d['s'] > 1))
    assert len(seen) == 4
    off = WR.record64(PatchWarp(), 7, R.sample_key(1, 3))
    assert np.array_equal(off, WR.IDENTITY.astype(np.float64))                # an off policy draws the identity


# ---------------------------------------------------------------- the GPU tests' fixtures
@pytest.mark.parametrize('S', [12, 64, 70])
def test_the_gpu_tests_committed_keys_cover_their_cases(S):
    """The sample keys of tests/test_gpu_warp.py are constants: here, without a device, they are the output of the search that made them
    and they cover what that file says they cover; the share of label pixels outside the city is above 0 and below one half."""
    from tests import test_gpu_warp as G
    G.assert_coverage(S)
    assert G.search_keys(S) == G.INDICES[S]
    assert 0.0 < G.out_of_city_share(S) < 0.5


# ---------------------------------------------------------------- CLI
def test_train_cli_refuses_warp_flags_without_device_patches():
    from fabric_amd.train import main
    for flags in (['--aug_rotate', '15'], ['--aug_scale', '0.8', '1.25'], ['--aug_misreg', '0.5']):
        with pytest.raises(SystemExit, match=f'{flags[0]} augment the patches the device cuts: add --device_patches true'):
            main(['--synthetic'] + flags)
    with pytest.raises(SystemExit, match='PatchWarp: rotate'):
        main(['--synthetic', '--device_patches', 'true', '--aug_rotate', '181'])
    with pytest.raises(SystemExit, match='PatchWarp: scale'):
        main(['--synthetic', '--device_patches', 'true', '--aug_scale', '2', '1'])
    with pytest.raises(SystemExit, match='PatchWarp: misreg'):
        main(['--synthetic', '--device_patches', 'true', '--aug_misreg', '65'])


def test_train_cli_builds_the_policies_from_the_warp_flags(monkeypatch):
    from fabric_amd import train as T
    seen = {}
    real_aug, real_warp = T.augment_from_opt, T.warp_from_opt

    def aug(opt):
        seen['augment'] = real_aug(opt)
        return seen['augment']

    def warp(opt):
        seen['warp'] = real_warp(opt)
        raise SystemExit('parsed')                             # stop before anything asks for a device

    monkeypatch.setattr(T, 'augment_from_opt', aug)
    monkeypatch.setattr(T, 'warp_from_opt', warp)
    with pytest.raises(SystemExit, match='parsed'):
        T.main(['--synthetic', '--device_patches', 'true', '--fused_step', 'true', '--ignore_label', '255', '--seed', '4', '--aug_rotate', '20',
                '--aug_scale', '0.8', '1.25', '--aug_misreg', '0.5'])
    assert repr(seen['warp']) == repr(PatchWarp(rotate=20.0, scale=(0.8, 1.25), misreg=0.5, oob_label=255))
    assert repr(seen['augment']) == repr(PatchAugment(seed=4, erase_label=255))          # the other stages at their defaults
    seen.clear()
    with pytest.raises(SystemExit, match='parsed'):
        T.main(['--synthetic', '--device_patches', 'true', '--augmentation', 'false', '--aug_misreg', '0.5'])
    assert repr(seen['warp']) == repr(PatchWarp(misreg=0.5)) and not seen['augment'].symmetry and seen['augment'].erase_label is None
    # without a warp flag no PatchWarp is built, and without any --aug flag neither policy is
    assert real_warp(type('O', (), dict(aug_rotate=0.0, aug_scale=None, aug_misreg=0.0, ignore_label=None))()) is None
