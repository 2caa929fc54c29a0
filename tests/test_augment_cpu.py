"""CPU tests of patch augmentation: Philox4x32-10 known answers (numpy twin and csrc/philox_core.hpp in a stand-alone host program),
the argument refusals of bdn_sample_patches_aug and PatchAugment (nothing reaches a device), header / signature agreement, and the
properties of the reference draws that need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from fabric_amd import _lib
from fabric_amd.augment import PatchAugment
from fabric_amd.parallel import ShardSampler
from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DEV = 1 << 20          # a non-null, aligned stand-in for device pointers: every call below fails validation first

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, answer)
KAT = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]


def _hex(words):
    return ' '.join(f'{int(w):08x}' for w in words)


def test_philox_known_answers_numpy():
    for ctr, key, want in KAT:
        assert _hex(R.philox4x32_10(ctr, key)) == want
    # vectorised over counters, and draw() lays the counter out as (key_lo, key_hi, slot, stream) with the seed as the key
    ctrs = np.array([k[0] for k in KAT], np.uint32)
    assert _hex(R.philox4x32_10(ctrs[2:], KAT[2][1])[0]) == KAT[2][2]
    assert _hex(R.draw(0x299f31d0a4093822, 0x85a308d3243f6a88, 0x03707344, 0x13198a2e)) == KAT[2][2]
    assert R.draw(1, 2, 3, np.arange(5)).shape == (5, 4)


def test_philox_core_header_on_the_host(tmp_path):
    """csrc/philox_core.hpp compiled for the host in tools/philox_host_check.cpp (its own main): the same three answers, range(), the
    clamps and the rectangle at the extremes -- with AddressSanitizer and UBSan when the compiler links them."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'philox_host_check')
    base = [cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'fabric_amd', 'csrc'), os.path.join(ROOT, 'tools', 'philox_host_check.cpp'), '-o', exe]
    r = subprocess.run(base + ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if r.returncode != 0:          # a toolchain without the sanitizer runtimes: the plain build still checks the answers
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split('\n')
    assert lines[:3] == [k[2] for k in KAT] and lines[3] == 'ok'


# ---------------------------------------------------------------- refusals of the entry point
GOOD_POLICY = dict(seed=5, J=3, flags=3, gain=0.1, bias=0.1, sigma=0.1, erase_p=0.5, lo=2, hi=6, erase_label=255, erase_fill=0.0)


def _call(desc=((0, 0, 0, 0), (1, 18, 38, 7)), hw=((40, 36), (30, 50)), S=12, C=3, n=None, cities=FAKE_DEV, desc_dev=FAKE_DEV,
          outs=(FAKE_DEV,) * 3, keys=FAKE_DEV, geom=None, radio=None, **policy):
    p = dict(GOOD_POLICY, **policy)
    hw = np.ascontiguousarray(hw, dtype=np.int32)
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 4)
    _lib.call('bdn_sample_patches_aug', cities, _lib.host_int32(hw), len(hw), C, _lib.host_int32(desc), desc_dev,
              len(desc) if n is None else n, S, *outs, keys, p['seed'], p['J'], p['flags'], p['gain'], p['bias'], p['sigma'], p['erase_p'],
              p['lo'], p['hi'], p['erase_label'], p['erase_fill'], geom, radio, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(J=-1), 'jitter J=-1'),
    (dict(J=(1 << 24) + 1), 'jitter'),
    (dict(flags=4), 'unknown flags'),
    (dict(gain=float('nan')), 'finite'),
    (dict(gain=float('inf')), 'finite'),
    (dict(bias=float('-inf')), 'finite'),
    (dict(erase_fill=float('nan')), 'finite'),
    (dict(sigma=-0.5), 'sigma >= 0'),
    (dict(sigma=float('nan')), 'sigma >= 0'),
    (dict(erase_p=-0.1), 'erase_p'),
    (dict(erase_p=1.5), 'erase_p'),
    (dict(erase_p=float('nan')), 'erase_p'),
    (dict(lo=0), 'lo=0 hi=6 S=12'),
    (dict(lo=7), 'lo=7 hi=6'),
    (dict(hi=13), 'hi=13 S=12'),
    (dict(erase_label=-2), 'erase_label -2'),
    (dict(erase_label=256), 'erase_label 256'),
    (dict(keys=None), 'null pointer'),
    (dict(keys=FAKE_DEV + 4), 'keys_dev must be 8-byte aligned'),
    (dict(geom=FAKE_DEV + 2), '4-byte aligned'),
    (dict(radio=FAKE_DEV + 1), '4-byte aligned'),
])
def test_sample_patches_aug_refuses_bad_policies(kw, msg):
    with pytest.raises(RuntimeError, match=f'sample_patches_aug: .*{re.escape(msg)}'):
        _call(**kw)


def test_erase_size_is_not_read_when_the_stage_is_off():
    """erase_p == 0: lo / hi are not validated (and not read); the call then fails later, on the base descriptor."""
    with pytest.raises(RuntimeError, match='descriptor 1: row 19'):
        _call(desc=((0, 0, 0, 0), (1, 19, 0, 0)), erase_p=0.0, lo=0, hi=99)


@pytest.mark.parametrize('bad, msg', [
    ([0, 29, 0, 0], 'row 29'), ([0, -1, 0, 0], 'row -1'), ([0, 0, 25, 0], 'col 25'), ([1, 0, -3, 3], 'col -3'),
    ([0, 0, 0, 8], 'sym 8'), ([0, 0, 0, -1], 'sym -1'), ([-1, 0, 0, 0], 'city -1'), ([2, 0, 0, 0], 'city 2'),
])
def test_sample_patches_aug_validates_the_base_descriptor_like_sample_patches(bad, msg):
    """The jitter is clamped on the device; the descriptor it starts from must be in range, exactly as for bdn_sample_patches."""
    with pytest.raises(RuntimeError, match=f'sample_patches_aug: descriptor 2: {msg}'):
        _call(desc=((0, 0, 0, 0), (1, 18, 38, 7), bad))


def test_sample_patches_aug_refuses_null_pointers_and_shapes():
    for kw in (dict(cities=None), dict(desc_dev=None), dict(outs=(None, FAKE_DEV, FAKE_DEV)), dict(outs=(FAKE_DEV, None, FAKE_DEV)),
               dict(outs=(FAKE_DEV, FAKE_DEV, None))):
        with pytest.raises(RuntimeError, match='sample_patches_aug: null pointer'):
            _call(**kw)
    for kw, msg in ((dict(S=0), 'S=0'), (dict(C=0), 'C=0'), (dict(n=0), 'n=0'), (dict(desc_dev=FAKE_DEV + 4), 'aligned')):
        with pytest.raises(RuntimeError, match=msg):
            _call(**kw)
    with pytest.raises(RuntimeError, match='host table'):
        _lib.host_int32(np.zeros((2, 2), np.int64))


def test_header_signature_and_library_agree_on_the_new_entry():
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'int bdn_sample_patches_aug\((.*?)\);', hdr, re.S)
    assert m, 'bdn_sample_patches_aug is not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    host = ctypes.POINTER(ctypes.c_int32)
    table = {'const int32_t* city_hw_host': host, 'const int32_t* desc_host': host, 'int': ctypes.c_int, 'float': ctypes.c_float,
             'uint64_t': ctypes.c_uint64}
    want = []
    for p in params:
        ty = p.rsplit(' ', 1)[0]
        want.append(table.get(p) or table.get(ty) or (ctypes.c_void_p if ty.endswith('*') else None))
    assert None not in want, params
    res, args = _lib.SIGNATURES['bdn_sample_patches_aug']
    assert res is ctypes.c_int and args == want
    assert args[:12].count(host) == 2 and args[1] is host and args[4] is host          # tests/guard.py would take a void* for a device pointer
    plain = _lib.SIGNATURES['bdn_sample_patches'][1]
    assert len(args) == len(plain) + 14 and args[-1] is ctypes.c_void_p                # what bdn_sample_patches takes, then keys + 11 + 2 exports
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'bdn_sample_patches_aug')
    assert 'utils/dataloaders.py:148-165' in hdr[:m.start()][-4000:]                    # the reference call site it extends


# ---------------------------------------------------------------- PatchAugment
@pytest.mark.parametrize('kw', [dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(jitter=-1), dict(jitter=2.0), dict(jitter=True),
                                dict(gain=float('nan')), dict(bias=float('inf')), dict(erase_fill=float('nan')), dict(noise_std=-1e-3),
                                dict(noise_std=float('inf')), dict(erase_p=-0.1), dict(erase_p=1.01), dict(erase_size=(0, 4)),
                                dict(erase_size=(5, 4)), dict(erase_size=3), dict(erase_size=(1.5, 2)), dict(erase_label=-1),
                                dict(erase_label=256), dict(erase_label=1.0)])
def test_patch_augment_refuses(kw):
    with pytest.raises(ValueError, match='PatchAugment'):
        PatchAugment(**kw)


def test_patch_augment_defaults_and_abi():
    p = PatchAugment()
    assert p.abi_args() == (0, 0, 3, 0.0, 0.0, 0.0, 0.0, 1, 1, -1, 0.0)          # symmetry and per_date default to on
    p = PatchAugment(seed=(1 << 64) - 1, jitter=np.int64(4), symmetry=False, gain=0.5, bias=0.25, per_date=False, noise_std=0.125,
                     erase_p=1.0, erase_size=(3, 9), erase_label=255, erase_fill=-2.0)
    assert p.abi_args() == ((1 << 64) - 1, 4, 0, 0.5, 0.25, 0.125, 1.0, 3, 9, 255, -2.0)
    assert PatchAugment(per_date=True, symmetry=False).flags == 2
    assert PatchAugment.sample_key(3, 7) == (3 << 32) | 7 == R.sample_key(3, 7)
    for e, i in ((-1, 0), (0, -1), (1 << 32, 0), (0, 1 << 32)):
        with pytest.raises(ValueError):
            PatchAugment.sample_key(e, i)
    with pytest.raises(ValueError, match='exceeds the patch size'):
        PatchAugment(erase_p=0.5, erase_size=(2, 13)).check_patch_size(12)
    PatchAugment(erase_p=0.0, erase_size=(2, 13)).check_patch_size(12)             # the stage is off: the size is not read


def test_train_cli_refuses_aug_flags_without_device_patches():
    from fabric_amd.train import main
    for flags in (['--aug_jitter', '4'], ['--aug_gain', '0.1'], ['--aug_bias', '0.1'], ['--aug_shared_dates'], ['--aug_noise', '0.1'],
                  ['--aug_erase_p', '0.5'], ['--aug_erase_size', '2', '4'], ['--aug_seed', '3']):
        with pytest.raises(SystemExit, match='--device_patches true'):
            main(['--synthetic'] + flags)
    with pytest.raises(SystemExit, match='PatchAugment'):
        main(['--synthetic', '--device_patches', 'true', '--aug_noise', '-1'])
    with pytest.raises(SystemExit, match='exceeds the patch size'):
        main(['--synthetic', '--device_patches', 'true', '--patch_size', '32', '--aug_erase_p', '0.5', '--aug_erase_size', '2', '40'])


# ---------------------------------------------------------------- reference properties
def test_range_never_leaves_its_interval():
    r = np.random.default_rng(0)
    words = np.concatenate([r.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32),
                            np.array([0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], np.uint32)])
    for n in (1, 2, 3, 7, 8, 13, 255, 256, (1 << 25) + 1, (1 << 32) - 1):
        v = R.rng(words, n)
        assert v.min() >= 0 and v.max() < n
    assert int(R.rng(0xffffffff, 7)) == 6 and int(R.rng(0, 7)) == 0
    uu = R.u(words)
    assert uu.dtype == np.float32 and uu.min() >= 0.0 and uu.max() < 1.0
    assert float(R.u(0xffffffff)) == 1.0 - 2.0 ** -24 and float(R.u(0xff)) == 0.0


def test_clamps_hold_for_a_jitter_larger_than_the_city():
    S = 12
    pol = PatchAugment(seed=11, jitter=1 << 20, erase_p=0.5, erase_size=(1, S))
    seen = set()
    for idx in range(400):
        for (H, W), (row, col) in (((12, 12), (0, 0)), ((20, 13), (3, 1)), ((13, 40), (1, 28))):
            g = R.geometry(pol, R.sample_key(2, idx), row, col, 0, H, W, S)
            assert 0 <= g['row'] <= H - S and 0 <= g['col'] <= W - S
            assert 1 <= g['eh'] <= S and 1 <= g['ew'] <= S and 0 <= g['top'] <= S - g['eh'] and 0 <= g['left'] <= S - g['ew']
            seen.add((g['row'] == 0, g['row'] == H - S, g['col'] == 0, g['col'] == W - S))
    assert len(seen) > 1                                      # both ends of the clamp are reached


def test_sample_key_is_independent_of_batch_split_and_rank():
    """The key of a dataset item is (epoch, index): whichever rank draws it, in whichever batch, the same words follow."""
    from fabric_amd.device_loader import plan_keys
    n = 37
    for epoch in (0, 3):
        single = ShardSampler(n, 0, 1, seed=5)
        single.set_epoch(epoch)
        keys1 = {i: int(k) for i, k in zip(list(single), plan_keys(list(single), epoch))}
        both = {}
        for rank in (0, 1):
            s = ShardSampler(n, rank, 2, seed=5)
            s.set_epoch(epoch)
            idx = list(s)
            for b in range(0, len(idx), 4):                   # batches of 4 and a ragged last one
                for i, k in zip(idx[b:b + 4], plan_keys(idx[b:b + 4], epoch)):
                    both[i] = int(k)
        assert both and all(keys1[i] == k == R.sample_key(epoch, i) for i, k in both.items())
        assert len(both) == (n // 2) * 2
    pol = PatchAugment(seed=9, jitter=5)
    a = R.geometry(pol, R.sample_key(1, 7), 4, 4, 0, 40, 40, 12)
    assert a == R.geometry(pol, R.sample_key(1, 7), 4, 4, 0, 40, 40, 12)
    assert any(R.geom_row(a) != R.geom_row(R.geometry(pol, R.sample_key(e, i), 4, 4, 0, 40, 40, 12)) for e, i in ((2, 7), (1, 8)))


def test_reference_noise_moments():
    """10^6 reference deviates: mean within 5 standard errors of 0, variance within 5 of 1 (Var[z^2] = 2 for a unit normal)."""
    S, planes = 250, 16
    z = np.concatenate([R.noise_z64(3, R.sample_key(0, 1), p, S).ravel() for p in range(planes)])
    n = z.size
    assert n == 10 ** 6
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs((z * z).mean() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.8          # u1 >= 2^-24: |z| <= sqrt(48 ln 2) = 5.77
    even, odd = z.reshape(planes, S, S)[..., 0::2].ravel(), z.reshape(planes, S, S)[..., 1::2].ravel()
    assert abs((even * odd).mean()) <= 5.0 / np.sqrt(even.size)      # the cosine and sine branches of a pair are uncorrelated


@pytest.mark.parametrize('S', [12, 64, 70])
def test_the_gpu_tests_committed_keys_cover_their_cases(S):
    """The sample keys of tests/test_gpu_augment.py are constants: here, without a device, they are the output of the search that made
    them and they cover what that file says they cover (all symmetries, both clamps on both axes, erased and kept, every border)."""
    from tests import test_gpu_augment as G
    G.assert_coverage(S)
    assert G.search_keys(S) == G.INDICES[S]
