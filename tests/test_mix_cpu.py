"""CPU tests of cross-sample mixing: bdn_mix_plan (host code of the library) against the numpy restatement tests/mix_ref.py element for
element, the statistics of the draws, every argument refusal of the three entries (fake non-null pointers: nothing reaches a device),
header / signature agreement, PatchMix and the CLI flags."""
import ctypes
import os
import re

import numpy as np
import pytest

from fabric_amd import _lib
from fabric_amd.augment import PatchAugment, PatchMix
from tests import augment_ref as R
from tests import mix_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DEV = 1 << 20          # a non-null, aligned stand-in for device pointers: every call below fails validation first
SEED = 0x5EED2026A10
N_KEYS = 4096
KEYS = np.array([R.sample_key(3, i) for i in range(N_KEYS)], np.uint64)
POOL8 = np.array([2, 3, 5, 7, 11, 13, 17, 19], np.int32)


def lib_plan(seed, keys, S, p, mode, lo, hi, pool=None, n_items=None):
    keys = np.ascontiguousarray(keys, np.uint64)
    out = np.full((len(keys), 8), -7, np.int32)
    _lib.call('bdn_mix_plan', seed, _lib.host_uint64(keys), len(keys), S, p, M.MODES[mode], lo, hi, _lib.host_int32(pool),
              len(pool) if pool is not None else n_items, _lib.host_int32(out))
    return out


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize('S', [1, 5, 130])
@pytest.mark.parametrize('mode', ['box', 'object'])
def test_mix_plan_equals_the_reference_element_for_element(S, mode):
    for p in (0.0, 2.0 ** -24, 0.5, 1.0):
        for pool, n_items in ((None, 1000), (POOL8, None)):
            for lo, hi in sorted({(1, S), (S, S), (max(1, S // 3), max(1, S // 2))}):
                got = lib_plan(SEED, KEYS, S, p, mode, lo, hi, pool, n_items)
                want = M.plan(SEED, KEYS, S, p, mode, lo, hi, pool, n_items)
                assert np.array_equal(got, want), (p, pool is not None, lo, hi, np.flatnonzero((got != want).any(1))[:5])
                on = got[:, 0] == 1
                assert on.sum() == {0.0: 0, 1.0: N_KEYS}.get(p, on.sum())
                assert (got[~on] == [0, 0, -1, 0, 0, 0, 0, 0]).all() and (got[:, 7] == 0).all()
                # donor_row: n + the number of mixed samples before this one
                assert np.array_equal(got[on, 2], N_KEYS + np.arange(on.sum()))
                t, l, h, w = (got[on, c] for c in (3, 4, 5, 6))
                assert (t >= 0).all() and (l >= 0).all() and (t + h <= S).all() and (l + w <= S).all()
                if mode == 'object':
                    assert (t == 0).all() and (l == 0).all() and (h == S).all() and (w == S).all()
                else:
                    assert (h >= lo).all() and (h <= hi).all() and (w >= lo).all() and (w <= hi).all()
                donors = got[on, 1]
                assert np.isin(donors, POOL8).all() if pool is not None else ((donors >= 0).all() and (donors < n_items).all())


def test_mix_plan_statistics():
    """p = 0.5 over 4096 keys: 2048 +- 160 mixed, five standard deviations (sigma = sqrt(4096 / 4) = 32); checked on the reference first."""
    for plan in (M.plan(SEED, KEYS, 16, 0.5, 'box', 2, 9, POOL8), lib_plan(SEED, KEYS, 16, 0.5, 'box', 2, 9, POOL8)):
        on = plan[:, 0] == 1
        assert abs(int(on.sum()) - 2048) <= 160
        assert set(plan[on, 1].tolist()) == set(POOL8.tolist()), 'every member of the pool of 8 is drawn'
        assert set(plan[on, 5].tolist()) == set(range(2, 10)) and set(plan[on, 6].tolist()) == set(range(2, 10))
        assert plan[on, 3].min() == 0 and (plan[on, 3] + plan[on, 5]).max() == 16 and plan[on, 4].min() == 0 and (plan[on, 4] + plan[on, 6]).max() == 16
    # 2^-24 mixes exactly the keys whose 24 bits are zero; another seed or epoch gives another plan
    a = lib_plan(SEED, KEYS, 16, 0.5, 'box', 2, 9, None, 500)
    assert not np.array_equal(a, lib_plan(SEED + 1, KEYS, 16, 0.5, 'box', 2, 9, None, 500))
    assert not np.array_equal(a, lib_plan(SEED, KEYS + np.uint64(1 << 32), 16, 0.5, 'box', 2, 9, None, 500))
    w0 = np.array([R.draw(SEED, int(k), M.MIX, 0)[0] for k in KEYS[:256]])
    assert np.array_equal(lib_plan(SEED, KEYS[:256], 16, 2.0 ** -24, 'box', 1, 1, None, 9)[:, 0], (w0 >> np.uint32(8)) == 0)


def test_the_mix_stream_collides_with_no_other_stream():
    from tests import warp_ref as WR
    core = open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'philox_core.hpp')).read()
    assert re.search(r'PHILOX_MIX = 0x4D495820u', core) and M.MIX == 0x4D495820 == int.from_bytes(b'MIX ', 'big')
    assert M.MIX != WR.WARP and M.MIX not in (R.GEOMETRY, R.RADIOMETRY) and M.MIX > R.NOISE + 2 * 64


# ---------------------------------------------------------------- reference properties
def test_reference_mask_and_mix():
    S = 9
    lab = np.zeros((S, S), np.uint8)
    lab[0, 0] = lab[8, 8] = lab[4, 5] = 1
    lab[2, 2] = 255
    row = (1, 0, 4, 0, 0, S, S, 0)
    assert np.array_equal(M.mask(row, lab, 'object', 1, 0), lab == 1)
    m1 = M.mask(row, lab, 'object', 1, 1)
    assert m1.sum() == 4 + 4 + 9 and m1[0:2, 0:2].all() and m1[7:, 7:].all() and m1[3:6, 4:7].all()
    assert M.mask(row, lab, 'object', 1, 16).all() and not M.mask(row, lab, 'object', 7, 16).any()
    assert M.mask(row, lab, 'object', 255, 0).sum() == 1 and not M.mask((0, 0, -1, 0, 0, 0, 0, 0), lab, 'object', 1, 3).any()
    box = M.mask((1, 0, 4, 2, 3, 4, 5, 0), lab, 'box')
    assert box.sum() == 20 and box[2:6, 3:8].all()
    a, b = 100 + np.arange(2 * 3 * S * S, dtype=np.uint32).reshape(2, 3, S, S), np.full((2, 3, S, S), 7, np.uint32)
    out = M.mix(a, b, np.stack([box, np.zeros_like(box)]))
    assert (out[0][:, 2:6, 3:8] == 7).all() and (out[0] == 7).sum() == 60 and np.array_equal(out[1], a[1])
    assert np.array_equal(M.mix(lab[None], (lab + 1)[None], box[None])[0], np.where(box, lab + 1, lab))


# ---------------------------------------------------------------- the entries
def _params(name):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'int ' + name + r'\((.*?)\);', hdr, re.S)
    assert m, f'{name} is not declared'
    return [' '.join(p.split()) for p in m.group(1).split(',')]


@pytest.mark.parametrize('name', ['bdn_mix_plan', 'bdn_mix_patches', 'bdn_patch_label_counts'])
def test_header_signature_and_library_agree(name):
    host, hostu = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
    table = {'const int32_t* city_hw_host': host, 'const int32_t* desc_host': host, 'const int32_t* plan_host': host, 'int32_t* plan_host': host,
             'const int32_t* pool_host': host, 'const uint64_t* keys_host': hostu, 'int': ctypes.c_int, 'float': ctypes.c_float,
             'uint64_t': ctypes.c_uint64}
    want = []
    for p in _params(name):
        ty = p.rsplit(' ', 1)[0]
        want.append(table.get(p) or table.get(ty) or (ctypes.c_void_p if ty.endswith('*') else None))
    assert None not in want
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and args == want
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    if name == 'bdn_mix_plan':                               # host only: a trailing void* would be taken for a stream
        assert args[-1] is not ctypes.c_void_p
    else:
        assert _params(name)[-1] == 'void* stream'
    assert 'mix.hip' in open(os.path.join(ROOT, 'fabric_amd', 'csrc', 'Makefile')).read()


GOOD_PLAN = dict(seed=5, keys=KEYS[:4], n=4, S=16, p=0.5, mode=0, lo=2, hi=9, pool=POOL8, n_pool=8, plan=np.zeros((4, 8), np.int32))


def _plan_call(**kw):
    a = dict(GOOD_PLAN, **kw)
    keys, pool, plan = a['keys'], a['pool'], a['plan']
    _lib.call('bdn_mix_plan', a['seed'], keys if keys is None or isinstance(keys, ctypes._Pointer) else _lib.host_uint64(keys), a['n'], a['S'],
              a['p'], a['mode'], a['lo'], a['hi'], pool if pool is None or isinstance(pool, ctypes._Pointer) else _lib.host_int32(pool),
              a['n_pool'], plan if plan is None or isinstance(plan, ctypes._Pointer) else _lib.host_int32(plan))


def _odd(ptr_type, offset):
    return ctypes.cast(FAKE_DEV + offset, ptr_type)


@pytest.mark.parametrize('kw, msg', [
    (dict(keys=None), 'null pointer'),
    (dict(plan=None), 'null pointer'),
    (dict(keys=_odd(_lib._hu, 4)), 'aligned'),
    (dict(plan=_odd(_lib._hi, 2)), 'aligned'),
    (dict(pool=_odd(_lib._hi, 1)), 'aligned'),
    (dict(n=0), 'n, S > 0'),
    (dict(n=-1), 'n, S > 0'),
    (dict(S=0), 'n, S > 0'),
    (dict(p=-0.25), 'p -0.25 outside'),
    (dict(p=1.5), 'p 1.5 outside'),
    (dict(p=float('nan')), 'outside [0, 1]'),
    (dict(mode=2), 'unknown mode 2'),
    (dict(mode=-1), 'unknown mode -1'),
    (dict(lo=0), 'lo=0 hi=9 S=16'),
    (dict(lo=10), 'lo=10 hi=9 S=16'),
    (dict(hi=17), 'lo=2 hi=17 S=16'),
    (dict(mode=1, hi=17), 'lo=2 hi=17 S=16'),
    (dict(n_pool=0), 'n_pool 0'),
    (dict(pool=None, n_pool=-3), 'n_pool -3'),
])
def test_mix_plan_refuses(kw, msg):
    with pytest.raises(RuntimeError, match=f'mix_plan: .*{re.escape(msg)}'):
        _plan_call(**kw)


def test_mix_plan_accepts_the_good_arguments():
    _plan_call()
    _plan_call(pool=None, n_pool=1)
    assert np.array_equal(GOOD_PLAN['plan'], M.plan(5, KEYS[:4], 16, 0.5, 'box', 2, 9, None, 1))


PLAN_ROWS = np.array([(1, 3, 4, 0, 0, 16, 16, 0), (0, 0, -1, 0, 0, 0, 0, 0), (1, 9, 5, 14, 3, 2, 13, 0), (1, 9, 5, 1, 2, 3, 4, 0)], np.int32)
GOOD_MIX = dict(plan=PLAN_ROWS, plan_dev=FAKE_DEV, n=4, rows=6, C=3, S=16, mode=0, paste_label=1, margin=2, d1=FAKE_DEV, d2=FAKE_DEV,
                labels=FAKE_DEV, mask_out=None)


def _plan_with(row, **fields):
    cols = dict(on=0, donor_row=2, top=3, left=4, h=5, w=6)
    p = PLAN_ROWS.copy()
    for k, v in fields.items():
        p[row, cols[k]] = v
    return p


def _mix_call(**kw):
    a = dict(GOOD_MIX, **kw)
    plan = a['plan']
    _lib.call('bdn_mix_patches', plan if plan is None or isinstance(plan, ctypes._Pointer) else _lib.host_int32(np.ascontiguousarray(plan)),
              a['plan_dev'], a['n'], a['rows'], a['C'], a['S'], a['mode'], a['paste_label'], a['margin'], a['d1'], a['d2'], a['labels'],
              a['mask_out'], None)


@pytest.mark.parametrize('kw, msg', [
    (dict(plan=None), 'null pointer'),
    (dict(plan_dev=None), 'null pointer'),
    (dict(d1=None), 'null pointer'),
    (dict(d2=None), 'null pointer'),
    (dict(labels=None), 'null pointer'),
    (dict(plan=_odd(_lib._hi, 2)), 'aligned'),
    (dict(plan_dev=FAKE_DEV + 8), 'aligned'),
    (dict(d1=FAKE_DEV + 2), 'aligned'),
    (dict(d2=FAKE_DEV + 1), 'aligned'),
    (dict(n=0), 'rows >= n'),
    (dict(rows=3), 'rows >= n'),
    (dict(C=0), 'rows >= n'),
    (dict(S=0), 'rows >= n'),
    (dict(S=(1 << 14) + 1), 'above 2^14'),
    (dict(mode=2), 'unknown mode 2'),
    (dict(paste_label=-1), 'paste_label -1'),
    (dict(paste_label=256), 'paste_label 256'),
    (dict(margin=-1), 'margin -1'),
    (dict(margin=17), 'margin 17'),
    (dict(plan=_plan_with(1, on=2)), 'plan row 1: on = 2'),
    (dict(plan=_plan_with(3, on=-1)), 'plan row 3: on = -1'),
    (dict(plan=_plan_with(0, donor_row=3)), 'plan row 0: donor_row 3 outside [4, 6)'),
    (dict(plan=_plan_with(2, donor_row=6)), 'plan row 2: donor_row 6 outside [4, 6)'),
    (dict(rows=5), 'plan row 2: donor_row 5 outside [4, 5)'),
    (dict(plan=_plan_with(2, top=15)), 'plan row 2: rectangle'),
    (dict(plan=_plan_with(3, left=13)), 'plan row 3: rectangle'),
    (dict(plan=_plan_with(3, top=-1)), 'plan row 3: rectangle'),
    (dict(plan=_plan_with(3, h=0)), 'plan row 3: rectangle'),
    (dict(plan=_plan_with(0, w=17)), 'plan row 0: rectangle'),
    (dict(S=15), 'plan row 0: rectangle'),
])
def test_mix_patches_refuses(kw, msg):
    with pytest.raises(RuntimeError, match=f'mix_patches: .*{re.escape(msg)}'):
        _mix_call(**kw)


HW = np.array([(40, 36), (30, 50)], np.int32)
GOOD_COUNTS = dict(cities=FAKE_DEV, hw=HW, n_cities=2, desc=np.array([(0, 0, 0, 0), (1, 18, 38, 7)], np.int32), desc_dev=FAKE_DEV, n=2, S=12,
                   value=1, counts=FAKE_DEV)


def _counts_call(**kw):
    a = dict(GOOD_COUNTS, **kw)
    hw, desc = a['hw'], a['desc']
    _lib.call('bdn_patch_label_counts', a['cities'], None if hw is None else _lib.host_int32(np.ascontiguousarray(hw, np.int32)), a['n_cities'],
              None if desc is None else _lib.host_int32(np.ascontiguousarray(desc, np.int32)), a['desc_dev'], a['n'], a['S'], a['value'],
              a['counts'], None)


@pytest.mark.parametrize('kw, msg', [
    (dict(cities=None), 'null pointer'),
    (dict(hw=None), 'null pointer'),
    (dict(desc=None), 'null pointer'),
    (dict(desc_dev=None), 'null pointer'),
    (dict(counts=None), 'null pointer'),
    (dict(desc_dev=FAKE_DEV + 8), 'aligned'),
    (dict(cities=FAKE_DEV + 4), 'aligned'),
    (dict(counts=FAKE_DEV + 2), 'aligned'),
    (dict(n=0), 'n, S, n_cities > 0'),
    (dict(S=0), 'n, S, n_cities > 0'),
    (dict(n_cities=0), 'n, S, n_cities > 0'),
    (dict(S=46341), 'does not fit int32'),
    (dict(value=-1), 'value -1'),
    (dict(value=256), 'value 256'),
    (dict(hw=[(40, 0), (30, 50)]), 'city 0 has shape 40 x 0'),
    (dict(desc=[(2, 0, 0, 0), (1, 0, 0, 0)]), 'descriptor 0: city 2'),
    (dict(desc=[(0, 0, 0, 0), (1, 0, 0, 8)]), 'descriptor 1: sym 8'),
    (dict(desc=[(0, 29, 0, 0), (1, 0, 0, 0)]), 'descriptor 0: row 29'),
    (dict(desc=[(0, 0, 0, 0), (1, 18, 39, 0)]), 'descriptor 1: col 39'),
    (dict(desc=[(0, -1, 0, 0), (1, 0, 0, 0)]), 'descriptor 0: row -1'),
])
def test_patch_label_counts_refuses(kw, msg):
    with pytest.raises(RuntimeError, match=f'patch_label_counts: .*{re.escape(msg)}'):
        _counts_call(**kw)


# ---------------------------------------------------------------- PatchMix
def test_patch_mix_defaults_repr_and_pool():
    p = PatchMix()
    assert p.off and (p.p, p.mode, p.box_size, p.paste_label, p.margin, p.donors) == (0.0, 'box', (1, 1), 1, 0, None)
    assert repr(p) == "PatchMix(p=0.0, mode='box', box_size=(1, 1), paste_label=1, margin=0, donors=None)"
    assert repr(eval(repr(p))) == repr(p)
    q = PatchMix(p=0.5, mode='object', box_size=(4, 8), paste_label=255, margin=16, donors=[1, 4, 9])
    assert not q.off and not PatchMix(p=2.0 ** -24).off and PatchMix(mode='object', margin=3).off
    assert repr(q) == "PatchMix(p=0.5, mode='object', box_size=(4, 8), paste_label=255, margin=16, donors=<3 indices>)"
    assert q.donors.dtype == np.int32 and q.donors.flags['C_CONTIGUOUS'] and q.donors.tolist() == [1, 4, 9]
    q.check(8, 10)
    with pytest.raises(ValueError, match='PatchMix: box_size .* exceeds the patch size 7'):
        q.check(7, 10)
    with pytest.raises(ValueError, match='PatchMix: donor 9 is no item of a dataset of 9'):
        q.check(8, 9)
    r = q.donors_from(np.array([0, 3, 1, 0, 7]), 2)
    assert r is not q and r.donors.tolist() == [1, 4] and (r.p, r.mode, r.box_size, r.paste_label, r.margin) == (0.5, 'object', (4, 8), 255, 16)
    assert q.donors_from(np.array([0, 3, 1, 0, 7])).donors.tolist() == [1, 2, 4] and q.donors.tolist() == [1, 4, 9]
    import torch
    assert q.donors_from(torch.tensor([0, 3, 1], dtype=torch.int32)).donors.tolist() == [1, 2]
    with pytest.raises(ValueError, match='PatchMix: .*the donor pool is empty'):
        q.donors_from(np.array([0, 3, 1]), 4)


@pytest.mark.parametrize('kw', [dict(p=-0.1), dict(p=1.5), dict(p=float('nan')), dict(p='x'), dict(p=None), dict(mode='cut'), dict(mode=0),
                                dict(box_size=3), dict(box_size=(3,)), dict(box_size=(0, 3)), dict(box_size=(4, 3)), dict(box_size=(1.0, 3)),
                                dict(box_size=(1, True)), dict(paste_label=-1), dict(paste_label=256), dict(paste_label=1.0),
                                dict(paste_label=None), dict(margin=-1), dict(margin=17), dict(margin=1.5), dict(margin=True),
                                dict(donors=[]), dict(donors=[[1, 2]]), dict(donors=[3, 1]), dict(donors=[-1, 2]), dict(donors=[0.5, 2.0]),
                                dict(donors=[1, 1 << 31]), dict(donors=7)])
def test_patch_mix_refuses(kw):
    with pytest.raises(ValueError, match='PatchMix: '):
        PatchMix(**kw)


# ---------------------------------------------------------------- CLI
def test_train_cli_refuses_mix_flags_without_device_patches():
    from fabric_amd.train import main
    for flags in (['--mix_p', '0.5'], ['--mix_mode', 'object'], ['--mix_box', '4', '8'], ['--mix_margin', '2'], ['--mix_donors', 'change'],
                  ['--mix_min_pixels', '5']):
        with pytest.raises(SystemExit, match=f'{flags[0]} augment the patches the device cuts: add --device_patches true'):
            main(['--synthetic'] + flags)
    for flags, msg in ((['--mix_p', '1.5'], 'PatchMix: p'), (['--mix_p', '0.5', '--mix_box', '8', '4'], 'PatchMix: box_size'),
                       (['--mix_p', '0.5', '--mix_box', '8', '4000'], 'PatchMix: box_size .* exceeds the patch size'),
                       (['--mix_p', '0.5', '--mix_mode', 'object', '--mix_margin', '17'], 'PatchMix: margin'),
                       (['--mix_p', '0.5', '--mix_donors', 'change', '--mix_min_pixels', '0'], '--mix_min_pixels 0')):
        with pytest.raises(SystemExit, match=msg):
            main(['--synthetic', '--device_patches', 'true'] + flags)


def test_train_cli_builds_the_policies_from_the_mix_flags(monkeypatch):
    from fabric_amd import train as T
    seen = {}
    real_aug, real_warp, real_mix = T.augment_from_opt, T.warp_from_opt, T.mix_from_opt

    def aug(opt):
        seen['order'] = ['augment']
        seen['augment'] = real_aug(opt)
        return seen['augment']

    def warp(opt):
        seen['order'].append('warp')
        seen['warp'] = real_warp(opt)
        return seen['warp']

    def mix(opt):
        seen['order'].append('mix')
        seen['mix'] = real_mix(opt)
        raise SystemExit('parsed')                             # stop before anything asks for a device

    monkeypatch.setattr(T, 'augment_from_opt', aug)
    monkeypatch.setattr(T, 'warp_from_opt', warp)
    monkeypatch.setattr(T, 'mix_from_opt', mix)
    with pytest.raises(SystemExit, match='parsed'):
        T.main(['--synthetic', '--device_patches', 'true', '--fused_step', 'true', '--ignore_label', '255', '--seed', '4', '--mix_p', '0.25',
                '--mix_mode', 'object', '--mix_margin', '3', '--mix_donors', 'change', '--mix_min_pixels', '6'])
    assert seen['order'] == ['augment', 'warp', 'mix'] and seen['warp'] is None
    assert repr(seen['mix']) == repr(PatchMix(p=0.25, mode='object', margin=3, paste_label=1))
    assert repr(seen['augment']) == repr(PatchAugment(seed=4, erase_label=255))          # a mix flag alone: the default policy
    seen.clear()
    with pytest.raises(SystemExit, match='parsed'):
        T.main(['--synthetic', '--device_patches', 'true', '--mix_p', '1', '--mix_box', '8', '32', '--aug_rotate', '10'])
    assert repr(seen['mix']) == repr(PatchMix(p=1.0, box_size=(8, 32))) and seen['warp'].rotate == 10.0
    # --mix_p 0 builds no PatchMix, and an options object from before the flags existed still builds its PatchAugment
    seen.clear()
    with pytest.raises(SystemExit, match='parsed'):
        T.main(['--synthetic', '--device_patches', 'true', '--mix_mode', 'object'])
    assert seen['mix'] is None and seen['augment'] is not None
    old = type('O', (), dict(aug_jitter=3, aug_gain=0.0, aug_bias=0.0, aug_shared_dates=False, aug_noise=0.0, aug_erase_p=0.0, aug_erase_size=None,
                             aug_seed=None, aug_rotate=0.0, aug_scale=None, aug_misreg=0.0, device_patches=True, seed=2, augmentation=True,
                             ignore_label=None, patch_size=64))()
    assert repr(real_aug(old)) == repr(PatchAugment(seed=2, jitter=3))
