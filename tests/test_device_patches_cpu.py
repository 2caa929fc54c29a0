"""CPU tests of the device patch sampler: bdn_sample_patches refuses bad descriptors before anything reaches a device, and the host
planner of DevicePatchLoader draws and crops exactly what OneraPreloader / DataLoader(num_workers=0) would."""
import random

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.device_loader import batch_sampler, plan_descriptors, plan_epoch
from fabric_amd.parallel import ShardSampler
from fabric_amd.utils.dataloaders import OneraPreloader, _apply_symmetry, synthetic_onera

FAKE_DEV = 1 << 20          # a non-null, aligned stand-in for device pointers: every call below fails validation first


def _call(desc, hw=((40, 36), (30, 50)), S=12, C=3, n=None, cities=FAKE_DEV, desc_dev=FAKE_DEV, outs=(FAKE_DEV,) * 3):
    hw = np.ascontiguousarray(hw, dtype=np.int32)
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 4)
    _lib.call('bdn_sample_patches', cities, hw.ctypes.data, len(hw), C, desc.ctypes.data, desc_dev,
              len(desc) if n is None else n, S, *outs, None)


GOOD = [[0, 0, 0, 0], [1, 18, 38, 7], [0, 28, 24, 5]]      # in range for S = 12 (H, W = 40 x 36 and 30 x 50)


@pytest.mark.parametrize('bad, msg', [
    ([0, 29, 0, 0], 'row 29'),          # row + S == H + 1
    ([1, 19, 0, 0], 'row 19'),
    ([0, -1, 0, 0], 'row -1'),
    ([0, 0, 25, 0], 'col 25'),          # col + S == W + 1
    ([1, 0, 39, 3], 'col 39'),
    ([1, 0, -3, 3], 'col -3'),
    ([0, 0, 0, 8], 'sym 8'),
    ([0, 0, 0, -1], 'sym -1'),
    ([-1, 0, 0, 0], 'city -1'),
    ([2, 0, 0, 0], 'city 2'),
])
def test_sample_patches_refuses_bad_descriptors(bad, msg):
    with pytest.raises(RuntimeError, match=f'descriptor 3: {msg}'):
        _call(GOOD + [bad])


def test_sample_patches_refuses_null_pointers_and_shapes():
    for kw in (dict(cities=None), dict(desc_dev=None), dict(outs=(None, FAKE_DEV, FAKE_DEV)), dict(outs=(FAKE_DEV, None, FAKE_DEV)),
               dict(outs=(FAKE_DEV, FAKE_DEV, None))):
        with pytest.raises(RuntimeError, match='null pointer'):
            _call(GOOD, **kw)
    hw = np.array([[40, 36]], np.int32)
    with pytest.raises(RuntimeError, match='null pointer'):        # host tables
        _lib.call('bdn_sample_patches', FAKE_DEV, None, 1, 3, np.zeros((1, 4), np.int32).ctypes.data, FAKE_DEV, 1, 12,
                  FAKE_DEV, FAKE_DEV, FAKE_DEV, None)
    with pytest.raises(RuntimeError, match='null pointer'):
        _lib.call('bdn_sample_patches', FAKE_DEV, hw.ctypes.data, 1, 3, None, FAKE_DEV, 1, 12, FAKE_DEV, FAKE_DEV, FAKE_DEV, None)
    for S in (0, -4):
        with pytest.raises(RuntimeError, match=f'S={S}'):
            _call(GOOD, S=S)
    with pytest.raises(RuntimeError, match='C=0'):
        _call(GOOD, C=0)
    with pytest.raises(RuntimeError, match='n=0'):
        _call(GOOD, n=0)
    with pytest.raises(RuntimeError, match='aligned'):
        _call(GOOD, desc_dev=FAKE_DEV + 4)
    with pytest.raises(RuntimeError, match='row 0 \\+ S 41'):     # a patch larger than the city
        _call([[0, 0, 0, 0]], S=41)


# ---------------------------------------------------------------- host planner
def _dataset(aug, seed=3):
    data = synthetic_onera(n_cities=3, bands=2, size=(70, 58), seed=seed)
    data['city1'] = {'images': data['city1']['images'][:, :, :50, :56], 'labels': data['city1']['labels'][:50, :56]}
    data['city1'] = {k: np.ascontiguousarray(v) for k, v in data['city1'].items()}
    meta = [[c, i, j] for c in sorted(data) for i in range(0, data[c]['labels'].shape[0] - 16, 5)
            for j in range(0, data[c]['labels'].shape[1] - 16, 7)]
    random.seed(11)
    ds = OneraPreloader('', meta, data, 17, aug)
    return ds, data, {c: k for k, c in enumerate(sorted(data))}


def _crop(data, cities, row):
    city, r, c, sym = (int(v) for v in row)
    d = data[cities[city]]
    t = (bool(sym & 4), bool(sym & 2), bool(sym & 1))
    S = 17
    pair = _apply_symmetry(d['images'][:, :, r:r + S, c:c + S], t)
    return pair[0], pair[1], _apply_symmetry(d['labels'][r:r + S, c:c + S], t)


def _host_batches(ds, batch_size, sampler, drop_last):
    return list(torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=sampler, drop_last=drop_last, num_workers=0))


@pytest.mark.parametrize('aug', [True, False])
@pytest.mark.parametrize('drop_last', [True, False])
def test_plan_matches_the_host_loader_item_by_item(aug, drop_last):
    ds, data, city_index = _dataset(aug)
    cities = sorted(city_index, key=city_index.get)
    bs = 7
    assert len(ds) % bs
    plans = {}
    for rank in (0, 1):
        sampler = ShardSampler(len(ds), rank, 2, seed=5)
        for epoch in (0, 1):
            sampler.set_epoch(epoch)
            random.seed(100 + epoch)
            host = _host_batches(ds, bs, sampler, drop_last)
            state = random.getstate()
            random.seed(100 + epoch)
            plan = list(plan_epoch(ds, city_index, bs, sampler, drop_last))
            assert random.getstate() == state                    # the same number of draws
            assert len(plan) == len(host) == len(batch_sampler(ds, bs, sampler, drop_last))
            assert [len(p) for p in plan] == [len(h[0]) for h in host]
            assert drop_last or len(plan[-1]) < bs
            idx = list(sampler)
            for b, (p, (x1, x2, lbl)) in enumerate(zip(plan, host)):
                assert p.dtype == np.int32 and p.shape == (len(x1), 4)
                for k, row in enumerate(p):
                    city, i, j = ds.imgs[idx[b * bs + k]]
                    assert (cities[row[0]], row[1], row[2]) == (city, i, j)
                    assert 0 <= row[3] < 8 and (aug or row[3] == 0)
                    a, bb, l = _crop(data, cities, row)
                    assert np.array_equal(x1[k].numpy().view(np.int32), a.view(np.int32))
                    assert np.array_equal(x2[k].numpy().view(np.int32), bb.view(np.int32))
                    assert np.array_equal(lbl[k].numpy(), l)
            plans[rank, epoch] = np.concatenate(plan)
            if aug:
                assert len(set(plan[0][:, 3].tolist())) > 1
    for epoch in (0, 1):
        r0 = {tuple(r[:3]) for r in plans[0, epoch]}
        r1 = {tuple(r[:3]) for r in plans[1, epoch]}
        assert not r0 & r1                                       # the two ranks' shards are disjoint
    assert not np.array_equal(plans[0, 0][:, :3], plans[0, 1][:, :3])     # set_epoch reshuffles


def test_plan_sequential_default_and_out_buffer():
    ds, data, city_index = _dataset(True)
    random.seed(1)
    host = _host_batches(ds, 5, None, False)
    random.seed(1)
    buf = np.full((5, 4), -7, np.int32)
    cities = sorted(city_index, key=city_index.get)
    for b, (x1, x2, lbl) in enumerate(host):
        idx = list(range(b * 5, min(len(ds), b * 5 + 5)))
        p = plan_descriptors(ds, idx, city_index, out=buf)
        assert p.base is buf or p is buf
        for k, row in enumerate(p):
            a, bb, l = _crop(data, cities, row)
            assert np.array_equal(x1[k].numpy(), a) and np.array_equal(lbl[k].numpy(), l)
