"""DevicePatchLoader(augment=..., mix=...): a mixed batch is select(mask, donor batch, recipient batch) of plain loaders bit for bit (the
plain loaders are pinned by tests/test_gpu_augment_loader.py and tests/test_gpu_warp_loader.py), a sample does not depend on the batch
split, an `off` policy changes nothing, the plan ring survives a host that runs ahead, and label_counts / donors_from."""
import random

import numpy as np
import pytest
import torch

from fabric_amd.augment import PatchAugment, PatchMix, PatchWarp
from tests import augment_ref as R
from tests import mix_ref as M
from tests import sched_stress as ss

pytestmark = pytest.mark.gpu

S = 16
POLICY = PatchAugment(seed=91, jitter=5, gain=0.2, bias=0.1, noise_std=0.05, erase_p=0.5, erase_size=(2, 9), erase_label=255)
WARP = PatchWarp(rotate=25.0, scale=(0.8, 1.6), misreg=0.75, oob_label=255)
BOX = PatchMix(p=0.5, mode='box', box_size=(3, 12))
OBJECT = PatchMix(p=0.5, mode='object', margin=2)
_CACHE = {}


def _dataset():
    """Two cities, 40 x 52 and 70 x 33, three bands, 16 x 16 patches every 8 pixels: 20 + 21 = 41 items."""
    if not _CACHE:
        from fabric_amd.device_loader import device_stacks
        from fabric_amd.utils.dataloaders import OneraPreloader
        r = np.random.default_rng(17)
        data = {}
        for name, (h, w) in (('east', (40, 52)), ('west', (70, 33))):
            labels = (r.uniform(0, 1, (h, w)) < 0.04).astype(np.uint8)
            labels[:S, :] = 0                                   # the top rows hold no change: the windows at row 0 count zero
            data[name] = {'images': r.standard_normal((2, 3, h, w)).astype(np.float32), 'labels': labels}
        meta = [[c, i, j] for c, d in sorted(data.items()) for i in range(0, d['labels'].shape[0] - S + 1, 8)
                for j in range(0, d['labels'].shape[1] - S + 1, 8)]
        random.seed(2)
        ds = OneraPreloader('', meta, data, S, True)
        ds.imgs.sort()
        _CACHE.update(ds=ds, data=data, stacks=device_stacks(data, torch.device('cuda', torch.cuda.current_device())))
    return _CACHE['ds'], _CACHE['data'], _CACHE['stacks']


def _loader(batch_size, sampler=None, **kw):
    from fabric_amd.device_loader import DevicePatchLoader
    ds, _, stacks = _dataset()
    return DevicePatchLoader(ds, stacks, batch_size, sampler=sampler, augment=POLICY, **kw)


def _plain(indices, epoch, warp):
    """The batch a loader WITHOUT mix yields for dataset items `indices` in `epoch`, as numpy (d1, d2 as uint32, labels)."""
    loader = _loader(len(indices), sampler=list(indices), warp=warp)
    loader.set_epoch(epoch)
    (x1, x2, y), = list(loader)
    return x1.cpu().numpy().view(np.uint32), x2.cpu().numpy().view(np.uint32), y.cpu().numpy()


def _epoch(loader, sync=False):
    """Every batch of one pass, cloned on the stream: [(x1, x2, y, plan or None)]."""
    out = []
    for x1, x2, y in loader:
        plan = loader.last_drawn[-1] if loader.export_drawn and loader.mix is not None else None
        out.append(tuple(t.clone() for t in (x1, x2, y) + (() if plan is None else (plan,))))
        if sync:
            torch.cuda.synchronize()
    return out


def _items(batches):
    """The per-item tensors of a pass in dataset order (a sequential sampler): uint8 views, so NaNs compare by their bits."""
    return [torch.cat([b[k] for b in batches]).view(torch.uint8) for k in range(3)]


def _same(a, b):
    return all(torch.equal(s, t) for s, t in zip(_items(a), _items(b)))


@pytest.mark.parametrize('warp', [None, WARP], ids=['aug', 'warp'])
@pytest.mark.parametrize('mix', [BOX, OBJECT], ids=['box', 'object'])
def test_a_mixed_batch_is_the_select_of_two_plain_batches(mix, warp):
    ds, _, _ = _dataset()
    epoch, bs = 3, 7
    loader = _loader(bs, warp=warp, mix=mix, export_drawn=True)
    loader.set_epoch(epoch)
    assert loader.slots[0].d1.shape[0] == 2 * bs and loader.slots[0].desc_pin.shape[0] == 2 * bs and loader.slots[0].plan_pin.shape == (bs, 8)
    mixed = seen = 0
    for b, (x1, x2, y) in enumerate(loader):
        idx = list(range(b * bs, min((b + 1) * bs, len(ds))))
        n = len(idx)
        drawn = loader.last_drawn
        assert len(drawn) == (3 if warp is None else 4) and all(t.shape[0] == n for t in drawn) and x1.shape[0] == n
        plan = drawn[-1].cpu().numpy()
        keys = [R.sample_key(epoch, i) for i in idx]
        assert np.array_equal(plan, M.plan(POLICY.seed, keys, S, mix.p, mix.mode, *mix.box_size, None, len(ds))), b
        A = _plain(idx, epoch, warp)
        donors = plan[plan[:, 0] == 1, 1].tolist()
        got = (x1.cpu().numpy().view(np.uint32), x2.cpu().numpy().view(np.uint32), y.cpu().numpy())
        if not donors:
            assert all(np.array_equal(g, a) for g, a in zip(got, A))
            continue
        B = _plain(donors, epoch, warp)                         # a donor is cut and augmented as the loader would yield it, never mixed
        rows = [int(p[2]) - n if p[0] else 0 for p in plan]
        masks = np.stack([M.mask(p, B[2][r], mix.mode, mix.paste_label, mix.margin) for p, r in zip(plan, rows)])
        for name, g, a, d in zip(('date 1', 'date 2', 'labels'), got, A, B):
            want = M.mix(a, d[rows], masks)
            assert np.array_equal(g, want), (b, name, np.argwhere(g != want)[:4])
        mixed += len(donors)
        seen += int(masks.any())
    assert 0 < mixed < len(ds) and seen > 0 and (loader.mixed, loader.seen) == (mixed, len(ds))


def test_a_sample_does_not_depend_on_the_batch_split_and_differs_between_epochs():
    from fabric_amd.parallel import ShardSampler
    ds, _, _ = _dataset()
    sampler = ShardSampler(len(ds), 0, 1, seed=3, shuffle=False)
    four, seven = _loader(4, sampler=sampler, mix=OBJECT), _loader(7, sampler=sampler, mix=OBJECT)
    sampler.set_epoch(2)
    e4, e7 = _epoch(four), _epoch(seven)
    assert len(e4) == 11 and len(e7) == 6 and _same(e4, e7)
    sampler.set_epoch(3)
    other = _epoch(four)
    assert not _same(other, e4)
    sampler.set_epoch(0)
    seven.set_epoch(2)                                          # a resumed epoch repeats it
    assert _same(_epoch(seven), e4)


def test_an_off_mix_is_the_loader_without_the_argument():
    from fabric_amd.device_loader import DevicePatchLoader
    ds, _, stacks = _dataset()
    traces, epochs = [], []
    for extra in ({}, dict(mix=None), dict(mix=PatchMix()), dict(mix=PatchMix(mode='object', margin=4, donors=[1, 2])), dict(mix=BOX)):
        loader = _loader(7, export_drawn=True, **extra)
        loader.set_epoch(1)
        on = extra.get('mix') is BOX
        assert loader.slots[0].d1.shape[0] == (14 if on else 7) and hasattr(loader.slots[0], 'plan_pin') == on
        assert (loader.mix is not None) == on
        with ss.Perturb(ss.sync()) as h:
            epochs.append(_epoch(loader))
        torch.cuda.synchronize()
        traces.append([name for name, _ in h.trace])
        assert len(loader.last_drawn) == (3 if on else 2)
    assert traces[0] == ['bdn_sample_patches_aug'] * len(loader) and traces[1] == traces[2] == traces[3] == traces[0]
    assert traces[4] == ['bdn_sample_patches_aug', 'bdn_mix_patches'] * len(loader)
    assert _same(epochs[1], epochs[0]) and _same(epochs[2], epochs[0]) and _same(epochs[3], epochs[0]) and not _same(epochs[4], epochs[0])
    with pytest.raises(ValueError, match='mix needs an augment policy'):
        DevicePatchLoader(ds, stacks, 7, mix=BOX)
    with pytest.raises(TypeError, match='PatchMix'):
        _loader(7, mix={'p': 0.5})
    with pytest.raises(ValueError, match='PatchMix: box_size .* exceeds the patch size 16'):
        _loader(7, mix=PatchMix(p=0.5, box_size=(4, 17)))
    with pytest.raises(ValueError, match='PatchMix: donor 41 is no item'):
        _loader(7, mix=PatchMix(p=0.5, donors=[0, 41]))


def test_the_plan_ring_survives_a_host_that_runs_ahead():
    """Eleven batches through three slots while the stream is held back: no host synchronisation but the ring's own, every batch cloned
    on the stream, and all of them equal a pass that waits for the device after every batch."""
    loader = _loader(4, mix=BOX, export_drawn=True)
    loader.set_epoch(4)
    want = _epoch(loader, sync=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 2_000_000
    e0.record()
    torch.cuda._sleep(cycles)
    e1.record()
    torch.cuda.synchronize()
    rate = cycles / (e0.elapsed_time(e1) * 1e3)                 # _sleep cycles per microsecond
    torch.cuda._sleep(int(5000 * rate))                         # 5 ms: longer than the host needs to plan the pass
    got = _epoch(loader)
    torch.cuda.synchronize()
    assert len(got) == 11 > loader.depth and _same(got, want)
    assert all(torch.equal(a[3], b[3]) for a, b in zip(got, want)) and sum(int(a[3][:, 0].sum()) for a in got) == loader.mixed > 0


def test_label_counts_and_donors_from():
    ds, data, _ = _dataset()
    loader = _loader(7)
    want = [int((data[c]['labels'][i:i + S, j:j + S] == 1).sum()) for c, i, j in ds.imgs]
    for chunk in (4096, 16):
        counts = loader.label_counts(1, chunk=chunk)
        assert counts.dtype == torch.int32 and counts.is_cuda and counts.cpu().tolist() == want
    assert loader.label_counts(7).cpu().tolist() == [0] * len(ds)
    assert 0 in want and max(want) >= 4
    pool = OBJECT.donors_from(loader.label_counts(1), 4)
    assert pool.donors.tolist() == [k for k, c in enumerate(want) if c >= 4] and 0 < len(pool.donors) < len(ds)
    with pytest.raises(ValueError, match='donor pool is empty'):
        OBJECT.donors_from(loader.label_counts(1), S * S + 1)
    # a loader with the pool draws its donors from it, by the reference's formula
    mixed = _loader(7, mix=pool, export_drawn=True)
    mixed.set_epoch(1)
    plans = np.concatenate([b[3].cpu().numpy() for b in _epoch(mixed)])
    on = plans[:, 0] == 1
    assert on.any() and np.isin(plans[on, 1], pool.donors).all()
    keys = [R.sample_key(1, i) for i in range(7)]
    assert np.array_equal(plans[:7], M.plan(POLICY.seed, keys, S, 0.5, 'object', 1, 1, pool.donors, None))


def test_train_cli_mixes_and_reports_the_mixed_fraction(tmp_path):
    """The flags end to end, which is what this test is about: one short fused epoch on object-mixed batches from the change pool."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64', '--stride', '128',
           '--num_workers', '0', '--log_dir', str(tmp_path), '--device_patches', 'true', '--fused_step', 'true', '--mix_p', '0.5',
           '--mix_mode', 'object', '--mix_margin', '2', '--mix_donors', 'change', '--mix_min_pixels', '8']
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = [json.loads(line) for line in r.stdout.splitlines() if line.startswith('{"epoch"')]
    assert len(rec) == 1 and 0.0 < rec[0]['train_mix_frac'] < 1.0 and np.isfinite(rec[0]['train_cd_losses'])


def test_make_device_loaders_mixes_training_only():
    from fabric_amd.train import make_device_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    data = synthetic_onera(n_cities=3, bands=3, size=(100, 90), seed=2)
    random.seed(4)
    tr, va = make_device_loaders(data, ['city2'], 32, 16, 5, True, seed=9, augment=POLICY, mix=BOX)
    assert tr.mix is BOX and va.mix is None and va.augment is None
    random.seed(4)
    tr0, _ = make_device_loaders(data, ['city2'], 32, 16, 5, True, seed=9, augment=POLICY)
    assert tr0.mix is None
    x1, x2, y = next(iter(tr))
    torch.cuda.synchronize()
    assert x1.shape == (5, 3, 32, 32) and y.shape == (5, 32, 32) and tr.seen == 5
