"""DevicePatchLoader(augment=..., warp=...): an epoch against the numpy twin given the exported records, the `off` policy taking the
bdn_sample_patches_aug path call for call, and a fused training step on a warped batch whose outside labels are ignored."""
import random

import numpy as np
import pytest
import torch

from fabric_amd.augment import PatchAugment, PatchWarp
from tests import augment_ref as R
from tests import sched_stress as ss
from tests import warp_ref as WR
from tests.test_gpu_augment_loader import POLICY, QUIET, _dataset

pytestmark = pytest.mark.gpu

WARP = PatchWarp(rotate=25.0, scale=(0.8, 1.6), misreg=0.75, oob_label=255)


def _epoch(loader):
    out = []
    for batch in loader:
        out.append(tuple(t.clone() for t in batch + tuple(loader.last_drawn or ())))
    return out


def _same(a, b):
    return len(a) == len(b) and all(len(p) == len(q) and all(torch.equal(s.view(torch.uint8), t.view(torch.uint8)) for s, t in zip(p, q))
                                    for p, q in zip(a, b))


def test_an_epoch_equals_the_reference_given_the_exported_records():
    from fabric_amd.device_loader import DevicePatchLoader
    from fabric_amd.parallel import ShardSampler
    ds, data = _dataset()
    S, bs, epoch = 16, 7, 2
    sampler = ShardSampler(len(ds), 0, 1, seed=3)
    sampler.set_epoch(epoch)
    order = list(sampler)
    loader = DevicePatchLoader(ds, data, bs, sampler=sampler, augment=QUIET, warp=WARP, export_drawn=True)
    cities = [data[c] for c in sorted(data)]
    index = {c: k for k, c in enumerate(sorted(data))}
    seen = outside = 0
    for b, (x1, x2, y) in enumerate(loader):
        assert len(loader.last_drawn) == 3
        geom, radio, records = (t.cpu().numpy() for t in loader.last_drawn)
        idx = order[b * bs:(b + 1) * bs]
        assert x1.shape[0] == len(idx) and records.shape == (len(idx), 2, 6)
        keys = [R.sample_key(epoch, i) for i in idx]
        desc = [(index[ds.imgs[i][0]], ds.imgs[i][1], ds.imgs[i][2], 0) for i in idx]
        ref = WR.reference_batch(QUIET, WARP, records, keys, desc, cities, S)
        x1, x2, y = x1.cpu().numpy(), x2.cpu().numpy(), y.cpu().numpy()
        for k, r in enumerate(ref):
            assert geom[k].tolist() == r['geom'] and np.array_equal(radio[k].view(np.uint32), r['radio'].view(np.uint32)), (b, k)
            assert np.array_equal(y[k], r['labels']), (b, k, 'labels')
            assert np.array_equal(x1[k].view(np.uint32), r['x'][0].view(np.uint32)), (b, k, 'date 1')
            assert np.array_equal(x2[k].view(np.uint32), r['x'][1].view(np.uint32)), (b, k, 'date 2')
            ti, tj = WR.record_shift32(WARP, QUIET.seed, keys[k])
            assert records[k][1, 2] == ti and records[k][1, 5] == tj and not records[k][0, [2, 5]].any()
            assert np.allclose(records[k], WR.record64(WARP, QUIET.seed, keys[k]), rtol=0, atol=1e-5)          # the bar proper: test_gpu_warp.py
            outside += int(r['outside'].sum())
        seen += len(idx)
    assert seen == len(ds) and outside > 0
    # without the export the batches are the same and nothing is allocated for the records
    quiet = DevicePatchLoader(ds, data, bs, sampler=sampler, augment=QUIET, warp=WARP)
    assert quiet.last_drawn is None and not hasattr(quiet.slots[0], 'warp')
    again = DevicePatchLoader(ds, data, bs, sampler=sampler, augment=QUIET, warp=WARP, export_drawn=True)
    assert _same([e[:3] for e in _epoch(again)], _epoch(quiet))


def test_an_off_warp_and_none_take_the_path_of_the_loader_without_the_argument():
    from fabric_amd.device_loader import DevicePatchLoader
    from fabric_amd.parallel import ShardSampler
    ds, data = _dataset()
    sampler = ShardSampler(len(ds), 0, 1, seed=3)
    traces, epochs = [], []
    for extra in ({}, dict(warp=None), dict(warp=PatchWarp()), dict(warp=PatchWarp(oob_label=255)), dict(warp=WARP)):
        loader = DevicePatchLoader(ds, data, 7, sampler=sampler, augment=POLICY, export_drawn=True, **extra)
        with ss.Perturb(ss.sync()) as h:
            epochs.append(_epoch(loader))
        torch.cuda.synchronize()
        traces.append([name for name, _ in h.trace])
        assert all(len(e) == (6 if extra.get('warp') is WARP else 5) for e in epochs[-1])          # last_drawn: three elements only with an active warp
    assert traces[0] == ['bdn_sample_patches_aug'] * len(loader) and traces[1] == traces[2] == traces[3] == traces[0]
    assert traces[4] == ['bdn_sample_patches_warp'] * len(loader)
    assert _same(epochs[1], epochs[0]) and _same(epochs[2], epochs[0]) and _same(epochs[3], epochs[0])
    assert not _same([e[:3] for e in epochs[4]], [e[:3] for e in epochs[0]])
    with pytest.raises(ValueError, match='warp needs an augment policy'):
        DevicePatchLoader(ds, data, 7, sampler=sampler, warp=WARP)
    with pytest.raises(ValueError, match='warp needs an augment policy'):
        DevicePatchLoader(ds, data, 7, sampler=sampler, warp=PatchWarp())
    with pytest.raises(TypeError, match='PatchWarp'):
        DevicePatchLoader(ds, data, 7, sampler=sampler, augment=POLICY, warp={'rotate': 3})


def test_make_device_loaders_warps_training_only():
    from fabric_amd.train import make_device_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    data = synthetic_onera(n_cities=3, bands=3, size=(100, 90), seed=2)
    random.seed(4)
    tr, va = make_device_loaders(data, ['city2'], 32, 16, 5, True, seed=9, augment=POLICY, warp=WARP)
    assert tr.warp is WARP and va.warp is None and va.augment is None
    random.seed(4)
    tr0, _ = make_device_loaders(data, ['city2'], 32, 16, 5, True, seed=9, augment=POLICY)
    assert tr0.warp is None


def test_a_fused_step_ignores_the_labels_the_warp_left_outside_the_city():
    from fabric_amd import BiDateNet
    from fabric_amd.criterion import Criterion
    from fabric_amd.train import make_device_loaders
    from fabric_amd.train_step import TrainStep
    from fabric_amd.utils.dataloaders import synthetic_onera
    data = synthetic_onera(n_cities=3, bands=13, size=(96, 96), seed=4)
    pol = PatchAugment(seed=5, jitter=8, gain=0.1, bias=0.05)
    tr, _ = make_device_loaders(data, ['city2'], 64, 32, 8, True, seed=1, augment=pol,
                                warp=PatchWarp(rotate=45.0, scale=(0.6, 1.0), misreg=1.0, oob_label=255))
    torch.manual_seed(0)
    model = BiDateNet(13, 2, precision='bf16').cuda()
    step = TrainStep(model, lr=0.01, criterion=Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255))
    with torch.cuda.stream(step.stream()):
        b1, b2, lbl = next(iter(tr))
        loss = step.step(b1, b2, lbl).clone()
        counts = step.last_counts.clone()
    torch.cuda.synchronize()
    assert torch.isfinite(b1).all() and torch.isfinite(b2).all()
    ignored = int((lbl == 255).sum())
    assert 0 < ignored < lbl.numel() and set(torch.unique(lbl).tolist()) <= {0, 1, 255}
    assert torch.isfinite(loss) and float(loss) > 0
    assert counts.shape == (5,) and int(counts[4]) == lbl.numel() - ignored
