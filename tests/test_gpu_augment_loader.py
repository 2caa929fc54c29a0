"""DevicePatchLoader(augment=...): epochs and the sample keys, the pinned key ring under injected launch delays (tests/sched_stress.py),
a fused training run fed by an augmenting loader, and the train.py flags."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd.augment import PatchAugment
from tests import augment_ref as R
from tests import sched_stress as ss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POLICY = PatchAugment(seed=77, jitter=5, gain=0.2, bias=0.1, noise_std=0.05, erase_p=0.5, erase_size=(2, 9), erase_label=255)
QUIET = PatchAugment(seed=77, jitter=5, gain=0.2, bias=0.1, erase_p=0.5, erase_size=(2, 9), erase_label=255)      # POLICY without the noise: exact


def _dataset(bands=3, aug=True):
    from fabric_amd.utils.dataloaders import OneraPreloader, synthetic_onera
    data = synthetic_onera(n_cities=3, bands=bands, size=(60, 52), seed=5)
    meta = [[c, i, j] for c in sorted(data) for i in range(0, 60 - 16, 11) for j in range(0, 52 - 16, 9)]
    return OneraPreloader('', meta, data, 16, aug), data


def _epoch(loader):
    out = []
    for x1, x2, y in loader:
        geom, radio = loader.last_drawn
        out.append(tuple(t.clone() for t in (x1, x2, y, geom, radio)))
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s.view(torch.uint8), t.view(torch.uint8)) for p, q in zip(a, b) for s, t in zip(p, q))


def test_epochs_set_epoch_and_the_global_random_state():
    from fabric_amd.device_loader import DevicePatchLoader
    from fabric_amd.parallel import ShardSampler
    ds, data = _dataset()
    sampler = ShardSampler(len(ds), 0, 1, seed=3, shuffle=False)          # the same index order every epoch: only the keys change
    loader = DevicePatchLoader(ds, data, 7, sampler=sampler, augment=POLICY, export_drawn=True)
    plain = DevicePatchLoader(ds, data, 7, sampler=sampler, augment=POLICY)
    assert plain.last_drawn is None and not hasattr(plain.slots[0], 'geom')          # export off: nothing is allocated
    assert not hasattr(DevicePatchLoader(ds, data, 7, sampler=sampler).slots[0], 'keys_pin')
    random.seed(12345)
    state = random.getstate()
    e0 = _epoch(loader)                                         # the sampler's epoch: 0
    sampler.set_epoch(1)
    e1 = _epoch(loader)
    sampler.set_epoch(0)
    e0_again = _epoch(loader)
    loader.set_epoch(1)                                         # overrides the sampler's
    e1_forced = _epoch(loader)
    loader.set_epoch(None)
    assert random.getstate() == state, 'an augmenting loader must not draw from the global random'
    assert len(e0) == len(loader) == -(-len(ds) // 7) and e0[-1][0].shape[0] == len(ds) % 7
    assert _same(e0, e0_again) and _same(e1, e1_forced) and not _same(e0, e1)
    # the draws are those of the reference for (seed, epoch, dataset index), and dataset.aug plays no part
    cities = [data[c] for c in sorted(data)]
    index = {c: k for k, c in enumerate(sorted(data))}
    geom = torch.cat([b[3] for b in e1]).cpu().numpy()
    for i in range(len(ds)):
        city, r, c = ds.imgs[i]
        H, W = data[city]['labels'].shape
        assert geom[i].tolist() == R.geom_row(R.geometry(POLICY, R.sample_key(1, i), r, c, 0, H, W, 16)), i
    ref = R.reference_sample(QUIET, R.sample_key(1, 3), (index[ds.imgs[3][0]], ds.imgs[3][1], ds.imgs[3][2], 0), cities, 16)
    quiet = DevicePatchLoader(ds, data, 7, sampler=sampler, augment=QUIET)
    quiet.set_epoch(1)
    x1, x2, y = next(iter(quiet))
    assert np.array_equal(x1[3].cpu().numpy().view(np.uint32), ref['x'][0].view(np.uint32))
    assert np.array_equal(x2[3].cpu().numpy().view(np.uint32), ref['x'][1].view(np.uint32)) and np.array_equal(y[3].cpu().numpy(), ref['labels'])
    ds_noaug, _ = _dataset(aug=False)
    ds_noaug.imgs[:] = ds.imgs
    other = DevicePatchLoader(ds_noaug, data, 7, sampler=sampler, augment=POLICY, export_drawn=True)
    assert _same(_epoch(other), e0)
    # without a sampler that has an epoch, passes are counted
    counted = DevicePatchLoader(ds, data, 7, augment=POLICY, export_drawn=True)
    p0, p1 = _epoch(counted), _epoch(counted)
    assert _same(p0, e0) and _same(p1, e1)
    with pytest.raises(TypeError, match='PatchAugment'):
        DevicePatchLoader(ds, data, 7, augment={'jitter': 3})
    with pytest.raises(ValueError, match='exceeds the patch size'):
        DevicePatchLoader(ds, data, 7, augment=PatchAugment(erase_p=0.5, erase_size=(2, 17)))
    with pytest.raises(ValueError, match='export_drawn'):
        DevicePatchLoader(ds, data, 7, export_drawn=True)


def test_make_device_loaders_augments_training_only():
    from fabric_amd.train import make_device_loaders
    from fabric_amd.utils.dataloaders import synthetic_onera
    data = synthetic_onera(n_cities=3, bands=3, size=(100, 90), seed=2)
    random.seed(4)                                              # the datasets' constructors shuffle their lists from the global random
    tr, va = make_device_loaders(data, ['city2'], 32, 16, 5, True, seed=9, augment=POLICY)
    assert tr.augment is POLICY and va.augment is None
    random.seed(4)
    tr0, va0 = make_device_loaders(data, ['city2'], 32, 16, 5, True, seed=9)
    assert tr0.augment is None and va0.augment is None
    a, b = [tuple(t.clone() for t in x) for x in va], [tuple(t.clone() for t in x) for x in va0]
    assert _same(a, b)


def test_the_key_ring_does_not_depend_on_stream_timing():
    """The sample keys travel through a pinned ring of `depth` slots beside the descriptors; the launch that reads a slot's device copy
    runs on the consumer's stream, delayed here while the host runs ahead and rewrites the ring."""
    from fabric_amd import streams
    from fabric_amd.device_loader import DevicePatchLoader
    from fabric_amd.parallel import ShardSampler
    ds, data = _dataset()
    sampler = ShardSampler(len(ds), 0, 1, seed=3)
    loader = DevicePatchLoader(ds, data, 4, sampler=sampler, augment=POLICY, export_drawn=True, depth=3)
    assert len(loader) > 2 * 3, 'fewer batches than reuse every ring slot twice'
    cons = streams.get('chain')

    def epoch():
        with torch.cuda.stream(cons):
            return _epoch(loader)

    epoch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 2_000_000
    e0.record()
    torch.cuda._sleep(cycles)
    e1.record()
    torch.cuda.synchronize()
    rate = cycles / (e0.elapsed_time(e1) * 1e3)                 # _sleep cycles per microsecond
    short, long_ = int(300 * rate), int(5000 * rate)            # 0.3 ms: several launches' worth; 5 ms: longer than the host needs for the pass
    with ss.Perturb(ss.sync()) as h:
        want = epoch()
    torch.cuda.synchronize()
    assert {name for name, _ in h.trace} == {'bdn_sample_patches_aug'} and len(h.trace) == len(loader)
    bad = []
    for pat in (ss.none(), ss.lag('chain'), ss.stall('chain', 0), ss.stall('chain', 4), ss.random(1, 0.5), ss.random(2, 0.5)):
        torch.cuda.synchronize()
        with ss.Perturb(pat, short, long_) as h:
            got = epoch()
        torch.cuda.synchronize()
        assert pat.kind == 'none' or h.log, f'{pat}: delayed nothing'
        if not _same(got, want):
            bad.append(repr(pat))
    assert not bad, f'augmented batches depend on stream timing under {bad}'


def test_fused_training_fed_by_an_augmenting_loader():
    """Erased rectangles carry the ignore label into the masked criterion of the fused step: the run goes through and every loss is finite."""
    from fabric_amd import BiDateNet
    from fabric_amd.criterion import Criterion
    from fabric_amd.train import make_device_loaders
    from fabric_amd.train_step import TrainStep
    from fabric_amd.utils.dataloaders import synthetic_onera
    data = synthetic_onera(n_cities=3, bands=13, size=(160, 160), seed=4)
    pol = PatchAugment(seed=5, jitter=8, gain=0.1, bias=0.05, noise_std=0.02, erase_p=1.0, erase_size=(8, 24), erase_label=255)
    tr, _ = make_device_loaders(data, ['city2'], 64, 32, 8, True, seed=1, augment=pol)
    torch.manual_seed(0)
    model = BiDateNet(13, 2, precision='bf16').cuda()
    step = TrainStep(model, lr=0.01, criterion=Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255))
    losses, ignored = [], []
    with torch.cuda.stream(step.stream()):
        for k, (b1, b2, lbl) in enumerate(tr):
            losses.append(step.step(b1, b2, lbl).clone())
            ignored.append((lbl == 255).sum())
            if k == 3:
                break
    torch.cuda.synchronize()
    losses = torch.stack(losses).cpu()
    assert len(losses) == 4 and torch.isfinite(losses).all() and (losses > 0).all(), losses
    assert all(int(v) >= 8 * 8 * 8 for v in ignored)             # every sample lost a rectangle of at least 8 x 8 labels
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_train_cli_refuses_the_flags_without_device_patches(tmp_path):
    common = [sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64',
              '--stride', '128', '--num_workers', '0', '--log_dir', str(tmp_path)]
    aug = ['--aug_jitter', '8', '--aug_gain', '0.1', '--aug_bias', '0.05', '--aug_noise', '0.02', '--aug_erase_p', '0.5',
           '--aug_erase_size', '8', '24', '--aug_seed', '3']
    r = subprocess.run(common + aug, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '--device_patches true' in r.stderr and '{"epoch"' not in r.stdout
