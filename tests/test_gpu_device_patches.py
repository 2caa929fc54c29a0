"""Device patch sampler (bdn_sample_patches, fabric_amd.device_loader) against the host path, bit for bit: the G7 fixture, every
symmetry through the C ABI, whole epochs of make_loaders vs make_device_loaders, fused training fed either way, and train.py."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils.dataloaders import OneraPreloader, _apply_symmetry, synthetic_onera
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    t = torch.as_tensor(t).cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def test_g7_fixture_on_the_device(golden_dir):
    from fabric_amd.device_loader import DevicePatchLoader
    g = np.load(os.path.join(golden_dir, 'g7_loader.npz'))
    r = np.random.default_rng(7)
    data = {'cityA': {'images': r.standard_normal((2, 3, 40, 36)).astype(np.float32),
                      'labels': (r.uniform(0, 1, (40, 36)) < 0.2).astype(np.uint8)},
            'cityB': {'images': r.standard_normal((2, 3, 30, 50)).astype(np.float32),
                      'labels': (r.uniform(0, 1, (30, 50)) < 0.2).astype(np.uint8)}}
    for bs in (5, 2):
        meta = [['cityA', 0, 0], ['cityA', 16, 8], ['cityB', 4, 30], ['cityB', 10, 0], ['cityA', 20, 20]]
        random.seed(1234)
        ds = OneraPreloader('unused/', meta, data, 12, aug=True)
        loader = DevicePatchLoader(ds, data, bs)
        assert len(loader) == -(-5 // bs)
        i = 0
        for a, b, lbl in loader:
            assert a.is_cuda and a.dtype == torch.float32 and lbl.dtype == torch.uint8 and a.shape[1:] == (3, 12, 12)
            for k in range(a.shape[0]):
                assert _same(a[k], g[f'img1_{i}']) and _same(b[k], g[f'img2_{i}']) and _same(lbl[k], g[f'lbl_{i}']), (bs, i)
                i += 1
        assert i == 5


# ---------------------------------------------------------------- every symmetry through the ABI
def _special(r, shape):
    """float32 noise with NaN payloads (quiet and signalling, both signs), -0.0, +-inf and denormals sprinkled in."""
    x = r.standard_normal(shape).astype(np.float32)
    bits = x.view(np.uint32)
    specials = np.array([0x7fc01234, 0xffc00001, 0x7f800001, 0xff912345, 0x80000000, 0x7f800000, 0xff800000, 0x00000001],
                        np.uint32)
    m = r.uniform(0, 1, shape) < 0.05
    bits[m] = specials[r.integers(0, len(specials), int(m.sum()))]
    return x


@pytest.mark.parametrize('C', [3, 13])
@pytest.mark.parametrize('S', [1, 7, 12, 90, 128])
@guarded
def test_every_symmetry_through_the_abi(S, C):
    r = np.random.default_rng(S * 100 + C)
    shapes = [(S + 5, S + 9), (S + 8, S + 3)]
    cities = [{'images': _special(r, (2, C, h, w)), 'labels': r.integers(0, 256, (h, w)).astype(np.uint8)} for h, w in shapes]
    dev = [{k: guard.guard(torch.from_numpy(v)) for k, v in c.items()} for c in cities]
    rec = np.array([[d['images'].data_ptr(), d['labels'].data_ptr(), h | (w << 32)] for d, (h, w) in zip(dev, shapes)], np.int64)
    table = guard.guard(torch.from_numpy(rec))
    hw = np.array(shapes, np.int32)
    desc = []
    for city, (h, w) in enumerate(shapes):
        for row, col in ((0, 0), (1, 3), (h - S, w - S), (min(3, h - S), w - S), (h - S, min(5, w - S))):
            desc += [(city, row, col, sym) for sym in range(8)]
    desc = np.array(desc, np.int32)
    n = len(desc)
    desc_dev = guard.guard(torch.from_numpy(desc))
    o1 = guard.full((n, C, S, S), float('nan'))
    o2 = guard.full_like(o1, float('nan'))
    ol = guard.full((n, S, S), 77, dtype=torch.uint8)
    _lib.call('bdn_sample_patches', table.data_ptr(), hw.ctypes.data, len(shapes), C, desc.ctypes.data, desc_dev.data_ptr(), n, S,
              o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    o1, o2, ol = o1.cpu().numpy(), o2.cpu().numpy(), ol.cpu().numpy()
    for k, (city, row, col, sym) in enumerate(desc):
        t = (bool(sym & 4), bool(sym & 2), bool(sym & 1))
        c = cities[city]
        pair = np.ascontiguousarray(_apply_symmetry(c['images'][:, :, row:row + S, col:col + S], t))
        lbl = np.ascontiguousarray(_apply_symmetry(c['labels'][row:row + S, col:col + S], t))
        assert np.array_equal(o1[k].view(np.uint32), pair[0].view(np.uint32)), (k, city, row, col, sym)
        assert np.array_equal(o2[k].view(np.uint32), pair[1].view(np.uint32)), (k, city, row, col, sym)
        assert np.array_equal(ol[k], lbl), (k, city, row, col, sym)


def test_loader_refuses_bad_stacks():
    from fabric_amd.device_loader import DevicePatchLoader
    data = synthetic_onera(n_cities=2, bands=3, size=(40, 40))
    ds = OneraPreloader('', [['city0', 0, 0]], data, 12)
    bad = dict(data, city1={'images': data['city1']['images'][:, :2].copy(), 'labels': data['city1']['labels']})
    with pytest.raises(RuntimeError, match='same number of bands'):
        DevicePatchLoader(ds, bad, 4)
    bad = dict(data, city1={'images': data['city1']['images'].astype(np.float64), 'labels': data['city1']['labels']})
    with pytest.raises(RuntimeError, match='float32'):
        DevicePatchLoader(ds, bad, 4)
    ds = OneraPreloader('', [['city0', 29, 0]], data, 12)          # an origin whose patch leaves the city
    with pytest.raises(RuntimeError, match='row 29'):
        next(iter(DevicePatchLoader(ds, data, 4)))


def test_device_stacks_are_used_in_place():
    from fabric_amd.train import make_device_loaders
    data = synthetic_onera(n_cities=3, bands=13, size=(100, 100))
    dev = {c: {'images': torch.from_numpy(d['images']).cuda(), 'labels': d['labels']} for c, d in data.items()}
    tr, va = make_device_loaders(dev, ['city2'], 32, 32, 4, True)
    for c in data:
        assert tr.stacks[c]['images'].data_ptr() == dev[c]['images'].data_ptr()
        assert tr.stacks[c]['labels'].data_ptr() == va.stacks[c]['labels'].data_ptr()     # one upload shared by both loaders
    assert tr.dataset.aug and not va.dataset.aug and tr.drop_last and not va.drop_last


# ---------------------------------------------------------------- whole epochs
@pytest.mark.parametrize('aug', [True, False])
def test_whole_epochs_match_make_loaders(aug):
    from fabric_amd.train import make_device_loaders, make_loaders
    data = synthetic_onera(n_cities=4, bands=13, size=(150, 130), seed=2)
    bs, S, stride = 5, 32, 16
    for rank in (0, 1):
        random.seed(3)
        h_tr, h_va = make_loaders(data, ['city3'], S, stride, bs, aug, num_workers=0, rank=rank, world_size=2, seed=9)
        random.seed(3)
        d_tr, d_va = make_device_loaders(data, ['city3'], S, stride, bs, aug, rank=rank, world_size=2, seed=9)
        assert len(h_tr.dataset) % 2 == 0 and (len(h_tr.dataset) // 2) % bs       # drop_last drops a partial batch
        assert len(h_va.dataset) % bs                                             # the validation loader ends with one
        assert h_tr.dataset.imgs == d_tr.dataset.imgs and h_va.dataset.imgs == d_va.dataset.imgs
        for epoch in (0, 1):
            h_tr.sampler.set_epoch(epoch)
            d_tr.sampler.set_epoch(epoch)
            for h, d in ((h_tr, d_tr), (h_va, d_va)):
                random.seed(100 * rank + epoch)
                hb = list(h)
                random.seed(100 * rank + epoch)
                n = 0
                for (h1, h2, hl), (d1, d2, dl) in zip(hb, d):
                    assert _same(h1, d1) and _same(h2, d2) and _same(hl, dl), (rank, epoch, n)
                    n += 1
                assert n == len(hb) == len(d) == len(h)
            assert len(hb[-1][0]) == len(h_va.dataset) % bs                          # the validation pass's partial last batch


# ---------------------------------------------------------------- training
def test_fused_training_fed_by_either_loader_is_identical():
    from fabric_amd import BiDateNet
    from fabric_amd.input_pipeline import DeviceFeeder
    from fabric_amd.train import make_device_loaders, make_loaders
    from fabric_amd.train_step import TrainStep
    data = synthetic_onera(n_cities=3, bands=13, size=(200, 200), seed=4)
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in BiDateNet(13, 2, precision='bf16').state_dict().items()}
    runs = []
    for device_side in (False, True):
        random.seed(5)
        if device_side:
            tr, _ = make_device_loaders(data, ['city2'], 64, 32, 8, True, seed=1)
        else:
            tr, _ = make_loaders(data, ['city2'], 64, 32, 8, True, num_workers=0, seed=1)
        model = BiDateNet(13, 2, precision='bf16')
        model.load_state_dict(sd)
        step = TrainStep(model.cuda(), lr=0.01, tversky_alpha=0.1, tversky_beta=0.9)
        feeder = None if device_side else DeviceFeeder(torch.device('cuda'))
        losses = []
        random.seed(6)
        with torch.cuda.stream(step.stream()):
            for k, (b1, b2, lbl) in enumerate(tr if device_side else feeder(tr)):
                losses.append(step.step(b1, b2, lbl).clone())
                if k == 3:
                    break
        torch.cuda.synchronize()
        if feeder is not None:
            feeder.close()
        runs.append((torch.stack(losses).cpu(), step.flat_params.cpu()))
    assert len(runs[0][0]) == 4
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])


def test_train_cli_device_patches_matches_the_host_path(tmp_path):
    common = [sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64',
              '--stride', '128', '--num_workers', '0']
    out = []
    for extra in ([], ['--device_patches', 'true']):
        log = tmp_path / ('dev' if extra else 'host')
        r = subprocess.run(common + ['--log_dir', str(log)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        out.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"epoch"')])
    assert len(out[0]) == 1 and out[0] == out[1], out
