"""-m gpu: fabric_amd.utils.distance.boundary_scores (bdn_boundary_mask, bdn_edt, bdn_boundary_score) against tests/edt_ref.py -- every count
and squared distance exactly, the ratios as the same divisions -- and the scene line of the training loop with --scene_boundary_tol."""
import json
import os

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import distance
from fabric_amd.utils import inference as inf
from gpu_util import dev, st
from tests import edt_ref as ER
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu


def _blobs(h, w, seed, density=0.5):
    """uint8 {0, 1} raster of 4 x 4 blocks: contours of every orientation, blobs that touch the image edge."""
    r = np.random.default_rng(seed)
    small = r.random(((h + 3) // 4, (w + 3) // 4)) < density
    return np.repeat(np.repeat(small, 4, axis=0), 4, axis=1)[:h, :w].astype(np.uint8)


def _pair(shape, ignore, seed=0):
    h, w = shape
    truth = _blobs(h, w, seed)
    pred = np.roll(truth, (1, 2), axis=(0, 1)) ^ (np.random.default_rng(seed + 1).random((h, w)) < 0.01)
    if ignore is not None:
        truth = truth.copy()
        truth[_blobs(h, w, seed + 2, 0.2) == 1] = ignore
    return pred.astype(np.uint8), truth


@pytest.mark.parametrize('ignore', [None, 255])
@pytest.mark.parametrize('tolerance', [0, 1, 3])
@pytest.mark.parametrize('shape', [(67, 93), (130, 257)])
def test_boundary_scores_match_the_reference(shape, tolerance, ignore):
    pred, truth = _pair(shape, ignore)
    want = ER.boundary_scores_ref(pred, truth, tolerance, 1, ignore)
    got = distance.boundary_scores(torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda(), tolerance, 1, ignore)
    print(shape, tolerance, ignore, got)
    assert got == want
    assert want['n_pred'] > 0 and want['n_true'] > 0 and 0 < want['boundary_f1'] <= 1 and want['hausdorff'] > 0
    if tolerance == 3:
        assert want['pred_hit'] > ER.boundary_scores_ref(pred, truth, 0, 1, ignore)['pred_hit']


@guarded
def test_boundary_sets_and_counts_on_guarded_buffers():
    """The two kernels of the scores through the C ABI: the boundary rasters equal the binary_erosion expression, the six integers the
    reference's."""
    shape = (67, 93)
    pred, truth = _pair(shape, 255, seed=4)
    h, w = shape
    p_d, t_d = dev(torch.from_numpy(pred), torch.uint8), dev(torch.from_numpy(truth), torch.uint8)
    bnd = guard.full((2, h, w), 7, dtype=torch.uint8)
    _lib.call('bdn_boundary_mask', p_d.data_ptr(), 1, t_d.data_ptr(), 255, bnd[0].data_ptr(), h, w, st())
    _lib.call('bdn_boundary_mask', t_d.data_ptr(), 1, t_d.data_ptr(), 255, bnd[1].data_ptr(), h, w, st())
    valid = truth != 255
    want = np.stack([ER.boundary_ref(pred == 1, valid), ER.boundary_ref(truth == 1, valid)]).astype(np.uint8)
    assert np.array_equal(bnd.cpu().numpy(), want)
    ws = guard.alloc_bytes(_lib.load().bdn_edt_workspace_bytes(2, h, w), label='edt workspace')
    d2 = guard.full((2, h, w), -7, dtype=torch.int32)
    _lib.call('bdn_edt', bnd.data_ptr(), 1, 1, None, 0, ER.LIMIT, d2.data_ptr(), ws.data_ptr(), 2, h, w, st())
    out = guard.full((6,), -7, dtype=torch.int64)
    _lib.call('bdn_boundary_score', bnd.data_ptr(), d2.data_ptr(), 4, out.data_ptr(), h, w, st())
    ref = ER.boundary_scores_ref(pred, truth, 2, 1, 255)
    assert out.tolist() == [ref[k] for k in ('n_pred', 'n_true', 'pred_hit', 'true_hit', 'hd2_pred_to_true', 'hd2_true_to_pred')]


def test_empty_and_identical_masks():
    h, w = 67, 93
    truth = _blobs(h, w, 3)
    t_d = torch.from_numpy(truth).cuda()
    zero = torch.zeros_like(t_d)
    for pred, tr in ((zero, t_d), (t_d, zero), (zero, zero)):
        got = distance.boundary_scores(pred, tr, 2)
        assert got == ER.boundary_scores_ref(pred.cpu().numpy(), tr.cpu().numpy(), 2)
        assert got['boundary_f1'] == 0.0 and got['hausdorff'] is None and got['hd2_pred_to_true'] == -1 and got['hd2_true_to_pred'] == -1
    same = distance.boundary_scores(t_d, t_d, 0)
    assert same['boundary_f1'] == 1.0 and same['hausdorff'] == 0.0 and same['n_pred'] == same['pred_hit'] > 0
    full = torch.ones_like(t_d)                             # all foreground: the image edge makes no contour
    assert distance.boundary_scores(full, full, 2)['n_pred'] == 0


def test_one_larger_case():
    shape = (1030, 2051)
    pred, truth = _pair(shape, 255, seed=9)
    got = distance.boundary_scores(torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda(), 2, 1, 255)
    assert got == ER.boundary_scores_ref(pred, truth, 2, 1, 255)


def test_train_loop_scene_boundary_keys(tmp_path, capsys, monkeypatch):
    """One epoch on synthesised band files, twice with the same seed (tests/test_gpu_objects.py's arrangement): the plain blended run has
    today's scene line; with --scene_boundary_tol the line gains the boundary keys, equal to the reference's on the written PNG and the
    label raster."""
    from fabric_amd import train as T_
    from fabric_amd.utils import ingest as ing
    from test_gpu_ingest import _synthetic_oscd
    root = str(tmp_path) + '/data/'
    bands = ['B01', 'B02', 'B03', 'B04', 'B05', 'B06', 'B07', 'B08', 'B8A', 'B09', 'B10', 'B11', 'B12']
    _synthetic_oscd(root, {'aa': (128, 160), 'cc': (100, 130)}, bands, seed=8)
    meta = {'band_ids': bands, 'band_means': {b: 3000.0 for b in bands}, 'band_stds': {b: 1500.0 for b in bands},
            'patch_size': 32, 'stride': 32, 'batch_size': 8, 'validation_cities': ['cc'], 'epochs': 1}
    mpath = str(tmp_path / 'metadata.json')
    json.dump(meta, open(mpath, 'w'))
    real, calls = inf.predict_scene_blended, []

    def spy(*a, **kw):
        proba, mask = real(*a, **kw)
        calls.append(proba.clone())
        return proba, mask
    monkeypatch.setattr(inf, 'predict_scene_blended', spy)
    keys = {'boundary_precision', 'boundary_recall', 'boundary_f1', 'hausdorff', 'boundary_tol'}

    def run(name, extra):
        log = tmp_path / name
        T_.main(['--metadata', mpath, '--dataset_dir', root, '--log_dir', str(log), '--augmentation', 'false', '--num_workers', '0',
                 '--scene_stride', '16'] + extra)
        lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')]
        return [x for x in lines if 'scene' in x][0]['scene']['cc'], (ing.read_png_gray(str(log / 'cc_epoch_0.png')) == 255).astype(np.uint8)

    cnt0, _ = run('plain', [])
    assert not keys & set(cnt0)
    t = float(torch.quantile(calls[0][1].flatten(), 0.7))  # the one-epoch model's argmax mask is empty: threshold at 30 % foreground
    cnt, mask = run('boundary', ['--scene_threshold', repr(t), '--scene_boundary_tol', '2'])
    label = (ing.read_png_gray(os.path.join(root, 'labels', 'cc', 'cm', 'cm.png')) > 0).astype(np.uint8)
    want = ER.boundary_scores_ref(mask, label, 2, 1, None)
    assert keys <= set(cnt) and want['n_pred'] > 0 and want['n_true'] > 0
    for k in keys:
        assert cnt[k] == want[k], k
