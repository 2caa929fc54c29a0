"""-m gpu: fabric_amd.utils.objects (label_components, remove_small_objects, component_table, object_scores) against tests/cc_ref.py,
predict_scene_blended(min_area=) on the smallest scene with overlap in both axes, and the training loop's --scene_min_area /
--scene_objects output against cc_ref computed from the written PNG and the label raster."""
import json
import os

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import inference as inf
from fabric_amd.utils import objects as O
from tests import cc_ref as R

pytestmark = pytest.mark.gpu

T = _lib.load().bdn_cc_tile()
CASES = [((2 * T + 3, 3 * T + 1), 'random 0.5', 4), ((96, 200), 'random 0.593', 8), ((7, 13), 'random 0.1', 8)]


def _truth(shape, seed):
    """A truth raster with blobs of class 1 and an ignore label 255 painted over a part of it."""
    r = np.random.default_rng(seed)
    t = (r.random(shape) < 0.3).astype(np.uint8)
    t[r.random(shape) < 0.1] = 255
    return t


@pytest.mark.parametrize('shape,pattern,conn', CASES)
def test_objects_api_matches_the_restatement(shape, pattern, conn):
    m = R.patterns(*shape, tile=T)[pattern]
    truth = _truth(shape, 4)
    g, gt = torch.from_numpy(m).cuda(), torch.from_numpy(truth).cuda()
    lab = R.label(m == 1, conn)
    n = R.counts(lab)[0]
    # labels: compact and canonical, a foreground value, an exclusion
    got, gn = O.label_components(g, conn)
    assert gn == n and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), R.compact(lab))
    got, gn = O.label_components(g, conn, compact=False)
    assert gn == n and np.array_equal(got.cpu().numpy(), lab)
    lab_x = R.label(R.foreground(truth, 1, m, 0), conn)
    got, gn = O.label_components(gt, conn, fg_value=1, exclude=g, exclude_value=0)
    assert gn == R.counts(lab_x)[0] and np.array_equal(got.cpu().numpy(), R.compact(lab_x))
    # the table of the compact labels
    comp, _ = O.label_components(g, conn)
    tab = O.component_table(comp, n, gt, 1)
    assert tuple(tab.shape) == (n, 8) and np.array_equal(tab.cpu().numpy(), R.stats_table(R.compact(lab), max(n, 1), truth, 1)[:n])
    assert np.array_equal(O.component_table(comp, n).cpu().numpy(), R.stats_table(R.compact(lab), max(n, 1))[:n])
    assert tuple(O.component_table(comp, 0).shape) == (0, 8)
    # small objects, into a fresh tensor, a given one and in place
    for k in (1, 3, 50):
        want = R.remove_small(m, k, conn)
        assert np.array_equal(O.remove_small_objects(g, k, conn).cpu().numpy(), want), k
        out = torch.full_like(g, 9)
        assert O.remove_small_objects(g, k, conn, out=out) is out and np.array_equal(out.cpu().numpy(), want)
        same = g.clone()
        O.remove_small_objects(same, k, conn, out=same)
        assert np.array_equal(same.cpu().numpy(), want)
    # object scores with the ignore label, min_area and min_overlap
    for ign in (None, 255):
        for min_area in (1, 3):
            for min_overlap in (1, 3):
                got = O.object_scores(g, gt, 1, ign, conn, min_area, min_overlap)
                assert got == R.object_scores(m, truth, 1, ign, conn, min_area, min_overlap), (ign, min_area, min_overlap)
    # empty prediction / empty truth: zeros, not NaN
    z = torch.zeros_like(g)
    for a, b in ((z, gt), (g, z), (z, z)):
        s = O.object_scores(a, b)
        assert s == R.object_scores(a.cpu().numpy(), b.cpu().numpy()) and s['object_f1'] == 0.0


def test_blended_scene_min_area():
    from test_gpu_scene_blend import _calibrated_model, _scene
    c, h, w, p = 3, 48, 48, 32                             # stride 16: two tiles by two, overlap in both axes
    d1, d2 = _scene(c, h, w, 3)
    model = _calibrated_model(c, 'fp32', d1, d2, p)
    g1, g2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    assert len(inf.blend_tile_origins(h, w, p, 16)[0]) == 4
    kw = dict(patch_size=p, stride=16, window='gaussian', symmetries=(0,), batch_size=4)
    proba0, mask0 = inf.predict_scene_blended(model, g1, g2, **kw)
    pn, mn = inf.predict_scene_blended(model, g1, g2, min_area=None, **kw)
    assert torch.equal(pn, proba0) and torch.equal(mn, mask0)
    m0 = mask0.cpu().numpy()
    print('mask: foreground', int(m0.sum()), 'components', R.counts(R.label(m0 == 1, 8))[0], 'largest', int(R.areas(R.label(m0 == 1, 8)).max()))
    for conn in (4, 8):
        biggest = int(R.areas(R.label(m0 == 1, conn)).max())
        for k in (1, 2, 5, biggest, biggest + 1):
            pr, m = inf.predict_scene_blended(model, g1, g2, min_area=k, connectivity=conn, **kw)
            assert torch.equal(pr, proba0), (conn, k)
            assert m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), R.remove_small(m0, k, conn)), (conn, k)
    pr, m = inf.predict_scene_blended(model, g1, g2, threshold=0.3, min_area=4, **kw)
    assert torch.equal(pr, proba0) and np.array_equal(m.cpu().numpy(), R.remove_small((proba0[1] >= 0.3).to(torch.uint8).cpu().numpy(), 4, 8))
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match='min_area'):
            inf.predict_scene_blended(model, g1, g2, min_area=bad, **kw)
    with pytest.raises(ValueError, match='connectivity'):
        inf.predict_scene_blended(model, g1, g2, min_area=2, connectivity=6, **kw)


@pytest.mark.parametrize('ign', [None, 0])
def test_train_loop_scene_objects(tmp_path, capsys, monkeypatch, ign):
    """One epoch on synthesised band files (the --synthetic data set carries no full scenes, so the scene pass never runs on it; these
    are the smallest sizes the scene tests of the training loop use), three times with the same seed, predict_scene_blended wrapped
    so that its arguments and what it returned are on record: a plain blended run, whose probabilities give a threshold that leaves
    about 30 % of the scene foreground (the one-epoch model's probabilities all lie within a few thousandths of one half: the argmax mask
    is empty); the run with --scene_min_area / --scene_objects / --scene_connectivity at that threshold; and --scene_min_area alone.
    The unfiltered mask has components on both sides of min_area, the written PNG is cc_ref's filter of it, and the scene line's object
    keys are cc_ref's object_scores of the unfiltered mask and the label raster.  ign = 0: the run carries --ignore_label 0 (the only
    other value a {0, 1} label raster holds), so the predicted objects are cut down to the pixels labelled 1 before their areas are
    measured."""
    from fabric_amd import train as T_
    from fabric_amd.utils import ingest as ing
    from test_gpu_ingest import _synthetic_oscd
    root = str(tmp_path) + '/data/'
    bands = ['B01', 'B02', 'B03', 'B04', 'B05', 'B06', 'B07', 'B08', 'B8A', 'B09', 'B10', 'B11', 'B12']
    cities = {'aa': (128, 160), 'cc': (100, 130)}
    _synthetic_oscd(root, cities, bands, seed=8)
    meta = {'band_ids': bands, 'band_means': {b: 3000.0 for b in bands}, 'band_stds': {b: 1500.0 for b in bands},
            'patch_size': 32, 'stride': 32, 'batch_size': 8, 'validation_cities': ['cc'], 'epochs': 1}
    mpath = str(tmp_path / 'metadata.json')
    json.dump(meta, open(mpath, 'w'))
    K, conn = 3, 4
    real, calls = inf.predict_scene_blended, []

    def spy(*a, **kw):
        proba, mask = real(*a, **kw)
        calls.append((kw, proba.clone(), mask.clone()))
        return proba, mask
    monkeypatch.setattr(inf, 'predict_scene_blended', spy)

    def run(name, extra):
        log = tmp_path / name
        del calls[:]
        T_.main(['--metadata', mpath, '--dataset_dir', root, '--log_dir', str(log), '--augmentation', 'false', '--num_workers', '0',
                 '--scene_stride', '16'] + ([] if ign is None else ['--fused_step', 'true', '--ignore_label', str(ign)]) + extra)
        lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')]
        cnt = [x for x in lines if 'scene' in x][0]['scene']['cc']
        assert len(calls) == 1
        return cnt, (ing.read_png_gray(str(log / 'cc_epoch_0.png')) == 255).astype(np.uint8), calls[0]

    cnt0, _, (kw0, proba0, _) = run('plain', [])
    assert not {'objects_pred', 'objects_true', 'object_f1', 'min_area'} & set(cnt0)       # the flags at their defaults: today's line,
    assert not {'min_area', 'connectivity', 'threshold'} & set(kw0)                        # today's call
    t = float(torch.quantile(proba0[1].flatten(), 0.7))                                    # a float32 value: exact as a double
    thr = ['--scene_threshold', repr(t)]
    cnt, mask, (kw, proba, raw_t) = run('objects', thr + ['--scene_min_area', str(K), '--scene_objects', 'true', '--scene_connectivity', str(conn)])
    assert torch.equal(proba, proba0) and kw['threshold'] == t                             # the same model in every run
    raw = raw_t.cpu().numpy()
    assert np.array_equal(raw, (proba0[1] >= t).to(torch.uint8).cpu().numpy())
    label = (ing.read_png_gray(os.path.join(root, 'labels', 'cc', 'cm', 'cm.png')) > 0).astype(np.uint8)
    sizes = R.areas(R.label(raw == 1, conn))
    sizes = sizes[sizes > 0]
    print(f'P(change) in [{float(proba0[1].min()):.4f}, {float(proba0[1].max()):.4f}], threshold {t!r}: foreground {raw.mean():.3f}, {sizes.size} '
          f'components, {int((sizes < K).sum())} below {K}, largest {int(sizes.max())}; scene line {cnt}')
    assert (sizes < K).any() and (sizes >= K).any()
    # the PNG is the filtered mask, and the pixel counts are its counts
    assert np.array_equal(mask, R.remove_small(raw, K, conn)) and not np.array_equal(mask, raw)
    assert (cnt['tp'], cnt['fp'], cnt['fn']) == (int((mask & label).sum()), int((mask & (1 - label)).sum()), int(((1 - mask) & label).sum()))
    # the object keys: cc_ref on the unfiltered mask and the label raster, the ignore label cut out before the areas are measured
    want = R.object_scores(raw, label, 1, ign, conn, K, 1)
    assert cnt['min_area'] == K and cnt['objects_pred'] > 0 and cnt['objects_true'] > 0 and cnt['object_f1'] > 0
    for key in ('objects_pred', 'objects_true', 'object_precision', 'object_recall', 'object_f1'):
        assert cnt[key] == want[key], key
    # a wrong exclusion, connectivity or min_area would show in the line
    assert R.object_scores(raw, label, 1, None if ign is not None else 0, conn, K, 1)['objects_pred'] != want['objects_pred']
    assert R.object_scores(raw, label, 1, ign, 8, K, 1) != want and R.object_scores(raw, label, 1, ign, conn, 1, 1) != want
    # --scene_min_area alone: predict_scene_blended filters, the same PNG, min_area on the line and no object keys
    cnt1, mask1, (kw1, _, ret1) = run('filter', thr + ['--scene_min_area', str(K), '--scene_connectivity', str(conn)])
    assert (kw1['min_area'], kw1['connectivity']) == (K, conn) and np.array_equal(mask1, mask) and np.array_equal(ret1.cpu().numpy(), mask)
    assert cnt1['min_area'] == K and 'objects_pred' not in cnt1 and (cnt1['tp'], cnt1['fp'], cnt1['fn']) == (cnt['tp'], cnt['fp'], cnt['fn'])
