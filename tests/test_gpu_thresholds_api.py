"""-m gpu: the label-free thresholds through their Python surface -- RasterHistogram (accumulation, merge, select, the one host read),
auto_threshold with the ends found on the device, mad.auto_change_mask on a 97 x 131 13-band pair against the restatements of IR-MAD and
of the thresholds, and predict_scene_blended(auto_threshold=) on a small scene.  Everything is compared with tests/thresholds_ref.py applied
to what the device holds (its raster, its edges), so every comparison is exact but for the selection's log and exp (test_gpu_thresholds.py)."""
import math

import numpy as np
import pytest
import torch

from fabric_amd.utils import inference as inf
from fabric_amd.utils import mad as MAD
from fabric_amd.utils import thresholds as T
from tests import mad_ref as MR
from tests import thresholds_ref as R

pytestmark = pytest.mark.gpu


def _twin_table(hist, table):
    return R.read_table(*R.hist_threshold(hist, table.coord.cpu().numpy(), table.edges.cpu().numpy()))


def _same_split(got, want, name):
    """The device's row against the restatement's: the same decision, the same counts."""
    assert got['ok'] == want['ok'], (name, got, want)
    if want['ok']:
        assert (got['bin'], got['n0'], got['n1'], got['n'], got['below'], got['above']) == \
               (want['bin'], want['n0'], want['n1'], want['n'], want['below'], want['above']), (name, got, want)
        assert got['thr'] == want['thr'] == got['value']
    else:
        assert math.isnan(got['thr'])


def test_raster_histogram_accumulates_and_merges():
    r = np.random.default_rng(21)
    a = r.normal(1.0, 1.0, (37, 53)).astype(np.float32)
    b = np.where(r.random((64, 64)) < 0.8, r.normal(0.0, 0.7, (64, 64)), r.normal(4.0, 0.5, (64, 64))).astype(np.float32)
    b[3, 4:8] = (np.nan, np.inf, -7.0, 9.0)
    ex = (r.random((64, 64)) < 0.2).astype(np.uint8)
    edges, coord = T.bin_edges(-2.0, 6.0, 200)
    assert np.array_equal(edges.numpy(), R.bin_edges(-2.0, 6.0, 200)[0])
    edges, coord = edges.cuda(), coord.cuda()
    ga, gb, gex = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(ex).cuda()
    h = T.RasterHistogram(edges, coord)
    h.update(ga)
    h.update(gb, gex, 1)
    want = R.raster_hist(b, edges.cpu().numpy(), ex, 1, hist=R.raster_hist(a, edges.cpu().numpy()))
    assert np.array_equal(h.counts.cpu().numpy().view(np.uint64), want) and want[200:].all()
    h1, h2 = T.RasterHistogram(edges, coord), T.RasterHistogram(edges, coord)
    h1.update(ga)
    h2.update(gb, gex, 1)
    h1.merge(h2)
    assert torch.equal(h1.counts, h.counts)
    table = h.select()
    got, twin = table.read(), _twin_table(want, table)
    assert set(got) == set(T.METHODS) and sum(d['ok'] for d in got.values()) >= 3
    for m in T.METHODS:
        _same_split(got[m], twin[m], m)
        mask = table.mask(gb, m, exclude=gex, exclude_value=1, excluded_out=9)
        assert np.array_equal(mask.cpu().numpy(), R.raster_mask(b, got[m]['thr'], False, ex, 1, 9)), m
        out = torch.empty(64, 64, dtype=torch.uint8, device='cuda')
        assert table.mask(gb, m, below=True, out=out) is out and np.array_equal(out.cpu().numpy(), R.raster_mask(b, got[m]['thr'], True)), m
    only = h.select('rosin').read()
    assert only['rosin'] == got['rosin'] and not only['otsu']['ok'] and math.isnan(only['otsu']['thr'])
    h.reset()
    assert not h.counts.any() and not any(d['ok'] for d in h.select().read().values())


def test_auto_threshold_finds_its_ends_on_the_device():
    r = np.random.default_rng(22)
    v = np.where(r.random((97, 131)) < 0.9, r.normal(0.0, 1.0, (97, 131)), r.normal(7.0, 1.0, (97, 131))).astype(np.float32)
    v[5, 5:8] = (np.nan, np.inf, -np.inf)
    ex = np.zeros((97, 131), np.uint8)
    ex[0, :] = 1
    v[0, 0], v[0, 1] = 1e6, -1e6                                     # excluded: they must not stretch the bins
    gv, gex = torch.from_numpy(v).cuda(), torch.from_numpy(ex).cuda()
    for method in T.METHODS:
        mask, table = T.auto_threshold(gv, method, 256, exclude=gex, exclude_value=1, excluded_out=2)
        e = table.edges.cpu().numpy()
        keep = np.isfinite(v) & (ex != 1)
        assert e[0] == v[keep].min() and e[-1] == v[keep].max() and (np.diff(e) >= 0).all()
        hist = R.raster_hist(v, e, ex, 1)
        assert hist[256] == hist[257] == 0 and hist[258] == 131 + 3
        got, twin = table.read(), _twin_table(hist, table)
        _same_split(got[method], twin[method], method)
        assert got[method]['ok'] and all(not got[m]['ok'] for m in T.METHODS if m != method)
        assert np.array_equal(mask.cpu().numpy(), R.raster_mask(v, got[method]['thr'], False, ex, 1, 2))
        assert int((mask == 1).sum().item()) == got[method]['n1']
    mask, table = T.auto_threshold(gv, 'otsu', 64, lo=-4.0, hi=12.0)          # given ends: the host's table
    assert np.array_equal(table.edges.cpu().numpy(), R.bin_edges(-4.0, 12.0, 64)[0])
    d = table.read()['otsu']
    assert d['ok'] and 2.0 < d['thr'] < 5.0 and int(mask.sum().item()) == d['n1'] + d['above']
    mask, table = T.auto_threshold(torch.full((8, 8), 2.5, device='cuda'), 'otsu')       # a constant raster: lo == hi, nothing to split
    assert not mask.any() and not table.read()['otsu']['ok']


def test_auto_change_mask_against_the_twins():
    d1, d2, changed = MR.scene(7, 13, 97, 131)
    d2 = d2.copy()
    d2[3, 10, 10:14] = np.nan                                        # invalid pixels: out of the histogram, excluded_out in the mask
    bands = list(range(13))
    res = MAD.irmad(torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda(), iters=4, tol=0.0)
    ref = MR.irmad_ref(d1, d2, bands, iters=4, tol=0.0)
    chi2 = res.chi2.cpu().numpy()
    assert np.allclose(chi2, ref['chi2'], rtol=1e-4, atol=1e-4)     # the pair is the one of test_gpu_mad.py; the masks below use the device's raster
    invalid = (~ref['valid']).astype(np.uint8)
    assert invalid.sum() == 4
    for method, on, spacing in (('rosin', 'chi2', 'sqrt'), ('otsu', 'chi2', 'sqrt'), ('kittler', 'chi2', 'linear'), ('em', 'chi2', 'sqrt'),
                                ('otsu', 'proba', 'linear')):
        mask, table = MAD.auto_change_mask(res, method, on, 512, spacing, excluded_out=3)
        raster = chi2 if on == 'chi2' else res.proba[1].cpu().numpy()
        e = table.edges.cpu().numpy()
        assert e[0] == 0 and e[-1] == (raster[ref['valid']].max() if on == 'chi2' else 1.0)
        hist = R.raster_hist(raster, e, invalid, 1)
        got, twin = table.read(), _twin_table(hist, table)
        _same_split(got[method], twin[method], (method, on))
        assert got[method]['ok'] and got[method]['n'] + got[method]['below'] + got[method]['above'] == 97 * 131 - 4
        want = R.raster_mask(raster, got[method]['thr'], False, invalid, 1, 3)
        assert np.array_equal(mask.cpu().numpy(), want) and (mask == 3).sum().item() == 4
        f1 = 2 * (want == 1)[changed].sum() / ((want == 1).sum() + changed.sum())
        print(f'{method} on {on} ({spacing}): threshold {got[method]["thr"]:.4g}, F1 against the planted change {f1:.3f}')
    mask, table = MAD.auto_change_mask(res, 'rosin', chi2_max=50.0, n_bins=128)
    assert table.edges[-1].item() == 50.0 and table.read()['rosin']['above'] > 0
    out = torch.empty(97, 131, dtype=torch.uint8, device='cuda')
    assert MAD.auto_change_mask(res, out=out)[0] is out


C_, H_, W_, P_ = 3, 100, 115, 32


@pytest.fixture(scope='module')
def scene():
    """(model, date 1, date 2) of one small scene with overlap in both axes at patch 32, stride 16."""
    from test_gpu_scene_blend import _calibrated_model, _scene
    d1, d2 = _scene(C_, H_, W_, 5)
    return _calibrated_model(C_, 'fp32', d1, d2, P_), torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()


def test_predict_scene_blended_auto_threshold(scene):
    model, g1, g2 = scene
    h, w, p = H_, W_, P_
    kw = dict(patch_size=p, stride=16, window='gaussian', symmetries=(0,), batch_size=16)
    proba0, mask0 = inf.predict_scene_blended(model, g1, g2, **kw)
    pn, mn = inf.predict_scene_blended(model, g1, g2, auto_threshold=None, threshold_out=None, **kw)
    assert torch.equal(pn, proba0) and torch.equal(mn, mask0)       # None: the call as it was
    p1 = proba0[1].cpu().numpy()
    for method in ('otsu', 'rosin'):
        got = {}
        pr, m = inf.predict_scene_blended(model, g1, g2, auto_threshold=method, threshold_out=got, **kw)
        table = got['table']
        d = table.read()[method]
        assert torch.equal(pr, proba0) and d['ok'] and 0.0 < d['thr'] < 1.0
        assert np.array_equal(table.edges.cpu().numpy(), R.bin_edges(0.0, 1.0, 1024)[0])
        assert torch.equal(m, (proba0[1] >= table.thr[T.METHODS.index(method)]).to(torch.uint8))
        _same_split(d, _twin_table(R.raster_hist(p1, table.edges.cpu().numpy()), table)[method], method)
        assert int(m.sum().item()) == d['n1'] and 0 < d['n1'] < h * w
    pr, m = inf.predict_scene_blended(model, g1, g2, auto_threshold='otsu', close_radius2=1, min_area=3, **kw)
    from fabric_amd.utils import morphology as M
    from fabric_amd.utils.objects import remove_small_objects
    plain = inf.predict_scene_blended(model, g1, g2, auto_threshold='otsu', **kw)[1]
    assert torch.equal(m, remove_small_objects(M.binary_closing(plain, 1), 3, 8))
    for bad, match in ((dict(auto_threshold='median'), 'method'), (dict(auto_threshold='otsu', threshold=0.5), 'by value'),
                       (dict(auto_threshold='otsu', threshold=0.5, hysteresis_low=0.2), 'by value'), (dict(threshold_out={}), 'threshold_out')):
        with pytest.raises(ValueError, match=match):
            inf.predict_scene_blended(model, None, None, **kw, **bad)               # refused before the scene is touched


def test_scene_pass_of_the_training_loop(scene, tmp_path, capsys):
    import json
    import types
    from fabric_amd import train as T_
    from fabric_amd.utils import ingest as ing
    model, g1, g2 = scene
    h, w, p = H_, W_, P_
    label = np.zeros((h, w), np.uint8)
    label[h // 4:h // 2, w // 3:w // 2] = 1                          # the changed block of the scene
    label[:6, :] = 255                                               # an ignored strip
    scenes = {'aa': {'images': (g1, g2), 'labels': label}}
    opt = types.SimpleNamespace(log_dir=str(tmp_path), scene_stride=16, patch_size=p, scene_window='gaussian', scene_tta=1, batch_size=16,
                                val_curve_bins=0, ignore_label=255, scene_connectivity=8, scene_objects=False)
    auto, mad = T_.check_auto_threshold_flags('otsu', 'rosin', 3, 'argmax', 16)
    T_._predict_scenes(model, scenes, ['aa'], opt, 0, auto_threshold=auto, mad_baseline=mad)
    line = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')][-1]['scene']['aa']
    got = {}
    _, want = inf.predict_scene_blended(model, g1, g2, patch_size=p, stride=16, batch_size=16, auto_threshold='otsu', threshold_out=got)
    d = got['table'].read()['otsu']
    assert line['auto_threshold'] == {'method': 'otsu', 'value': d['value'], 'bin': d['bin'], 'ok': True}
    png = (ing.read_png_gray(str(tmp_path / 'aa_epoch_0.png')) == 255).astype(np.uint8)
    assert np.array_equal(png, want.cpu().numpy()) and png.any()
    assert {k: line[k] for k in ('tp', 'fp', 'fn')} == {k: v for k, v in T_.cleaned_scores(png, label, 255).items() if k in ('tp', 'fp', 'fn')}
    b = line['mad_baseline']
    assert set(b) == {'method', 'threshold', 'iters', 'tp', 'fp', 'fn', 'precision', 'recall', 'f1'} and b['method'] == 'rosin' and b['iters'] == 3
    ex = torch.from_numpy(label).cuda()
    res = MAD.irmad(g1, g2, exclude=ex, exclude_value=255, iters=3)
    m, table = MAD.auto_change_mask(res, 'rosin')
    assert b['threshold'] == table.read()['rosin']['value']
    assert {k: b[k] for k in ('tp', 'fp', 'fn')} == {k: v for k, v in T_.cleaned_scores(m.cpu().numpy(), label, 255).items() if k in ('tp', 'fp', 'fn')}
    assert b['tp'] + b['fn'] == int((label == 1).sum()) and b['recall'] > 0.5          # the planted block stands out of the noise
    # the flags off: today's line
    T_._predict_scenes(model, scenes, ['aa'], opt, 1)
    line = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')][-1]['scene']['aa']
    assert 'auto_threshold' not in line and 'mad_baseline' not in line
