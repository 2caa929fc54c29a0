"""-m gpu: the Python surface of the score curve -- fabric_amd.utils.metrics.ScoreCurve against tests/curve_ref.py on the concatenated
batches, predict_scene_blended(threshold=) and the training loop's --val_curve_bins / --scene_threshold."""
import json
import os

import numpy as np
import pytest
import torch

from fabric_amd.utils import inference as inf
from fabric_amd.utils.metrics import ScoreCurve
from tests import curve_ref as CR

pytestmark = pytest.mark.gpu
IGN = 255


def _batches(seed=0, ncls=2, hw=(45, 38), sizes=(3, 2, 4)):
    r = np.random.default_rng(seed)
    out = []
    for k, b in enumerate(sizes):
        logits = (3 * r.standard_normal((b, ncls) + hw)).astype(np.float32)
        labels = r.integers(0, ncls, (b,) + hw)
        labels[r.random((b,) + hw) < 0.2] = IGN
        out.append((logits, labels))
    return out


def _fed(curve, batches, dtypes=(torch.int64, torch.uint8, torch.int32)):
    """Feed the batches (labels in turn as [B,H,W] / [B,1,H,W] and in several integer dtypes); returns the exported scores, concatenated."""
    scores = []
    for k, (lg, lb) in enumerate(batches):
        t = torch.from_numpy(lb).to(dtypes[k % len(dtypes)]).cuda()
        out = torch.full(lb.shape, float('nan'), device='cuda')
        curve.update(torch.from_numpy(lg).cuda(), t[:, None] if k % 2 else t, scores_out=out)
        scores.append(out.cpu().numpy().reshape(-1))
    return np.concatenate(scores)


@pytest.mark.parametrize('n_bins,ncls,pos', [(1024, 2, 1), (64, 3, 2), (4096, 2, 0)])
def test_score_curve_over_batches_matches_the_reference(n_bins, ncls, pos):
    batches = _batches(n_bins, ncls)
    sc = ScoreCurve(n_bins, pos, IGN)
    s = _fed(sc, batches)
    labels = np.concatenate([lb.reshape(-1) for _, lb in batches])
    ref64 = np.concatenate([CR.softmax_scores(lg, pos).reshape(-1) for lg, _ in batches])
    assert np.abs(s - ref64)[labels != IGN].max() <= 2e-6 and (s[labels == IGN] == 0).all()
    h = CR.histogram(s, labels, n_bins, pos, IGN)
    assert sc.hist.dtype == torch.int64 and sc.hist.shape == (2, n_bins) and np.array_equal(sc.hist.cpu().numpy(), h)
    want, got = CR.summary(h), sc.compute()
    assert set(got) == {'best_f1', 'best_threshold', 'best_bin', 'precision', 'recall', 'ap', 'n_pos', 'n_neg'}
    assert (got['best_f1'], got['best_threshold'], got['best_bin'], got['precision'], got['recall'], got['n_pos'], got['n_neg']) == \
           (want['F_best'], want['t_best'], want['i_best'], want['P_best'], want['R_best'], want['n_pos'], want['n_neg'])
    assert abs(got['ap'] - want['AP']) <= 1e-12
    assert all(type(got[k]) is int for k in ('best_bin', 'n_pos', 'n_neg')) and type(got['ap']) is float
    c = CR.curve(h)
    for t, k in zip(sc.curve(), ('TP', 'FP', 'P', 'R')):
        assert t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), c[k].astype(np.float64)), k
    # at(): an arbitrary threshold is rounded down to a bin edge; 0.5 is one
    valid, posl = labels != IGN, labels == pos
    for thr in (0.5, 0.3, 0.0, 1.0, 0.77):
        i = min(int(thr * n_bins), n_bins - 1)
        pred = s >= np.float32(i / n_bins)
        tp, fp, fn = int((pred & valid & posl).sum()), int((pred & valid & ~posl).sum()), int((~pred & valid & posl).sum())
        a = sc.at(thr)
        assert (a['tp'], a['fp'], a['fn']) == (tp, fp, fn), thr
        assert a['precision'] == (tp / (tp + fp) if tp + fp else 0.0) and a['recall'] == tp / (tp + fn) and a['f1'] == 2 * tp / (2 * tp + fp + fn)
    assert (sc.at(0.5)['tp'], sc.at(0.5)['fp']) == (int(((s >= 0.5) & valid & posl).sum()), int(((s >= 0.5) & valid & ~posl).sum()))


def test_merge_reset_and_probability_input():
    batches = _batches(5)
    whole, a, b = ScoreCurve(256, 1, IGN), ScoreCurve(256, 1, IGN), ScoreCurve(256, 1, IGN)
    s = _fed(whole, batches)
    _fed(a, batches[:1])
    _fed(b, batches[1:])
    a.merge(b)
    assert torch.equal(a.hist, whole.hist)
    empty = ScoreCurve(256, 1, IGN)
    empty.merge(whole)                                       # into an instance that has seen nothing yet
    assert torch.equal(empty.hist, whole.hist)
    whole.reset()
    assert not whole.hist.any() and whole.compute() == {'best_f1': 0.0, 'best_threshold': 0.0, 'best_bin': 0, 'precision': 0.0, 'recall': 0.0,
                                                        'ap': 0.0, 'n_pos': 0, 'n_neg': 0}
    assert ScoreCurve(64).compute()['n_neg'] == 0            # never fed: an all-zero histogram
    # probabilities as they are: a [ncls,H,W] scene and a [B,ncls,H,W] batch
    lg, lb = batches[0]
    p = torch.softmax(torch.from_numpy(lg).cuda(), 1)
    one, many = ScoreCurve(256, 1, IGN), ScoreCurve(256, 1, IGN)
    many.update_proba(p, torch.from_numpy(lb).cuda())
    for k in range(p.shape[0]):
        one.update_proba(p[k], torch.from_numpy(lb[k]).cuda())
    want = CR.histogram(p[:, 1].cpu().numpy(), lb, 256, 1, IGN)
    assert np.array_equal(many.hist.cpu().numpy(), want) and torch.equal(one.hist, many.hist)
    with pytest.raises(RuntimeError):
        many.update(torch.zeros(2, 2, 4, 4, device='cuda'), torch.zeros(2, 5, 4, device='cuda', dtype=torch.uint8))


def test_predict_scene_blended_threshold():
    from test_gpu_scene_blend import _calibrated_model, _scene
    c, h, w, p = 3, 88, 75, 32
    d1, d2 = _scene(c, h, w, 3)
    model = _calibrated_model(c, 'fp32', d1, d2, p)
    g1, g2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    kw = dict(patch_size=p, stride=12, window='gaussian', symmetries=(0, 5), batch_size=9)
    proba0, mask0 = inf.predict_scene_blended(model, g1, g2, **kw)
    pn, mn = inf.predict_scene_blended(model, g1, g2, threshold=None, **kw)
    assert torch.equal(pn, proba0) and torch.equal(mn, mask0) and torch.equal(mask0, torch.max(proba0, 0)[1].to(torch.uint8))
    present = float(proba0[1].flatten()[proba0[1].numel() // 3])             # a value the map holds
    for t in (present, 0.5, 0.0, 1.0, 0.123):
        pr, m = inf.predict_scene_blended(model, g1, g2, threshold=t, **kw)
        assert torch.equal(pr, proba0), t
        assert m.dtype == torch.uint8 and torch.equal(m, (proba0[1] >= t).to(torch.uint8)), t
    ties = proba0[0] == proba0[1]
    _, m5 = inf.predict_scene_blended(model, g1, g2, threshold=0.5, **kw)
    assert torch.equal(m5[~ties], mask0[~ties])                              # 0.5 and the argmax differ only at exact ties
    _, m0 = inf.predict_scene_blended(model, g1, g2, threshold=present, pos_class=0, **kw)
    assert torch.equal(m0, (proba0[0] >= present).to(torch.uint8))
    for bad in (1.5, -0.1, float('nan'), '0.5'):
        with pytest.raises(ValueError, match='threshold'):
            inf.predict_scene_blended(model, g1, g2, threshold=bad, **kw)
    with pytest.raises(ValueError, match='pos_class'):
        inf.predict_scene_blended(model, g1, g2, threshold=0.5, pos_class=2, **kw)


_SYNTH = ['--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64', '--stride', '128', '--num_workers', '0',
          '--learning_rate', '0.02']


def _epoch_line(capsys):
    return [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{"epoch"') and 'scene' not in json.loads(x)][-1]


def test_cli_synthetic_epoch_with_and_without_the_curve(tmp_path, capsys):
    from fabric_amd import train as T
    T.main(_SYNTH + ['--log_dir', str(tmp_path / 'plain')])
    plain = _epoch_line(capsys)
    T.main(_SYNTH + ['--log_dir', str(tmp_path / 'curve'), '--val_curve_bins', '256', '--scene_stride', '64', '--scene_threshold', 'val'])
    curve = _epoch_line(capsys)
    new = {'validate_best_f1', 'validate_best_threshold', 'validate_ap'}
    # without the flags: exactly the record of the code before the feature
    assert set(plain) == {'epoch'} | {f'train_{k}' for k in ('cd_losses', 'cd_corrects', 'cd_precisions', 'cd_recalls', 'cd_f1scores')} | \
        {f'validate_{k}' for k in ('cd_losses', 'cd_corrects', 'cd_precisions', 'cd_recalls', 'cd_f1scores')}
    assert set(curve) == set(plain) | new
    assert 0.0 <= curve['validate_ap'] <= 1.0 and 0.0 <= curve['validate_best_f1'] <= 1.0
    assert curve['validate_best_threshold'] * 256 == int(curve['validate_best_threshold'] * 256) and 0.0 <= curve['validate_best_threshold'] < 1.0
    meta = json.load(open(tmp_path / 'curve' / 'metadata_epoch_0.json'))['validation_metrics']
    assert {k[len('validate_'):] for k in new} <= set(meta) and meta['ap'] == curve['validate_ap']
    assert not {k[len('validate_'):] for k in new} & set(json.load(open(tmp_path / 'plain' / 'metadata_epoch_0.json'))['validation_metrics'])


def test_train_loop_scene_threshold_from_validation(tmp_path, capsys):
    """Real band files: the scene masks are P(change) >= the validation pass's best-F1 threshold, and the scene line comes from the
    device curve over the probabilities and the label raster."""
    from fabric_amd import train as T
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
    log = tmp_path / 'log'
    T.main(['--metadata', mpath, '--dataset_dir', root, '--log_dir', str(log), '--augmentation', 'false', '--scene_stride', '16',
            '--val_curve_bins', '64', '--scene_threshold', 'val'])
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')]
    epoch = [x for x in lines if 'validate_ap' in x][0]
    cnt = [x for x in lines if 'scene' in x][0]['scene']['cc']
    thr = epoch['validate_best_threshold']
    assert cnt['threshold'] == thr and {'ap', 'best_f1', 'best_threshold', 'tp', 'fp', 'fn', 'precision', 'recall', 'f1'} <= set(cnt)
    assert 0 <= cnt['ap'] <= 1 and cnt['f1'] <= cnt['best_f1'] <= 1
    mask = ing.read_png_gray(str(log / 'cc_epoch_0.png')) == 255
    label = ing.read_png_gray(os.path.join(root, 'labels', 'cc', 'cm', 'cm.png')) > 0
    # thr is a bin edge of the 64-bin curve, so the mask's own counts are the curve's counts at it
    assert (cnt['tp'], cnt['fp'], cnt['fn']) == (int((mask & label).sum()), int((mask & ~label).sum()), int((~mask & label).sum()))
