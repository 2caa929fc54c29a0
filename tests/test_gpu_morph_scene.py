"""-m gpu: the mask clean-up arguments of predict_scene_blended and of the training loop's scene pass.  One small model, one scene of
200 x 230 at patch 64, stride 32; every mask is compared bit for bit with fabric_amd.utils.morphology applied, in the stated order, to
the mask of a plain call, and with the host restatement tests/morph_ref.py."""
import json
import types

import numpy as np
import pytest
import torch

from fabric_amd.utils import inference as inf
from fabric_amd.utils import morphology as M
from fabric_amd.utils.objects import remove_small_objects
from tests import morph_ref as R

pytestmark = pytest.mark.gpu

C, H, W, P, STRIDE = 3, 200, 230, 64, 32
KW = dict(patch_size=P, stride=STRIDE, window='gaussian', symmetries=(0,), batch_size=16)


@pytest.fixture(scope='module')
def scene():
    """(model, date 1, date 2, proba and argmax mask of a plain call, a high and a low threshold that leave about 35 % / 55 % foreground)."""
    from test_gpu_scene_blend import _calibrated_model, _scene
    d1, d2 = _scene(C, H, W, 5)
    model = _calibrated_model(C, 'fp32', d1, d2, P)
    g1, g2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    proba, mask = inf.predict_scene_blended(model, g1, g2, **KW)
    q = torch.quantile(proba[1].flatten(), torch.tensor([0.45, 0.65], device='cuda')).tolist()
    return types.SimpleNamespace(model=model, g1=g1, g2=g2, proba=proba, mask=mask, low=q[0], high=q[1])


def test_blended_scene_cleanup(scene):
    s = scene
    run = lambda **kw: inf.predict_scene_blended(s.model, s.g1, s.g2, **KW, **kw)         # noqa: E731
    # all four None: the bits of a call without them
    pn, mn = run(hysteresis_low=None, close_radius2=None, fill_holes=None, open_radius2=None)
    assert torch.equal(pn, s.proba) and torch.equal(mn, s.mask)
    _, plain = run(threshold=s.high)
    plain_np = plain.cpu().numpy()
    proba_np = s.proba.cpu().numpy()
    print('foreground at the high threshold', float(plain_np.mean()))
    assert 0.2 < plain_np.mean() < 0.5

    def both(kw, want_dev, want_np):
        pr, m = run(threshold=s.high, **kw)
        assert torch.equal(pr, s.proba), kw
        assert m.dtype == torch.uint8 and torch.equal(m, want_dev), kw
        assert np.array_equal(m.cpu().numpy(), want_np), kw
        return m

    hyst = both(dict(hysteresis_low=s.low), M.hysteresis_mask(s.proba, s.low, s.high), R.hysteresis_mask(proba_np, s.low, s.high))
    assert int(hyst.sum()) > int(plain.sum())
    closed = both(dict(close_radius2=2), M.binary_closing(plain, 2), R.binary_closing(plain_np, 2))
    filled = both(dict(fill_holes=True), M.fill_holes(plain), R.fill_holes(plain_np))
    both(dict(fill_holes=3), M.fill_holes(plain, 3), R.fill_holes(plain_np, 3))
    opened = both(dict(open_radius2=2), M.binary_opening(plain, 2), R.binary_opening(plain_np, 2))
    assert not torch.equal(closed, plain) and not torch.equal(filled, plain) and not torch.equal(opened, plain)
    # all together, 4-connectivity, with the area filter behind: the stated order
    want = M.binary_opening(M.fill_holes(M.binary_closing(M.hysteresis_mask(s.proba, s.low, s.high, 1, 4), 2), 30, 4), 5)
    want_np = R.cleanup(R.hysteresis_mask(proba_np, s.low, s.high, 1, 4), 2, 30, 5, 4)
    assert np.array_equal(want.cpu().numpy(), want_np)
    pr, m = run(threshold=s.high, hysteresis_low=s.low, close_radius2=2, fill_holes=30, open_radius2=5, connectivity=4, min_area=40)
    assert torch.equal(pr, s.proba) and torch.equal(m, remove_small_objects(want, 40, 4))
    # another order gives another mask: the order is what is tested
    assert not torch.equal(M.binary_closing(M.binary_opening(M.fill_holes(M.hysteresis_mask(s.proba, s.low, s.high, 1, 4), 30, 4), 5), 2), want)
    # without a threshold the clean-up works on the argmax mask
    pr, m = run(close_radius2=1, open_radius2=1)
    assert torch.equal(pr, s.proba) and torch.equal(m, M.binary_opening(M.binary_closing(s.mask, 1), 1))
    for kw, match in ((dict(hysteresis_low=0.2), 'needs a threshold'), (dict(threshold=0.3, hysteresis_low=0.4), 'hysteresis_low'),
                      (dict(close_radius2=-1), 'radius2'), (dict(open_radius2=1.5), 'radius2'), (dict(fill_holes=0), 'max_area'),
                      (dict(fill_holes=True, connectivity=6), 'connectivity')):
        with pytest.raises(ValueError, match=match):
            inf.predict_scene_blended(s.model, None, None, **KW, **kw)               # refused before the scene is touched


@pytest.mark.parametrize('curve', [0, 64])
def test_scene_pass_of_the_training_loop(scene, tmp_path, capsys, curve):
    from fabric_amd import train as T_
    from fabric_amd.utils import ingest as ing
    s = scene
    label = np.zeros((H, W), np.uint8)
    label[H // 4:H // 2, W // 3:W // 2] = 1                          # the changed block of the scene
    label[:10, :] = 255                                              # an ignored strip
    scenes = {'aa': {'images': (s.g1, s.g2), 'labels': label}}
    cleanup = T_.check_cleanup_flags(s.low, 2, 30, 5, s.high, 4, STRIDE)
    opt = types.SimpleNamespace(log_dir=str(tmp_path), scene_stride=STRIDE, patch_size=P, scene_window='gaussian', scene_tta=1, batch_size=16,
                                val_curve_bins=curve, ignore_label=255, scene_connectivity=4, scene_objects=True)
    T_._predict_scenes(s.model, scenes, ['aa'], opt, 0, threshold=s.high, min_area=40, cleanup=cleanup)
    line = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')][-1]['scene']['aa']
    assert line['cleanup'] == {'hysteresis_low': s.low, 'close_radius2': 2, 'fill_holes': 30, 'open_radius2': 5}
    after_open = M.binary_opening(M.fill_holes(M.binary_closing(M.hysteresis_mask(s.proba, s.low, s.high, 1, 4), 2), 30, 4), 5)
    want = remove_small_objects(after_open, 40, 4).cpu().numpy()
    png = (ing.read_png_gray(str(tmp_path / 'aa_epoch_0.png')) == 255).astype(np.uint8)
    assert np.array_equal(png, want) and want.any()
    keep = label != 255
    tp, fp, fn = int((want == 1)[keep & (label == 1)].sum()), int((want == 1)[keep & (label == 0)].sum()), int((want == 0)[keep & (label == 1)].sum())
    c = line['cleaned']
    assert (c['tp'], c['fp'], c['fn']) == (tp, fp, fn) and set(c) == {'tp', 'fp', 'fn', 'precision', 'recall', 'f1'}
    assert c['precision'] == (tp / (tp + fp) if tp + fp else 0.0) and c['recall'] == tp / (tp + fn)
    # --scene_objects scores the mask after the opening, before the area filter
    from fabric_amd.utils.objects import object_scores
    obj = object_scores(after_open, torch.from_numpy(label).cuda(), 1, 255, 4, 40)
    assert line['objects_pred'] == obj['objects_pred'] and line['object_f1'] == obj['object_f1'] and line['min_area'] == 40
    if curve:
        assert 'ap' in line and 'best_threshold' in line
    # the flags off: today's line
    T_._predict_scenes(s.model, scenes, ['aa'], opt, 1, threshold=s.high, min_area=40)
    line = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')][-1]['scene']['aa']
    assert 'cleanup' not in line and 'cleaned' not in line
