"""-m gpu: the blended full-scene scan (predict_scene_blended) -- symmetric tile gather, the fold / stitch / finalize kernels,
model-level probabilities against a float64 host restatement, equivalence with predict_scene, arrangement invariance, a 2000^2
scene and the training loop's --scene_stride output."""
import json
import os

import numpy as np
import pytest
import torch

from fabric_amd import BiDateNet
from fabric_amd._lib import call, ptr
from fabric_amd.utils import inference as inf
from fabric_amd.utils.dataloaders import _apply_symmetry
from oracle import filler
from gpu_util import DT, st, rnd
from tests import guard
from tests.guard import guarded

pytestmark = pytest.mark.gpu


def _scene(c, h, w, seed):
    r = np.random.default_rng(seed)
    d1 = r.standard_normal((c, h, w)).astype(np.float32)
    d2 = (d1 + 0.5 * r.standard_normal((c, h, w))).astype(np.float32)
    d2[:, h // 4:h // 2, w // 3:w // 2] += 2.0                    # a "changed" block
    return d1, d2


def _sym(x, code, inverse=False):
    """_apply_symmetry of the code (or of its inverse) on the last two axes."""
    return _apply_symmetry(x, inf.symmetry_bits(inf.inverse_symmetry(code) if inverse else code))


def _table(o, syms):
    S = len(syms)
    return np.concatenate([np.repeat(o, S, 0), np.tile(np.asarray(syms, np.int32), len(o))[:, None]], 1).astype(np.int32)


def _restate(logits, table, win, h, w):
    """float64 restatement of the blend: sum over images of w * softmax mapped back through the inverse symmetry, over sum of w."""
    ncls, p = logits.shape[1], logits.shape[2]
    acc, ws = np.zeros((ncls, h, w)), np.zeros((h, w))
    win = np.asarray(win, dtype=np.float64)
    for l, (y, x, s) in zip(np.asarray(logits, dtype=np.float64), table):
        e = np.exp(l - l.max(0))
        acc[:, y:y + p, x:x + p] += win * _sym(e / e.sum(0), s, inverse=True)
        ws[y:y + p, x:x + p] += win
    return acc / ws


# ---------------------------------------------------------------- 1. symmetric gather
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(3, 150, 141, 40), (5, 96, 64, 32), (13, 70, 80, 64)])
@guarded
def test_gather_tiles_sym_matches_host(prec, shape):
    c, h, w, p = shape
    d1, d2 = _scene(c, h, w, 1)
    r = np.random.default_rng(5)
    n = 16
    o = np.stack([r.integers(0, h - p + 1, n), r.integers(0, w - p + 1, n)], 1).astype(np.int32)
    o[0], o[1] = (0, 0), (h - p, w - p)
    table = np.concatenate([o, (np.arange(n) % 8)[:, None]], 1).astype(np.int32)
    cp = 16
    dt, td = DT[prec]
    g1, g2 = guard.guard(torch.from_numpy(d1)), guard.guard(torch.from_numpy(d2))
    out = guard.full((2 * n, p, p, cp), 7.0, dtype=td)
    call('bdn_gather_tiles_sym', dt, ptr(g1), ptr(g2), ptr(guard.guard(torch.from_numpy(table))), ptr(out), n, c, h, w, p, cp, st())
    got = out.float().cpu()
    ref = np.stack([np.ascontiguousarray(_sym(d[:, y:y + p, x:x + p], s).transpose(1, 2, 0))
                    for d in (d1, d2) for y, x, s in table])
    assert torch.equal(got[..., :c], rnd(prec, torch.from_numpy(ref)))
    assert (got[..., c:] == 0).all()
    # symmetry 0 is bdn_gather_tiles
    t0 = table.copy()
    t0[:, 2] = 0
    a = guard.full_like(out, 3.0)
    b = guard.full_like(out, 5.0)
    call('bdn_gather_tiles_sym', dt, ptr(g1), ptr(g2), ptr(guard.guard(torch.from_numpy(t0))), ptr(a), n, c, h, w, p, cp, st())
    call('bdn_gather_tiles', dt, ptr(g1), ptr(g2), ptr(guard.guard(torch.from_numpy(np.ascontiguousarray(o)))), ptr(b), n, c, h, w, p, cp, st())
    assert torch.equal(a, b)


# ---------------------------------------------------------------- 2. blend kernels on synthetic logits
def _blend_kernels(logits, table, win, h, w, p, stride, S, batch):
    """fold + stitch per batch of `batch` images (in order, one stream), then finalize: what predict_scene_blended launches."""
    n, ncls = logits.shape[0], logits.shape[1]
    proba = guard.zeros(ncls, h, w)
    wsum = guard.zeros(h, w)
    mask = guard.empty(h, w, dtype=torch.uint8)
    fold = guard.empty(min(batch, n), ncls, p, p)
    for i in range(0, n, batch):
        nb = min(n, i + batch) - i
        call('bdn_blend_fold', ptr(logits[i:i + nb]), ptr(table[i:i + nb]), ptr(win), ptr(fold), nb, ncls, p, st())
        call('bdn_blend_stitch', ptr(fold), ptr(win), ptr(proba), ptr(wsum), i, nb, S, ncls, h, w, p, stride, st())
    call('bdn_blend_finalize', ptr(proba), ptr(wsum), ptr(mask), ncls, h, w, st())
    return proba, mask


def _custom_window(p):
    r = np.random.default_rng(11)
    return torch.from_numpy(r.uniform(0.05, 2.0, (p, p)).astype(np.float32))


@pytest.mark.parametrize('ncls', [2, 3])
@pytest.mark.parametrize('h,w,p,stride,window,syms', [
    (96, 64, 32, 32, 'flat', (0,)),
    (100, 90, 32, 16, 'gaussian', (0, 5, 6, 3)),
    (100, 90, 32, 12, 'custom', tuple(range(8))),
    (77, 70, 40, 25, 'gaussian', (6, 1, 4)),
])
@guarded
def test_blend_kernels_match_float64(ncls, h, w, p, stride, window, syms):
    o, _, _ = inf.blend_tile_origins(h, w, p, stride)
    table = _table(o, syms)
    n = len(table)
    r = np.random.default_rng(ncls * 100 + stride)
    logits = r.integers(-3, 4, (n, ncls, p, p)).astype(np.float32)          # exact ties
    big = r.uniform(0, 1, (n, 1, p, p)) < 0.2
    logits = np.where(big, r.uniform(-80, 80, (n, ncls, p, p)).astype(np.float32), logits)
    win = _custom_window(p) if window == 'custom' else inf.blend_window(p, window)
    lg, tb, wd = guard.guard(torch.from_numpy(logits)), guard.guard(torch.from_numpy(table)), guard.guard(win)
    proba, mask = _blend_kernels(lg, tb, wd, h, w, p, stride, len(syms), 64)
    ref = _restate(logits, table, win.numpy(), h, w)
    got = proba.double().cpu().numpy()
    assert np.abs(got - ref).max() <= 2e-6
    assert np.abs(got.sum(0) - 1).max() <= 1e-5
    top = np.sort(ref, 0)
    sure = top[-1] - top[-2] > 1e-5
    assert np.array_equal(mask.cpu().numpy()[sure], ref.argmax(0)[sure])
    assert torch.equal(mask, torch.max(proba, 0)[1].to(torch.uint8))
    p2, m2 = _blend_kernels(lg, tb, wd, h, w, p, stride, len(syms), 64)
    assert torch.equal(proba, p2) and torch.equal(mask, m2)
    for batch in (1, 5, 7, n):                               # any split of the same logits: the same bits
        p3, m3 = _blend_kernels(lg, tb, wd, h, w, p, stride, len(syms), batch)
        assert torch.equal(proba, p3) and torch.equal(mask, m3), batch


# ---------------------------------------------------------------- 3. model level
def _calibrated_model(c, prec, d1, d2, p, ncls=2):
    """Filled model whose running statistics have seen the scene (a few train-mode forwards on its tiles), so the
    eval-mode mask has both classes (restated from test_gpu_scene.py)."""
    model = filler.fill_module(BiDateNet(c, ncls, precision='fp32')).cuda().train()
    t1 = torch.from_numpy(np.ascontiguousarray(inf._get_patches(d1.transpose(1, 2, 0), p)[0].transpose(0, 3, 1, 2))).cuda()
    t2 = torch.from_numpy(np.ascontiguousarray(inf._get_patches(d2.transpose(1, 2, 0), p)[0].transpose(0, 3, 1, 2))).cuda()
    with torch.no_grad():
        for _ in range(25):
            model(t1, t2)
    model.precision = prec
    return model.eval()


def _host_scan(model, d1, d2, p, stride, syms, batch_size):
    """The scan restated on the host: windows cut and transformed with _apply_symmetry, model(b1, b2) in the scan's own batches."""
    _, h, w = d1.shape
    o, _, _ = inf.blend_tile_origins(h, w, p, stride)
    table = _table(o, syms)
    logits = []
    with torch.no_grad():
        for i in range(0, len(table), batch_size):
            t = table[i:i + batch_size]
            b1 = np.stack([np.ascontiguousarray(_sym(d1[:, y:y + p, x:x + p], s)) for y, x, s in t])
            b2 = np.stack([np.ascontiguousarray(_sym(d2[:, y:y + p, x:x + p], s)) for y, x, s in t])
            logits.append(model(torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda()).float().cpu().numpy())
    return np.concatenate(logits), table


@pytest.mark.parametrize('prec,ncls', [('fp32', 2), ('bf16', 2), ('fp32', 3), ('bf16', 3)])
def test_model_level_probabilities(prec, ncls):
    c, h, w, p = 3, 88, 75, 32
    d1, d2 = _scene(c, h, w, 3)
    model = _calibrated_model(c, prec, d1, d2, p, ncls)
    stride, syms, bs = 12, (0, 5, 6, 3, 7), 9
    proba, mask = inf.predict_scene_blended(model, torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda(), patch_size=p,
                                            stride=stride, window='gaussian', symmetries=syms, batch_size=bs)
    logits, table = _host_scan(model, d1, d2, p, stride, syms, bs)
    ref = _restate(logits, table, inf.blend_window(p, 'gaussian').numpy(), h, w)
    assert proba.shape == (ncls, h, w) and proba.dtype == torch.float32
    assert np.abs(proba.double().cpu().numpy() - ref).max() <= 1e-5
    assert len(np.unique(mask.cpu().numpy())) >= 2                  # the calibrated scene shows more than one class
    assert torch.equal(mask, torch.max(proba, 0)[1].to(torch.uint8))


# ---------------------------------------------------------------- 4. equivalence with predict_scene
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_stride_p_flat_matches_predict_scene(prec):
    c, h, w, p = 3, 96, 128, 32
    d1, d2 = _scene(c, h, w, 4)
    model = _calibrated_model(c, prec, d1, d2, p)
    g1, g2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    ref = inf.predict_scene(model, g1, g2, patch_size=p, batch_size=8)
    proba, mask = inf.predict_scene_blended(model, g1, g2, patch_size=p, stride=p, window='flat', symmetries=(0,), batch_size=8)
    differ = proba[0] != proba[1]
    assert differ.float().mean().item() > 0.9
    assert torch.equal(mask[differ], ref[differ])
    assert len(torch.unique(ref)) == 2


# ---------------------------------------------------------------- 5. arrangement invariance
def _run(model, s1, s2, **kw):
    args = dict(patch_size=64, stride=24, window='gaussian', symmetries='all', batch_size=32)
    args.update(kw)
    proba, mask = inf.predict_scene_blended(model, s1, s2, **args)
    torch.cuda.synchronize()
    return proba.clone(), mask.clone()


def test_arrangement_invariance():
    c, h, w = 13, 300, 260
    d1, d2 = _scene(c, h, w, 6)
    model = _calibrated_model(c, 'bf16', d1, d2, 64)
    g1, g2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    base = _run(model, g1, g2)
    variants = {
        'again': _run(model, g1, g2),
        'one lane': _run(model, g1, g2, two_streams=False),
        'two lanes': _run(model, g1, g2, two_streams=True),
        'pinned host': _run(model, torch.from_numpy(d1).pin_memory(), torch.from_numpy(d2).pin_memory(), band_rows=64),
        'pageable host': _run(model, torch.from_numpy(d1), torch.from_numpy(d2), band_rows=64),
    }
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        variants['side stream'] = _run(model, g1, g2)
    torch.cuda.current_stream().wait_stream(side)
    for name, (pr, m) in variants.items():
        assert torch.equal(pr, base[0]) and torch.equal(m, base[1]), name
    assert not any(k[4] == 1 for k in model.engine()._ws)           # the second lane's workspace is gone
    # batch splits: the fold / stitch sums are split-invariant; the forward itself decides the rest
    for prec in ('bf16', 'fp32'):
        model.precision = prec
        runs = {bs: _run(model, g1, g2, batch_size=bs) for bs in (6, 7, 64)}
        top = torch.sort(runs[64][0], 0)[0]
        for bs in (6, 7):
            if prec == 'fp32':
                assert (runs[bs][0] - runs[64][0]).abs().max().item() <= 1e-6, bs
            sure = top[-1] - top[-2] > 1e-3
            assert torch.equal(runs[bs][1][sure], runs[64][1][sure]), (prec, bs)


# ---------------------------------------------------------------- 6. size
def test_scene_2000():
    c, h, w, p = 13, 2000, 2000, 128
    g = torch.Generator(device='cuda').manual_seed(3)
    g1 = torch.randn(c, h, w, device='cuda', generator=g)
    g2 = g1 + 0.3 * torch.randn(c, h, w, device='cuda', generator=g)
    torch.manual_seed(0)
    model = BiDateNet(c, 2, precision='bf16').cuda().eval()
    proba, mask = inf.predict_scene_blended(model, g1, g2, patch_size=p, stride=64, symmetries='all', batch_size=128)
    assert torch.isfinite(proba).all() and (proba >= 0).all() and (proba <= 1).all()
    assert (proba.sum(0) - 1).abs().max().item() <= 1e-5
    assert torch.equal(mask, torch.max(proba, 0)[1].to(torch.uint8))
    for sl in (np.s_[:, -1, :], np.s_[:, :, -1], np.s_[:, -p:, -p:]):       # far-edge rows and columns are covered (not left at 0 / NaN)
        assert (proba[sl].sum(0) - 1).abs().max().item() <= 1e-5


# ---------------------------------------------------------------- 7. training loop
def test_train_loop_scene_stride(tmp_path, capsys):
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
    T.main(['--metadata', mpath, '--dataset_dir', root, '--log_dir', str(log), '--augmentation', 'false',
            '--scene_stride', '16', '--scene_tta', '8'])
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith('{')]
    scene = [x for x in lines if 'scene' in x]
    assert len(scene) == 1 and scene[0]['epoch'] == 0 and set(scene[0]['scene']) == {'cc'}
    mask = ing.read_png_gray(str(log / 'cc_epoch_0.png'))
    prob = ing.read_png_gray(str(log / 'cc_epoch_0_proba.png'))
    assert mask.shape == cities['cc'] and prob.shape == cities['cc'] and set(np.unique(mask)) <= {0, 255}
    label = (ing.read_png_gray(os.path.join(root, 'labels', 'cc', 'cm', 'cm.png')) > 0)
    m = mask == 255
    cnt = scene[0]['scene']['cc']
    assert (cnt['tp'], cnt['fp'], cnt['fn']) == (int((m & label).sum()), int((m & ~label).sum()), int((~m & label).sum()))
    assert 0 <= cnt['f1'] <= 1
    # the probability map and the mask agree: class 1 wins exactly where its probability is above one half, up to the PNG's rounding
    assert not (m & (prob < 127)).any() and not (~m & (prob > 128)).any()
