"""Generate tests/golden/*.npz by running the REFERENCE ITSELF in the build
container (TEST INFRASTRUCTURE; see oracle/__init__.py).

    python oracle/make_golden.py            # needs /root/reference (read-only)
    python oracle/make_golden.py losses     # only the loss fixtures (G5, G9)
    python oracle/make_golden.py pickle     # only the reference checkpoint fixture (G10)

The reference's Python never travels to the GPU box; only the outputs written
here do.  Parameters are not stored: both sides regenerate them from
oracle/filler.py.  The script also cross-checks oracle/bidate_oracle.py against
the reference on every case and aborts if they disagree, so a committed fixture
implies "oracle == reference" at generation time.
"""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('BIDATE_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden')


def _stub_modules():
    """The reference's utils import rasterio/cv2/comet/polyaxon at module top
    (utils/dataloaders.py:5-6, utils/helpers.py:2-3); none is needed by the
    functions exercised here."""
    for name in ('rasterio', 'cv2', 'comet_ml', 'polyaxon_client', 'polyaxon_client.tracking',
                 'polystores', 'polystores.stores', 'polystores.stores.manager'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['polyaxon_client.tracking'].get_data_paths = lambda: {}
    sys.modules['polyaxon_client.tracking'].Experiment = object
    sys.modules['polystores.stores.manager'].StoreManager = object
    sys.modules['comet_ml'].Experiment = object
    import matplotlib
    matplotlib.use('Agg')
    from sklearn.feature_extraction import image
    if not hasattr(image, 'extract_patches'):          # public name removed upstream
        image.extract_patches = image._extract_patches


def _import_reference():
    # keep our own repo's `models` / `utils` shims out of the way
    sys.path = [p for p in sys.path if os.path.abspath(p or '.') != ROOT]
    for m in [m for m in sys.modules if m == 'models' or m.startswith('models.')
              or m == 'utils' or m.startswith('utils.')]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    _stub_modules()
    from models.bidate_model import BiDateNet
    from utils import metrics as ref_metrics
    from utils import dataloaders as ref_dl
    from utils import inference as ref_inf
    return BiDateNet, ref_metrics, ref_dl, ref_inf


def _grad_summary(grads):
    """Per-parameter L2 norm + 64 strided samples."""
    out = {}
    for k, g in grads.items():
        flat = g.reshape(-1).double()
        idx = np.unique(np.linspace(0, flat.numel() - 1, 64).astype(np.int64))
        out['gnorm/' + k] = np.float64(flat.norm().item())
        out['gsamp/' + k] = flat[idx].numpy().astype(np.float32)
        out['gidx/' + k] = idx
    return out


def _train_case(BiDateNet, ref_metrics, oracle, filler, name, c, b, s, different_dates=False, sw=None):
    torch.manual_seed(0)
    x1, x2, lbl = filler.make_inputs(b, c, s, seed=0, different_dates=different_dates, size_w=sw)
    x1, x2, lbl_t = torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(lbl)
    model = filler.fill_module(BiDateNet(c, 2))
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    crit = ref_metrics.TverskyLoss(alpha=0.1, beta=0.9)         # metadata.json:42-44
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)          # train.py:55
    model.train()
    opt.zero_grad()
    logits = model(x1, x2)                                      # train.py:91
    loss = crit(logits, lbl_t.long())                           # train.py:85,92
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    bufs = {k: v.detach().clone() for k, v in model.state_dict().items() if 'running_' in k or 'num_batches' in k}
    opt.step()
    logits2 = model(x1, x2).detach()                            # train mode again, updated weights
    # ---- oracle cross-check
    o = oracle.train_step(sd0, x1, x2, lbl_t, lr=1e-3, alpha=0.1, beta=0.9)
    assert torch.allclose(o['logits'], logits.detach(), atol=2e-5, rtol=1e-5), name
    assert abs(float(o['loss']) - float(loss)) < 1e-6, name
    worst = 0.0
    for k in grads:
        # float32 weight gradients are only reproducible to ~1e-2 of their scale between two
        # float32 implementations (both sit ~3e-3 from the float64 result; DESIGN.md "tolerances")
        rel = float((o['grads'][k] - grads[k]).norm() / (grads[k].norm() + 1e-12))
        if float(grads[k].norm()) >= 1e-6:
            worst = max(worst, rel)
        assert rel < 2e-2 or float(grads[k].norm()) < 1e-6, (name, k, rel)
    for k in bufs:
        assert torch.allclose(o['new_sd'][k].float(), bufs[k].float(), atol=1e-5), (name, k)
    o2, _ = oracle.bidate_forward(o['new_sd'], x1, x2, training=True)
    assert torch.allclose(o2.detach(), logits2, atol=5e-5, rtol=1e-5), name
    # ---- eval-mode logits on the freshly-filled weights (G3)
    m2 = filler.fill_module(BiDateNet(c, 2)).eval()
    with torch.no_grad():
        ev = m2(x1, x2)
    oe, _ = oracle.bidate_forward(sd0, x1, x2, training=False)
    assert torch.allclose(oe, ev, atol=2e-6 * float(ev.abs().max()) + 2e-5, rtol=1e-5), name
    preds = torch.max(logits, 1)[1]
    from sklearn.metrics import precision_recall_fscore_support as prfs
    rep = prfs(lbl.flatten(), preds.numpy().flatten(), average='binary', pos_label=1, zero_division=0)
    out = dict(logits=logits.detach().numpy(), loss=np.float64(loss.item()),
               logits_after_step=logits2.numpy(), eval_logits=ev.numpy(),
               prf=np.array(rep[:3], dtype=np.float64),
               meta=np.array([c, b, s, s if sw is None else sw, int(different_dates)]))
    for k, v in bufs.items():
        out['buf/' + k] = v.numpy()
    out.update(_grad_summary(grads))
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **out)
    print(f'{name}: loss={loss.item():.6f} logits std={logits.std().item():.4f} '
          f'|oracle-ref|max={float((o["logits"] - logits.detach()).abs().max()):.2e} worst grad relL2={worst:.2e}')


def _loss_case(ref_metrics, oracle):
    r = np.random.default_rng(5)
    logits = torch.from_numpy(r.standard_normal((3, 2, 24, 20)).astype(np.float32))
    lbl3 = torch.from_numpy((r.uniform(0, 1, (3, 24, 20)) < 0.3).astype(np.int64))
    lbl4 = lbl3[:, None]
    out = dict(logits=logits.numpy(), labels=lbl3.numpy().astype(np.uint8))
    for rank, lbl in (('r3', lbl3), ('r4', lbl4)):
        tv = ref_metrics.TverskyLoss(alpha=0.1, beta=0.9)(logits, lbl)
        tv5 = ref_metrics.TverskyLoss()(logits, lbl)
        dc = ref_metrics.dice_loss(logits, lbl)
        jc = ref_metrics.jaccard_loss(logits, lbl)
        assert abs(float(oracle.tversky_loss(logits, lbl, 0.1, 0.9)) - float(tv)) < 1e-6
        assert abs(float(oracle.tversky_loss(logits, lbl, 0.5, 0.5)) - float(tv5)) < 1e-6
        assert abs(float(oracle.dice_loss(logits, lbl)) - float(dc)) < 1e-6
        assert abs(float(oracle.jaccard_loss(logits, lbl)) - float(jc)) < 1e-6
        out[f'tversky_0.1_0.9_{rank}'] = np.float64(tv.item())
        out[f'tversky_0.5_0.5_{rank}'] = np.float64(tv5.item())
        out[f'dice_{rank}'] = np.float64(dc.item())
        out[f'jaccard_{rank}'] = np.float64(jc.item())
    # gradient of the train.py form wrt logits
    lg = logits.clone().requires_grad_(True)
    ref_metrics.TverskyLoss(alpha=0.1, beta=0.9)(lg, lbl3).backward()
    out['dlogits_tversky_r3'] = lg.grad.numpy()
    np.savez_compressed(os.path.join(OUT, 'g5_losses.npz'), **out)
    print('g5_losses:', {k: float(v) for k, v in out.items() if np.ndim(v) == 0})


def _loader_case(ref_dl, ref_inf, oracle):
    r = np.random.default_rng(7)
    data = {'cityA': {'images': r.standard_normal((2, 3, 40, 36)).astype(np.float32),
                      'labels': (r.uniform(0, 1, (40, 36)) < 0.2).astype(np.uint8)},
            'cityB': {'images': r.standard_normal((2, 3, 30, 50)).astype(np.float32),
                      'labels': (r.uniform(0, 1, (30, 50)) < 0.2).astype(np.uint8)}}
    meta = [['cityA', 0, 0], ['cityA', 16, 8], ['cityB', 4, 30], ['cityB', 10, 0], ['cityA', 20, 20]]
    random.seed(1234)
    ds = ref_dl.OneraPreloader('unused/', [list(m) for m in meta], data, 12, aug=True)
    out = {'order': np.array([[m[1], m[2], 0 if m[0] == 'cityA' else 1] for m in ds.imgs])}
    for i in range(len(ds)):
        a, b, l = ds[i]
        out[f'img1_{i}'], out[f'img2_{i}'], out[f'lbl_{i}'] = a, b, l
    np.savez_compressed(os.path.join(OUT, 'g7_loader.npz'), **out)
    # tiling on a 300x260x13 array with p=128 -> hs,ws,lc,lr = 2,2,2,2 ; 9 tiles
    bands = r.standard_normal((300, 260, 13)).astype(np.float32)
    tiles, hs, ws, lc, lr, h, w = ref_inf._get_patches(bands, patch_dim=128)
    assert (hs, ws, lc, lr, tiles.shape[0]) == (2, 2, 2, 2, 9)
    ot = oracle.tile_scene(bands, 128)
    assert np.array_equal(ot[0], tiles) and ot[1:] == (hs, ws, lc, lr, h, w)
    pred = r.integers(0, 2, (tiles.shape[0], 128, 128)).astype(np.float64)
    img = ref_inf._get_bands(pred, hs, ws, lc, lr, h, w, patch_size=128)
    assert np.array_equal(oracle.stitch_scene(pred, hs, ws, lc, lr, h, w, 128), img)
    np.savez_compressed(os.path.join(OUT, 'g7_tiling.npz'), meta=np.array([hs, ws, lc, lr, h, w]),
                        tile_checksums=tiles.reshape(9, -1).astype(np.float64).sum(1),
                        pred=pred.astype(np.uint8), stitched=img.astype(np.uint8))
    print('g7 loader/tiling ok')


def _loss_case_more(ref_metrics, oracle):
    """G9: focal loss (all constructor forms) and the gradients of dice / jaccard / tversky in both label ranks,
    on 2-class and 5-class logits."""
    import warnings
    warnings.filterwarnings('ignore')            # the reference calls F.log_softmax without dim
    r = np.random.default_rng(9)
    out = {}
    for tag, nc, shape in (('c2', 2, (3, 24, 20)), ('c5', 5, (2, 16, 12))):
        logits = torch.from_numpy((2.0 * r.standard_normal((shape[0], nc) + shape[1:])).astype(np.float32))
        lbl3 = torch.from_numpy(r.integers(0, nc, shape).astype(np.int64))
        out[f'{tag}/logits'], out[f'{tag}/labels'] = logits.numpy(), lbl3.numpy().astype(np.uint8)
        forms = [('g0', dict(gamma=0)), ('g2', dict(gamma=2)), ('g1.5_sum', dict(gamma=1.5, size_average=False))]
        if nc == 2:
            forms += [('g2_a0.25', dict(gamma=2, alpha=0.25))]
        else:
            forms += [('g2_alist', dict(gamma=2, alpha=[0.1, 0.2, 0.3, 0.15, 0.25]))]
        for name, kw in forms:
            lg = logits.clone().requires_grad_(True)
            v = ref_metrics.FocalLoss(**kw)(lg, lbl3)
            v.backward()
            lo = logits.clone().requires_grad_(True)
            vo = oracle.focal_loss(lo, lbl3, **kw)
            vo.backward()
            assert abs(float(vo) - float(v)) < 1e-5 * max(1.0, abs(float(v))), (name, float(vo), float(v))
            assert float((lo.grad - lg.grad).abs().max()) < 1e-6 * max(1.0, float(lg.grad.abs().max()))
            out[f'{tag}/focal_{name}'] = np.float64(v.item())
            out[f'{tag}/dfocal_{name}'] = lg.grad.numpy()
        for rank, lbl in (('r3', lbl3), ('r4', lbl3[:, None])):
            for name, fn, ofn in (('dice', ref_metrics.dice_loss, oracle.dice_loss),
                                  ('jaccard', ref_metrics.jaccard_loss, oracle.jaccard_loss),
                                  ('tversky_0.3_0.7', ref_metrics.TverskyLoss(alpha=0.3, beta=0.7),
                                   lambda a, b: oracle.tversky_loss(a, b, 0.3, 0.7))):
                lg = logits.clone().requires_grad_(True)
                v = fn(lg, lbl)
                v.backward()
                lo = logits.clone().requires_grad_(True)
                vo = ofn(lo, lbl)
                vo.backward()
                assert abs(float(vo) - float(v)) < 1e-6, (name, rank)
                assert float((lo.grad - lg.grad).abs().max()) < 1e-7
                out[f'{tag}/{name}_{rank}'] = np.float64(v.item())
                out[f'{tag}/d{name}_{rank}'] = lg.grad.numpy()
    np.savez_compressed(os.path.join(OUT, 'g9_losses_more.npz'), **out)
    print('g9_losses_more:', {k: round(float(v), 6) for k, v in out.items() if np.ndim(v) == 0})


def _pickle_case(BiDateNet):
    """G10: the reference's own whole-module checkpoint -- torch.save of nn.DataParallel(BiDateNet(3, 2)) as train.py:222 writes it,
    wrapped as utils/helpers.py:333-335 does -- and the state dict of the same wrapper, gzip-compressed.  Every parameter holds a ramp
    of period 251 offset by its position in parameters() instead of random values: the 54 MB of tensors compress to a few kB, and a
    key or layout mix-up on loading still changes what a test compares."""
    import gzip
    import io
    torch.manual_seed(3)
    m = torch.nn.DataParallel(BiDateNet(3, 2)).cpu()
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(((torch.arange(p.numel()) % 251).float() / 251.0 + i).reshape(p.shape))
    for name, obj in (('g10_reference_module_pickle.pt.gz', m), ('g10_reference_state_dict.pt.gz', m.state_dict())):
        buf = io.BytesIO()
        torch.save(obj, buf)
        with gzip.GzipFile(os.path.join(OUT, name), 'wb', compresslevel=9, mtime=0) as f:
            f.write(buf.getvalue())


def main():
    sys.path.insert(0, ROOT)
    from oracle import bidate_oracle as oracle
    from oracle import filler
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    BiDateNet, ref_metrics, ref_dl, ref_inf = _import_reference()
    if len(sys.argv) > 1 and sys.argv[1] == 'losses':        # regenerate only the loss fixtures
        _loss_case(ref_metrics, oracle)
        _loss_case_more(ref_metrics, oracle)
        return
    if len(sys.argv) > 1 and sys.argv[1] == 'pickle':        # regenerate only the checkpoint fixture
        _pickle_case(BiDateNet)
        return
    _train_case(BiDateNet, ref_metrics, oracle, filler, 'g1_c3_b4_s32', 3, 4, 32)
    _train_case(BiDateNet, ref_metrics, oracle, filler, 'g2_c13_b2_s128', 13, 2, 128)
    _train_case(BiDateNet, ref_metrics, oracle, filler, 'g4_c13_b2_s90', 13, 2, 90)
    _train_case(BiDateNet, ref_metrics, oracle, filler, 'g6_c3_b4_s32_diffdates', 3, 4, 32, different_dates=True)
    _train_case(BiDateNet, ref_metrics, oracle, filler, 'g8_c13_b3_h40_w72', 13, 3, 40, sw=72)
    _loss_case(ref_metrics, oracle)
    _loss_case_more(ref_metrics, oracle)
    _loader_case(ref_dl, ref_inf, oracle)
    _pickle_case(BiDateNet)


if __name__ == '__main__':
    main()
