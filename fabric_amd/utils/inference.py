"""Full-scene sliding-window inference: the reference's utils/inference.py + train.py:182-205.

Two ways in:

* the reference's own API -- ``_get_patches`` / ``_get_bands`` (host numpy, same tile order and paste order,
  pinned by fixture G7) and ``predict_patches`` (the ``train.py:190-203`` batch loop over a host patch stack);
* ``predict_scene`` -- the MI355X layout of the same computation: both dates of the scene are uploaded ONCE as
  band planes (a 10 000 x 10 000 x 13 x 2 float32 scene is 10.4 GB of the 288 GB HBM), every batch of tiles is
  gathered on the device straight into the packed NHWC encoder input (``bdn_gather_tiles``), and the class
  index of every pixel is written straight into the scene mask (``bdn_argmax_stitch``).  No host patch stack,
  no per-batch host<->device copy, no host sync inside the loop.

Tiles are independent: several GPUs take disjoint slices of the tile list (``shard=(rank, world)``); the only
exchange is the optional final merge of the uint8 masks.

``predict_scene_blended`` goes beyond the reference: overlapping tiles at any stride (``blend_tile_origins``), every tile
optionally under several symmetries of the square (test-time augmentation), and a window-weighted average of the softmax
probabilities instead of the last tile's argmax -- class probabilities [ncls,H,W] and their argmax, the same bits for any batch
split and for one scan lane or two (``bdn_gather_tiles_sym``, ``bdn_blend_fold`` / ``_stitch`` / ``_finalize``).

``generate_patches`` (utils/inference.py:20-70) reads the band files through fabric_amd.utils.ingest; comet logging
(``log_full_image``) is outside this path.
"""
from os import path

import numpy as np
import torch

from .. import _lib



def get_path(path_list):
    """utils/inference.py:15-17."""
    return path.join(*[i.strip('/') for i in path_list])


def tile_origins(h, w, patch_dim):
    """(y0, x0) of every tile in the reference's order (utils/inference.py:156-184): hs*ws aligned tiles row by
    row, then hs tiles anchored on the right edge, then ws tiles anchored on the bottom edge, then the corner.
    Returns (int32 [n,2], hs, ws, lc, lr)."""
    p = patch_dim
    if h < p or w < p:
        raise ValueError(f'scene {h}x{w} is smaller than one {p}x{p} patch')
    hs, ws = h // p, w // p
    o = [(i * p, j * p) for i in range(hs) for j in range(ws)]
    o += [(i * p, w - p) for i in range(hs)]
    o += [(h - p, j * p) for j in range(ws)]
    o.append((h - p, w - p))
    return np.asarray(o, dtype=np.int32), hs, ws, hs, ws


def _get_patches(bands, patch_dim=64):
    """utils/inference.py:134-184: [H,W,C] scene -> (patches [n,p,p,C], hs, ws, lc, lr, H, W)."""
    h, w = bands.shape[:2]
    o, hs, ws, lc, lr = tile_origins(h, w, patch_dim)
    patches = np.stack([bands[y:y + patch_dim, x:x + patch_dim] for y, x in o])
    return patches, hs, ws, lc, lr, h, w


def _get_bands(patches, hs, ws, lc, lr, h, w, patch_size=64):
    """utils/inference.py:187-236: paste [n,p,p] prediction tiles back into an [h,w] float64 image; the edge
    tiles are pasted last (column, row, corner), overwriting the aligned tiles where they overlap."""
    o, hs2, ws2, _, _ = tile_origins(h, w, patch_size)
    if (hs2, ws2, hs2, ws2) != (hs, ws, lc, lr) or len(patches) != len(o):
        raise ValueError('tile counts do not belong to this scene size')
    img = np.zeros((h, w))
    for t, (y, x) in zip(patches, o):
        img[y:y + patch_size, x:x + patch_size] = t
    return img


def full_image_mask(out, hs, ws, lc, lr, h, w, patch_size):
    """The array part of log_full_image (utils/inference.py:72-104): list of per-batch predictions -> scene mask."""
    return _get_bands(np.vstack(out), hs, ws, lc, lr, h, w, patch_size=patch_size)


def generate_patches(opt, validation_city):
    """utils/inference.py:20-70: both dates of a city as patch stacks [n,C,p,p] + the reconstruction metadata.  Band files
    are decoded by fabric_amd.utils.ingest (own TIFF reader, device-side normalise + resize) instead of rasterio / cv2."""
    import glob
    from . import ingest
    city_dir = path.join(opt.dataset_dir, 'images', validation_city)      # (get_path would strip the root of an absolute dir)
    d1_bands = sorted(glob.glob(path.join(city_dir, 'imgs_1', '*')))
    template = ingest.read_tiff(d1_bands[2])                   # band 2 gives the 10 m grid (utils/inference.py:47)
    stack = ingest.city_loader([city_dir, template.shape[1], template.shape[0], opt])
    p1, hs, ws, lc, lr, h, w = _get_patches(stack[0].transpose(1, 2, 0), patch_dim=opt.patch_size)
    p2 = _get_patches(stack[1].transpose(1, 2, 0), patch_dim=opt.patch_size)[0]
    return p1.transpose(0, 3, 1, 2), p2.transpose(0, 3, 1, 2), hs, ws, lc, lr, h, w


def log_full_image(*_a, **_k):
    raise ImportError('fabric_amd: log_full_image (reference utils/inference.py:72-131) uploads figures through comet_ml and '
                      'cv2, which are outside this path; full_image_mask() returns the stitched array')


def _eval_params(model):
    if model.training:
        raise RuntimeError('full-scene inference runs on running BatchNorm statistics: call model.eval() first '
                           '(train.py:117)')
    return {k: v.detach() for k, v in model.state_dict(keep_vars=True).items()}


@torch.no_grad()
def predict_patches(model, patches1, patches2, batch_size, device='cuda'):
    """The loop of train.py:190-203 on host patch stacks [n,C,p,p]: returns the list `out` of per-batch int64
    numpy arrays [b,p,p] (= `torch.max(preds, 1)[1].cpu().numpy()`)."""
    P = _eval_params(model)
    eng = model.engine()
    out = []
    for i in range(0, patches1.shape[0], batch_size):
        b1 = torch.from_numpy(np.ascontiguousarray(patches1[i:i + batch_size])).to(device)
        b2 = torch.from_numpy(np.ascontiguousarray(patches2[i:i + batch_size])).to(device)
        cd, _ = eng.forward(b1, b2, P, training=False, class_map=True)       # uint8 [b,p,p] = torch.max(preds, 1)[1]
        out.append(cd.cpu().numpy().astype(np.int64))
    return out


@torch.no_grad()
def predict_scene(model, scene_d1, scene_d2, patch_size=128, batch_size=64, shard=None, merge=True, band_rows=None, two_streams=None):
    """Change mask of a whole scene.

    scene_d1, scene_d2: [C,H,W] float32 tensors (what the reference's city_loader returns per date,
    utils/dataloaders.py:86-101), resident on the model's device or in HOST memory.  Host scenes are streamed up in bands of
    `band_rows` rows (default 256) on the copy stream while the tiles of the bands that have arrived run (pin the tensors:
    pageable memory is staged through pinned buffers by host threads and is host-memcpy bound).
    Returns a uint8 [H,W] device tensor equal to ``_get_bands(argmax(model(tiles)))`` of the reference loop.
    shard=(rank, world): process only this rank's contiguous slice of the tile list; merge=True then combines
    the per-rank masks with one all-reduce(MAX) over the default process group (unwritten pixels are 0).
    batch_size: tiles per forward batch (256 is the fastest on MI355X, bench.py scene leg).  Every tensor a kernel addresses must
    stay below 4 GB (32-bit byte offsets); the widest one is the operand of a 64-channel full-resolution layer at 2 * batch_size
    images: 64 channels x 2 bytes in the bf16 setting (<= 1023 tiles of 128 x 128), 64 x 4 bytes in fp32 (<= 511) and the
    [hi | lo] split of the concatenated 128-channel decoder input, 256 x 2 bytes at batch_size images, in bf16x3 (<= 511)."""
    _check_widest(model.engine(), batch_size, patch_size)
    P = _eval_params(model)
    eng = model.engine()
    dev = next(model.parameters()).device
    s1, s2 = torch.as_tensor(scene_d1), torch.as_tensor(scene_d2)
    if s1.dim() != 3 or s1.shape != s2.shape:
        raise RuntimeError(f'expected two [C,H,W] scenes of one shape, got {tuple(s1.shape)} and {tuple(s2.shape)}')
    _, h, w = s1.shape
    o_np, _, _, _, _ = tile_origins(h, w, patch_size)
    n = len(o_np)
    lo, hi = 0, n
    if shard is not None:
        rank, world = shard
        per = -(-n // world)
        lo, hi = min(n, rank * per), min(n, (rank + 1) * per)
    feed = None
    if s1.is_cuda and s2.is_cuda:
        d1 = s1.to(device=dev, dtype=torch.float32).contiguous()
        d2 = s2.to(device=dev, dtype=torch.float32).contiguous()
    else:
        # scene in HOST memory (what the reference's city_loader returns): the planes go up in row bands on the copy stream while
        # the tiles of the bands that have arrived are already being predicted -- the upload (10.4 GB at 10 000^2 x 13 x 2 dates,
        # as long over PCIe as the whole forward takes) hides behind the compute instead of preceding it
        feed = _SceneFeeder(s1.cpu(), s2.cpu(), dev, band_rows or max(patch_size, 256))
        d1, d2 = feed.d1, feed.d2
    origins = torch.from_numpy(o_np).to(dev)
    mask = torch.zeros(h, w, dtype=torch.uint8, device=dev) if shard is not None \
        else torch.empty(h, w, dtype=torch.uint8, device=dev)
    cur, lanes, seen = _open_lanes(eng, P, dev, hi - lo, batch_size, patch_size, two_streams)
    _fork_lanes(cur, lanes, (d1, d2, mask, origins))
    try:
        for it, i in enumerate(range(lo, hi, batch_size)):
            j = min(hi, i + batch_size)
            o = origins[i:j]
            nb = o.shape[0]
            k = it % len(lanes)
            with torch.cuda.stream(lanes[k]):
                if feed is not None:
                    feed.need_rows(int(o_np[i:j, 0].max()) + patch_size, lanes[k])     # this lane waits for the last band these tiles read
                eng.forward_tiles(d1, d2, o, P, patch_size, reuse_eval_bn=nb in seen[k], slot=k, scene_mask=mask)
                seen[k].add(nb)
    finally:
        _join_lanes(eng, cur, lanes)
        if feed is not None:
            feed.close()          # also on an exception: the consumer stream joins every upload before the planes can be freed
    if shard is not None and merge and shard[1] > 1:
        import torch.distributed as dist
        dist.all_reduce(mask, op=dist.ReduceOp.MAX)
    return mask


# ------------------------------------------------------------------ blended scan: overlapping tiles, softmax blend, symmetry averaging
TTA_SYMMETRIES = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3), 8: tuple(range(8))}       # train.py --scene_tta


def symmetry_bits(code):
    """Symmetry code 4 t + 2 rr + rc -> the (t, rr, rc) of fabric_amd.utils.dataloaders._apply_symmetry (transpose if t, then reverse
    the rows if rr, then the columns if rc; bdn_sample_patches' encoding)."""
    return bool(code & 4), bool(code & 2), bool(code & 1)


def inverse_symmetry(code):
    """The code that undoes `code`: flips and the plain transpose are their own inverses; transpose-then-flip is undone by the other flip."""
    t, rr, rc = symmetry_bits(code)
    return 4 + 2 * rc + rr if t else code


def blend_tile_origins(h, w, p, stride):
    """Tile plan of the blended scan: ys = 0, s, 2s, ... while <= h - p, then h - p if the last one is not; xs alike.
    Returns (origins int32 [len(ys) * len(xs), 2] in row-major order (tile iy * len(xs) + ix at (ys[iy], xs[ix])), ys, xs).
    stride == p on multiples of p gives the reference's tile set (tile_origins)."""
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= p:
        raise ValueError(f'stride must be an integer in [1, {p}], got {stride!r}')
    if h < p or w < p:
        raise ValueError(f'scene {h}x{w} is smaller than one {p}x{p} patch')

    def axis(n):
        v = list(range(0, n - p + 1, stride))
        if v[-1] != n - p:
            v.append(n - p)
        return np.asarray(v, dtype=np.int64)
    ys, xs = axis(h), axis(w)
    origins = np.stack(np.meshgrid(ys, xs, indexing='ij'), -1).reshape(-1, 2).astype(np.int32)
    return origins, ys, xs


def blend_window(p, window='gaussian'):
    """float32 [p,p] CPU tensor of the blending weights.  'flat': ones; 'gaussian': g(y) g(x), g(t) = exp(-(t + 0.5 - p/2)^2 / (2 (p/8)^2)),
    evaluated in float64 and rounded once; a tensor: the caller's weights as they are (check_blend_args checks them)."""
    if isinstance(window, torch.Tensor):
        return window.detach().to('cpu', torch.float32).contiguous()
    if window == 'flat':
        return torch.ones(p, p, dtype=torch.float32)
    t = np.arange(p, dtype=np.float64)
    g = np.exp(-0.5 * ((t + 0.5 - p / 2) / (p / 8)) ** 2)
    return torch.from_numpy(np.outer(g, g).astype(np.float32))


def check_blend_args(h, w, patch_size, stride, window, symmetries, n_classes, batch_size=1):
    """Validate the arguments of predict_scene_blended without touching a device.  Returns (stride, symmetry codes as a tuple)."""
    p = patch_size
    if isinstance(p, bool) or int(p) != p or p < 1:
        raise ValueError(f'patch_size must be a positive integer, got {p!r}')
    if h < p or w < p:
        raise ValueError(f'scene {h}x{w} is smaller than one {p}x{p} patch')
    stride = p // 2 if stride is None else stride
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= p:
        raise ValueError(f'stride must be an integer in [1, {p}] (None: {p // 2}), got {stride!r}')
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f'batch_size must be a positive integer, got {batch_size!r}')
    syms = tuple(range(8)) if isinstance(symmetries, str) and symmetries == 'all' else symmetries
    if isinstance(syms, str) or not hasattr(syms, '__iter__'):
        raise ValueError(f"symmetries must be codes in 0..7 or 'all', got {symmetries!r}")
    syms = tuple(syms)
    if not syms or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c <= 7 for c in syms):
        raise ValueError(f'symmetries must be a non-empty sequence of codes in 0..7, got {symmetries!r}')
    if len(set(syms)) != len(syms):
        raise ValueError(f'symmetry codes must be distinct, got {syms}')
    if isinstance(window, torch.Tensor):
        if window.dtype != torch.float32 or tuple(window.shape) != (p, p):
            raise ValueError(f'a window tensor must be float32 [{p},{p}], got {window.dtype} {tuple(window.shape)}')
        if not bool(torch.isfinite(window).all()) or not bool((window > 0).all()):
            raise ValueError('window weights must be finite and strictly positive')
    elif not (isinstance(window, str) and window in ('flat', 'gaussian')):
        raise ValueError(f"window must be 'gaussian', 'flat' or a float32 [{p},{p}] tensor, got {window!r}")
    if n_classes == 1:
        raise ValueError('one class: its softmax is constant 1; the blended scan needs n_classes >= 2 (a sigmoid head is not supported)')
    if n_classes < 2:
        raise ValueError(f'n_classes must be >= 2, got {n_classes}')
    return int(stride), tuple(int(c) for c in syms)


@torch.no_grad()
def predict_scene_blended(model, scene_d1, scene_d2, patch_size=128, stride=None, window='gaussian', symmetries=(0,), batch_size=64,
                          band_rows=None, two_streams=None, threshold=None, pos_class=1, min_area=None, auto_threshold=None,
                          threshold_out=None, connectivity=8, hysteresis_low=None, close_radius2=None, fill_holes=None, open_radius2=None):
    """Class probabilities of a whole scene from overlapping tiles.

    Tiles of patch_size at `stride` (default patch_size // 2; blend_tile_origins), each under every code of `symmetries` (codes 0..7 of
    _apply_symmetry, or 'all').  Forward images are (tile, symmetry) pairs in tile-major order, the symmetries in the order given; a
    batch is batch_size consecutive images (the 4 GB bound of predict_scene applies to batch_size).  Every image's softmax is mapped back
    through the inverse symmetry and weighted by `window` ('gaussian', 'flat' or a strictly positive float32 [p,p] tensor in scene
    orientation).  Returns (proba float32 [n_classes,H,W] = sum w softmax / sum w over every image that covers a pixel, mask uint8 [H,W]
    = its argmax, first maximum winning), both on the model's device.  Bit-reproducible, and the same bits for any batch_size split of
    the same logits and for one lane or two.  scene_d1 / scene_d2, band_rows and two_streams as in predict_scene.
    threshold: None: the argmax mask (the launches and the bits of a call without the argument); a number in [0, 1]: mask =
    proba[pos_class] >= threshold instead (bdn_threshold_mask, one more launch; proba keeps its bits) -- e.g. the best-F1 threshold of a
    validation pass (fabric_amd.utils.metrics.ScoreCurve).  For two classes 0.5 and the argmax differ only at exact ties, proba[0] ==
    proba[1]: the argmax gives class 0 there (the first maximum), the threshold 0.5 class 1.
    min_area: None: the mask as it is (the launches and the bits of a call without the argument); an integer >= 1: the connected components
    (`connectivity` 4 or 8) of mask == 1 with fewer pixels are removed from the mask (fabric_amd.utils.objects.remove_small_objects, on the
    current stream behind the finalize / threshold launch, no host read; proba keeps its bits).
    hysteresis_low, close_radius2, fill_holes, open_radius2: None: off (all four None: the launches and the bits of a call without them).
    They clean the mask with fabric_amd.utils.morphology on the current stream, no host read, proba keeps its bits, in this order behind
    the finalize launch: hysteresis_low (needs threshold, and hysteresis_low <= threshold): the mask is hysteresis_mask(proba,
    hysteresis_low, threshold, pos_class, connectivity) instead of the plain threshold; close_radius2: binary_closing with that disc;
    fill_holes (True, or the largest hole area filled): fill_holes under `connectivity`; open_radius2: binary_opening; then min_area.
    auto_threshold: None: off (the launches and the bits of a call without it); 'otsu', 'kittler', 'rosin' or 'em': the threshold is
    selected on the device from the histogram of proba[pos_class] over [0, 1] in 1024 linear bins (fabric_amd.utils.thresholds) and the mask
    is proba[pos_class] >= that threshold (bdn_raster_mask in place of bdn_threshold_mask: the number never leaves the device; all zeros
    when the rule finds no split); three more launches, proba keeps its bits.  Refused together with threshold or hysteresis_low, which
    take their numbers by value.  threshold_out: a dict that receives the ThresholdTable under 'table'."""
    from .metrics import check_threshold
    eng = model.engine()
    threshold, pos_class = check_threshold(threshold, pos_class, eng.n_classes)
    check_auto_threshold_args(auto_threshold, threshold_out, threshold, hysteresis_low)
    cleanup = not (hysteresis_low is None and close_radius2 is None and fill_holes is None and open_radius2 is None)
    if cleanup:
        from . import morphology
        morphology.check_cleanup_args(threshold, hysteresis_low, close_radius2, fill_holes, open_radius2, connectivity)
    if min_area is not None:
        from .objects import check_cc_args, remove_small_objects
        check_cc_args(torch.empty(1, 1, dtype=torch.uint8, device='meta'), connectivity, min_area=min_area)
    s1, s2 = torch.as_tensor(scene_d1), torch.as_tensor(scene_d2)
    if s1.dim() != 3 or s1.shape != s2.shape:
        raise RuntimeError(f'expected two [C,H,W] scenes of one shape, got {tuple(s1.shape)} and {tuple(s2.shape)}')
    _, h, w = s1.shape
    p, ncls = patch_size, eng.n_classes
    stride, syms = check_blend_args(h, w, p, stride, window, symmetries, ncls, batch_size)
    _check_widest(eng, batch_size, p)
    P = _eval_params(model)
    dev = next(model.parameters()).device
    o_np, _, _ = blend_tile_origins(h, w, p, stride)
    S = len(syms)
    table_np = np.concatenate([np.repeat(o_np, S, axis=0), np.tile(np.asarray(syms, dtype=np.int32), len(o_np))[:, None]], 1).astype(np.int32)
    n = len(table_np)
    feed = None
    if s1.is_cuda and s2.is_cuda:
        d1 = s1.to(device=dev, dtype=torch.float32).contiguous()
        d2 = s2.to(device=dev, dtype=torch.float32).contiguous()
    else:
        feed = _SceneFeeder(s1.cpu(), s2.cpu(), dev, band_rows or max(p, 256))
        d1, d2 = feed.d1, feed.d2
    table = torch.from_numpy(table_np).to(dev)
    win = blend_window(p, window).to(dev)
    proba = torch.zeros(ncls, h, w, dtype=torch.float32, device=dev)        # sum of w softmax until bdn_blend_finalize divides in place
    wsum = torch.zeros(h, w, dtype=torch.float32, device=dev)
    mask = torch.empty(h, w, dtype=torch.uint8, device=dev)
    cur, lanes, seen = _open_lanes(eng, P, dev, n, batch_size, p, two_streams)
    folds = [torch.empty(min(batch_size, n), ncls, p, p, dtype=torch.float32, device=dev) for _ in lanes]   # per lane: the batch's weighted probabilities
    _fork_lanes(cur, lanes, (d1, d2, table, win, proba, wsum, *folds))
    # Each lane runs gather -> forward -> fold of its batch; the stitches, which add into the shared sums, are chained across the lanes by
    # events (batch i's stitch waits for batch i - 1's) while the other lane's next forward runs under them.
    prev = None
    try:
        for it, i in enumerate(range(0, n, batch_size)):
            j = min(n, i + batch_size)
            nb, k = j - i, it % len(lanes)
            with torch.cuda.stream(lanes[k]):
                if feed is not None:
                    feed.need_rows(int(table_np[i:j, 0].max()) + p, lanes[k])
                logits, _ = eng.forward_tiles(d1, d2, table[i:j], P, p, reuse_eval_bn=nb in seen[k], slot=k)
                seen[k].add(nb)
                st = _lib.stream_ptr()
                _lib.call('bdn_blend_fold', _lib.ptr(logits), _lib.ptr(table[i:j]), _lib.ptr(win), _lib.ptr(folds[k]), nb, ncls, p, st)
                if prev is not None:
                    lanes[k].wait_event(prev)
                _lib.call('bdn_blend_stitch', _lib.ptr(folds[k]), _lib.ptr(win), _lib.ptr(proba), _lib.ptr(wsum), i, nb, S, ncls, h, w, p, stride, st)
                if len(lanes) > 1:
                    prev = torch.cuda.Event()
                    prev.record(lanes[k])
    finally:
        _join_lanes(eng, cur, lanes)
        if feed is not None:
            feed.close()
    _lib.call('bdn_blend_finalize', _lib.ptr(proba), _lib.ptr(wsum), _lib.ptr(mask), ncls, h, w, _lib.stream_ptr())
    if hysteresis_low is not None:
        morphology.hysteresis_mask(proba, hysteresis_low, threshold, pos_class, connectivity, out=mask)
    elif threshold is not None:
        _lib.call('bdn_threshold_mask', _lib.ptr(proba), pos_class, threshold, _lib.ptr(mask), ncls, h * w, _lib.stream_ptr())
    elif auto_threshold is not None:
        from . import thresholds
        _, table = thresholds.auto_threshold(proba[pos_class], auto_threshold, 1024, 'linear', 0.0, 1.0, out=mask)
        if threshold_out is not None:
            threshold_out['table'] = table
    if cleanup:
        morphology.cleanup_mask(mask, close_radius2, fill_holes, open_radius2, connectivity)
    if min_area is not None:
        remove_small_objects(mask, min_area, connectivity, out=mask)
    return proba, mask


def check_auto_threshold_args(auto_threshold=None, threshold_out=None, threshold=None, hysteresis_low=None):
    """Validate the auto_threshold= / threshold_out= pair of predict_scene_blended without touching a device."""
    if threshold_out is not None and not isinstance(threshold_out, dict):
        raise ValueError(f'threshold_out must be None or a dict, got {type(threshold_out).__name__}')
    if auto_threshold is None:
        if threshold_out is not None:
            raise ValueError('threshold_out needs auto_threshold')
        return
    from .thresholds import check_method
    check_method(auto_threshold)
    if threshold is not None or hysteresis_low is not None:
        raise ValueError('auto_threshold selects the threshold on the device; threshold and hysteresis_low take theirs by value: give one or the other')


def _check_widest(eng, batch_size, patch_size):
    widest = max(2 * batch_size * 64 * eng.esize, batch_size * 2 * 128 * 2 if eng.x3 else 0)      # bytes per pixel position of the widest tensor
    if widest * patch_size * patch_size >= 1 << 32:
        raise ValueError(f'batch_size={batch_size} tiles of {patch_size} px make a 4 GB tensor in the {eng.precision} setting; use a smaller batch')


def _open_lanes(eng, P, dev, n, batch_size, patch_size, two_streams):
    """The scan lanes of n forward images in batches of batch_size: returns (caller's stream, lanes, per-lane set of batch sizes whose
    eval BatchNorm tables are already folded).
    Tile batches are independent: they alternate between the caller's stream and the library's second stream (idle outside training),
    each with its own workspace, so that one batch's HBM-bound stages (tile gather, pooling, upsampling, classifier, stitching) run
    under the other's convolutions (+1.5 %).  The second lane needs a second full workspace (several GB at 256 tiles): it is created
    under the CALLER's stream (its blocks belong to the caller's allocator pool) and dropped again on exit (_join_lanes), so a training
    workspace of the same process can take the memory over.  two_streams=None: only when the device has room for it; False: the
    single-stream loop."""
    from .. import streams as _streams
    cur = torch.cuda.current_stream(dev)
    want_two = n > batch_size and two_streams is not False
    if want_two:
        nb0 = min(batch_size, n)
        a0 = torch.cuda.memory_allocated(dev)
        eng.workspace(nb0, patch_size, patch_size, dev, 0)
        first_ws = max(torch.cuda.memory_allocated(dev) - a0, 0)           # 0 when slot 0 existed already: then size it from the tensors
        if first_ws == 0:
            w0 = eng.workspace(nb0, patch_size, patch_size, dev, 0)
            first_ws = sum(t.numel() * t.element_size() for d_ in (w0.z, w0.pool, w0.f, w0.U) for t in d_.values()) + w0.x0.numel() * w0.x0.element_size()
        free_dev = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if two_streams is None and free_dev < 1.5 * first_ws:
            want_two = False
    lanes = [cur, _streams.get('wgrad', dev)] if want_two else [cur]
    seen = [set() for _ in lanes]
    if len(lanes) > 1:
        # the filter images are packed once, on the caller's stream, before the fork.  The staleness check comes first: after an
        # optimizer step with no forward since, the images are old but still marked valid, and the repack would otherwise happen
        # inside lane 0's first batch, on lane 0's stream, while lane 1 (ordered only behind the fork) reads them
        eng._check_packed(P)
        eng._weights(eng.layers[0], P, False)
        if eng._use_eval_schedule():
            eng.eval_tables(P)                           # and so are the folded BatchNorm tables both lanes read
            seen = [{min(batch_size, n), n % batch_size or batch_size} for _ in lanes]
        for nb_ in {min(batch_size, n), n % batch_size or batch_size}:
            eng.workspace(nb_, patch_size, patch_size, dev, 1)             # second lane's buffers: allocated under the caller's stream
    return cur, lanes, seen


def _fork_lanes(cur, lanes, tensors):
    """The second lane starts behind everything the caller's stream has enqueued; the tensors both lanes use stay theirs until it is done."""
    if len(lanes) > 1:
        lanes[1].wait_stream(cur)
        for t in tensors:
            t.record_stream(lanes[1])


def _join_lanes(eng, cur, lanes):
    for ln in lanes[1:]:
        cur.wait_stream(ln)
    if len(lanes) > 1:
        eng.drop_workspaces(slot=1)                  # back to the caller's pool (ordered behind the join above)


class _SceneFeeder:
    """Uploads two [C,H,W] float32 host scenes into device planes band by band (rows [k R, (k+1) R) of every plane of both
    dates per band), date 1 on the process-wide copy stream and date 2 on a second one (two DMA engines keep PCIe busier beside
    the running forward than one: 0.209 -> 0.199 s for the 10 000^2 scene), one event per band and stream.  Pinned sources are DMA'd in place; pageable ones
    are first copied into two alternating pinned band buffers by a few host threads (slower: the host memcpy, not PCIe, is
    then the limit).  The reference copies every batch of host patches synchronously (train.py:194-197)."""

    def __init__(self, s1, s2, dev, band_rows):
        from concurrent.futures import ThreadPoolExecutor
        from .. import streams
        self.src = [s1.float().contiguous() if s1.dtype != torch.float32 or not s1.is_contiguous() else s1,
                    s2.float().contiguous() if s2.dtype != torch.float32 or not s2.is_contiguous() else s2]
        C, H, W = self.src[0].shape
        self.R, self.H = band_rows, H
        self.copy = streams.get('copy', dev)
        self.cur = torch.cuda.current_stream(dev)
        self.copy2 = streams.get('copy2', dev)            # one stream (= one DMA engine) per date: 49.8 -> 52.1 GB/s sustained beside the forward
        with torch.cuda.stream(self.copy):
            # allocated UNDER the copy stream (see input_pipeline.py: a block of the consumer stream's pool may still be in use
            # by kernels that stream has queued)
            self.d1 = torch.empty(C, H, W, dtype=torch.float32, device=dev)
            self.d2 = torch.empty(C, H, W, dtype=torch.float32, device=dev)
            alloc = torch.cuda.Event()
            alloc.record(self.copy)
        self.copy2.wait_event(alloc)          # d2 came from the copy stream's pool: whatever that stream still has queued on the block
        self.d2.record_stream(self.copy2)     # (a feeder that just closed) precedes copy2's writes, and the block is not re-used under them
        self.events, self.waited, self.issued = [], {}, 0
        self.nbands = -(-H // band_rows)
        self.pinned = all(t.is_pinned() for t in self.src)
        self.pool = None if self.pinned else ThreadPoolExecutor(max_workers=8)
        self.stage = None if self.pinned else [[torch.empty(C, min(band_rows, H), W, dtype=torch.float32, pin_memory=True)
                                                 for _ in range(2)] for _ in range(2)]
        self.stage_free = [None, None]                   # event after which a staging slot may be overwritten by the host
        self.d1.record_stream(self.cur)
        self.d2.record_stream(self.cur)
        self._issue(self.LOOKAHEAD)

    # pinned sources: one hipMemcpy2DAsync per band and date (bdn_upload_band) instead of one copy per plane (26 -> 2 copies per band).  Boxes come in two
    # kinds (same plain-copy rate, 57.6 GB/s): on one the per-plane form sustains 53 GB/s beside the forward and the 2-D form 52 (0.196 vs 0.200 s for
    # the 10 000^2 scene), on the other the per-plane form sustains 37.7 GB/s (0.276 s, 0.66 of max(compute, PCIe) -- the driver's box of rounds 5) and
    # the 2-D form 52.7 (0.197 s, 0.91).  False = the per-plane form (tools/bench_scene_hostfed.py, BAND2D=0)
    band_copy_2d = True
    LOOKAHEAD = 4        # bands enqueued beyond the one a batch waits for: the copy stream never runs dry, the host never runs far ahead

    def _issue(self, upto):
        """Enqueue the uploads of bands [issued, upto]."""
        C = self.src[0].shape[0]
        while self.issued <= min(upto, self.nbands - 1):
            k = self.issued
            r0, r1 = k * self.R, min(self.H, (k + 1) * self.R)
            if not self.pinned:
                slot = k % 2
                if self.stage_free[slot] is not None:
                    for e_ in self.stage_free[slot]:
                        e_.synchronize()
                jobs = [self.pool.submit(self.stage[d][slot][c, :r1 - r0].copy_, self.src[d][c, r0:r1]) for d in range(2) for c in range(C)]
                for j in jobs:
                    j.result()
            evs = []
            for d, (dst, cs) in enumerate(((self.d1, self.copy), (self.d2, self.copy2))):
                with torch.cuda.stream(cs):
                    if self.pinned and self.band_copy_2d:        # all planes' rows of the band in ONE 2-D copy (26 copies per band -> 2)
                        _lib.call('bdn_upload_band', dst.data_ptr(), self.src[d].data_ptr(), C, self.H, self.src[d].shape[2], r0, r1, cs.cuda_stream)
                    else:
                        for c in range(C):               # one contiguous [rows, W] block per plane
                            src = self.src[d][c, r0:r1] if self.pinned else self.stage[d][k % 2][c, :r1 - r0]
                            dst[c, r0:r1].copy_(src, non_blocking=True)
                    e_ = torch.cuda.Event()
                    e_.record(cs)
                    evs.append(e_)
            ev = evs
            self.events.append(ev)
            if not self.pinned:
                self.stage_free[k % 2] = ev
            self.issued += 1

    def need_rows(self, rows, stream=None):
        """Make the consumer stream (default: the one the feeder was created under) wait until scene rows [0, rows) have arrived, and keep
        the copy stream LOOKAHEAD bands ahead.  Every consumer stream keeps its own high-water mark."""
        k = min(self.nbands - 1, (min(rows, self.H) - 1) // self.R)
        self._issue(k + self.LOOKAHEAD)
        stream = stream or self.cur
        key = stream.cuda_stream
        if k > self.waited.get(key, -1):
            for e_ in self.events[k]:                    # bands are uploaded in order on each stream: band k implies 0..k
                stream.wait_event(e_)
            self.waited[key] = k

    def close(self):
        try:
            self.need_rows(self.H)
        finally:
            if self.pool is not None:
                self.pool.shutdown(wait=True)
                self.pool = None
