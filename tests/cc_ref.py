"""Host restatement of the connected-component contract of include/bidate_hip.h (bdn_cc_label / _compact / _filter / _stats) and of
fabric_amd.utils.objects.object_scores, in numpy: a sequential union-find over the row runs of the raster (runs are numbered in the order
of their first pixel's linear index, the smaller root wins, so a set's root is the run that holds its smallest index), areas at the
roots, ranks of the roots, the statistics table, the area filter and the object scores.  Written from the contract, not from the
kernels; tests/test_cc_cpu.py pins it to scipy.ndimage.label, np.bincount, scipy.ndimage.find_objects and brute force."""
import numpy as np


def foreground(src, fg_value=1, exclude=None, exclude_value=None):
    """bool [H,W]: src == fg_value, and not excluded (exclude == exclude_value)."""
    fg = np.asarray(src) == fg_value
    if exclude is not None and exclude_value is not None:
        fg &= np.asarray(exclude) != exclude_value
    return fg


def label(fg, connectivity=8):
    """int32 [H,W]: 0 on background, 1 + (smallest linear index of the pixel's component) elsewhere."""
    if connectivity not in (4, 8):
        raise ValueError(connectivity)
    fg = np.asarray(fg, dtype=bool)
    H, W = fg.shape
    reach = 1 if connectivity == 8 else 0              # a run [s, e) touches a run [ps, pe) of the row above iff s < pe + reach and ps < e + reach
    parent, first, lens = [], [], []                   # per run: union-find parent, linear index of its first pixel, length

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    prev = ()
    for y in range(H):
        d = np.diff(np.concatenate(([0], fg[y].astype(np.int8), [0])))
        starts, ends = np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()
        cur = []
        k = 0
        for s, e in zip(starts, ends):
            rid = len(parent)
            parent.append(rid)
            first.append(y * W + s)
            lens.append(e - s)
            cur.append((s, e, rid))
            while k < len(prev) and prev[k][1] + reach <= s:          # runs above that end before this one begins
                k += 1
            j = k
            while j < len(prev) and prev[j][0] < e + reach:
                a, b = find(rid), find(prev[j][2])
                if a != b:
                    parent[max(a, b)] = min(a, b)
                j += 1
        prev = cur
    out = np.zeros(H * W, dtype=np.int32)
    if parent:
        roots = np.asarray([first[find(r)] + 1 for r in range(len(parent))], dtype=np.int32)
        # row runs in row-major order are the foreground pixels in raster order
        out[fg.ravel()] = np.repeat(roots, lens)
    return out.reshape(H, W)


def areas(labels):
    """int32 [H,W]: the component's pixel count at its root pixel, 0 elsewhere."""
    lab = np.asarray(labels)
    a = np.bincount(lab[lab > 0] - 1, minlength=lab.size)[:lab.size]
    return a.astype(np.int32).reshape(lab.shape)


def counts(labels):
    """(n_components, n_foreground)."""
    lab = np.asarray(labels)
    return int((lab.ravel() == np.arange(1, lab.size + 1)).sum()), int((lab > 0).sum())


def compact(labels):
    """int32 [H,W]: 0 on background, elsewhere the 1-based rank of the pixel's root among all roots in ascending index."""
    lab = np.asarray(labels)
    roots = np.unique(lab[lab > 0])
    out = np.zeros(lab.shape, dtype=np.int32)
    out[lab > 0] = np.searchsorted(roots, lab[lab > 0]) + 1
    return out


def stats_table(comp, n_max, other=None, other_value=1, other_exclude_value=-1):
    """int32 [n_max, 8] = {area, ymin, xmin, ymax, xmax, overlap, 0, 0} per compact label; {0, H, W, -1, -1, 0, 0, 0} for absent ones."""
    comp = np.asarray(comp)
    H, W = comp.shape
    t = np.zeros((n_max, 8), dtype=np.int32)
    t[:, 1], t[:, 2], t[:, 3], t[:, 4] = H, W, -1, -1
    ys, xs = np.nonzero(comp)
    k = comp[ys, xs].astype(np.int64)
    sel = k <= n_max
    if other is not None:
        sel &= np.asarray(other)[ys, xs] != other_exclude_value
    ys, xs, k = ys[sel], xs[sel], k[sel] - 1
    t[:, 0] = np.bincount(k, minlength=n_max)
    np.minimum.at(t[:, 1], k, ys)
    np.minimum.at(t[:, 2], k, xs)
    np.maximum.at(t[:, 3], k, ys)
    np.maximum.at(t[:, 4], k, xs)
    if other is not None:
        t[:, 5] = np.bincount(k[np.asarray(other)[ys, xs] == other_value], minlength=n_max)
    return t


def filter_mask(labels, area, min_area):
    """uint8 [H,W]: 1 iff labels != 0 and the component's area >= min_area."""
    lab = np.asarray(labels)
    a = np.asarray(area).ravel()
    out = np.zeros(lab.shape, dtype=np.uint8)
    fgm = lab > 0
    out[fgm] = a[lab[fgm] - 1] >= min_area
    return out


def remove_small(mask, min_area, connectivity=8, fg_value=1, exclude=None, exclude_value=None):
    lab = label(foreground(mask, fg_value, exclude, exclude_value), connectivity)
    return filter_mask(lab, areas(lab), min_area)


def prf(hit_pred, n_pred, hit_true, n_true):
    p = hit_pred / n_pred if n_pred else 0.0
    r = hit_true / n_true if n_true else 0.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


def object_scores(pred_mask, truth, pos_class=1, ignore_index=None, connectivity=8, min_area=1, min_overlap=1):
    """The dict of fabric_amd.utils.objects.object_scores."""
    pred_mask, truth = np.asarray(pred_mask), np.asarray(truth)
    kept = remove_small(pred_mask, min_area, connectivity, 1, truth, ignore_index)
    cp = compact(label(kept == 1, connectivity))
    ct = compact(label(truth == pos_class, connectivity))
    n_pred, n_true = int(cp.max(initial=0)), int(ct.max(initial=0))
    tp = stats_table(cp, max(n_pred, 1), truth, pos_class)[:n_pred]
    tt = stats_table(ct, max(n_true, 1), kept, 1)[:n_true]
    pred_hit, true_hit = int((tp[:, 5] >= min_overlap).sum()), int((tt[:, 5] >= min_overlap).sum())
    p, r, f = prf(pred_hit, n_pred, true_hit, n_true)
    return {'objects_pred': n_pred, 'objects_true': n_true, 'pred_hit': pred_hit, 'true_hit': true_hit,
            'object_precision': p, 'object_recall': r, 'object_f1': f}


# ---------------------------------------------------------------- the pattern set of the tests
def patterns(H, W, tile, seed=0):
    """name -> uint8 [H,W] (1 = foreground): the rasters the kernel tests run, at any size."""
    r = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {'background': np.zeros((H, W), np.uint8), 'foreground': np.ones((H, W), np.uint8)}
    for d in (0.1, 0.5, 0.593, 0.9):                   # 0.593: the 4-connected percolation threshold
        out[f'random {d}'] = (r.random((H, W)) < d).astype(np.uint8)
    out['checkerboard'] = ((yy + xx) & 1).astype(np.uint8)
    out['diagonals'] = ((yy % W == xx) | ((yy + 3) % W == W - 1 - xx)).astype(np.uint8)
    sp = np.zeros((H, W), np.uint8)                    # a one-pixel-wide rectangular spiral, one pixel apart
    t, b, l, rt = 0, H - 1, 0, W - 1
    while t <= b and l <= rt:
        sp[t, l:rt + 1] = 1
        sp[t:b + 1, rt] = 1
        if b - t >= 2:
            sp[b, l + 2:rt + 1] = 1
            if rt - l >= 2:
                sp[t + 2:b + 1, l + 2] = 1
        t, b, l, rt = t + 2, b - 2, l + 2, rt - 2
        if t <= b and l <= rt:
            sp[t, l] = 1
    out['spiral'] = sp
    out['serpentine'] = ((yy % 2 == 0) | np.where((yy // 2) % 2 == 0, xx == W - 1, xx == 0)).astype(np.uint8)
    out['rows'] = (yy % 2 == 0).astype(np.uint8)
    out['columns'] = (xx % 2 == 0).astype(np.uint8)
    back = np.zeros((H, W), np.uint8)                  # smallest index in the last (tile) column, reaching back to column 0 lower down
    back[0:min(2, H), W - 1] = 1
    back[min(2, H - 1), :] = 1
    out['reach back'] = back
    corner = np.zeros((H, W), np.uint8)                # two pixels touching only diagonally, exactly at a four-tile corner (or the centre)
    cy, cx = (tile, tile) if H > tile and W > tile else (max(H // 2, 1), max(W // 2, 1))
    if cy < H and cx < W:
        corner[cy - 1, cx] = 1
        corner[cy, cx - 1] = 1
    out['corner'] = corner
    return out
