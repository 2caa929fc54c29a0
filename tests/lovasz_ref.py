"""float64 restatement of the Lovasz-Softmax term (bdn_lovasz_softmax, include/bidate_hip.h; Criterion(w_lovasz=)): the definition the
kernels are held to in tests/test_gpu_lovasz.py and tests/test_gpu_step_lovasz.py, pinned by tests/test_lovasz_cpu.py.  Batch level
(Berman, Rahman Triki, Blaschko, CVPR 2018, per_image = False).

    valid     the n pixels whose label is not the ignore label; a valid label >= C is foreground of no class
    p         softmax(logits) per pixel
    err       per class c: fg = (label == c), G = sum fg, err = |fg - p_c|
    order     the valid pixels by err descending; equal errors: the lower linear pixel index (b*H + y)*W + x first
    g         at 0-based rank r with c_prev foreground pixels at ranks < r:  I = G - c_prev, U = G + r - c_prev,
              g = 1 / U (foreground), I / (U (U + 1)) otherwise, 1 when U = 0                                      (coefficients)
    L_c       sum_r err_r g_r;  term = the mean of L_c over the included classes: G > 0 ('present') or every class ('all');
              no included class or n = 0: term 0, gradient 0
    gradient  the order is a constant; m included classes: q_c = (fg ? -g : +g) / m (0 for a class that is not included),
              dlogit_j = p_j (q_j - sum_c q_c p_c); 0 at an ignored pixel

evaluate() takes the orders as given (the kernel's, rebuilt from its ranks) or forms them from the float64 errors; order_from_errors() is
the kernel's rule on given float32 errors in integer arithmetic: the monotone key of the bit pattern (tests/topk_ref.keys), ties by index."""
import numpy as np
import torch

from tests import topk_ref as TR


def coefficients(fg_sorted):
    """float64 [n]: the coefficients along an order whose foreground flags are `fg_sorted` (bool [n]), from integers."""
    fg = np.asarray(fg_sorted, dtype=bool).reshape(-1)
    n = fg.size
    G = int(fg.sum())
    r = np.arange(n, dtype=np.int64)
    c_prev = np.cumsum(fg, dtype=np.int64) - fg
    I, U = G - c_prev, G + r - c_prev
    Uf = np.maximum(U, 1).astype(np.float64)
    return np.where(fg, 1.0 / Uf, np.where(U == 0, 1.0, I.astype(np.float64) / (Uf * (Uf + 1.0))))


def order_from_errors(err_f32, valid):
    """int64 [n_valid]: the pixel indices in rank order for float32 errors (any shape, read in linear order): key descending under the
    key map, the lower index first among equal keys; only the pixels where `valid`.  Integer arithmetic only."""
    k = TR.keys(err_f32).astype(np.int64)
    idx = np.nonzero(np.asarray(valid, dtype=bool).reshape(-1))[0]
    return idx[np.lexsort((idx, -k[idx]))]


def ranks_of(order, n_pixels):
    """int64 [n_pixels]: the rank of every pixel of `order`, -1 elsewhere (the kernel's `ranks` output of one class)."""
    out = np.full(n_pixels, -1, dtype=np.int64)
    out[np.asarray(order)] = np.arange(len(order))
    return out


def flatten(logits, labels, ignore_index=None):
    """(x float64 [N, C] in linear pixel order, t int64 [N], valid bool [N])."""
    B, C = logits.shape[:2]
    x = logits.detach().double().reshape(B, C, -1).permute(0, 2, 1).reshape(-1, C)
    t = labels.reshape(-1).long()
    valid = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != ignore_index
    return x, t, valid


def errors(logits, labels, ignore_index=None):
    """(err float64 [C, N] -- 0 at ignored pixels --, fg bool [C, N], valid bool [N], p float64 [N, C]); the logits of an ignored pixel
    are not used."""
    x, t, valid = flatten(logits, labels, ignore_index)
    C = x.shape[1]
    p = torch.softmax(torch.where(valid[:, None], x, torch.zeros_like(x)), dim=1)
    fg = (t[None, :] == torch.arange(C)[:, None]) & valid[None, :]
    err = torch.where(valid[None, :], (fg.double() - p.t()).abs(), torch.zeros(1, dtype=torch.float64))
    return err, fg, valid, p


def evaluate(logits, labels, ignore_index=None, classes='present', orders=None):
    """dict(term, class_terms [C], included [C] bool, m, dlogits float64 [B,C,H,W], err [C,N], fg, valid, orders) in float64.  `orders`:
    per class the valid pixel indices in rank order (e.g. the kernel's), or None: formed here from the float64 errors by a stable
    descending sort."""
    assert classes in ('present', 'all')
    B, C, H, W = logits.shape
    err, fg, valid, p = errors(logits, labels, ignore_index)
    err_n, fg_n, valid_n = err.numpy(), fg.numpy(), valid.numpy()
    idx = np.nonzero(valid_n)[0]
    n = idx.size
    if orders is None:
        orders = [idx[np.argsort(-err_n[c, idx], kind='stable')] for c in range(C)]
    included = np.array([n > 0 and (classes == 'all' or bool(fg_n[c].any())) for c in range(C)])
    m = int(included.sum())
    L = np.zeros(C)
    q = np.zeros((C, B * H * W))
    for c in range(C):
        o = np.asarray(orders[c], dtype=np.int64)
        assert o.size == n and (np.sort(o) == idx).all(), 'an order must be a permutation of the valid pixels'
        g = coefficients(fg_n[c, o])
        L[c] = float(np.sum(err_n[c, o] * g))
        if included[c]:
            q[c, o] = np.where(fg_n[c, o], -g, g) / m
    term = float(L[included].sum() / m) if m else 0.0
    qt, pn = q.T, p.numpy()                                                  # [N, C]
    d = pn * (qt - (qt * pn).sum(1, keepdims=True))
    d[~valid_n] = 0.0
    dlogits = torch.from_numpy(d).reshape(B, H * W, C).permute(0, 2, 1).reshape(B, C, H, W).contiguous()
    return dict(term=term, class_terms=L, included=included, m=m, dlogits=dlogits, err=err, fg=fg, valid=valid, orders=orders)
