"""float64 restatement of fabric_amd.criterion.Criterion with a topk (bdn_criterion_topk, include/bidate_hip.h), built on
tests/ignore_ref.py: the definition the kernels are held to in tests/test_gpu_topk.py and tests/test_gpu_step_topk.py.

    ppm      round(f * 1e6)
    K        max(1, n_valid * ppm // 1e6), 0 without a valid pixel                                   (kept_count)
    terms    the focal term of every pixel, ignore_ref.masked_focal's expression per pixel; 0 at a label >= ncls and at an ignored pixel
    kept     the first K valid pixels of a stable descending sort of the terms (ties: the lower linear pixel index (b*H + y)*W + x first)
    Focal    sum of the kept terms, / K with size_average (0 when K = 0); the kept set is a constant for the gradient
    Overlap  ignore_ref.masked_overlap, over all valid pixels

select() is the kernel's selection rule on given float32 values in integer arithmetic: the monotone key of the bit pattern, ties by index."""
import numpy as np
import torch

from tests import ignore_ref as IR


def ppm_of(f):
    return int(round(float(f) * 1e6))


def kept_count(n_valid, ppm):
    """K in exact integers (Python's are unbounded; the kernel's 64-bit product n_valid * ppm < 2^31 * 1e6 < 2^51 cannot overflow)."""
    n_valid, ppm = int(n_valid), int(ppm)
    return max(1, n_valid * ppm // 1_000_000) if n_valid else 0


def keys(values_f32):
    """uint32 keys of float32 values: u ^ 0x80000000 with the sign bit clear, ~u otherwise -- ascending keys are ascending floats, -0 < +0,
    +inf above every finite value, every bit pattern (NaN included) has a place."""
    u = np.ascontiguousarray(np.asarray(values_f32, dtype=np.float32)).view(np.uint32).astype(np.uint64).reshape(-1)
    neg = (u >> np.uint64(31)) != 0
    return np.where(neg, u ^ np.uint64(0xFFFFFFFF), u ^ np.uint64(0x80000000)).astype(np.uint64)


def select(keys_f32, valid, K):
    """bool [n]: the kept set of the float32 terms `keys_f32` (any shape, read in linear order) among the pixels where `valid`: the first K
    of the order (key descending, linear index ascending).  Integer arithmetic only."""
    k = keys(keys_f32).astype(np.int64)
    v = np.asarray(valid, dtype=bool).reshape(-1)
    idx = np.nonzero(v)[0]
    assert 0 <= K <= idx.size
    order = idx[np.lexsort((idx, -k[idx]))]                 # primary: -key ascending = key descending; secondary: index ascending
    kept = np.zeros(v.size, dtype=bool)
    kept[order[:K]] = True
    return kept


def _flat(c, logits, labels):
    """(x [n, C] in pixel order, t [n], valid [n], has_class [n])."""
    lab = labels.reshape(labels.shape[0], *labels.shape[-2:]).long()
    v = IR.valid_mask(c, lab) if c.ignore_index is not None else torch.ones_like(lab, dtype=torch.bool)
    nc = logits.shape[1]
    lg = torch.where(v[:, None], logits, torch.zeros_like(logits))
    x = lg.reshape(lg.shape[0], nc, -1).transpose(1, 2).reshape(-1, nc)
    t, vv = lab.reshape(-1), v.reshape(-1)
    return x, t, vv, vv & (t < nc), lab, v, lg


def pixel_terms(c, logits, labels):
    """The per-pixel focal term on `logits`' graph, [n] in linear pixel order; 0 at ignored pixels and at labels >= ncls."""
    x, t, vv, has_class, _, _, _ = _flat(c, logits, labels)
    tc = torch.where(has_class, t, torch.zeros_like(t))[:, None]
    logpt = torch.log_softmax(x, dim=1).gather(1, tc).view(-1)
    pt = logpt.detach().exp()
    if c.class_alpha is not None:
        a = torch.tensor(list(c.class_alpha))               # float32, as the oracle builds it
        logpt = logpt * a.to(x.dtype).gather(0, tc.view(-1))
    return torch.where(has_class, -1 * (1 - pt) ** c.gamma * logpt, torch.zeros_like(logpt)), vv


def selection(c, logits, labels):
    """(kept bool [n], K, terms float64 [n], valid [n]) in float64: a stable descending sort of the valid pixels' terms."""
    terms, vv = pixel_terms(c, logits.detach().double(), labels)
    idx = torch.nonzero(vv).view(-1)
    K = kept_count(idx.numel(), c.topk_ppm)
    order = idx[torch.sort(terms[idx], descending=True, stable=True)[1]]
    kept = torch.zeros_like(vv)
    kept[order[:K]] = True
    return kept, K, terms.detach(), vv


def gap(c, logits, labels):
    """(K-th largest term, (K+1)-th largest term or None) in float64: how well separated the selection is."""
    _, K, terms, vv = selection(c, logits, labels)
    s = torch.sort(terms[vv], descending=True)[0]
    if K == 0:
        return None, None
    return float(s[K - 1]), (float(s[K]) if K < s.numel() else None)


def loss(c, logits, labels, kept=None):
    """(L, overlap, focal, K, kept) on `logits`' graph; the kept set is a constant (computed from the detached float64 terms unless given)."""
    if kept is None:
        kept, K, _, _ = selection(c, logits, labels)
    else:
        K = int(kept.sum())
    _, _, _, _, lab, v, lg = _flat(c, logits, labels)
    zero = logits.new_zeros(())
    ov = IR.masked_overlap(lg, lab, v, c.alpha, c.beta, c.eps, c.reduce) if c.w_overlap > 0 else zero
    terms, _ = pixel_terms(c, logits, labels)
    S = torch.where(kept, terms, torch.zeros_like(terms)).sum()
    fo = (S / K if K else zero) if c.size_average else S
    return c.w_overlap * ov + c.w_focal * fo, ov, fo, K, kept


def reference(c, logits, labels):
    """dict(loss, overlap, focal, threshold: floats; K; kept bool [n]; terms float64 [n]; dloss, doverlap, dfocal: float64 [B,C,H,W])."""
    lo = logits.detach().double().requires_grad_(True)
    kept, K, terms, vv = selection(c, lo, labels)
    total, ov, fo, _, _ = loss(c, lo, labels, kept)
    zeros = torch.zeros_like(lo)
    dov = torch.autograd.grad(ov, lo, retain_graph=True)[0] if c.w_overlap > 0 else zeros
    dfo = torch.autograd.grad(fo, lo, retain_graph=True)[0] if K else zeros
    dl = c.w_overlap * dov + c.w_focal * dfo
    thr = float(terms[kept].min()) if K else 0.0
    return dict(loss=float(total.detach()), overlap=float(ov.detach()), focal=float(fo.detach()), threshold=thr, K=K, kept=kept,
                terms=terms, valid=vv, dloss=dl, doverlap=dov, dfocal=dfo)


def counts(logits, labels, ignore_index, ppm):
    """{TP, FP, FN, correct, valid, K}."""
    c5 = IR.counts(logits, labels, -1 if ignore_index is None else ignore_index)
    return c5 + [kept_count(c5[4], ppm)]
