"""float64 restatement of fabric_amd.criterion.Criterion on soft targets (bdn_criterion_soft, include/bidate_hip.h): the definition the
kernels are held to in tests/test_gpu_soft.py and tests/test_gpu_soft_step.py; pinned by tests/test_soft_cpu.py to tests/ignore_ref.py
(one-hot targets, 0 / 1 weights) and to torch.nn.functional.cross_entropy (label_smoothing=, probability targets).

Every pixel has a target q_c >= 0 per class and a weight w >= 0; v = [w > 0]; p = softmax(logits).

    hard labels t, smoothing e     lo = e / ncls, hi = (1 - e) + lo, float32 operations of one rounding each; q_c = hi if t == c else lo;
                                   q = 0 for a valid label >= ncls; w = 0 where t == ignore_index
    float targets [B, ncls, H, W]  q as given
    weights [B, H, W]              multiply into w (w = 1 at every pixel that is not ignored without them)

    Overlap  TP_c = sum w p_c q_c, FP_c = sum w p_c (1 - q_c), FN_c = sum w (1 - p_c) q_c over the cells of c.reduce;
             1 - mean TP / (TP + alpha FP + beta FN + eps)
    Focal    f = sum_c [q_c > 0] q_c a_c m_c (-log p_c), m_c = max(1 - p_c, 0)^gamma detached (1 at gamma 0);
             scale * sum w f, scale = 1 / #[w > 0] with size_average (1 with no valid pixel), else 1

The logits (and float targets) of a pixel with v = 0 are replaced by 0 before anything is computed from them (a select, not a product):
inf / NaN there cannot reach the loss and autograd gives exactly 0 there."""
import numpy as np
import torch


def smoothed_pair(e, ncls):
    """(hi, lo) as float32 scalars, formed with the library's float32 operations."""
    e = np.float32(e)
    lo = e / np.float32(ncls)
    hi = (np.float32(1.0) - e) + lo
    return np.float32(hi), np.float32(lo)


def targets_and_weights(c, ncls, labels, weights=None, smoothing=None):
    """-> (q float64 [B,C,H,W], w float64 [B,H,W], cls int64 [B,H,W]) of uint8 / integer class-index labels or float [B,C,H,W] targets.
    cls is the pixel's class for the counts: the label, or the first maximum of q."""
    e = float(getattr(c, 'label_smoothing', 0.0) if smoothing is None else smoothing)
    if labels.is_floating_point():
        assert e == 0.0 and labels.dim() == 4 and labels.shape[1] == ncls
        q = labels.double()
        w = torch.ones(q.shape[0], *q.shape[-2:], dtype=torch.float64)
        cls = None
    else:
        lab = labels.reshape(labels.shape[0], *labels.shape[-2:]).long()
        hi, lo = smoothed_pair(e, ncls)
        one_hot = (lab[..., None] == torch.arange(ncls)).permute(0, 3, 1, 2)
        q = torch.where(one_hot, torch.tensor(float(hi), dtype=torch.float64), torch.tensor(float(lo), dtype=torch.float64))
        q = torch.where((lab < ncls)[:, None], q, torch.zeros_like(q))
        w = (lab != (-1 if c.ignore_index is None else c.ignore_index)).double()
        cls = lab
    if weights is not None:
        w = w * weights.reshape(w.shape).double()
    if cls is None:
        qs = torch.where((w > 0)[:, None], q, torch.zeros_like(q))
        cls = torch.max(qs, 1)[1]                           # the first maximum wins ties
    return q, w, cls


def loss(c, logits, labels, weights=None, smoothing=None):
    """(L, overlap, focal) as tensors on `logits`' graph; a term with weight 0 is not evaluated and reported as 0."""
    nc = logits.shape[1]
    q, w, _ = targets_and_weights(c, nc, labels, weights, smoothing)
    v = w > 0
    w = torch.where(v, w, torch.zeros_like(w))              # (a NaN weight is not > 0)
    lg = torch.where(v[:, None], logits, torch.zeros_like(logits))
    q = torch.where(v[:, None], q, torch.zeros_like(q)).to(logits.dtype)
    wf = w[:, None].to(logits.dtype)
    zero = logits.new_zeros(())
    ov = fo = zero
    if c.w_overlap > 0:
        p = torch.softmax(lg, dim=1)
        dims = (0, 2) if c.reduce == 'columns' else (0, 2, 3)
        tp = torch.sum(wf * p * q, dims)
        fp = torch.sum(wf * p * (1 - q), dims)
        fn = torch.sum(wf * (1 - p) * q, dims)
        ov = 1 - (tp / (tp + c.alpha * fp + c.beta * fn + c.eps)).mean()
    if c.w_focal > 0:
        logp = torch.log_softmax(lg, dim=1)
        m = torch.clamp(1 - logp.detach().exp(), min=0) ** c.gamma if c.gamma != 0 else torch.ones_like(logp)
        a = torch.ones(nc, dtype=logits.dtype) if c.class_alpha is None else torch.tensor(c.class_alpha[:nc], dtype=torch.float32).to(logits.dtype)
        per_class = torch.where(q > 0, q * a.view(1, nc, 1, 1) * m * (-logp), torch.zeros_like(logp))
        total = (wf * per_class).sum()
        n = int(v.sum())
        fo = total / n if c.size_average and n else total
    return c.w_overlap * ov + c.w_focal * fo, ov, fo


def reference(c, logits, labels, weights=None, smoothing=None):
    """dict(loss, overlap, focal: floats; dloss, doverlap, dfocal: float64 [B,C,H,W]) of float64 (or float32, promoted) CPU logits."""
    lo = logits.detach().double().requires_grad_(True)
    total, ov, fo = loss(c, lo, labels, weights, smoothing)
    zeros = torch.zeros_like(lo)
    dov = torch.autograd.grad(ov, lo, retain_graph=True)[0] if c.w_overlap > 0 else zeros
    dfo = torch.autograd.grad(fo, lo, retain_graph=True)[0] if c.w_focal > 0 else zeros
    (dl,) = torch.autograd.grad(total, lo)
    return dict(loss=float(total.detach()), overlap=float(ov.detach()), focal=float(fo.detach()), dloss=dl, doverlap=dov, dfocal=dfo)


def valid(c, ncls, labels, weights=None):
    """bool [B,H,W]: the pixels with w > 0."""
    return targets_and_weights(c, ncls, labels, weights, 0.0)[1] > 0


def counts(c, logits, labels, weights=None):
    """{TP, FP, FN, correct, valid} of argmax(logits, 1) against the pixel's class over the valid pixels, class 1 positive."""
    _, w, cls = targets_and_weights(c, logits.shape[1], labels, weights, 0.0)
    v = w > 0
    lg = torch.where(v[:, None], logits, torch.zeros_like(logits))
    pred = torch.max(lg, 1)[1]                              # the first maximum wins ties
    return [int(((pred == 1) & (cls == 1) & v).sum()), int(((pred == 1) & (cls != 1) & v).sum()),
            int(((pred != 1) & (cls == 1) & v).sum()), int(((pred == cls) & v).sum()), int(v.sum())]
