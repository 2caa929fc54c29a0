"""float64 restatement of fabric_amd.criterion.Criterion: the weighted sum of the oracle's own loss functions (oracle/bidate_oracle.py:
tversky_loss / dice_loss / jaccard_loss / focal_loss), with autograd for the gradients.  The yardstick of tests/test_gpu_criterion.py and
tests/test_gpu_step_criterion.py; pinned by tests/test_criterion_cpu.py."""
import torch

from oracle import bidate_oracle as O


def overlap_fn(c):
    """The oracle function of the criterion's overlap term: dice_loss for (0.5, 0.5, eps / 2), jaccard_loss for (1, 1, eps) -- the forms
    the reference writes them in -- and tversky_loss otherwise (the three are one function of (alpha, beta, eps))."""
    if (c.alpha, c.beta) == (0.5, 0.5):
        return lambda lg, lb: O.dice_loss(lg, lb, 2.0 * c.eps)
    if (c.alpha, c.beta) == (1.0, 1.0):
        return lambda lg, lb: O.jaccard_loss(lg, lb, c.eps)
    return lambda lg, lb: O.tversky_loss(lg, lb, c.alpha, c.beta, c.eps)


def loss(c, logits, labels):
    """(L, overlap, focal) as tensors on `logits`' graph; labels [B,H,W] class indices (the criterion's `reduce` picks the label rank the
    reference would have been given); a term with weight 0 is not evaluated and reported as 0."""
    labels = labels.reshape(labels.shape[0], *labels.shape[-2:]).long()
    zero = logits.new_zeros(())
    ov = overlap_fn(c)(logits, labels if c.reduce == 'columns' else labels[:, None]) if c.w_overlap > 0 else zero
    fo = O.focal_loss(logits, labels, c.gamma, list(c.class_alpha) if c.class_alpha is not None else None, c.size_average) \
        if c.w_focal > 0 else zero
    return c.w_overlap * ov + c.w_focal * fo, ov, fo


def reference(c, logits, labels):
    """dict(loss, overlap, focal: floats; dloss, doverlap, dfocal: float64 [B,C,H,W]) of float64 (or float32, promoted) CPU logits."""
    lo = logits.detach().double().requires_grad_(True)
    total, ov, fo = loss(c, lo, labels)
    zeros = torch.zeros_like(lo)
    dov = torch.autograd.grad(ov, lo, retain_graph=True)[0] if c.w_overlap > 0 else zeros
    dfo = torch.autograd.grad(fo, lo, retain_graph=True)[0] if c.w_focal > 0 else zeros
    (dl,) = torch.autograd.grad(total, lo)
    return dict(loss=float(total.detach()), overlap=float(ov.detach()), focal=float(fo.detach()), dloss=dl, doverlap=dov, dfocal=dfo)


def counts(logits, labels):
    """{TP, FP, FN, correct} of argmax(logits, 1) against the labels, class 1 positive (train.py:96-106)."""
    labels = labels.reshape(labels.shape[0], *labels.shape[-2:])
    pred = logits.argmax(1)
    return [int(((pred == 1) & (labels == 1)).sum()), int(((pred == 1) & (labels != 1)).sum()),
            int(((pred != 1) & (labels == 1)).sum()), int((pred == labels).sum())]
