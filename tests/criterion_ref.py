"""float64 restatement of fabric_amd.criterion.Criterion: the weighted sum of the oracle's own loss functions (oracle/bidate_oracle.py:
tversky_loss / dice_loss / jaccard_loss / focal_loss), with autograd for the gradients.  The yardstick of tests/test_gpu_criterion.py and
tests/test_gpu_step_criterion.py; pinned by tests/test_criterion_cpu.py.

Labels >= ncls (the OSCD masks are {0, 255}): the reference fails on them (it indexes torch.eye(ncls) with the label), so the library's
rule (include/bidate_hip.h, "labels outside the classes") is restated here by overlap_void / focal_void, which equal the oracle's functions
on valid labels (tests/test_illcond_cpu.py): such a pixel has no true class -- its probabilities add to FP of every class, its focal term
is 0 while it still counts in the size_average denominator, it is never a correct prediction."""
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


def overlap_void(logits, true, alpha, beta, eps):
    """1 - mean TP / (TP + alpha FP + beta FN + eps) with a one-hot that is all zero for a label >= ncls; label rank as the oracle's
    functions ([B,H,W]: cells per (class, column); [B,1,H,W]: per class).  dice is (0.5, 0.5, eps / 2)-, jaccard (1, 1, eps)-Tversky."""
    nc = logits.shape[1]
    lab = true.squeeze(1) if true.dim() == 4 else true
    one_hot = (lab.long()[..., None] == torch.arange(nc)).permute(0, 3, 1, 2).to(logits.dtype)
    probas = torch.softmax(logits, dim=1)
    dims = (0,) + tuple(range(2, true.dim()))
    tp = torch.sum(probas * one_hot, dims)
    fp = torch.sum(probas * (1 - one_hot), dims)
    fn = torch.sum((1 - probas) * one_hot, dims)
    return 1 - (tp / (tp + alpha * fp + beta * fn + eps)).mean()


def focal_void(logits, true, gamma=0.0, alpha=None, size_average=True):
    """The oracle's focal_loss with the term of a pixel labelled >= ncls set to 0 (the class weights are never indexed with it); the mean
    still divides by the number of all pixels."""
    nc = logits.shape[1]
    x = logits.reshape(logits.shape[0], nc, -1).transpose(1, 2).reshape(-1, nc)
    t = true.reshape(-1).long()
    valid = t < nc
    tc = torch.where(valid, t, torch.zeros_like(t))[:, None]
    logpt = torch.log_softmax(x, dim=1).gather(1, tc).view(-1)
    pt = logpt.detach().exp()
    if alpha is not None:
        a = torch.tensor([alpha, 1 - alpha]) if isinstance(alpha, (float, int)) else torch.tensor(alpha)
        logpt = logpt * a.to(x.dtype).gather(0, tc.view(-1))
    loss = torch.where(valid, -1 * (1 - pt) ** gamma * logpt, torch.zeros_like(logpt))
    return loss.mean() if size_average else loss.sum()


def loss(c, logits, labels):
    """(L, overlap, focal) as tensors on `logits`' graph; labels [B,H,W] class indices (the criterion's `reduce` picks the label rank the
    reference would have been given); a term with weight 0 is not evaluated and reported as 0.  Labels >= ncls: see the module docstring."""
    labels = labels.reshape(labels.shape[0], *labels.shape[-2:]).long()
    zero = logits.new_zeros(())
    if bool((labels >= logits.shape[1]).any()):
        ov = overlap_void(logits, labels if c.reduce == 'columns' else labels[:, None], c.alpha, c.beta, c.eps) if c.w_overlap > 0 else zero
        fo = focal_void(logits, labels, c.gamma, list(c.class_alpha) if c.class_alpha is not None else None, c.size_average) \
            if c.w_focal > 0 else zero
        return c.w_overlap * ov + c.w_focal * fo, ov, fo
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
    pred = torch.max(logits, 1)[1]                         # the first maximum wins ties (train.py:199)
    return [int(((pred == 1) & (labels == 1)).sum()), int(((pred == 1) & (labels != 1)).sum()),
            int(((pred != 1) & (labels == 1)).sum()), int((pred == labels).sum())]
