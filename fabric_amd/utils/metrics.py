"""Losses and batch metrics: drop-in for the reference's utils/metrics.py.

TverskyLoss (the default criterion, metadata.json:42-44) is a fused HIP kernel
(softmax + the reference's TP/FP/FN sums + loss + d loss / d logits + argmax
TP/FP/FN counts for F1) behind ``bdn_overlap_loss``; dice_loss and jaccard_loss
are the same kernel with other coefficients, FocalLoss is ``bdn_focal``;
CompoundLoss is a weighted focal + overlap sum as one criterion (``bdn_criterion``,
fabric_amd/criterion.py).  Both
label ranks of the reference are supported ([B,H,W] -> dims (0,2), [B,1,H,W] ->
dims (0,2,3)).  The sigmoid single-class branch (utils/metrics.py:65-72,
100-107, 149-157) is never reached by BiDateNet(13, 2) and is not built.
"""
import torch
import torch.nn as nn

from .. import _lib


def _check_labels(logits, labels):
    """-> (uint8 labels, reduce_w).  [B,H,W] labels make the reference reduce over dims (0,2) only; [B,1,H,W]
    labels over (0,2,3) (utils/metrics.py:80,115,164) -- two different loss values, both supported."""
    B, C, H, W = logits.shape
    lb = labels.detach()
    if lb.dim() == 4 and lb.shape == (B, 1, H, W):
        reduce_w = 1
    elif lb.shape == (B, H, W):
        reduce_w = 0
    else:
        raise RuntimeError(f'labels must be [B,H,W] or [B,1,H,W] for logits {tuple(logits.shape)}, got {tuple(lb.shape)}')
    return lb.to(torch.uint8).contiguous(), reduce_w


class _OverlapFunction(torch.autograd.Function):
    """TP / (TP + alpha FP + beta FN + eps) family: Tversky, Dice (0.5, 0.5, eps/2), Jaccard (1, 1, eps)."""

    @staticmethod
    def forward(ctx, logits, labels, alpha, beta, eps, holder):
        if not logits.is_cuda:
            raise RuntimeError('fabric_amd: the losses run only on a ROCm device -- there is no CPU path')
        B, C, H, W = logits.shape
        lg = logits.detach().contiguous().float()
        lb, reduce_w = _check_labels(logits, labels)
        ws = torch.empty(_lib.load().bdn_overlap_workspace_bytes(B, C, H, W, reduce_w) // 4, dtype=torch.float32, device=lg.device)
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        counts = torch.empty(4, dtype=torch.int32, device=lg.device)
        dl = torch.empty_like(lg)
        _lib.call('bdn_overlap_loss', lg.data_ptr(), lb.data_ptr(), float(alpha), float(beta), float(eps), reduce_w,
                  ws.data_ptr(), loss.data_ptr(), counts.data_ptr(), dl.data_ptr(), B, C, H, W, _lib.stream_ptr())
        ctx.save_for_backward(dl)
        if holder is not None:
            holder['counts'] = counts
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None, None, None


_TverskyFunction = _OverlapFunction


def dice_loss(logits, true, eps=1e-7):
    """reference utils/metrics.py:51-83: 1 - mean(2I / (sum(p) + sum(t) + eps)) = Tversky(0.5, 0.5, eps/2)."""
    return _OverlapFunction.apply(logits, true, 0.5, 0.5, 0.5 * eps, None)


def jaccard_loss(logits, true, eps=1e-7):
    """reference utils/metrics.py:86-119: 1 - mean(I / (sum(p) + sum(t) - I + eps)) = Tversky(1, 1, eps)."""
    return _OverlapFunction.apply(logits, true, 1.0, 1.0, eps, None)


class _FocalFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, gamma, alpha, size_average, holder):
        if not logits.is_cuda:
            raise RuntimeError('fabric_amd: the losses run only on a ROCm device -- there is no CPU path')
        if logits.dim() != 4:
            raise RuntimeError('fabric_amd: FocalLoss is built for [B,C,H,W] logits (train.py:91)')
        B, C, H, W = logits.shape
        lg = logits.detach().contiguous().float()
        if target.numel() != B * H * W:
            raise RuntimeError(f'target must hold B*H*W={B * H * W} class indices, got {tuple(target.shape)}')
        lb = target.detach().reshape(B, H, W).to(torch.uint8).contiguous()
        ws = torch.empty(_lib.load().bdn_focal_workspace_bytes(), dtype=torch.uint8, device=lg.device)
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        counts = torch.empty(4, dtype=torch.int32, device=lg.device)
        dl = torch.empty_like(lg)
        a = alpha.to(device=lg.device, dtype=torch.float32).contiguous() if alpha is not None else None
        if a is not None and a.numel() < C:
            raise RuntimeError(f'alpha holds {a.numel()} class weights for {C} classes')
        _lib.call('bdn_focal', lg.data_ptr(), lb.data_ptr(), float(gamma), a.data_ptr() if a is not None else None,
                  1 if size_average else 0, ws.data_ptr(), loss.data_ptr(), counts.data_ptr(), dl.data_ptr(),
                  B, C, H, W, _lib.stream_ptr())
        ctx.save_for_backward(dl)
        holder['counts'] = counts
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None, None, None


class FocalLoss(nn.Module):
    """reference utils/metrics.py:8-48 (same constructor; the modulating factor is detached like there)."""

    def __init__(self, gamma=0, alpha=None, size_average=True):
        super(FocalLoss, self).__init__()
        self.gamma = gamma
        self.alpha = alpha
        if isinstance(alpha, (float, int)):
            self.alpha = torch.Tensor([alpha, 1 - alpha])
        if isinstance(alpha, list):
            self.alpha = torch.Tensor(alpha)
        self.size_average = size_average
        self._holder = {}

    def forward(self, input, target):
        return _FocalFunction.apply(input, target, self.gamma, self.alpha, self.size_average, self._holder)

    @property
    def last_counts(self):
        return self._holder.get('counts')


class TverskyLoss(nn.Module):
    """reference utils/metrics.py:122-171"""

    def __init__(self, alpha=0.5, beta=0.5, eps=1e-7, size_average=True):
        super(TverskyLoss, self).__init__()
        self.alpha = alpha
        self.beta = beta
        self.size_average = size_average
        self.eps = eps
        self._holder = {}

    def forward(self, logits, true):
        return _TverskyFunction.apply(logits, true, self.alpha, self.beta, self.eps, self._holder)

    @property
    def last_counts(self):
        """int32[4] device tensor {TP, FP, FN, correct} of argmax(logits) vs labels for the last call."""
        return self._holder.get('counts')


class _CriterionFunction(torch.autograd.Function):
    """fabric_amd.criterion.Criterion.evaluate as one autograd node; without a gradient to compute no gradient pass is launched."""

    @staticmethod
    def forward(ctx, logits, labels, criterion, holder, weights=None):
        want = ctx.needs_input_grad[0]
        kw = {} if weights is None else {'weights': weights.detach()}
        loss, terms, counts, dl = criterion.evaluate(logits.detach().contiguous().float(), labels.detach(), want_grad=want, **kw)
        if want:
            ctx.save_for_backward(dl)
        holder['counts'], holder['terms'] = counts, terms
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None, None


class CompoundLoss(nn.Module):
    """w_overlap * (dice | jaccard | Tversky) + w_focal * FocalLoss as one criterion (fabric_amd.criterion.Criterion, bdn_criterion):
    the module form for validation and the autograd route.  The criterion's `reduce` decides the overlap reduction, not the label
    rank.  A criterion with a topk (bdn_criterion_topk) runs here as any other: the selection is a constant for the gradient; so does one
    with a w_lovasz (bdn_lovasz_softmax): the order is a constant for the gradient; and one with a w_boundary (bdn_boundary_loss): the
    signed distance is a constant for the gradient, last_terms[-1] the unweighted boundary value.  Soft targets (bdn_criterion_soft) come
    in as they do in Criterion.evaluate: a criterion with label_smoothing, `weights` (float32 [B,H,W]) beside the labels, or float32
    [B,C,H,W] targets as `true`; targets and weights are constants for the gradient, last_counts is int32[5] on that route."""

    def __init__(self, criterion):
        super(CompoundLoss, self).__init__()
        self.criterion = criterion
        self._holder = {}

    def forward(self, logits, true, weights=None):
        return _CriterionFunction.apply(logits, true, self.criterion, self._holder, weights)

    @property
    def last_counts(self):
        """int32[4] device tensor {TP, FP, FN, correct} of argmax(logits) vs labels for the last call; int32[5] = {.., valid}, over the
        valid pixels, when the criterion has an ignore_index; int32[6] = {.., valid, K} when it has a topk (K the kept pixels)."""
        return self._holder.get('counts')

    @property
    def last_terms(self):
        """f32[2] device tensor: the unweighted overlap and focal values of the last call; f32[3] = {.., the K-th largest focal term} when
        the criterion has a topk."""
        return self._holder.get('terms')


def confusion_counts(logits, labels, ignore_index=None):
    """int32[4] device tensor {TP, FP, FN, correct} of argmax(logits, 1) vs labels (what train.py:96-106 hands to sklearn),
    for criteria that do not report it themselves: one pass of the overlap-loss kernel, loss and gradient discarded.
    ignore_index: a label byte 0..255 -> int32[5] = {TP, FP, FN, correct, valid} over the pixels whose label is not ignore_index
    (the statistics and finish passes of bdn_criterion_masked).  Hard labels only: the counts of soft targets (argmax_c q_c as the pixel's
    class, the pixels with weight > 0) are the `counts` of Criterion.evaluate on that route."""
    if ignore_index is not None:
        from ..criterion import Criterion
        lg = logits.detach().contiguous().float()
        return Criterion(ignore_index=ignore_index).evaluate(lg, labels.detach(), want_grad=False)[2]
    holder = {}
    with torch.no_grad():
        _OverlapFunction.apply(logits.detach(), labels, 0.5, 0.5, 1e-7, holder)
    return holder['counts']


def batch_prf_from_counts(counts):
    """sklearn precision_recall_fscore_support(average='binary', pos_label=1) as called at reference
    train.py:103-106, from on-device counts; zero division -> 0 like sklearn's default."""
    tp, fp, fn = [int(v) for v in counts[:3].tolist()]
    p = tp / (tp + fp) if tp + fp else 0.0
    r = tp / (tp + fn) if tp + fn else 0.0
    f = 2 * p * r / (p + r) if p + r else 0.0
    return p, r, f


def check_threshold(threshold, pos_class=1, n_classes=2):
    """Validate the threshold= / pos_class= pair of predict_scene_blended and ScoreCurve.at without touching a device: threshold None
    (the argmax) or a real number in [0, 1], pos_class an integer class index.  Returns (None or float, int)."""
    if isinstance(pos_class, bool) or not isinstance(pos_class, int) or not 0 <= pos_class < n_classes:
        raise ValueError(f'pos_class must be an integer in 0..{n_classes - 1}, got {pos_class!r}')
    if threshold is None:
        return None, pos_class
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= float(threshold) <= 1.0:       # NaN fails the comparison
        raise ValueError(f'threshold must be None (the argmax) or a number in [0, 1], got {threshold!r}')
    return float(threshold), pos_class


class ScoreCurve:
    """Threshold-free validation of one class against the rest: a fixed-bin histogram of the score s = softmax(logits)[pos_class] of every
    valid pixel, split by label, accumulated on the device over any number of batches (bdn_score_hist: integers, so exact, order-independent
    and bit-reproducible), and turned by one launch (bdn_score_curve) into the precision / recall curve over the thresholds t_i = i / n_bins
    (predict positive iff s >= t_i), the best-F1 threshold and the average precision -- sklearn's average_precision_score on the
    bin-quantised scores.  Replaces the argmax-only precision_recall_fscore_support of the reference (train.py:96-106, 151-158).

    n_bins: a power of two in 2..4096.  ignore_index: a label byte 0..255 left out of every count (None: no label is).  A pixel is
    positive iff its label equals pos_class; every other valid label is negative.  Everything runs on the current stream; nothing waits
    for the device except compute() and at(), which read one small buffer back.  CPU tensors raise: there is no CPU path."""

    def __init__(self, n_bins=1024, pos_class=1, ignore_index=None):
        if isinstance(n_bins, bool) or not isinstance(n_bins, int) or not 2 <= n_bins <= 4096 or n_bins & (n_bins - 1):
            raise ValueError(f'n_bins must be a power of two in 2..4096, got {n_bins!r}')
        if isinstance(pos_class, bool) or not isinstance(pos_class, int) or not 0 <= pos_class <= 255:
            raise ValueError(f'pos_class must be a class index 0..255, got {pos_class!r}')
        if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 0 <= ignore_index <= 255):
            raise ValueError(f'ignore_index must be None or a label byte 0..255, got {ignore_index!r}')
        self.n_bins, self.pos_class, self.ignore_index = n_bins, pos_class, ignore_index
        self._hist = None                                  # made on first use, on the device of the first batch

    @property
    def hist(self):
        """The int64 [2, n_bins] device tensor of the counts, negatives first."""
        return self._hist_on(self._hist.device if self._hist is not None else torch.device('cuda', torch.cuda.current_device()))

    def _hist_on(self, device):
        if self._hist is None:
            self._hist = torch.zeros(2, self.n_bins, dtype=torch.int64, device=device)
        elif self._hist.device != device:
            raise RuntimeError(f'ScoreCurve: the histogram lives on {self._hist.device}, got tensors on {device}')
        return self._hist

    def _add(self, x, labels, is_logits, scores_out):
        if not x.is_cuda:
            raise RuntimeError('fabric_amd: ScoreCurve runs only on a ROCm device -- there is no CPU path')
        B, C, H, W = x.shape
        if not self.pos_class < C:
            raise RuntimeError(f'pos_class {self.pos_class} is not a class of {C}-class scores')
        xs = x.detach().contiguous().float()
        lb, _ = _check_labels(xs, labels.to(xs.device))
        if scores_out is not None:
            if not (scores_out.is_cuda and scores_out.dtype == torch.float32 and scores_out.is_contiguous() and scores_out.numel() == B * H * W):
                raise RuntimeError(f'scores_out must be a contiguous float32 device tensor of {B * H * W} elements')
        _lib.call('bdn_score_hist', xs.data_ptr(), 1 if is_logits else 0, lb.data_ptr(), -1 if self.ignore_index is None else self.ignore_index,
                  self.pos_class, B, C, H * W, self.n_bins, self._hist_on(xs.device).data_ptr(), _lib.ptr(scores_out), _lib.stream_ptr())

    def update(self, logits, labels, scores_out=None):
        """Add a batch: logits [B,ncls,H,W], labels [B,H,W] or [B,1,H,W] of any integer dtype.  scores_out: a float32 [B,H,W] device tensor
        that receives every pixel's score (0 at an ignored pixel)."""
        if logits.dim() != 4:
            raise RuntimeError(f'logits must be [B,ncls,H,W], got {tuple(logits.shape)}')
        self._add(logits, labels, True, scores_out)

    def update_proba(self, proba, labels, scores_out=None):
        """Add probabilities as they are: proba [ncls,H,W] (a scene of predict_scene_blended; labels [H,W]) or [B,ncls,H,W]."""
        if proba.dim() == 3:
            proba, labels = proba[None], labels[None]
        if proba.dim() != 4:
            raise RuntimeError(f'proba must be [ncls,H,W] or [B,ncls,H,W], got {tuple(proba.shape)}')
        self._add(proba, labels, False, scores_out)

    def reset(self):
        if self._hist is not None:
            self._hist.zero_()

    def merge(self, other):
        """Add another instance's histogram (same bins, class and ignore label)."""
        if (other.n_bins, other.pos_class, other.ignore_index) != (self.n_bins, self.pos_class, self.ignore_index):
            raise ValueError('ScoreCurve.merge: the two curves differ in n_bins, pos_class or ignore_index')
        if other._hist is not None:
            self._hist_on(other._hist.device).add_(other._hist)

    def all_reduce(self, group=None):
        """One SUM of the int64 histogram over the process group: exact whatever the world size."""
        import torch.distributed as dist
        dist.all_reduce(self.hist, op=dist.ReduceOp.SUM, group=group)

    def _curve(self, want_curve):
        dev = self.hist.device
        summary = torch.empty(8, dtype=torch.float64, device=dev)
        curve = torch.empty(4, self.n_bins, dtype=torch.float64, device=dev) if want_curve else None
        _lib.call('bdn_score_curve', self.hist.data_ptr(), self.n_bins, _lib.ptr(curve), summary.data_ptr(), _lib.stream_ptr())
        return summary, curve

    def compute(self):
        """One bdn_score_curve and one host read: best_f1, best_threshold (= best_bin / n_bins, the first maximum of F1 in ascending
        threshold), best_bin, precision and recall at it, ap, n_pos, n_neg -- Python floats and ints."""
        s = self._curve(False)[0].tolist()
        return {'best_f1': s[0], 'best_threshold': s[1], 'best_bin': int(s[2]), 'precision': s[3], 'recall': s[4], 'ap': s[5],
                'n_pos': int(s[6]), 'n_neg': int(s[7])}

    def curve(self):
        """(TP, FP, precision, recall): four float64 [n_bins] device tensors over the thresholds i / n_bins."""
        c = self._curve(True)[1]
        return c[0], c[1], c[2], c[3]

    def at(self, threshold):
        """Counts and scores at an arbitrary threshold, rounded down to a bin edge: {tp, fp, fn, precision, recall, f1}."""
        t, _ = check_threshold(threshold)
        if t is None:
            raise ValueError('ScoreCurve.at needs a threshold in [0, 1]')
        i = min(int(t * self.n_bins), self.n_bins - 1)
        tp, fp, _, _ = self.curve()
        tp0, tpi, fpi = [int(v) for v in torch.stack([tp[0], tp[i], fp[i]]).tolist()]
        fn = tp0 - tpi
        return {'tp': tpi, 'fp': fpi, 'fn': fn, 'precision': tpi / (tpi + fpi) if tpi + fpi else 0.0, 'recall': tpi / tp0 if tp0 else 0.0,
                'f1': 2 * tpi / (2 * tpi + fpi + fn) if 2 * tpi + fpi + fn else 0.0}
