"""The criterion of a run as one object: L = w_overlap * Overlap(alpha, beta, eps, reduce) + w_focal * Focal(gamma, class_alpha,
size_average) behind ``bdn_criterion`` (include/bidate_hip.h; reference utils/helpers.py:303-312 over utils/metrics.py:8-171).

Overlap is the TP / (TP + alpha FP + beta FN + eps) family: Tversky as given, jaccard = (1, 1, eps), dice = (0.5, 0.5, eps / 2).
Focal is FocalLoss with the modulating factor a constant for the gradient.  The compound forms (focal + an overlap term, what change
detection trains with on imbalanced data) run as one three-launch kernel sequence.  Importable without a GPU; evaluate() needs one.

ignore_index (None or a label byte 0..255, torch's name for it): pixels with that label are left out of the loss -- ``bdn_criterion_masked``.
The overlap sums TP / FP / FN run over the other (valid) pixels only, the focal mean divides by the number of valid pixels, dlogits is
exactly 0 at an ignored pixel, the counts become {TP, FP, FN, correct, valid} over valid pixels, and the logits of an ignored pixel (inf
and NaN included) reach no output.  A valid label >= ncls keeps the library's "labels outside the classes" rule.  A batch without a valid
pixel gives overlap = 1, focal = 0 and an all-zero gradient (counts[4] = 0): a train step on it still runs and weight decay still
applies; nothing checks for it on the host.  Data-parallel: each rank normalises by its own valid count and the ranks' gradients are
averaged with equal weight, as torch's DistributedDataParallel does with ignore_index.

topk (None or a fraction 0 < f <= 1): hard-pixel mining -- nnU-Net's TopKLoss, "bootstrapped cross-entropy", OHEM -- ``bdn_criterion_topk``.
The focal term is averaged over the K hardest valid pixels of the batch only: ppm = round(f * 1e6), K = max(1, n_valid * ppm // 1e6) (0
without a valid pixel), the pixels ranked by their float32 focal term (ties: the lower pixel index first) by an exact select on the device.
The focal gradient is exactly 0 at a valid pixel that is not kept; the selection is a constant for the gradient, as torch.topk is under
autograd.  The overlap term still runs over all valid pixels.  terms becomes f32[3] = overlap, focal, the K-th largest term (the
threshold), counts int32[6] = {TP, FP, FN, correct, valid, K}.  It needs a focal weight (gamma = 0 is top-k cross-entropy) and class
weights >= 0, and composes with ignore_index.  Data-parallel: each rank selects its own K from its own batch; with gradient accumulation
the selection is per micro-step.  topk=None is the criterion as it was, call for call.

w_lovasz (>= 0) adds w_lovasz * the Lovasz-Softmax term (Berman, Rahman Triki, Blaschko, CVPR 2018, batch level: the loss that optimises
the Jaccard index itself) -- ``bdn_lovasz_softmax``, an add-on pass behind whichever entry point above has run: per class the valid pixels
are sorted by |fg - p_c| descending on the device (the top-k key map, ties: the lower pixel index first) and weighted by the increments of
the Jaccard index along that order; the term is the mean over the classes present among the valid pixels (lovasz_classes='present') or
over every class ('all'); the order is a constant for the gradient, as torch.sort is under autograd.  `terms` gains one trailing element,
the unweighted Lovasz value; counts keep their shape.  With the Lovasz term alone the counts are those of confusion_counts().  It composes
with ignore_index and topk.  Data-parallel: each rank sorts its own batch; with gradient accumulation the sort is per micro-step.
w_lovasz=0 is the criterion as it was, call for call.

w_boundary (>= 0) adds w_boundary * the boundary term of Kervadec et al. (MIDL 2019) -- ``bdn_boundary_loss``, a second add-on pass through
the same seam (behind the Lovasz one if both are present): per image and included class the signed distance phi to the contour of the
class is computed on the device each call (exact integer distance transforms of the label patch, the ignored pixels out of both site
sets), and the term is the mean over the valid pixels of sum_c softmax_c * phi_c; phi is a constant for the gradient.  boundary_classes
'foreground' (classes 1.., the paper's choice for the binary case) or 'all'; boundary_max_dist clamps phi to [-d, d].  The term can be
negative, and it is meant to be ramped up beside a region loss: the weight is passed per call, so ``criterion.w_boundary = x`` between
two steps takes effect at the next one (it must have been > 0 at construction, which decides the buffers).  `terms` gains one trailing
element, after the Lovasz one.  With add-on terms alone the counts are those of confusion_counts().  Data-parallel: each rank normalises by
its own valid count; with gradient accumulation the maps are computed per micro-step.  w_boundary=0 is the criterion as it was.

Soft targets -- ``bdn_criterion_soft``, the same overlap and focal terms with a target q_c >= 0 per class and a weight w >= 0 per pixel
(include/bidate_hip.h states the definition; TP = sum w p q, FP = sum w p (1 - q), FN = sum w (1 - p) q; the focal term sums
q_c a_c m_c (-log p_c) over the classes with q_c > 0 and is normalised by the NUMBER of pixels with w > 0).  Three inputs take this route:
label_smoothing e in [0, 1) (torch.nn.CrossEntropyLoss's: q = (1 - e) + e / ncls at the label's class and e / ncls elsewhere, a valid
label >= ncls keeps q = 0), `weights` given to evaluate() (float32 [B,H,W], multiplied into the 0 / 1 weight of ignore_index: confidence
weights, border down-weighting), and float32 [B,C,H,W] `labels`, taken as the targets themselves (probability maps of a teacher, MixUp
blends; label_smoothing must be 0 and ignore_index None then: give a weight of 0 instead).  dlogits is exactly 0 where w is not > 0 and
nothing of such a pixel reaches an output; counts are int32[5] = {TP, FP, FN, correct, valid} of argmax(logits) against the label or
argmax_c q_c.  Nothing is read back: negative or non-finite targets at a valid pixel are the caller's error.  topk ranks a hard-label term
and refuses every soft input (ValueError).  w_lovasz and w_boundary compose with label_smoothing and with weights on hard labels: their
passes run behind the soft entry point on the unchanged labels (and ignore_index), unweighted; with float targets they raise ValueError.
The soft route needs buffers(soft=True) (label_smoothing > 0 implies it): evaluate() raises on smaller ones rather than reallocate.  With
label_smoothing 0, no weights and class-index labels every call is issued as it always was.
"""

NAMES = ('tversky', 'dice', 'jaccard', 'focal', 'focal+tversky', 'focal+dice', 'focal+jaccard')
COMPOUND = tuple(n for n in NAMES if '+' in n)
LOVASZ_NAMES = ('lovasz', 'focal+lovasz')
LOVASZ_CLASSES = {'present': 0, 'all': 1}
BOUNDARY_CLASSES = {'foreground': 0, 'all': 1}
REDUCE = {'columns': 0, 'image': 1}


class Criterion:
    def __init__(self, w_overlap=1.0, alpha=0.5, beta=0.5, eps=1e-7, reduce='columns', w_focal=0.0, gamma=0.0, class_alpha=None,
                 size_average=True, ignore_index=None, topk=None, w_lovasz=0.0, lovasz_classes='present', w_boundary=0.0,
                 boundary_classes='foreground', boundary_max_dist=None, label_smoothing=0.0):
        """reduce: 'columns' -- what the reference's train.py gets from [B,H,W] labels, sums over dims (0,2), one ratio per (class,
        column) -- or 'image', dims (0,2,3), one ratio per class ([B,1,H,W] labels there).  class_alpha: None, a float a (class
        weights [a, 1 - a], utils/metrics.py:13-14) or a sequence of ncls class weights.  ignore_index: None -- every pixel carries a label,
        bdn_criterion -- or the label byte (0..255) of the pixels to leave out (module docstring), bdn_criterion_masked.  topk: None, or the fraction 0 < f <= 1 of the valid pixels the
        focal term is averaged over, the hardest first (module docstring), bdn_criterion_topk.  w_lovasz: the weight of the Lovasz-Softmax term,
        lovasz_classes 'present' or 'all' (module docstring), bdn_lovasz_softmax.  w_boundary: the weight of the boundary term,
        boundary_classes 'foreground' or 'all', boundary_max_dist None or the clamp of the signed distance in pixels (module docstring),
        bdn_boundary_loss.  label_smoothing: 0 <= e < 1, the smoothed hard-label targets of bdn_criterion_soft (module docstring)."""
        if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)) or not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f'label_smoothing must be a number in [0, 1), got {label_smoothing!r}')
        self.label_smoothing = float(label_smoothing)
        w_overlap, w_focal, w_lovasz, w_boundary = float(w_overlap), float(w_focal), float(w_lovasz), float(w_boundary)
        if not w_boundary >= 0.0:
            raise ValueError(f'criterion weights must be >= 0, got w_boundary={w_boundary}')
        if boundary_classes not in BOUNDARY_CLASSES:
            raise ValueError(f"boundary_classes must be 'foreground' or 'all', got {boundary_classes!r}")
        if boundary_max_dist is not None:
            if isinstance(boundary_max_dist, bool) or not isinstance(boundary_max_dist, (int, float)) or not 0.0 < float(boundary_max_dist) < float('inf'):
                raise ValueError(f'boundary_max_dist must be None or a positive number of pixels, got {boundary_max_dist!r}')
            boundary_max_dist = float(boundary_max_dist)
        self._w_boundary, self._boundary_pass = w_boundary, w_boundary > 0.0
        self.boundary_classes, self.boundary_max_dist = boundary_classes, boundary_max_dist
        if not (w_overlap >= 0.0 and w_focal >= 0.0):
            raise ValueError(f'criterion weights must be >= 0, got w_overlap={w_overlap}, w_focal={w_focal}')
        if not w_lovasz >= 0.0:
            raise ValueError(f'criterion weights must be >= 0, got w_lovasz={w_lovasz}')
        if lovasz_classes not in LOVASZ_CLASSES:
            raise ValueError(f"lovasz_classes must be 'present' or 'all', got {lovasz_classes!r}")
        if w_overlap == 0.0 and w_focal == 0.0 and w_lovasz == 0.0 and w_boundary == 0.0:
            raise ValueError('criterion weights are both zero')
        self.w_lovasz, self.lovasz_classes = w_lovasz, lovasz_classes
        if reduce not in REDUCE:
            raise ValueError(f"reduce must be 'columns' or 'image', got {reduce!r}")
        if not float(gamma) >= 0.0:
            raise ValueError(f'focal gamma must be >= 0, got {gamma}')
        if ignore_index is not None:
            if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index or not 0 <= int(ignore_index) <= 255:
                raise ValueError(f'ignore_index must be None or a label byte 0..255, got {ignore_index!r}')
            ignore_index = int(ignore_index)
        self.ignore_index = ignore_index
        self.w_overlap, self.alpha, self.beta, self.eps, self.reduce = w_overlap, float(alpha), float(beta), float(eps), reduce
        self.w_focal, self.gamma, self.size_average = w_focal, float(gamma), bool(size_average)
        if isinstance(class_alpha, (float, int)):
            class_alpha = [float(class_alpha), 1.0 - float(class_alpha)]
        self.class_alpha = None if class_alpha is None else tuple(float(v) for v in class_alpha)
        self.topk_ppm = None
        if topk is not None:
            if isinstance(topk, bool) or not isinstance(topk, (float, int)) or not 0.0 < float(topk) <= 1.0:
                raise ValueError(f'topk must be None or a fraction 0 < f <= 1, got {topk!r}')
            ppm = int(round(float(topk) * 1e6))
            if not 1 <= ppm <= 1_000_000:
                raise ValueError(f'topk={topk!r} is {ppm} parts per million: it must lie in 1..1000000')
            if not w_focal > 0.0:
                raise ValueError('topk ranks the focal term: the criterion needs a focal weight (gamma = 0 is top-k cross-entropy)')
            if self.class_alpha is not None and not all(v >= 0.0 for v in self.class_alpha):
                raise ValueError(f'topk needs class weights >= 0, got class_alpha={self.class_alpha}')
            topk, self.topk_ppm = float(topk), ppm
        self.topk = topk
        if self.label_smoothing > 0.0:
            if topk is not None:
                raise ValueError('topk ranks a hard-label focal term: it does not take label_smoothing (soft targets)')
            if w_overlap == 0.0 and w_focal == 0.0:
                raise ValueError('label_smoothing acts on the overlap and focal terms: the criterion needs one of their weights')
        self._alpha_dev = {}

    @property
    def has_boundary(self):
        """True when the criterion was built with w_boundary > 0: the boundary pass runs, `terms` carries its value, the workspace its part."""
        return self._boundary_pass

    @property
    def w_boundary(self):
        return self._w_boundary

    @w_boundary.setter
    def w_boundary(self, value):
        """The weight goes to bdn_boundary_loss with every call: a loop may ramp it between steps.  Whether the pass exists (workspace,
        terms) was decided at construction."""
        value = float(value)
        if not value >= 0.0:
            raise ValueError(f'criterion weights must be >= 0, got w_boundary={value}')
        if value > 0.0 and not self.has_boundary:
            raise ValueError('w_boundary can only be changed on a criterion built with w_boundary > 0')
        self._w_boundary = value

    @classmethod
    def parse(cls, name, tversky_alpha=0.5, tversky_beta=0.5, focal_gamma=None, focal_alpha=None, weights=(1, 1), eps=1e-7,
              reduce='columns', ignore_index=None, topk=None, lovasz_classes='present', w_boundary=0.0, boundary_classes='foreground',
              boundary_max_dist=None, label_smoothing=0.0):
        """The criterion of a --loss_function name.  weights = (w_focal, w_overlap), used by the compound names only.  topk: a name with a
        focal term only (Criterion raises ValueError otherwise).  LOVASZ_NAMES: 'lovasz' is the Lovasz-Softmax term alone; 'focal+lovasz'
        has weights = (w_focal, w_lovasz) and, with focal_gamma None, gamma 0: cross-entropy + Lovasz, the usual pairing.  w_boundary,
        boundary_classes, boundary_max_dist: the boundary term beside any name (--boundary_weight).  label_smoothing: --label_smoothing."""
        bnd = dict(w_boundary=w_boundary, boundary_classes=boundary_classes, boundary_max_dist=boundary_max_dist,      # validated at any weight
                   label_smoothing=label_smoothing)
        if name in LOVASZ_NAMES:
            focal = name != 'lovasz'
            w_focal, w_lovasz = (float(weights[0]), float(weights[1])) if focal else (0.0, 1.0)
            return cls(0.0, eps=eps, reduce=reduce, w_focal=w_focal, gamma=(focal_gamma or 0.0) if focal else 0.0,
                       class_alpha=focal_alpha if focal else None, ignore_index=ignore_index, topk=topk, w_lovasz=w_lovasz,
                       lovasz_classes=lovasz_classes, **bnd)
        if name not in NAMES:
            raise ValueError(f'unknown criterion {name!r}: one of {", ".join(NAMES + LOVASZ_NAMES)}')
        parts = name.split('+')
        focal, overlap = 'focal' in parts, parts[-1] if parts[-1] != 'focal' else None
        if focal and focal_gamma is None:
            raise ValueError(f'criterion {name!r} needs a focal gamma')
        w_focal, w_overlap = (float(weights[0]), float(weights[1])) if focal and overlap else (float(focal), float(overlap is not None))
        coef = {'tversky': (tversky_alpha, tversky_beta, eps), 'dice': (0.5, 0.5, 0.5 * eps), 'jaccard': (1.0, 1.0, eps),
                None: (0.5, 0.5, eps)}[overlap]
        return cls(w_overlap, *coef, reduce=reduce, w_focal=w_focal, gamma=focal_gamma if focal else 0.0,
                   class_alpha=focal_alpha if focal else None, ignore_index=ignore_index, topk=topk, **bnd)

    def __repr__(self):
        return (f'Criterion(w_overlap={self.w_overlap}, alpha={self.alpha}, beta={self.beta}, eps={self.eps}, reduce={self.reduce!r}, '
                f'w_focal={self.w_focal}, gamma={self.gamma}, class_alpha={self.class_alpha}, size_average={self.size_average}'
                + (f', ignore_index={self.ignore_index}' if self.ignore_index is not None else '')
                + (f', topk={self.topk}' if self.topk is not None else '')
                + (f', label_smoothing={self.label_smoothing}' if self.label_smoothing else '')
                + (f', w_lovasz={self.w_lovasz}, lovasz_classes={self.lovasz_classes!r}' if self.w_lovasz else '')
                + (f', w_boundary={self.w_boundary}, boundary_classes={self.boundary_classes!r}, boundary_max_dist={self.boundary_max_dist}'
                   if self.has_boundary else '') + ')')

    # ------------------------------------------------------------------ device side
    def _class_alpha(self, device, ncls):
        if self.class_alpha is None:
            return None
        if len(self.class_alpha) < ncls:
            raise RuntimeError(f'class_alpha holds {len(self.class_alpha)} class weights for {ncls} classes')
        import torch
        t = self._alpha_dev.get(device)
        if t is None:
            t = self._alpha_dev[device] = torch.tensor(self.class_alpha, dtype=torch.float32).to(device)
        return t

    def buffers(self, shape, device, soft=False):
        """Persistent outputs for logits of `shape`: (workspace, loss, terms, counts), the `out` of evaluate().  counts is int32[4], or
        int32[5] with an ignore_index; with topk, terms is f32[3] and counts int32[6].  With w_lovasz the workspace also holds
        bdn_lovasz_softmax's (behind the other, 256-byte aligned) and terms has one more element, the last.  soft=True (implied by
        label_smoothing > 0): the buffers of the soft route -- bdn_criterion_soft's workspace in front, counts int32[5] -- which a call
        with `weights` or float targets needs; such buffers serve that route only."""
        import torch
        from . import _lib
        B, C, H, W = shape
        soft = bool(soft) or self.label_smoothing > 0.0
        if soft and self.topk is not None:
            raise ValueError('topk ranks a hard-label focal term: it has no soft route')
        masked = self.ignore_index is not None or soft
        query = _lib.load().bdn_criterion_masked_workspace_bytes if masked else _lib.load().bdn_criterion_workspace_bytes
        if self.topk is not None:
            query = _lib.load().bdn_criterion_topk_workspace_bytes
        if soft:
            query = _lib.load().bdn_criterion_soft_workspace_bytes
        n = query(B, C, H, W, REDUCE[self.reduce])
        if n == 0:
            raise RuntimeError(f'fabric_amd: the criterion takes logits [B, 2..8, H, W] with B*H*W < 2^31, got {tuple(shape)}')
        n_terms = 3 if self.topk is not None else 2
        if self.w_lovasz:
            n = self._lovasz_offset(n) + _lib.load().bdn_lovasz_workspace_bytes(B, C, H, W)
            n_terms += 1
        if self.has_boundary:
            nb = _lib.load().bdn_boundary_workspace_bytes(B, C, H, W)
            if nb == 0:
                raise RuntimeError(f'fabric_amd: the boundary term takes H, W <= 32767 and 2*C*B*H*W < 2^31, got {tuple(shape)}')
            n = self._lovasz_offset(n) + nb
            n_terms += 1
        # add-on terms alone: the entry point that counts writes no term, so the terms in front of theirs are zeroed here, once
        terms = (torch.zeros if self._addon_only else torch.empty)(n_terms, dtype=torch.float32, device=device)
        return (torch.empty((n + 15) // 16 * 16, dtype=torch.uint8, device=device), torch.empty((), dtype=torch.float32, device=device), terms,
                torch.empty(6 if self.topk is not None else 5 if masked else 4, dtype=torch.int32, device=device))

    @staticmethod
    def _lovasz_offset(n):
        """Where bdn_lovasz_softmax's workspace starts behind the n bytes of the other entry point's."""
        return (n + 255) // 256 * 256

    @property
    def _lovasz_only(self):
        return self.w_lovasz > 0.0 and self.w_overlap == 0.0 and self.w_focal == 0.0 and not self.has_boundary

    @property
    def _addon_only(self):
        """Only add-on terms (Lovasz, boundary): the overlap / focal entry point runs for the counts alone."""
        return (self.w_lovasz > 0.0 or self.has_boundary) and self.w_overlap == 0.0 and self.w_focal == 0.0

    def _lovasz(self, logits, labels, ws, n_base, loss, terms, dlogits, accumulate, pixel_errors, ranks):
        from . import _lib
        B, C, H, W = logits.shape
        _lib.call('bdn_lovasz_softmax', logits.data_ptr(), labels.data_ptr(), -1 if self.ignore_index is None else self.ignore_index,
                  LOVASZ_CLASSES[self.lovasz_classes], self.w_lovasz, int(accumulate), ws.data_ptr() + self._lovasz_offset(n_base),
                  loss.data_ptr(), terms.data_ptr() + 4 * (terms.numel() - 1 - int(self.has_boundary)), _lib.ptr(dlogits),
                  _lib.ptr(pixel_errors), _lib.ptr(ranks), B, C, H, W, _lib.stream_ptr())

    def _boundary(self, logits, labels, ws, n_front, loss, terms, dlogits, accumulate, phi):
        """bdn_boundary_loss behind n_front bytes of the workspace (the other entry points'), its term the last of `terms`."""
        from . import _lib
        B, C, H, W = logits.shape
        _lib.call('bdn_boundary_loss', logits.data_ptr(), labels.data_ptr(), -1 if self.ignore_index is None else self.ignore_index,
                  BOUNDARY_CLASSES[self.boundary_classes], self.boundary_max_dist or 0.0, self._w_boundary, int(accumulate),
                  ws.data_ptr() + self._lovasz_offset(n_front), loss.data_ptr(), terms.data_ptr() + 4 * (terms.numel() - 1), _lib.ptr(dlogits),
                  _lib.ptr(phi), B, C, H, W, _lib.stream_ptr())

    def _soft_inputs(self, logits, labels, weights):
        """(soft, targets) of one evaluate() call: whether it takes the soft route, and whether `labels` are float targets.  Checks dtype,
        shape, device and contiguity of `weights` and of float targets -- nothing is read from them -- and refuses what has no soft form."""
        import torch
        B, C, H, W = logits.shape
        targets = labels.is_floating_point() and tuple(labels.shape) == (B, C, H, W)
        if not (targets or weights is not None or self.label_smoothing > 0.0):
            return False, False
        if self.topk is not None:
            raise ValueError('topk ranks a hard-label focal term: it takes neither weights nor float targets')
        if self.w_overlap == 0.0 and self.w_focal == 0.0:
            raise ValueError('weights and float targets act on the overlap and focal terms: the criterion needs one of their weights')
        if targets:
            if self.w_lovasz or self.has_boundary:
                raise ValueError('the Lovasz and boundary terms are defined on class-index labels: they do not take float targets')
            if self.label_smoothing > 0.0 or self.ignore_index is not None:
                raise ValueError('float targets are taken as given: label_smoothing must be 0 and ignore_index None (give a weight of 0)')
            if labels.dtype != torch.float32 or labels.device != logits.device or not labels.is_contiguous():
                raise RuntimeError(f'fabric_amd: float targets must be a contiguous float32 [B,C,H,W] tensor on {logits.device}')
        if weights is not None:
            if (weights.dtype != torch.float32 or weights.device != logits.device or not weights.is_contiguous()
                    or tuple(weights.shape) not in ((B, H, W), (B, 1, H, W))):
                raise RuntimeError(f'fabric_amd: weights must be a contiguous float32 [B,H,W] tensor on {logits.device} for logits '
                                   f'{tuple(logits.shape)}, got {weights.dtype} {tuple(weights.shape)}')
        return True, targets

    def _evaluate_soft(self, logits, labels, targets, weights, ws, loss, terms, counts, dlogits, ca):
        """bdn_criterion_soft: the overlap / focal entry point of a call with label smoothing, weights or float targets."""
        from . import _lib
        B, C, H, W = logits.shape
        _lib.call('bdn_criterion_soft', logits.data_ptr(), None if targets else labels.data_ptr(), labels.data_ptr() if targets else None,
                  _lib.ptr(weights), -1 if self.ignore_index is None else self.ignore_index, self.label_smoothing, self.w_overlap,
                  self.alpha, self.beta, self.eps, REDUCE[self.reduce], self.w_focal, self.gamma, _lib.ptr(ca), int(self.size_average),
                  ws.data_ptr(), loss.data_ptr(), terms.data_ptr(), counts.data_ptr(), _lib.ptr(dlogits), B, C, H, W, _lib.stream_ptr())
        return loss, terms, counts, dlogits

    def evaluate(self, logits, labels, want_grad=True, out=None, pixel_terms=None, kept=None, pixel_errors=None, ranks=None, phi=None,
                 weights=None):
        """-> (loss, terms, counts, dlogits) of float32 [B,C,H,W] logits and [B,H,W] or [B,1,H,W] class-index labels, on the current
        stream: loss a 0-dim tensor, terms f32[2] = the unweighted overlap and focal values, counts int32[4] = {TP, FP, FN, correct} of
        argmax(logits), dlogits = d loss / d logits (None without want_grad: no gradient pass is launched).  `out`: buffers() of this
        shape, overwritten by every call that is given them; fresh ones otherwise.  The reduction is the criterion's `reduce`,
        whichever rank the labels have.  With an ignore_index: counts int32[5] = {TP, FP, FN, correct, valid} over the valid pixels and
        dlogits exactly 0 at the ignored ones (module docstring).  With topk: terms f32[3] = overlap, focal, threshold and counts int32[6]
        = {.., valid, K}; `pixel_terms` (contiguous float32, B*H*W elements) and `kept` (contiguous uint8, B*H*W) are optional caller
        tensors that receive every pixel's ranked term (unspecified at ignored pixels) and its 0 / 1 kept flag.  With w_lovasz: the entry
        point above runs as it always did, then bdn_lovasz_softmax adds its term to loss and dlogits on the same stream (the term alone:
        the counts of confusion_counts(), then bdn_lovasz_softmax writes loss and dlogits); terms[-1] is the unweighted Lovasz value;
        `pixel_errors` (contiguous float32, C*B*H*W) and `ranks` (contiguous int32, C*B*H*W) are optional caller tensors that receive
        every class's errors and 0-based ranks (-1 at ignored pixels).  With w_boundary: bdn_boundary_loss runs last through the same seam;
        terms[-1] is the unweighted boundary value (the Lovasz one, if present, is terms[-2]); `phi` (contiguous float32, C*B*H*W) is an
        optional caller tensor that receives every class's signed distance (0 for a class that is not included).
        Soft targets (module docstring): with label_smoothing, with `weights` (contiguous float32 [B,H,W] on the logits' device) or with
        contiguous float32 [B,C,H,W] `labels` -- taken as targets -- bdn_criterion_soft runs in place of the entry point above; counts is
        int32[5] and `out` must come from buffers(soft=True).  Only dtype, shape, device and contiguity are checked: no host read."""
        import torch
        from . import _lib
        if logits.dim() != 4 or logits.dtype != torch.float32 or not logits.is_contiguous():
            if not logits.is_cuda:
                raise RuntimeError('fabric_amd: the losses run only on a ROCm device -- there is no CPU path')
            raise RuntimeError('fabric_amd: the criterion takes contiguous float32 [B,C,H,W] logits')
        B, C, H, W = logits.shape
        soft, targets = self._soft_inputs(logits, labels, weights)     # (what has no soft form is refused wherever the tensors live)
        if not logits.is_cuda:
            raise RuntimeError('fabric_amd: the losses run only on a ROCm device -- there is no CPU path')
        if not targets:
            if labels.numel() != B * H * W or tuple(labels.shape) not in ((B, H, W), (B, 1, H, W)):
                raise RuntimeError(f'labels must be [B,H,W] or [B,1,H,W] for logits {tuple(logits.shape)}, got {tuple(labels.shape)}')
            if labels.dtype != torch.uint8:
                labels = labels.to(torch.uint8)
            labels = labels.contiguous()
        ws, loss, terms, counts = out if out is not None else self.buffers(logits.shape, logits.device, soft=soft)
        if soft:
            if pixel_terms is not None or kept is not None:
                raise RuntimeError('fabric_amd: pixel_terms / kept are outputs of a criterion with topk')
            n_soft = _lib.load().bdn_criterion_soft_workspace_bytes(B, C, H, W, REDUCE[self.reduce])
            if n_soft == 0:
                raise RuntimeError(f'fabric_amd: the criterion takes logits [B, 2..8, H, W] with B*H*W < 2^31, got {tuple(logits.shape)}')
            if counts.numel() < 5 or ws.numel() * ws.element_size() < n_soft:
                raise RuntimeError('fabric_amd: weights and float targets need the buffers of the soft route: buffers(shape, device, soft=True)')
        dlogits = torch.empty_like(logits) if want_grad else None
        ca = self._class_alpha(logits.device, C)
        if not self.w_lovasz and (pixel_errors is not None or ranks is not None):
            raise RuntimeError('fabric_amd: pixel_errors / ranks are outputs of a criterion with w_lovasz')
        if not self.has_boundary and phi is not None:
            raise RuntimeError('fabric_amd: phi is an output of a criterion with w_boundary')
        if not self.w_lovasz and not self.has_boundary:
            if soft:
                return self._evaluate_soft(logits, labels, targets, weights, ws, loss, terms, counts, dlogits, ca)
            return self._evaluate_base(logits, labels, ws, loss, terms, counts, dlogits, ca, pixel_terms, kept)
        for t, dt, what in ((pixel_errors, torch.float32, 'pixel_errors'), (ranks, torch.int32, 'ranks'), (phi, torch.float32, 'phi')):
            if t is not None and (t.device != logits.device or t.dtype != dt or t.numel() != C * B * H * W or not t.is_contiguous()):
                raise RuntimeError(f'fabric_amd: {what} must be a contiguous {dt} tensor of {C * B * H * W} elements on {logits.device}')
        masked = self.ignore_index is not None
        query = 'bdn_criterion_soft_workspace_bytes' if soft else 'bdn_criterion_topk_workspace_bytes' if self.topk is not None else \
            'bdn_criterion_masked_workspace_bytes' if masked else 'bdn_criterion_workspace_bytes'
        n_base = getattr(_lib.load(), query)(B, C, H, W, REDUCE[self.reduce])
        if self._addon_only:                               # the counts: the statistics and finish passes of the overlap loss, no gradient pass
            if pixel_terms is not None or kept is not None:
                raise RuntimeError('fabric_amd: pixel_terms / kept are outputs of a criterion with topk')
            if masked:
                _lib.call('bdn_criterion_masked', logits.data_ptr(), labels.data_ptr(), self.ignore_index, 1.0, self.alpha, self.beta, self.eps,
                          REDUCE[self.reduce], 0.0, 0.0, None, 1, ws.data_ptr(), loss.data_ptr(), None, counts.data_ptr(), None, B, C, H, W,
                          _lib.stream_ptr())
            else:
                _lib.call('bdn_criterion', logits.data_ptr(), labels.data_ptr(), 1.0, self.alpha, self.beta, self.eps, REDUCE[self.reduce], 0.0,
                          0.0, None, 1, ws.data_ptr(), loss.data_ptr(), None, counts.data_ptr(), None, B, C, H, W, _lib.stream_ptr())
        elif soft:                                          # (never add-on only: _soft_inputs refuses that); the add-ons see the labels as they are
            self._evaluate_soft(logits, labels, targets, weights, ws, loss, terms, counts, dlogits, ca)
        else:
            self._evaluate_base(logits, labels, ws, loss, terms, counts, dlogits, ca, pixel_terms, kept)
        accumulate, n_front = not self._addon_only, n_base    # the first add-on pass of an add-on-only criterion writes, every other one adds
        if self.w_lovasz:
            self._lovasz(logits, labels, ws, n_base, loss, terms, dlogits, accumulate, pixel_errors, ranks)
            accumulate, n_front = True, self._lovasz_offset(n_base) + _lib.load().bdn_lovasz_workspace_bytes(B, C, H, W)
        if self.has_boundary:
            self._boundary(logits, labels, ws, n_front, loss, terms, dlogits, accumulate, phi)
        return loss, terms, counts, dlogits

    def _evaluate_base(self, logits, labels, ws, loss, terms, counts, dlogits, ca, pixel_terms, kept):
        """The overlap / focal entry point of this criterion, as evaluate() has always called it."""
        import torch
        from . import _lib
        B, C, H, W = logits.shape
        if self.topk is None:
            if pixel_terms is not None or kept is not None:
                raise RuntimeError('fabric_amd: pixel_terms / kept are outputs of a criterion with topk')
        else:
            for t, dt, what in ((pixel_terms, torch.float32, 'pixel_terms'), (kept, torch.uint8, 'kept')):
                if t is not None and (t.device != logits.device or t.dtype != dt or t.numel() != B * H * W or not t.is_contiguous()):
                    raise RuntimeError(f'fabric_amd: {what} must be a contiguous {dt} tensor of {B * H * W} elements on {logits.device}')
            _lib.call('bdn_criterion_topk', logits.data_ptr(), labels.data_ptr(), -1 if self.ignore_index is None else self.ignore_index,
                      self.w_overlap, self.alpha, self.beta, self.eps, REDUCE[self.reduce], self.w_focal, self.gamma, _lib.ptr(ca),
                      int(self.size_average), self.topk_ppm, ws.data_ptr(), loss.data_ptr(), terms.data_ptr(), counts.data_ptr(),
                      _lib.ptr(dlogits), _lib.ptr(pixel_terms), _lib.ptr(kept), B, C, H, W, _lib.stream_ptr())
            return loss, terms, counts, dlogits
        if self.ignore_index is not None:
            _lib.call('bdn_criterion_masked', logits.data_ptr(), labels.data_ptr(), self.ignore_index, self.w_overlap, self.alpha, self.beta,
                      self.eps, REDUCE[self.reduce], self.w_focal, self.gamma, _lib.ptr(ca), int(self.size_average), ws.data_ptr(),
                      loss.data_ptr(), terms.data_ptr(), counts.data_ptr(), _lib.ptr(dlogits), B, C, H, W, _lib.stream_ptr())
            return loss, terms, counts, dlogits
        _lib.call('bdn_criterion', logits.data_ptr(), labels.data_ptr(), self.w_overlap, self.alpha, self.beta, self.eps,
                  REDUCE[self.reduce], self.w_focal, self.gamma, _lib.ptr(ca), int(self.size_average), ws.data_ptr(), loss.data_ptr(),
                  terms.data_ptr(), counts.data_ptr(), _lib.ptr(dlogits), B, C, H, W, _lib.stream_ptr())
        return loss, terms, counts, dlogits
