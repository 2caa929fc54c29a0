"""The train.py step (reference train.py:83-101 + optim.SGD, train.py:55) as one fused schedule:

    to-device tensors -> forward -> Tversky loss, or the `criterion` given (+ argmax TP/FP/FN counts) -> backward
    -> bucketed gradient all-reduce overlapped with backward -> SGD (or momentum SGD / Adam / AdamW / LAMB / LARS: fabric_amd/optim.py)

with no host synchronisation inside the step (the reference syncs every step for sklearn
P/R/F1 and a comet upload, train.py:103-115; here the counts stay on the device).
Parameters and gradients live in two flat float32 buffers (fabric_amd/parallel.py); the
module's nn.Parameters are re-pointed at views of them, so ``model.state_dict()``,
``model.parameters()`` and ``p.grad`` keep working for callers that expect the reference's
surface.
"""
import contextlib

import torch
import torch.distributed as dist

from . import _lib
from . import optim as _optim
from .engine import param_order
from .parallel import FlatLayout, GradBucketer


class TrainStep:
    def __init__(self, model, lr=1e-3, tversky_alpha=0.1, tversky_beta=0.9, eps=1e-7,
                 process_group=None, n_buckets=4, distributed=True, force_collectives=False, guard=True,
                 optimizer='sgd', momentum=0.0, dampening=0.0, nesterov=False, weight_decay=None, betas=(0.9, 0.999), adam_eps=1e-8,
                 param_groups=None, bn='batch', criterion=None, accumulate=1, max_grad_norm=None,
                 ema_decay=None, average='ema', ema_every=1, ema_start=0, ema_buffers=True,
                 trust_coef=1e-3, lars_eps=1e-8, max_trust=None, adapt_1d=False, sam_rho=None, sam_adaptive=False, sam_eps=1e-12):
        """optimizer: 'sgd' (torch.optim.SGD: momentum, dampening, nesterov, weight_decay), 'adam' or 'adamw' (torch.optim.Adam / AdamW:
        betas, adam_eps, weight_decay); weight_decay=None is torch's default (0 for sgd and adam, 1e-2 for adamw).  The default, plain
        SGD, is the reference's optim.SGD(lr) (train.py:55) and keeps no state; the other rules keep theirs in flat f32 buffers in the
        gradient layout (`opt_state`), with `opt_step` the number of updates applied.  `lr` may be reassigned between steps.
        'lamb' (betas, adam_eps, decoupled weight_decay, max_trust) and 'lars' (momentum, dampening, nesterov, weight_decay, trust_coef,
        lars_eps, max_trust) scale every tensor's update by a trust ratio (fabric_amd/optim.py; bdn_lamb_step / bdn_lars_step: three
        launches, no host round trip).  adapt_1d=False: tensors of ndim <= 1 take ratio 1.  They always run on the per-tensor table
        (with groups and frozen parameters, or one implicit group), compose with accumulate, max_grad_norm (the clip coefficient
        reaches the rule on the device), the averaged weights and data-parallel runs (every rank forms the same norms from the
        all-reduced gradients).  `last_trust` is the device [n_tensors, 3] tensor {||p||, ||u|| or ||g||, applied ratio} of the last
        update, in layout order, {0, 0, 0} for a frozen tensor; trust_ratios() reads it on demand.

        param_groups: None (one set of hyperparameters, today's kernels), or a list of dicts {'params': [state-dict names or the
        nn.Parameter objects], 'lr': ..., 'weight_decay': ...} as torch.optim takes them (a missing key takes the step's value; at most 8
        groups; momentum / betas / eps are one per step, a group that names another value is refused).  `step.param_groups` is then a
        list of plain dicts read at every update: `step.param_groups[i]['lr'] = x` works the way a scheduler drives a torch optimizer.
        Parameters with requires_grad=False when the step is built, or at set_param_groups(), are FROZEN: never updated or decayed, no
        optimizer state, no weight-gradient GEMM, and backward stops at the last trainable layer (engine.chain_end).  A trainable
        parameter that no group lists raises ValueError: it is never silently frozen.  With groups or frozen parameters the update
        runs bdn_*_step_grouped; with neither, the ungrouped entry points as before.

        criterion: None (the reference's default, TverskyLoss(tversky_alpha, tversky_beta, eps) on [B,H,W] labels through bdn_tversky:
        the step as it always was), a fabric_amd.criterion.Criterion, or one of its names ('tversky', 'dice', 'jaccard', 'focal+dice',
        ...: Criterion.parse with this step's tversky_alpha / tversky_beta / eps; a focal term needs a gamma, so build the Criterion).
        With a criterion the loss runs bdn_criterion, labels may be [B,H,W] or [B,1,H,W] (the criterion's `reduce` decides the overlap
        reduction), `last_terms` holds the unweighted overlap and focal values beside `last_counts`, and `last_dlogits` the loss gradient.
        A Criterion with an ignore_index (bdn_criterion_masked) leaves the pixels with that label out: `last_counts` then has five entries,
        {TP, FP, FN, correct, valid}, `last_dlogits` is exactly 0 at the ignored pixels, and a batch without a valid pixel is a step with
        a zero gradient (weight decay still applies).  Data-parallel, every rank normalises by its own valid count and the gradients are
        averaged over the ranks with equal weight, as torch's DistributedDataParallel does with ignore_index.
        A Criterion with a topk (bdn_criterion_topk, hard-pixel mining) averages the focal term over the hardest fraction of the valid
        pixels of the batch: `last_counts` has six entries, {.., valid, K}, `last_terms` three, {overlap, focal, the K-th largest focal
        term}.  The selection is per call: per micro-step with accumulate > 1, per rank in a data-parallel run.
        A Criterion with a w_lovasz (bdn_lovasz_softmax, the names 'lovasz' and 'focal+lovasz': gamma 0, cross-entropy + Lovasz) adds the
        Lovasz-Softmax term behind that entry point: `last_terms` gains one trailing element, the unweighted term; `last_counts` keeps its
        shape.  The sort is per call: per micro-step with accumulate > 1, per rank in a data-parallel run.
        A Criterion with a w_boundary (bdn_boundary_loss) adds the boundary term last: `last_terms[-1]` is its unweighted value (the
        Lovasz one, if present, moves to [-2]).  The distance maps are computed per call -- per micro-step, per rank, each rank normalising
        by its own valid count -- and the weight is read per call: `step.criterion.w_boundary = x` takes effect at the next step.

        bn: 'batch' (BatchNorm on batch statistics, running statistics updated: a training step) or 'frozen' (BatchNorm on its running
        statistics, which are constants: running_mean / running_var / num_batches_tracked are not touched, and the conv biases in
        front of a BatchNorm have real gradients, which are then reduced across ranks like every other).  The module's .training flag
        is not consulted.

        accumulate: K >= 1.  Every step() is a micro-step (forward, loss, backward; BatchNorm running statistics update as in torch; the
        micro-batch's own unscaled loss is returned); the update runs on every K-th call with the MEAN of the K micro-batch gradients
        (grad_scale = 1 / (world * K)).  `micro` counts the pending micro-steps (0..K-1), `opt_step` counts updates.  The sum is kept in
        one flat float32 buffer in the gradient layout, `flat_accum`, in a fixed order: micro-step 1 acc = g1; micro-steps 2..K-1
        acc += g; micro-step K flat_grads = gK + acc (bdn_grad_accumulate, one float32 add per element each).  Micro-steps 1..K-1 issue
        no collective and leave the engine's packed weights valid (not under sam_rho: every micro-step perturbs and restores the weights
        and repacks twice); on micro-step K the pending sum is added bucket by bucket right before
        each bucket's all-reduce (GradBucketer.before_reduce), so there is one exchange per UPDATE and it still overlaps backward.
        flush() applies (or drops) an incomplete accumulation, e.g. at the end of an epoch.

        max_grad_norm: None, x > 0, or float('inf') (measure only).  torch.nn.utils.clip_grad_norm_(parameters, x) between backward and
        the update: bdn_grad_norm leaves the norm of the averaged gradients of the trainable parameters and the clip coefficient in a
        persistent device buffer (`last_grad_norm`, `last_clip_coef`: 0-dim views that the next update overwrites; clone them to keep
        them), and the update reads the coefficient from there (bdn_*_step_grouped_ex): no host synchronisation, no pass that rescales
        the gradients.  flat_grads, and with it p.grad, therefore keeps the UNCLIPPED (and unaveraged) sum.

        ema_decay, average, ema_every, ema_start, ema_buffers: an averaged copy of the weights, torch.optim.swa_utils.AveragedModel's.
        On when ema_decay is a number in [0, 1) (average='ema': avg = lerp(avg, p, 1 - ema_decay)) or average='swa' (the equal-weight
        running mean, avg = lerp(avg, p, 1 / (n_averaged + 1)); no decay); off, the default, nothing is allocated or launched and
        `flat_avg` is None.  `flat_avg` is one more flat buffer in `layout` (it starts as a clone of flat_params), `avg_buffers` holds one
        tensor per averaged BatchNorm buffer by state-dict key, `n_averaged` is a host int.  The averaging update is ONE launch
        (bdn_ema_update) on the step's stream right after the optimizer update of an updating call -- never on a micro-step of
        accumulate=K, also after flush() -- of the u-th update of this step object when u > ema_start and (u - ema_start) is a multiple
        of ema_every.  The first averaging update is a copy, as AveragedModel's is; the weight is formed in double on the host and
        passed as float32.  Frozen parameters are skipped through the step's segment table, and a frozen tensor's average is its value:
        set_param_groups() re-reads the table and sets the average of every tensor that is frozen then to the tensor's value (its
        history is dropped: the value is constant from there on, and ema_weights() and ema_state_dict() keep describing one model).
        ema_start counts the updates of this step object; load_ema_state_dict() of a state with n_averaged > 0 ends the delay (a
        resumed run goes on averaging at once, the ema_every phase starting at the load).  ema_buffers=True (AveragedModel(use_buffers=True)): running_mean / running_var are
        averaged with the same weight in one more launch (bdn_ema_update_multi, its descriptor uploaded once); False
        (use_buffers=False): the averaged model uses the live buffers.  num_batches_tracked is NEVER averaged, the averaged model
        carries the live count: a deliberate departure from AveragedModel(use_buffers=True), which pushes the int64 count through the
        float formula.  Data-parallel: every rank holds bit-identical parameters after the update, so every rank computes the same
        average and nothing is communicated (the BatchNorm buffers are per rank, as they always were; rank 0's are saved).
        ema_state_dict() / load_ema_state_dict() exchange the state in AveragedModel's format; `with step.ema_weights():` evaluates
        on the averaged weights.

        sam_rho, sam_adaptive, sam_eps: sharpness-aware minimisation (SAM, Foret et al. 2021; sam_adaptive=True: the scale-invariant ASAM
        of Kwon et al. 2021).  sam_rho=None, the default: nothing is allocated or launched and the step is the one above, call for call.
        With sam_rho > 0 every step() call -- every micro-step of accumulate=K -- runs two passes over its batch on the step's stream:
        pass 1 (forward, criterion, backward at w; no collective; BatchNorm's running statistics update, once); bdn_sam_perturb with
        this rank's own gradient (the paper's m-sharpness: nothing is exchanged in pass 1), which keeps w in `flat_sam` and moves the
        trainable parameters to w + e, e = rho * t^2 * g / (||t * g|| + sam_eps), t = |w| (adaptive) or 1; pass 2 at w + e on batch
        statistics that move NO running statistics (engine.forward(track_running=False)), carrying the step's usual bucketed exchange
        and accumulation; bdn_sam_restore, a bit-exact copy of `flat_sam` back, so data-parallel ranks stay bit-equal; then the update
        at w with pass 2's gradient -- norm and clip, any update rule, the averaged weights, all unchanged.  Both kernels are issued
        where the update is: behind backward's joined streams, because backward reads parameters directly (classifier, BatchNorm
        weight and bias, conv biases, the first layer's master weight); the engine's packed filter images are invalidated after each.
        With bn='frozen' both passes run on the running statistics.  Frozen parameters are not perturbed and are not in the norm; the
        table is the layer-wise rules' per-tensor one, rebuilt at set_param_groups().  step() returns the loss at w; `last_counts` and
        `last_terms` are pass 1's (copied on the device before pass 2 reuses the criterion's buffers); `last_logits` and `last_dlogits`
        are pass 2's, those of the perturbed weights.  `last_sam_loss` is the loss at w + e (a 0-dim device tensor),
        `last_sam_norm` and `last_sam_scale` are 0-dim views of the kernel's {||t * g||, rho / (norm + sam_eps)}: overwritten by the
        next step, like `last_grad_norm`.  `flat_sam` is scratch, valid only inside a step; SAM keeps no state between steps, so
        optimizer_state_dict() does not know it.

        guard: when the step issues collectives (world > 1, or force_collectives) and guard_collectives() has not been called, the
        first step() runs it in its measure-only form (replace_streams=False: it may defer the buckets, it never swaps a stream the
        caller may already have adopted) and reports / warns about a stream arrangement in which they slow the step down."""
        if bn not in ('batch', 'frozen'):
            raise ValueError(f"bn must be 'batch' or 'frozen', got {bn!r}")
        self.accumulate = _optim.check_accumulate(accumulate)
        ema_on, self.ema_decay, self.average, self.ema_every, self.ema_start = _optim.check_ema(ema_decay, average, ema_every, ema_start)
        self.ema_buffers = bool(ema_buffers)
        self.flat_avg, self.avg_buffers, self.n_averaged = None, {}, 0
        self._updates, self._ema_hold, self._swapped, self._avg_desc = 0, False, False, None
        self.max_grad_norm = _optim.check_max_grad_norm(max_grad_norm)
        self.sam_rho, self.sam_adaptive, self.sam_eps = _optim.check_sam(sam_rho, sam_adaptive, sam_eps)
        self.flat_sam = self._sam = None
        self.last_sam_loss = self.last_sam_norm = self.last_sam_scale = None
        self._sam_pending = False
        self.micro = 0
        self.flat_accum = self._norm = self._clip_table = None
        self.last_grad_norm = self.last_clip_coef = None
        self.model, self.lr, self.bn = model, lr, bn
        self.optim = _optim.OptimConfig(optimizer, lr=lr, momentum=momentum, dampening=dampening, nesterov=nesterov,
                                        weight_decay=weight_decay, betas=betas, eps=adam_eps, trust_coef=trust_coef, lars_eps=lars_eps,
                                        max_trust=max_trust, adapt_1d=adapt_1d)
        self._lw, self.last_trust = None, None
        self._guard = guard
        self.collectives_report = None
        self.alpha, self.beta, self.eps = tversky_alpha, tversky_beta, eps
        if isinstance(criterion, str):
            from .criterion import Criterion
            criterion = Criterion.parse(criterion, tversky_alpha=tversky_alpha, tversky_beta=tversky_beta, eps=eps)
        self.criterion = criterion
        self.group = process_group
        self.high_priority_chain = True
        self._hp = None
        self.world = (dist.get_world_size(process_group)
                      if distributed and dist.is_available() and dist.is_initialized() else 1)
        named = list(model.named_parameters())
        dev = named[0][1].device
        if dev.type != 'cuda':
            raise RuntimeError('fabric_amd: TrainStep needs the model on a ROCm device (model.cuda() first)')
        self._names = [k for k, _ in named]                  # model.parameters() order: torch.optim's state indices
        self._by_id = {id(p): k for k, p in named}
        self._checked_groups(param_groups)                   # a refused grouping leaves the module as it was
        order = param_order(model.n_channels)
        self.layout = FlatLayout([(k, p.shape) for k, p in named], order)
        self.flat_params = torch.zeros(self.layout.total, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(self.layout.total, dtype=torch.float32, device=dev)
        for k, p in named:
            v = self.layout.view(self.flat_params, k)
            v.copy_(p.data)
            p.data = v
            p.grad = self.layout.view(self.flat_grads, k)
        self.grads = {k: self.layout.view(self.flat_grads, k) for k, _ in named}
        self.opt_state = {key: torch.zeros_like(self.flat_params) for key in self.optim.state_keys()}
        self.opt_step = 0
        bias_tail = [k for k in order if k.endswith('.bias') and k.split('.')[-2] in ('0', '3')]
        if bn == 'frozen':
            bias_tail = []                                   # on running statistics those biases have gradients (scale * dbeta): reduce them
        # bn='batch': backward never writes those bias gradients (zero_bias_grads=False), it relies on the zeros they were born with.
        # p.grad is a view of flat_grads, so an eager backward on the module adds into them -- an eval-mode graph adds real values.
        # Such a write moves flat_grads' version counter (the library's own kernels do not): _step() zeroes the slices again only then
        self._zero_tail = [(k, self.layout.view(self.flat_grads, k)) for k in bias_tail]
        self.bucketer = GradBucketer(self.layout, self.flat_grads, n_buckets, process_group, keys_no_reduce=bias_tail,
                                     enabled=self.world > 1 or force_collectives, force=force_collectives)
        if self.world > 1:                                   # identical start on every rank (DataParallel broadcasts)
            dist.broadcast(self.flat_params, src=0, group=process_group)
        self._tv = None
        self._tv_soft, self._weights = None, None              # the soft route's criterion buffers; the pixel weights of the step under way
        self.last_counts = self.last_terms = self.last_dlogits = None
        # detached aliases of every parameter / buffer (same storage), built once: no per-step dict walk
        self._P = {k: v.detach() for k, v in self.model.state_dict(keep_vars=True).items()}
        self._bound = self._bindings()
        self.param_groups = self._groups = self._seg = self._need = None
        self._implicit_group = False
        if param_groups is not None or any(not p.requires_grad for _, p in named):
            self.set_param_groups(param_groups)
        if self.accumulate > 1:
            self.flat_accum = torch.empty_like(self.flat_grads)             # written (add = 0) before it is ever read: no zero-fill
            self.bucketer.before_reduce = self._add_pending
        self._adding = False
        if self.max_grad_norm is not None:
            ws = torch.empty(_lib.load().bdn_grad_norm_workspace_bytes(self.layout.total) // 8, dtype=torch.float64, device=dev)
            out = torch.zeros(2, dtype=torch.float32, device=dev)
            self._norm = (ws, out)
            self.last_grad_norm, self.last_clip_coef = out[0], out[1]
            if self._groups is None:
                self._implicit_table()                       # uploaded now: the step itself never waits for the device
        if ema_on:
            self._init_average()
        if self.optim.kind in _optim.LAYERWISE:
            self._layerwise_table()                          # uploaded now: the step itself never waits for the device
        if self.sam_rho is not None:
            self.flat_sam = torch.empty_like(self.flat_params)              # written by bdn_sam_perturb before bdn_sam_restore reads it
            self._sam_table()                                # uploaded now, like the layer-wise table
        self._grads_version = self.flat_grads._version

    def _sam_table(self):
        """(groups, the three device arrays of bdn_sam_perturb's per-tensor table, n_tensors, workspace, out), built through the
        layer-wise rules' route (the step's groups, or the one implicit group of every parameter) and rebuilt when the groups object
        changed (set_param_groups), never per step.  `last_sam_norm` / `last_sam_scale` are views of out."""
        pg = self._layerwise_groups()
        if self._sam is None or self._sam[0] is not pg:
            dev = self.flat_params.device
            n_ten = len(self.layout.order)
            ends, lens, ids, _ = (t.to(dev) for t in _optim.tensor_table(self.layout, pg))
            if self._sam is None:
                ws = torch.empty(_lib.load().bdn_sam_workspace_bytes(self.layout.total, n_ten) // 8, dtype=torch.float64, device=dev)
                out = torch.zeros(2, dtype=torch.float32, device=dev)
                self.last_sam_norm, self.last_sam_scale = out[0], out[1]
            else:
                ws, out = self._sam[3], self._sam[4]
            self._sam = (pg, (ends, lens, ids), n_ten, ws, out)
        return self._sam

    def _implicit_table(self):
        """The clipped update runs the grouped (_ex) entry points; without groups or frozen parameters, on one implicit group of every
        parameter.  Built when the step is, unless groups or frozen parameters give it a table already; after a set_param_groups(None) that
        returns to no groups, at the next update.  The group's lr and weight_decay follow the step's at every update."""
        if self._clip_table is None:
            dev = self.flat_params.device
            pg = _optim.ParamGroups(self.optim, self._names, None, ())
            ends, ids = _optim.segment_table(self.layout, pg)
            self._clip_table = (pg, (torch.tensor(ends, dtype=torch.int64).to(torch.int32).to(dev),
                                     torch.tensor(ids, dtype=torch.int32).to(dev), len(ends)))
        return self._clip_table

    def _layerwise_groups(self):
        """The ParamGroups the layer-wise rules run on: the step's, or the one implicit group of every parameter, following the step's
        lr / weight_decay as the clipped update's does."""
        if self._groups is not None:
            pg = self._groups
            if self._implicit_group:
                pg.groups[0]['lr'] = float(self.lr)
        else:
            pg = self._implicit_table()[0]
            pg.groups[0]['lr'], pg.groups[0]['weight_decay'] = float(self.lr), self.optim.weight_decay
        return pg

    def _layerwise_table(self):
        """(groups, the four device arrays of the per-tensor table, n_tensors, workspace, trust_out) of bdn_lamb_step / bdn_lars_step,
        rebuilt and uploaded when the groups object or adapt_1d changed (set_param_groups, a loaded state), never per step.  trust_out
        is `last_trust`."""
        pg = self._layerwise_groups()
        if self._lw is None or self._lw[0] is not pg or self._lw[5] != self.optim.adapt_1d:
            dev = self.flat_params.device
            n_ten = len(self.layout.order)
            table = tuple(t.to(dev) for t in _optim.tensor_table(self.layout, pg, self.optim.adapt_1d))
            ws = torch.empty(_lib.load().bdn_layerwise_workspace_bytes(self.layout.total, n_ten) // 8, dtype=torch.float64, device=dev)
            self.last_trust = torch.zeros(n_ten, 3, dtype=torch.float32, device=dev)
            self._lw = (pg, table, n_ten, ws, self.last_trust, self.optim.adapt_1d)
        return self._lw

    def trust_ratios(self, adapted_only=False):
        """{parameter name: the trust ratio applied at the last update} for every trainable parameter (1.0 where the rule does not adapt:
        ndim <= 1 without adapt_1d, a zero norm); adapted_only: only the tensors whose adapt flag is set.  One host read of
        `last_trust`, on demand only; empty before the first update."""
        if self.optim.kind not in _optim.LAYERWISE:
            raise RuntimeError(f'trust_ratios(): optimizer {self.optim.kind!r} has no trust ratios (lamb and lars do)')
        if self.opt_step == 0 or self.last_trust is None:
            return {}
        dev = self.flat_params.device
        torch.cuda.current_stream(dev).wait_stream(self.stream(dev))
        pg = self._layerwise_table()[0]
        r = self.last_trust[:, 2].tolist()
        every = not adapted_only or self.optim.adapt_1d
        return {k: r[i] for i, k in enumerate(self.layout.order)
                if pg.group_id(k) != _optim.FROZEN and (every or len(self.layout.slices[k][2]) > 1)}

    def _init_average(self, rebind=False):
        """flat_avg (a clone of flat_params), and with ema_buffers the averaged running statistics: views of one flat buffer, a scratch
        copy of it for the exchange, and the two descriptor tables of bdn_ema_update_multi ({average <- live}, {live <- scratch}).
        rebind: the live buffers moved (_rebind): only the two tables are rebuilt, every average keeps its value."""
        import struct
        dev = self.flat_params.device
        if not rebind:
            self.flat_avg = self.flat_params.clone()
        if not self.ema_buffers:
            return
        keys = [k for k in self._P if k.endswith(('.running_mean', '.running_var'))]
        if not keys:
            return
        offs, total = {}, 0
        for k in keys:
            offs[k] = total
            total += (self._P[k].numel() + 3) // 4 * 4            # every view starts on a float4
        if rebind and self._avg_desc is not None:
            flat, tmp = self._avg_desc[4], self._avg_desc[5]
        else:
            rebind = False
            flat = torch.zeros(total, dtype=torch.float32, device=dev)
            tmp = torch.empty_like(flat)
        upd = back = b''
        for k in keys:
            live = self._P[k]
            if live.dtype != torch.float32 or not live.is_contiguous():
                raise RuntimeError(f'fabric_amd: BatchNorm buffer {k} must be contiguous float32')
            n = live.numel()
            v = flat[offs[k]:offs[k] + n].view(live.shape)
            if not rebind:
                v.copy_(live)
            self.avg_buffers[k] = v
            upd += struct.pack('<QQii', v.data_ptr(), live.data_ptr(), n, 0)
            back += struct.pack('<QQii', live.data_ptr(), tmp.data_ptr() + 4 * offs[k], n, 0)
        up = lambda rec: torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev)
        self._avg_desc = (up(upd), up(back), len(keys), max(self._P[k].numel() for k in keys), flat, tmp)

    def _table(self):
        """(seg_end, seg_group, n_seg) device addresses of the step's segment table for the averaging kernels; n_seg = 0 without groups
        or frozen parameters: every vector counts."""
        if self._groups is None:
            return None, None, 0
        ends, ids, n_seg = self._seg
        return ends.data_ptr(), ids.data_ptr(), n_seg

    def _average(self, st):
        """Count one optimizer update and, when it is due, fold the new parameters (and running statistics) into the average on `st`."""
        if self.flat_avg is None or self._ema_hold:
            return
        self._updates += 1
        u = self._updates - self.ema_start
        if u <= 0 or u % self.ema_every:
            return
        copy = int(self.n_averaged == 0)
        w = 0.0 if copy else _optim.average_weight(self.average, self.ema_decay, self.n_averaged)
        _lib.call('bdn_ema_update', self.flat_avg.data_ptr(), self.flat_params.data_ptr(), *self._table(), w, copy, self.layout.total, st)
        if self._avg_desc is not None:
            _lib.call('bdn_ema_update_multi', self._avg_desc[0].data_ptr(), self._avg_desc[2], self._avg_desc[3], w, copy, st)
        self.n_averaged += 1

    def _need_average(self, what):
        if self.flat_avg is None:
            raise RuntimeError(f"{what}: this step keeps no averaged weights (build it with ema_decay=... or average='swa')")

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f'{what}: not inside `with step.ema_weights()`, where the live and the averaged weights are exchanged')

    def _no_pending(self, what):
        if self.micro != 0:
            raise RuntimeError(f'{what}: {self.micro} of {self.accumulate} micro-steps are pending; call flush() (or flush(apply=False)) first')

    def set_param_groups(self, groups):
        """Install parameter groups (the constructor's `param_groups`) and re-read every parameter's requires_grad flag: rebuilds and
        uploads the segment table of the grouped update kernels.  groups=None: one group of every trainable parameter with the step's lr
        and weight_decay (`step.lr` keeps driving it); with nothing frozen either, the step returns to the ungrouped kernels.  The
        optimizer state of parameters that stay trainable is kept; that of a parameter frozen now is zeroed, so it starts afresh if it
        is released later (with the step's one update count).  Raises ValueError as fabric_amd.optim.ParamGroups does."""
        self._no_pending('set_param_groups()')
        self._not_swapped('set_param_groups()')
        dev = self.flat_params.device
        pg = self._checked_groups(groups)
        hp, cur = self.stream(dev), torch.cuda.current_stream(dev)
        cur.wait_stream(hp)                                  # a step in flight still reads the old table and writes state and gradients
        if pg is None:
            self.param_groups = self._groups = self._seg = self._need = None
            self._implicit_group = False
            if self.optim.kind in _optim.LAYERWISE:
                self._layerwise_table()
            if self.sam_rho is not None:
                self._sam_table()
            return
        ends, ids = _optim.segment_table(self.layout, pg)
        seg = (torch.tensor(ends, dtype=torch.int64).to(torch.int32).to(dev), torch.tensor(ids, dtype=torch.int32).to(dev), len(ends))
        frozen = pg.frozen
        for k in frozen:                                     # zero-filled once: reduced as zeros, and no stale state if released later
            self.grads[k].zero_()
            for t in self.opt_state.values():
                self.layout.view(t, k).zero_()
            if self.flat_avg is not None:
                # a frozen tensor's average is its value: the exchange of ema_weights() skips frozen vectors, so an average left behind
                # its (now constant) tensor would make the model inside the block differ from ema_state_dict(); the value is also what
                # an average of the constant converges to
                self.layout.view(self.flat_avg, k).copy_(self.layout.view(self.flat_params, k))
        hp.wait_stream(cur)
        self._groups, self._seg = pg, seg
        self.param_groups = pg.groups
        self._implicit_group = groups is None
        self._need = set(pg.trainable()) if frozen else None
        if self.optim.kind in _optim.LAYERWISE:
            self._layerwise_table()
        if self.sam_rho is not None:
            self._sam_table()

    def _checked_groups(self, groups):
        """fabric_amd.optim.ParamGroups of `groups` (names or nn.Parameter objects) and the parameters' requires_grad flags as they are
        now; None when no groups are given and nothing is frozen."""
        frozen = {k for k, p in self.model.named_parameters() if not p.requires_grad}
        if groups is None:
            return _optim.ParamGroups(self.optim, self._names, None, frozen) if frozen else None

        def name_of(q):
            k = q if isinstance(q, str) else self._by_id.get(id(q))
            if k is None:
                raise ValueError('param group lists a tensor that is not a parameter of the model')
            return k
        return _optim.ParamGroups(self.optim, self._names, [dict(g, params=[name_of(q) for q in g['params']]) for g in groups], frozen)

    def _state(self):
        return self._P

    def _bindings(self):
        """(owning dict, attribute, state-dict key, device address) of every parameter and buffer of the module as the step bound it: the
        flat buffers, `_P` and the descriptor tables all hold these addresses."""
        out = []
        for prefix, mod in self.model.named_modules():
            for d in (mod._parameters, mod._buffers):
                out += [(d, name, f'{prefix}.{name}' if prefix else name, t.data_ptr()) for name, t in d.items() if t is not None]
        return out

    def _check_bound(self):
        """The step trains flat_params through aliases built once.  When a parameter or buffer of the module was re-pointed since
        (load_state_dict(assign=True), p.data = t, a second TrainStep built on the same module) the module is the truth: the step
        binds it again (_rebind) and goes on exactly as a step built on the module as it now is, with the optimizer state and
        averages it has.  Host-side address comparisons only: no device synchronisation."""
        for d, name, key, addr in self._bound:
            t = d.get(name)
            if t is None or t.data_ptr() != addr:
                return self._rebind(key)

    def _rebind(self, key):
        """Take the module's tensors over again, as the constructor did: the values of every re-pointed parameter are copied into
        its view of flat_params and p.data / p.grad are pointed back at the flat buffers; re-pointed buffers are adopted where they
        are.  The aliases `_P`, the averaging tables (which hold buffer addresses) and the engine's packed images are re-derived.
        Raises RuntimeError naming `key` when the module can no longer be bound: other parameter names or shapes, another device."""
        dev = self.flat_params.device
        named = list(self.model.named_parameters())
        state = self.model.state_dict(keep_vars=True)
        if [k for k, _ in named] != self._names or any(tuple(p.shape) != tuple(self.layout.slices[k][2]) for k, p in named) \
                or any(t.device != dev for t in state.values()):
            raise RuntimeError(f'fabric_amd: {key} was re-pointed at other storage after this TrainStep was built and the module no '
                               f'longer fits the step (a device move, or other parameter names or shapes): build a new TrainStep')
        hp, cur = self.stream(dev), torch.cuda.current_stream(dev)
        cur.wait_stream(hp)                                  # a step in flight still reads and writes the flat buffers
        for k, p in named:
            v = self.layout.view(self.flat_params, k)
            if p.data_ptr() != v.data_ptr():
                v.copy_(p.data)
                p.data = v
            p.grad = self.layout.view(self.flat_grads, k)
        hp.wait_stream(cur)
        self._by_id = {id(p): k for k, p in named}
        self._P = {k: v.detach() for k, v in self.model.state_dict(keep_vars=True).items()}
        if self.flat_avg is not None:
            self._init_average(rebind=True)
        self.model.engine().invalidate_weights()
        self._bound = self._bindings()

    def step(self, x_d1, x_d2, labels, weights=None):
        """One optimisation step.  Returns the loss as a fresh 0-dim device tensor (no sync; safe to keep in a list like
        the reference loop does with `cd_loss`).  `last_counts` / `last_logits` are persistent buffers that the NEXT step
        overwrites: clone them if they have to outlive it.

        The step's dependency chain (forward, loss, dz chain, SGD) is enqueued on a HIGH-priority HIP stream; the
        weight-gradient GEMMs run beside it on a normal-priority stream (engine.backward), so the chain's kernels get
        compute units first (A/B tools/archive/ab_prio.py: -0.8 % step time).  The caller's current stream is joined on both
        sides, so the usual stream semantics hold for inputs and outputs.

        Soft targets (bdn_criterion_soft; fabric_amd.criterion's module docstring), with a Criterion only: `weights`, float32 [B,H,W] pixel
        weights, and / or float32 [B,C,H,W] `labels`, taken as per-pixel target distributions; a Criterion with label_smoothing takes that
        route with plain labels.  Nothing else in the step changes -- accumulation, SAM (both passes see the same targets and weights),
        clipping, averaging, frozen BatchNorm, parameter groups and data-parallel runs sit behind dlogits; data-parallel, each rank
        normalises by its own valid count.  `last_counts` has five entries, {TP, FP, FN, correct, valid}, `last_terms` its usual length."""
        self._not_swapped('step()')
        self._check_bound()
        if self.criterion is None and (weights is not None or (labels.is_floating_point() and labels.dim() == 4 and labels.shape[1] > 1)):
            raise ValueError('the default step (criterion=None, bdn_tversky) takes class-index labels only: give TrainStep a criterion, '
                             "e.g. criterion='tversky', to train on weights or float targets")
        self._weights = weights
        try:
            return self._step_streams(x_d1, x_d2, labels)
        finally:
            self._weights = None

    def _step_streams(self, x_d1, x_d2, labels):
        if self._guard and self.collectives_report is None and self.bucketer.active():
            # measure only: the caller may already run its loop on step.stream(), which must not be swapped under it
            self.guard_collectives(*[int(v) for v in (x_d1.shape[0], x_d1.shape[2], x_d1.shape[3])], replace_streams=False)
        if not self.high_priority_chain:
            return self._step(x_d1, x_d2, labels)
        cur = torch.cuda.current_stream(x_d1.device)
        hp = self.stream(x_d1.device)
        if cur.cuda_stream == hp.cuda_stream:              # the caller already runs its loop on the step's stream: no joins
            return self._step(x_d1, x_d2, labels)
        self._hp.wait_stream(cur)
        with torch.cuda.stream(self._hp):
            loss = self._step(x_d1, x_d2, labels)
        cur.wait_stream(self._hp)
        for t in (loss, self.last_logits, self.last_counts, self.last_terms, self.last_dlogits, self.last_grad_norm, self.last_sam_loss,
                  self.last_sam_norm):
            if t is not None:
                t.record_stream(cur)                          # (last_clip_coef shares last_grad_norm's buffer, last_sam_scale last_sam_norm's)
        return loss

    def flush(self, apply=True):
        """End an incomplete accumulation.  With m = `micro` > 0 pending micro-steps and apply=True: flat_grads = the pending sum, one
        set of bucket all-reduces, the norm if clipping is on, and the update with the mean of the m gradients (grad_scale =
        1 / (world * m)); returns True.  apply=False drops the pending gradients (returns False).  With nothing pending nothing is
        launched and False is returned.  Every rank must call it alike (it issues collectives)."""
        self._not_swapped('flush()')
        m = self.micro
        if m == 0:
            return False
        if not apply:
            self.micro = 0
            return False
        self._check_bound()
        dev = self.flat_params.device

        def run():
            st = _lib.stream_ptr()
            _lib.call('bdn_grad_accumulate', self.flat_grads.data_ptr(), self.flat_accum.data_ptr(), self.layout.total, 0, st)
            self.micro = 0
            self.bucketer.finish()
            self._apply(st, 1.0 / (self.world * m))
            self.model.engine().invalidate_weights()
        cur, hp = torch.cuda.current_stream(dev), self.stream(dev)
        if not self.high_priority_chain or cur.cuda_stream == hp.cuda_stream:
            run()
            return True
        hp.wait_stream(cur)
        with torch.cuda.stream(hp):
            run()
        cur.wait_stream(hp)
        if self.last_grad_norm is not None:
            self.last_grad_norm.record_stream(cur)
        return True

    def stream(self, device=None):
        """The high-priority stream the step's chain runs on: the process-wide 'chain' stream of the device (fabric_amd/streams.py;
        every TrainStep shares it, so the N-th instance of a process is as fast as the first).  A training loop that makes it
        the current stream (``with torch.cuda.stream(step.stream()): ...``) saves the two cross-stream joins per step
        (~25 us of idle GPU)."""
        from . import streams
        self._hp = streams.get('chain', device if device is not None else self.flat_params.device)      # not cached: streams.replace() may swap it
        return self._hp

    # ------------------------------------------------------------------ run-time guard for the collectives' stream placement
    def _time_steps(self, x1, x2, lbl, n, warm):
        import time
        dev = x1.device
        with torch.cuda.stream(self.stream(dev)):
            for _ in range(warm):
                self._step(x1, x2, lbl)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                self._step(x1, x2, lbl)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / n

    def _time_exchange(self, n):
        """Seconds per step of the bucket all-reduces ALONE: issued back to back from the chain's stream on an otherwise idle device
        (max over ranks).  The gradients are overwritten by the next backward anyway."""
        import time
        dev = self.flat_params.device
        b = self.bucketer
        with torch.cuda.stream(self.stream(dev)):
            for it in range(n + 2):
                if it == 2:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                works = [dist.all_reduce(b.flat[a:e], op=dist.ReduceOp.SUM, group=self.group, async_op=True) for a, e, _ in b.buckets]
                for w in works:
                    w.wait()
            torch.cuda.synchronize(dev)
            t = torch.tensor([(time.perf_counter() - t0) / n], dtype=torch.float64, device=dev)
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return float(t[0])

    def guard_collectives(self, B, H, W, steps=8, threshold=0.05, verbose=False, replace_streams=True):
        """Is the step slowed down by WHERE its collectives run?  RCCL's collective stream is created by torch, not by this library,
        and its hardware-queue placement relative to the chain / weight-gradient streams depends on creation order, priority and
        GPU_MAX_HW_QUEUES: one combination measured +48...+59 % step time, invisible to a sleep-kernel probe.
        So it is MEASURED, on synthetic inputs of the run's shape, `steps` steps each:

          local      the step without its collectives,
          overlap    the bucket all-reduces launched from backward (the intended arrangement),
          exchange   (only if overlap costs more than `threshold`) the five bucket all-reduces ALONE on an otherwise idle device: what
                     the exchange itself costs (xGMI transfer, RCCL's kernels) when nothing hides it.

        overlap <= local + 1.1 exchange + 2 % means the overhead is explained by the exchange even if none of it were hidden: the
        arrangement is fine, nothing is changed and nothing is warned about, however large it is (a slow interconnect is not a stream
        problem).  Anything beyond that is interference, i.e. a placement problem, and the remedies are tried in order -- (1) a new
        weight-gradient stream, (2) a new chain stream, each measured in the overlap arrangement, then (3) the buckets launched from
        the chain's stream after backward (bucketer.defer) on the best streams found.  (Deferring is a remedy, not a reference: with
        the collective stream on the chain's hardware queue it measured as slow as overlapping.)  Afterwards the arrangement that
        measured BEST is the one restored -- streams.restore() puts a displaced stream back -- and the report's `overhead_frac` is
        the number measured on exactly that arrangement.  With several ranks every decision is taken on the MAX
        over ranks, so all ranks walk the same path.  Parameters, BatchNorm buffers, the optimizer state (and its step count) and the
        bucketer state are restored.

        replace_streams=False (what the automatic call inside the first step() uses): the stream remedies are skipped -- a caller that
        already runs its loop on step.stream() must not have that stream swapped under it -- and only deferring is available.
        Call this method yourself BEFORE `with torch.cuda.stream(step.stream())` to get the full repair (train.py and bench.py do)."""
        import warnings
        from . import streams
        dev = self.flat_params.device
        if not self.bucketer.active():
            self.collectives_report = {'active': False}
            return self.collectives_report
        backend = str(dist.get_backend(self.group))
        if 'nccl' not in backend:                                       # gloo (tests on one GPU / CPU): reductions run on the host, no collective stream
            self.collectives_report = {'active': True, 'guarded': False, 'reason': f'backend {backend}: no device-side collective stream'}
            return self.collectives_report
        self.collectives_report = {'running': True}                     # re-entrancy: _step below must not call the guard again
        ok = False
        eng = self.model.engine()
        saved = saved_flat = saved_opt = saved_acc = None
        tried = []
        from . import streams as _streams
        orig_streams = (_streams.get('chain', dev), _streams.get('wgrad', dev))     # put back if a measurement raises half-way
        try:
            g = torch.Generator(device='cpu').manual_seed(99)
            C = self.model.n_channels
            x1 = torch.randn(B, C, H, W, generator=g).to(dev)
            x2 = (x1 + 0.3 * torch.randn(B, C, H, W, generator=g).to(dev))
            lbl = (torch.rand(B, H, W, generator=g) < 0.1).to(torch.uint8).to(dev)
            saved = {k: v.clone() for k, v in self._P.items()}
            saved_flat = self.flat_params.clone()
            saved_opt = ({k: v.clone() for k, v in self.opt_state.items()}, self.opt_step)
            # every timed step exchanges: accumulation is switched to 1 for the measurement and put back with what it had pending
            saved_acc = (self.accumulate, self.micro, None if self.flat_accum is None else self.flat_accum.clone(),
                         None if self._norm is None else self._norm[1].clone())
            self.accumulate, self.micro = 1, 0
            self._ema_hold = True                                       # the timed steps are not updates of the run: not averaged

            def timed(collectives, defer=False):
                self.bucketer.enabled, self.bucketer.defer = collectives, defer
                # inputs and the saved copies were produced on the caller's stream: the chain stream (possibly a new one) joins it first
                self.stream(dev).wait_stream(torch.cuda.current_stream(dev))
                t = torch.tensor([self._time_steps(x1, x2, lbl, steps, 3)], dtype=torch.float64, device=dev)
                if self.world > 1:
                    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
                return float(t[0])

            def measure(name):
                t_local = timed(False)
                t_ov = timed(True)
                rec = {'arrangement': name, 'local_ms': t_local * 1e3, 'overlap_ms': t_ov * 1e3, 'overhead_frac': t_ov / t_local - 1.0,
                       'streams': (streams.get('chain', dev), streams.get('wgrad', dev))}
                tried.append(rec)
                if verbose:
                    print(f'guard_collectives: {name}: overlap overhead {rec["overhead_frac"] * 100:+.1f} %', flush=True)
                return rec

            first = measure('original')
            kept, placement, t_ex = first, None, None
            if first['overhead_frac'] > threshold:
                t_ex = self._time_exchange(steps)
                first['exchange_alone_ms'] = t_ex * 1e3
                explained = first['local_ms'] * 1.02 + 1.1 * t_ex * 1e3
                placement = first['overlap_ms'] > explained               # more than the fully exposed exchange would cost: interference
                if placement and replace_streams:
                    for remedy in ('new_wgrad_stream', 'new_chain_stream'):
                        if kept['overhead_frac'] <= threshold:
                            break
                        streams.replace('wgrad' if remedy == 'new_wgrad_stream' else 'chain', dev)
                        rec = measure(remedy)
                        if rec['overhead_frac'] < kept['overhead_frac']:
                            kept = rec
                # back to the best overlap arrangement found; if that is still a placement problem, try deferring ON it
                streams.restore('chain', kept['streams'][0], dev)
                streams.restore('wgrad', kept['streams'][1], dev)
                if placement and kept['overlap_ms'] > explained:
                    t_def = timed(True, defer=True)
                    kept['deferred_ms'] = t_def * 1e3
                    if t_def * 1e3 < kept['overlap_ms']:
                        kept = dict(kept, arrangement=kept['arrangement'] + ' + deferred_buckets', deferred=True,
                                    overhead_frac=t_def * 1e3 / kept['local_ms'] - 1.0)
            self.bucketer.defer = bool(kept.get('deferred'))
            rep = {'active': True, 'threshold': threshold, 'steps': steps, 'world': self.world,
                   'tried': [{k: v for k, v in r.items() if k != 'streams'} for r in tried],
                   'kept': kept['arrangement'], 'overhead_frac': kept['overhead_frac'], 'deferred_buckets': bool(kept.get('deferred')),
                   'placement_problem': placement, 'stream_remedies_allowed': bool(replace_streams),
                   'recovered': bool(placement) and kept is not first}
            still_bad = bool(placement) and kept['overhead_frac'] > threshold and \
                (kept['deferred_ms'] if kept.get('deferred') else kept['overlap_ms']) > kept['local_ms'] * 1.02 + 1.1 * t_ex * 1e3
            rep['ok'] = not still_bad
            rep['exchange_alone_ms'] = None if t_ex is None else t_ex * 1e3
            if still_bad:
                hint = ('' if replace_streams else '  The stream remedies were skipped because the guard ran inside step(): call '
                        'step.guard_collectives(B, H, W) before adopting step.stream().')
                warnings.warn(f'fabric_amd: launching the gradient all-reduces from backward costs the step {first["overhead_frac"] * 100:+.0f} % '
                              f'here, more than the exchange alone ({t_ex * 1e3:.2f} ms) explains -- a stream-placement problem; kept: {kept["arrangement"]} '
                              f'({kept["overhead_frac"] * 100:+.0f} %, threshold {threshold * 100:.0f} %).{hint}  Creating the process group BEFORE the '
                              f'first TrainStep, the default collective-stream priority and the default GPU_MAX_HW_QUEUES avoid it.', RuntimeWarning)
            ok = True
        finally:
            self.bucketer.enabled = True
            self._ema_hold = False
            if not ok:
                self.bucketer.defer = False
                # a measurement raised (OOM, RCCL error) while a remedy's stream was in place: back to the arrangement the guard started
                # from -- the next guard must not start from a half-tried one (displaced streams are retired by restore, not leaked)
                _streams.restore('chain', orig_streams[0], dev)
                _streams.restore('wgrad', orig_streams[1], dev)
            self.bucketer.reset()
            torch.cuda.synchronize(dev)                    # chain-stream steps may still be in flight (exception path): restore after them
            if saved is not None and saved_flat is not None:
                for k, v in saved.items():
                    self._P[k].copy_(v)
                self.flat_params.copy_(saved_flat)
            if saved_opt is not None:
                for k, v in saved_opt[0].items():
                    self.opt_state[k].copy_(v)
                self.opt_step = saved_opt[1]
            if saved_acc is not None:
                self.accumulate, self.micro = saved_acc[0], saved_acc[1]
                if saved_acc[2] is not None:
                    self.flat_accum.copy_(saved_acc[2])
                if saved_acc[3] is not None:
                    self._norm[1].copy_(saved_acc[3])
            eng.invalidate_weights()
            torch.cuda.synchronize(dev)
            if not ok:
                self.collectives_report = None             # a failed guard has measured nothing: the next call starts over
        self.collectives_report = rep
        return rep

    def _step(self, x_d1, x_d2, labels):
        if self.sam_rho is None:
            return self._pass(x_d1, x_d2, labels)
        # ---- sharpness-aware: the gradient at w, w -> w + e, the step's usual pass there, w back, the update at w
        eng = self.model.engine()
        st = _lib.stream_ptr()
        loss, counts = self._pass(x_d1, x_d2, labels, sam=1)
        # pass 1's loss, counts and terms, copied on the device: pass 2 reuses the criterion's buffers
        loss, counts = loss.clone(), counts.clone()
        terms = None if self.last_terms is None else self.last_terms.clone()
        _, (ends, lens, ids), n_ten, ws, out = self._sam_table()
        # issued where the update is, behind backward's joined streams: backward reads parameters directly (the classifier, BatchNorm
        # weight and bias, the conv biases, the first layer's master weight)
        _lib.call('bdn_sam_perturb', self.flat_params.data_ptr(), self.flat_sam.data_ptr(), self.flat_grads.data_ptr(), ends.data_ptr(),
                  lens.data_ptr(), ids.data_ptr(), n_ten, self.sam_rho, int(self.sam_adaptive), self.sam_eps, ws.data_ptr(),
                  out.data_ptr(), self.layout.total, st)
        self._sam_pending = True
        eng.invalidate_weights()                              # the packed images hold w, the parameters w + e
        try:
            self.last_sam_loss = self._pass(x_d1, x_d2, labels, sam=2)
        finally:
            if self._sam_pending:                             # pass 2 raised before its restore: the model must not keep w + e
                self._sam_restore(st)
        self.last_counts, self.last_terms = counts, terms
        return loss

    def _sam_restore(self, st):
        """w back from flat_sam, bit for bit, behind pass 2's backward (the ordering rule of the perturbation), and the packed images
        of w + e marked stale."""
        _, (ends, _, ids), n_ten, _, _ = self._sam_table()
        _lib.call('bdn_sam_restore', self.flat_params.data_ptr(), self.flat_sam.data_ptr(), ends.data_ptr(), ids.data_ptr(), n_ten,
                  self.layout.total, st)
        self._sam_pending = False
        self.model.engine().invalidate_weights()

    def _pass(self, x_d1, x_d2, labels, sam=0):
        """Forward, criterion, backward and what follows them.  sam=0: the whole step.  sam=1, the first pass of a sharpness-aware step:
        no collective, no accumulation, no update; returns the criterion's (loss, counts) buffers.  sam=2, its second pass: the whole
        step on batch statistics that move no running statistics, with the restore between backward and the update."""
        model = self.model
        eng = model.engine()
        P = self._state()
        frozen_bn = self.bn == 'frozen'
        if self.flat_grads._version != self._grads_version:   # somebody wrote p.grad since the last step (host-side check, no launch otherwise)
            skip = self._groups.frozen if self._groups is not None else ()
            for k, g in self._zero_tail:
                if k not in skip:                             # a frozen tensor's gradient has no reader: left as it is
                    g.zero_()
            self._grads_version = self.flat_grads._version
        if frozen_bn:                                         # the training-layout forward on the running statistics, as an eval-mode
            from .models.bidate_model import _Lease           # autograd graph recomputes it (_BiDateFunction.backward)
            logits, ws = eng.forward(x_d1, x_d2, P, training=False, frozen=True)
            lease = _Lease(ws)
        else:
            logits, ws = eng.forward(x_d1, x_d2, P, training=True, **({'track_running': False} if sam == 2 else {}))
        st = _lib.stream_ptr()
        if self.criterion is not None:
            loss, counts, dlogits = self._criterion_loss(logits, labels)
        else:
            loss, counts, dlogits = self._tversky_loss(logits, labels, st)
        pending = self.micro                                  # micro-steps already in flat_accum
        closing = pending + 1 >= self.accumulate              # this call ends with the update (always, without accumulation)
        on_ready = self.bucketer.on_ready if closing and sam != 1 else None
        self._adding = pending > 0 and sam != 1               # closing: the buckets take the pending sum in right before their all-reduce
        try:
            if frozen_bn:
                try:
                    eng.backward(ws, dlogits, P, self.grads, on_ready=on_ready, zero_bias_grads=False, bn_mode='running', need=self._need)
                finally:
                    lease.release()
                    if eng.x3:
                        ws.release_split()
            else:
                eng.backward(ws, dlogits, P, self.grads, on_ready=on_ready, zero_bias_grads=False, need=self._need)
            if sam == 1:
                return loss, counts
            if sam == 2:                                      # backward has joined its streams: nothing reads the parameters any more
                self._sam_restore(st)
            self.last_counts = counts
            self.last_logits = logits
            if not closing:                                   # acc = g1, then acc += g: no collective, no update; the packed weights stay valid,
                                                              # except under SAM, whose perturbation and restore have each made them stale
                _lib.call('bdn_grad_accumulate', self.flat_accum.data_ptr(), self.flat_grads.data_ptr(), self.layout.total, int(pending > 0), st)
                self.micro = pending + 1
                self._grads_version = self.flat_grads._version
                return loss.clone()
            if pending:                                       # flat_grads = gK + acc
                if self.bucketer.active():
                    self._add_pending(self.bucketer.reduce_end, self.layout.total)       # the tail that is not exchanged
                else:
                    self._add_pending(0, self.layout.total)
            self.bucketer.finish()
        finally:
            self._adding = False
        self.micro = 0
        self._apply(st, 1.0 / (self.world * (pending + 1)))
        eng.invalidate_weights()                              # packed bf16/f32 GEMM images are now stale
        self._grads_version = self.flat_grads._version        # whatever the step itself moved it by (the buckets' all-reduces)
        return loss.clone()

    def _add_pending(self, a, b):
        """flat_grads[a:b] += flat_accum[a:b] on the current stream (GradBucketer.before_reduce: a bucket, right before its all-reduce)."""
        if self._adding and b > a:
            _lib.call('bdn_grad_accumulate', self.flat_grads.data_ptr() + 4 * a, self.flat_accum.data_ptr() + 4 * a, b - a, 1,
                      _lib.stream_ptr())

    def _apply(self, st, grad_scale):
        """The norm (when clipping is on), the update with g = grad_scale * flat_grads, and the averaging update when one is due."""
        if self._norm is None:
            self._update(st, grad_scale)
            return self._average(st)
        ws, out = self._norm
        pg, (ends, ids, n_seg) = (self._groups, self._seg) if self._groups is not None else self._implicit_table()
        _lib.call('bdn_grad_norm', self.flat_grads.data_ptr(), ends.data_ptr(), ids.data_ptr(), n_seg, grad_scale, self.max_grad_norm,
                  ws.data_ptr(), out.data_ptr(), self.layout.total, st)
        self._update_grouped(st, grad_scale, out.data_ptr() + 4)
        self._average(st)

    def _tversky_loss(self, logits, labels, st):
        """The default criterion: bdn_tversky on persistent buffers -> (loss, counts, dlogits)."""
        B, C, H, W = logits.shape
        dev = logits.device
        if self._tv is None or self._tv[3] != (B, C, H, W):
            n = _lib.load().bdn_overlap_workspace_bytes(B, C, H, W, 0) // 4
            self._tv = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty((), dtype=torch.float32, device=dev),
                        torch.empty(4, dtype=torch.int32, device=dev), (B, C, H, W))
        tvws, loss, counts, _ = self._tv
        if labels.dtype != torch.uint8:
            labels = labels.to(torch.uint8)
        labels = labels.contiguous()
        dlogits = torch.empty_like(logits)
        _lib.call('bdn_tversky', logits.data_ptr(), labels.data_ptr(), float(self.alpha), float(self.beta),
                  float(self.eps), tvws.data_ptr(), loss.data_ptr(), counts.data_ptr(), dlogits.data_ptr(), B, C, H, W, st)
        return loss, counts, dlogits

    def _criterion_loss(self, logits, labels):
        """An explicit criterion: bdn_criterion on persistent buffers sized once per shape -> (loss, counts, dlogits); sets last_terms
        and last_dlogits (the gradient this step's backward starts from)."""
        shape = tuple(logits.shape)
        weights = self._weights
        if weights is None and not (labels.is_floating_point() and tuple(labels.shape) == shape):
            # the step as it always was (a criterion with label_smoothing: its buffers() are the soft route's)
            if self._tv is None or self._tv[1] != shape:
                self._tv = (self.criterion.buffers(shape, logits.device), shape)
            loss, terms, counts, dlogits = self.criterion.evaluate(logits, labels, out=self._tv[0])
        else:                                                                  # weights / float targets: the soft route's buffers, kept apart
            if self._tv_soft is None or self._tv_soft[1] != shape:
                self._tv_soft = (self.criterion.buffers(shape, logits.device, soft=True), shape)
            loss, terms, counts, dlogits = self.criterion.evaluate(logits, labels, out=self._tv_soft[0], weights=weights)
        self.last_terms, self.last_dlogits = terms, dlogits
        return loss, counts, dlogits

    def _update(self, st, grad_scale):
        """The optimizer update on stream `st` with g = grad_scale * (sum of rank gradients), grad_scale = 1 / world (times 1 / the number
        of accumulated micro-steps): per-rank loss, averaged gradients (standard DDP).  Host-side scalars only: the step
        count is a Python int, nothing syncs."""
        o, n = self.optim, self.layout.total
        if o.kind in _optim.LAYERWISE:
            return self._update_layerwise(st, grad_scale)
        if self._groups is not None:
            return self._update_grouped(st, grad_scale)
        if o.plain:                                          # p -= lr * g: the reference's optim.SGD(lr)
            _lib.call('bdn_sgd_step', self.flat_params.data_ptr(), self.flat_grads.data_ptr(), float(self.lr), grad_scale, n, st)
            return
        first = self.opt_step == 0
        self.opt_step += 1
        if o.kind == 'sgd':
            buf = self.opt_state.get('momentum_buffer')
            _lib.call('bdn_sgd_momentum_step', self.flat_params.data_ptr(), self.flat_grads.data_ptr(), _lib.ptr(buf), float(self.lr),
                      grad_scale, o.momentum, o.dampening, o.weight_decay, int(o.nesterov), int(first), n, st)
        else:
            _lib.call('bdn_adam_step', self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.opt_state['exp_avg'].data_ptr(),
                      self.opt_state['exp_avg_sq'].data_ptr(), float(self.lr), grad_scale, o.betas[0], o.betas[1], o.eps,
                      o.weight_decay, int(o.kind == 'adamw'), self.opt_step, n, st)

    def _update_grouped(self, st, grad_scale, dev_scale=None):
        """_update through bdn_*_step_grouped: per-group lr / weight_decay read from `param_groups` now, frozen segments skipped.
        dev_scale: None, or the device address of the clip coefficient: the _ex entry points, g = (grad_scale * coefficient) * grad."""
        o, n = self.optim, self.layout.total
        if o.kind in _optim.LAYERWISE:
            return self._update_layerwise(st, grad_scale, dev_scale)
        if self._groups is not None:
            pg, seg = self._groups, self._seg
            if self._implicit_group:
                pg.groups[0]['lr'] = float(self.lr)
        else:                                                # clipping without groups: the one implicit group follows the step's values
            pg, seg = self._implicit_table()
            pg.groups[0]['lr'], pg.groups[0]['weight_decay'] = float(self.lr), o.weight_decay
        lrs, wds = pg.hyper('lr'), pg.hyper('weight_decay')
        ends, ids, n_seg = seg
        table = (ends.data_ptr(), ids.data_ptr(), n_seg, len(lrs))
        lr, wd = _lib.floats(lrs), _lib.floats(wds)
        ex, ds = ('', ()) if dev_scale is None else ('_ex', (dev_scale,))
        if o.kind == 'sgd' and o.momentum == 0 and not any(wds):
            _lib.call('bdn_sgd_step_grouped' + ex, self.flat_params.data_ptr(), self.flat_grads.data_ptr(), *table, lr, grad_scale, *ds, n, st)
            return
        first = self.opt_step == 0
        self.opt_step += 1
        if o.kind == 'sgd':
            _lib.call('bdn_sgd_momentum_step_grouped' + ex, self.flat_params.data_ptr(), self.flat_grads.data_ptr(),
                      _lib.ptr(self.opt_state.get('momentum_buffer')), *table, lr, wd, grad_scale, *ds, o.momentum, o.dampening,
                      int(o.nesterov), int(first), n, st)
        else:
            _lib.call('bdn_adam_step_grouped' + ex, self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.opt_state['exp_avg'].data_ptr(),
                      self.opt_state['exp_avg_sq'].data_ptr(), *table, lr, wd, grad_scale, *ds, o.betas[0], o.betas[1], o.eps,
                      int(o.kind == 'adamw'), self.opt_step, n, st)

    def _update_layerwise(self, st, grad_scale, dev_scale=None):
        """_update through bdn_lamb_step / bdn_lars_step: always on the per-tensor table, per-group lr / weight_decay read now, the
        clip coefficient (dev_scale, or None) multiplied in on the device."""
        o, n = self.optim, self.layout.total
        pg, (ends, lens, ids, adapt), n_ten, ws, trust, _ = self._layerwise_table()
        lrs, wds = pg.hyper('lr'), pg.hyper('weight_decay')
        table = (ends.data_ptr(), lens.data_ptr(), ids.data_ptr(), adapt.data_ptr(), n_ten, len(lrs))
        lr, wd = _lib.floats(lrs), _lib.floats(wds)
        first = self.opt_step == 0
        self.opt_step += 1
        if o.kind == 'lamb':
            _lib.call('bdn_lamb_step', self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.opt_state['exp_avg'].data_ptr(),
                      self.opt_state['exp_avg_sq'].data_ptr(), *table, lr, wd, grad_scale, dev_scale, o.betas[0], o.betas[1], o.eps,
                      o.max_trust, self.opt_step, ws.data_ptr(), trust.data_ptr(), n, st)
        else:
            _lib.call('bdn_lars_step', self.flat_params.data_ptr(), self.flat_grads.data_ptr(),
                      _lib.ptr(self.opt_state.get('momentum_buffer')), *table, lr, wd, grad_scale, dev_scale, o.momentum, o.dampening,
                      int(o.nesterov), int(first), o.trust_coef, o.lars_eps, o.max_trust, ws.data_ptr(), trust.data_ptr(), n, st)

    # ------------------------------------------------------------------ optimizer state in torch.optim's format
    def optimizer_state_dict(self):
        """The optimizer state as ``torch.optim.{SGD,Adam,AdamW}(model.parameters()).state_dict()`` holds it (state keyed by the index in
        model.parameters(); param_groups with torch 2.10's keys).  The tensors are copies taken on the current stream, not views of the
        live buffers.  With parameter groups: one 'param_groups' entry per group and no state for a frozen parameter, which is what
        torch.optim built with the same groups holds (fabric_amd.optim.groups_to_torch)."""
        self._no_pending('optimizer_state_dict()')
        self._not_swapped('optimizer_state_dict()')
        self.optim.lr = float(self.lr)
        self.stream(self.flat_params.device)
        torch.cuda.current_stream(self.flat_params.device).wait_stream(self._hp)        # after the last step's update
        if self._groups is not None:
            if self._implicit_group:
                self._groups.groups[0]['lr'] = float(self.lr)
            return _optim.groups_to_torch(self.optim, self._groups, self.layout, self.opt_state, self.opt_step)
        return _optim.flat_to_torch(self.optim, self.layout, self._names, self.opt_state, self.opt_step)

    def load_optimizer_state_dict(self, sd):
        """Load a torch.optim SGD / Adam / AdamW ``state_dict()`` of ``model.parameters()`` (or optimizer_state_dict()'s output).  As
        torch does, the saved group's hyperparameters (lr included) replace the step's own.  Raises ValueError when the saved rule is
        of the other family (SGD vs Adam), or its parameter count, shapes or per-parameter state do not fit this model.  With parameter
        groups the state of an optimizer built with the same groups is expected (fabric_amd.optim.torch_to_groups; a single-group state
        over all parameters is accepted too and leaves the groups' lr / weight_decay as they are)."""
        self._no_pending('load_optimizer_state_dict()')
        self._not_swapped('load_optimizer_state_dict()')
        dev = self.flat_params.device
        if self._groups is not None:
            cfg, hyper, flat, step = _optim.torch_to_groups(sd, self._groups, self.layout, dev)
        else:
            cfg, flat, step = _optim.torch_to_flat(sd, self.layout, self._names, dev)
        if cfg.family != self.optim.family:
            raise ValueError(f'optimizer state of {cfg.kind}, but this step runs {self.optim.kind}')
        hp = self.stream(dev)
        hp.wait_stream(torch.cuda.current_stream(dev))                                   # the copies above are ordered before the next step
        for t in self.opt_state.values():
            t.record_stream(hp)                                                          # a step still in flight may read the old buffers
        if self._groups is not None:
            if hyper is None:                                                            # an ungrouped state: the groups keep their values
                cfg.lr, cfg.weight_decay = float(self.lr), self.optim.weight_decay
            else:
                for g, h in zip(self._groups.groups, hyper):
                    g.update(h)
                cfg.lr, cfg.weight_decay = hyper[0]['lr'], hyper[0]['weight_decay']
        self.optim, self.lr, self.opt_state, self.opt_step = cfg, cfg.lr, flat, step
        if cfg.kind in _optim.LAYERWISE:
            self._layerwise_table()                          # adapt_1d is the saved rule's now

    # ------------------------------------------------------------------ averaged weights in torch.optim.swa_utils.AveragedModel's format
    def _avg_entries(self):
        """{state-dict key: the tensor the averaged model holds for a buffer}: the averaged running statistics with ema_buffers, the live
        ones without, and always the live num_batches_tracked."""
        return {k: self.avg_buffers.get(k, v) for k, v in self._P.items() if k not in self.layout.slices}

    def ema_state_dict(self):
        """The averaged model as ``torch.optim.swa_utils.AveragedModel(model, use_buffers=ema_buffers).state_dict()`` holds it:
        'n_averaged' (int64 scalar) and 'module.<key>' for every parameter and buffer (with ema_buffers=False the live buffers, as torch
        keeps them in sync; num_batches_tracked is always the live count).  It loads into an AveragedModel with
        load_state_dict(strict=True) and, through fabric_amd.utils.helpers.load_checkpoint, gives a BiDateNet on the averaged weights.
        Until the first averaging update (n_averaged == 0) the average IS the live model.  The tensors are copies taken on the current
        stream after the step's stream."""
        self._need_average('ema_state_dict()')
        self._no_pending('ema_state_dict()')
        self._not_swapped('ema_state_dict()')
        dev = self.flat_params.device
        torch.cuda.current_stream(dev).wait_stream(self.stream(dev))                     # after the last step's averaging update
        if self.n_averaged == 0:
            return _optim.avg_to_torch(self.layout, list(self._P), self.flat_params, self._P, 0)
        return _optim.avg_to_torch(self.layout, list(self._P), self.flat_avg, self._avg_entries(), self.n_averaged)

    def load_ema_state_dict(self, sd):
        """Load an AveragedModel ``state_dict()`` of this model (or ema_state_dict()'s output): the averaged parameters, with
        ema_buffers the averaged running_mean / running_var, and n_averaged.  The saved num_batches_tracked (and, with
        ema_buffers=False, the saved running statistics) are checked for their shape and otherwise ignored: the averaged model uses the
        live ones.  With n_averaged > 0 the ema_start delay is over: the next update is averaged (then every ema_every-th).  Raises ValueError on missing or unexpected keys or wrong shapes, before anything is written."""
        self._need_average('load_ema_state_dict()')
        self._no_pending('load_ema_state_dict()')
        self._not_swapped('load_ema_state_dict()')
        dev = self.flat_params.device
        n, vals = _optim.torch_to_avg(sd, self.layout, list(self._P), self._avg_entries())
        hp, cur = self.stream(dev), torch.cuda.current_stream(dev)
        cur.wait_stream(hp)                                                              # a step in flight still writes the average
        for k, v in vals.items():
            dst = self.layout.view(self.flat_avg, k) if k in self.layout.slices else self.avg_buffers.get(k)
            if dst is not None:
                dst.copy_(v.to(device=dev, dtype=torch.float32))
        hp.wait_stream(cur)                                                              # ordered before the next step
        self.n_averaged = n
        if n > 0:                                            # the average was running already: no second start delay
            self._updates = max(self._updates, self.ema_start)

    def _exchange(self):
        """Exchange the live and the averaged parameters (and running statistics) in place on the step's stream, ordered against the
        caller's current stream on both sides, and re-derive what the engine keeps of their values: the packed GEMM images and the
        folded eval-mode BatchNorm tables."""
        dev = self.flat_params.device
        eng = self.model.engine()
        hp, cur = self.stream(dev), torch.cuda.current_stream(dev)
        hp.wait_stream(cur)
        if self.n_averaged == 0:
            # The average is the live model still (ema_state_dict() says the same): nothing is exchanged, and nothing is repacked or
            # refolded either.  That relies on no VALUE having changed; if a state with n_averaged == 0 ever comes to carry other
            # weights than the live ones, this branch has to exchange and refresh like the other.
            return cur.wait_stream(hp)
        with torch.cuda.stream(hp):
            st = _lib.stream_ptr()
            _lib.call('bdn_swap_segments', self.flat_params.data_ptr(), self.flat_avg.data_ptr(), *self._table(), self.layout.total, st)
            if self._avg_desc is not None:                   # scratch = average; average = live; live = scratch
                upd, back, n, max_len, flat, tmp = self._avg_desc
                tmp.copy_(flat)
                _lib.call('bdn_ema_update_multi', upd.data_ptr(), n, max_len, 0.0, 1, st)
                _lib.call('bdn_ema_update_multi', back.data_ptr(), n, max_len, 0.0, 1, st)
            eng.invalidate_weights()                         # in-place writes bump no version counter (BiDateEngine._check_packed)
            eng._weights(eng.layers[0], self._P, False)
            if eng._use_eval_schedule():
                eng.eval_tables(self._P)
        cur.wait_stream(hp)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with step.ema_weights():`` -- the model carries the averaged weights (and, with ema_buffers, the averaged running
        statistics) inside the block: validate, predict or model.state_dict() there.  The live and the averaged values are exchanged
        in place (bdn_swap_segments: the parameters stay views of flat_params, frozen tensors are not touched, no third buffer), the
        engine's packed weight images and eval-mode BatchNorm tables are rebuilt, and on exit -- also when the body raises --
        everything is exchanged back and rebuilt again.  Entry and exit order the caller's current stream against the step's stream in
        both directions.  Inside the block step(), flush(), set_param_groups() and the state-dict methods raise RuntimeError.  Before
        any averaging update has run (n_averaged == 0) the average is the live model, so nothing is exchanged; it does not raise."""
        self._need_average('ema_weights()')
        self._no_pending('ema_weights()')
        self._not_swapped('ema_weights()')
        self._exchange()
        self._swapped = True
        try:
            yield self
        finally:
            self._swapped = False
            self._exchange()
