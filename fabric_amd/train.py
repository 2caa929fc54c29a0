"""The reference's train.py loop (train.py:65-172) on the HIP path: epochs of fused train steps followed by a
validation pass that reports the reference's metrics -- per-batch accuracy and sklearn-style binary
precision / recall / F1, averaged over batches (utils/helpers.py:45-59).  Tracking SaaS clients (comet,
polyaxon), the GCS download and checkpoint upload of the reference are out of scope.

    python -m fabric_amd.train --synthetic --epochs 1                                   # needs an MI355X
    python -m fabric_amd.train --metadata metadata.json --dataset_dir ./onera/          # an OSCD directory tree
    python -m fabric_amd.train --synthetic --epochs 4 --optimizer adamw --resume ./log/checkpoint_epoch_1.state_dict.pt
    python -m fabric_amd.train --synthetic --fused_step true --loss_function focal+dice --focal_gamma 2 --freeze inc --optimizer adamw
    python -m fabric_amd.train --synthetic --fused_step true --optimizer adamw --accumulate 4 --max_grad_norm 1.0
    python -m fabric_amd.train --synthetic --fused_step true --loss_function focal+dice --focal_gamma 2 --ignore_label 255
    python -m fabric_amd.train --synthetic --fused_step true --loss_function focal+dice --focal_gamma 2 --loss_topk 0.25
    python -m fabric_amd.train --synthetic --fused_step true --loss_function focal+lovasz --focal_gamma 0       # cross-entropy + Lovasz-Softmax
    python -m fabric_amd.train --synthetic --fused_step true --loss_function focal+dice --focal_gamma 2 --boundary_weight 0.01      # + the boundary term
    python -m fabric_amd.train --synthetic --fused_step true --optimizer adamw --ema_decay 0.999        # validate and save the averaged weights
    python -m fabric_amd.train --synthetic --fused_step true --optimizer lamb --lr_warmup_updates 4 --lr_schedule cosine   # layer-wise trust ratios
    python -m fabric_amd.train --metadata metadata.json --val_curve_bins 1024 --scene_stride 64 --scene_threshold val      # best-F1 threshold, AP

With real data the loop also does what train.py:182-205 does after validation: the full validation scenes are
predicted tile by tile (utils/inference.py) -- here on the device-resident city stacks -- and written as PNG masks.
"""
import argparse
import contextlib
import json
import os
import re

import numpy as np
import torch
import torch.utils.data

from .models.bidate_model import BiDateNet
from .train_step import TrainStep
from .utils.dataloaders import OneraPreloader, metadata_from_shapes, synthetic_onera
from .utils.helpers import get_mean_metrics, initialize_metrics, set_metrics
from .utils.metrics import batch_prf_from_counts

DEFAULTS = dict(patch_size=90, stride=180, augmentation=True, num_workers=2, epochs=1, batch_size=32,
                learning_rate=1e-3, loss_function='tversky', tversky_alpha=0.1, tversky_beta=0.9,
                validation_cities=['cupertino', 'rennes'], dataset_dir='./onera/', log_dir='./log/')   # reference metadata.json:32-48


def make_loaders(full_load, val_cities, patch_size, stride, batch_size, augmentation, num_workers=0,
                 rank=0, world_size=1, seed=0):
    """utils/helpers.py:211-258 (get_loaders) given an already loaded dataset dict.  For data-parallel runs the training
    indices are sharded by a ShardSampler: every rank derives the same epoch permutation from (seed, epoch) and takes a
    disjoint stride-by-rank slice of it -- independent of the per-process `random` state that OneraPreloader's in-place
    shuffle (utils/dataloaders.py:171) consumes, and sorted first so that the reference's set-ordered city list
    (utils/dataloaders.py:55) cannot differ between ranks.  Call `train_loader.sampler.set_epoch(e)` every epoch."""
    from .parallel import ShardSampler
    train_ds, val_ds = _patch_datasets(full_load, val_cities, patch_size, stride, augmentation)
    sampler = ShardSampler(len(train_ds), rank, world_size, seed=seed)
    kw = dict(batch_size=batch_size, num_workers=num_workers, pin_memory=True)   # pinned batches: the copy stream DMAs them without staging
    # Augmentation draws (global `random`, utils/dataloaders.py:150-156) must differ between ranks.  With worker processes every worker
    # re-seeds `random` from base_seed + worker_id, and base_seed comes from the loader's generator: torch.manual_seed(seed) makes that
    # identical on every rank, so the loader gets a PER-RANK generator, and each worker additionally folds the rank into its seed.
    gen = torch.Generator()
    gen.manual_seed(seed * 7919 + rank)
    return (torch.utils.data.DataLoader(train_ds, sampler=sampler, drop_last=True, generator=gen,
                                        worker_init_fn=_RankWorkerSeed(seed, rank), **kw),
            torch.utils.data.DataLoader(val_ds, shuffle=False, **kw))


def _patch_datasets(full_load, val_cities, patch_size, stride, augmentation):
    """The training and validation OneraPreloader datasets of make_loaders / make_device_loaders."""
    shapes = {c: tuple(d['labels'].shape) for c, d in full_load.items()}
    train_meta, val_meta = metadata_from_shapes(shapes, val_cities, patch_size, stride)
    train_meta = sorted(train_meta)                        # rank-independent base order; the sampler owns the shuffling
    train_ds = OneraPreloader('', train_meta, full_load, patch_size, augmentation)
    train_ds.imgs.sort()                                   # undo the constructor's process-local shuffle (same list object)
    val_ds = OneraPreloader('', val_meta, full_load, patch_size, False)
    return train_ds, val_ds


def make_device_loaders(full_load, val_cities, patch_size, stride, batch_size, augmentation, rank=0, world_size=1, seed=0,
                        device=None, augment=None, warp=None, mix=None):
    """make_loaders with the patches cut on the device (fabric_amd.device_loader): the same datasets, built and sorted the same way,
    the same ShardSampler and drop_last for training, no augmentation and no drop_last for validation.  `full_load`'s city stacks are
    used in place when they are device tensors (ingest's device= output) and uploaded once otherwise; both loaders share them.  The
    augmentation draws come from the process's global `random` at iteration time, as with make_loaders(num_workers=0).
    `augment`: a fabric_amd.augment.PatchAugment for the TRAINING loader only (its draws then come from the policy's counter-based
    generator and `augmentation` is ignored for it); `warp`: a fabric_amd.augment.PatchWarp beside it, for the training loader only too;
    `mix`: a fabric_amd.augment.PatchMix beside it, likewise; validation is never augmented."""
    from .device_loader import DevicePatchLoader, device_stacks
    from .parallel import ShardSampler
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    train_ds, val_ds = _patch_datasets(full_load, val_cities, patch_size, stride, augmentation)
    stacks = device_stacks(full_load, device)
    sampler = ShardSampler(len(train_ds), rank, world_size, seed=seed)
    extra = {} if augment is None else dict(augment=augment)
    if warp is not None:
        extra['warp'] = warp
    if mix is not None:
        extra['mix'] = mix
    return (DevicePatchLoader(train_ds, stacks, batch_size, sampler=sampler, drop_last=True, device=device, **extra),
            DevicePatchLoader(val_ds, stacks, batch_size, device=device))


MIX_FLAGS = (('p', 0.0), ('mode', 'box'), ('box', None), ('margin', 0), ('donors', 'all'), ('min_pixels', 1))      # --mix_*: name, default


def augment_from_opt(opt):
    """The PatchAugment of the --aug_* flags, or None when all are at their defaults.  Raises ValueError for flags that cannot be
    honoured: without --device_patches true (the patches of any other loader are cut on the host) or with values the policy refuses.
    A warp flag (--aug_rotate / --aug_scale / --aug_misreg) alone is enough: the PatchWarp of warp_from_opt rides on this policy; so is
    a --mix_* flag, for the PatchMix of mix_from_opt."""
    given = [f'--aug_{k}' for k, off in (('jitter', 0), ('gain', 0.0), ('bias', 0.0), ('shared_dates', False), ('noise', 0.0),
                                         ('erase_p', 0.0), ('erase_size', None), ('seed', None), ('rotate', 0.0), ('scale', None),
                                         ('misreg', 0.0)) if getattr(opt, f'aug_{k}') != off]
    given += [f'--mix_{k}' for k, off in MIX_FLAGS if getattr(opt, f'mix_{k}', off) != off]
    if not given:
        return None
    if not opt.device_patches:
        raise ValueError(f'{" / ".join(given)} augment the patches the device cuts: add --device_patches true')
    from .augment import PatchAugment
    policy = PatchAugment(seed=opt.seed if opt.aug_seed is None else opt.aug_seed, jitter=opt.aug_jitter, symmetry=bool(opt.augmentation),
                          gain=opt.aug_gain, bias=opt.aug_bias, per_date=not opt.aug_shared_dates, noise_std=opt.aug_noise,
                          erase_p=opt.aug_erase_p, erase_size=tuple(opt.aug_erase_size) if opt.aug_erase_size else (1, 1),
                          erase_label=opt.ignore_label)
    policy.check_patch_size(opt.patch_size)
    return policy


def warp_from_opt(opt):
    """The PatchWarp of --aug_rotate / --aug_scale / --aug_misreg, or None when all three are at their defaults; oob_label is
    --ignore_label.  augment_from_opt refuses the flags without --device_patches true and builds the PatchAugment it rides on."""
    if not opt.aug_rotate and opt.aug_scale is None and not opt.aug_misreg:
        return None
    from .augment import PatchWarp
    return PatchWarp(rotate=opt.aug_rotate, scale=tuple(opt.aug_scale) if opt.aug_scale else (1.0, 1.0), misreg=opt.aug_misreg,
                     oob_label=opt.ignore_label)


def mix_from_opt(opt):
    """The PatchMix of the --mix_* flags, or None when --mix_p is 0; paste_label is 1, the change class.  The pool of --mix_donors change
    needs the loader (label_counts) and is set by main.  augment_from_opt refuses the flags without --device_patches true and builds
    the PatchAugment it rides on."""
    if not opt.mix_p:
        return None
    from .augment import PatchMix
    mix = PatchMix(p=opt.mix_p, mode=opt.mix_mode, box_size=tuple(opt.mix_box) if opt.mix_box else (1, 1), paste_label=1,
                   margin=opt.mix_margin)
    mix.check(opt.patch_size, 1)
    if opt.mix_min_pixels < 1:
        raise ValueError(f'--mix_min_pixels {opt.mix_min_pixels}: a donor holds at least one change pixel')
    return mix


def _device_batches(loader, dev, feeder):
    """The device batches of `loader`: a DevicePatchLoader samples them itself (on the current stream), any other loader goes through
    `feeder` or, without one, a plain copy per batch."""
    from .device_loader import DevicePatchLoader
    if isinstance(loader, DevicePatchLoader):
        return iter(loader)
    if feeder is not None:
        return feeder(loader)
    return ((b1.to(dev), b2.to(dev), lb.to(dev)) for b1, b2, lb in loader)


class _RankWorkerSeed:
    """worker_init_fn: Python's `random` of loader worker w on rank r is seeded from (seed, r, w, the worker's torch seed -- which the
    loader advances every epoch)."""

    def __init__(self, seed, rank):
        self.seed, self.rank = int(seed), int(rank)

    def __call__(self, worker_id):
        import random
        random.seed((self.seed * 7919 + self.rank) * 1000003 + worker_id * 65537 + torch.initial_seed() % 65521)


def batch_accuracy(counts, n_pixels):
    """Per-batch accuracy in percent from a criterion's counts: correct / all pixels, or, with the five counts of a criterion that has
    an ignore label, correct / valid pixels -- 0 for a batch without a valid pixel, like the zero-division default of the P / R / F1."""
    n = int(counts[4]) if len(counts) > 4 else n_pixels
    return 100.0 * int(counts[3]) / n if n else 0.0


def train_epoch(step, loader, dev, patch_size, feeder=None, schedule=None, epoch=0):
    """train.py:73-118 without the per-step host round trip: losses / counts are read back once per epoch, and the
    host -> device copies of batch k+1 (train.py:83-85) run on a copy stream under the step of batch k.
    schedule: None, or a fabric_amd.schedule.LRSchedule: the learning rates of the update batch i of `epoch` belongs to are set before
    each call (host floats only).  With --optimizer lamb / lars the result gains trust_min / trust_max, the adapted tensors' ratios at
    the epoch's last update (one read of step.last_trust per epoch).  With --sam_rho it gains sam_sharpness_mean, the mean over the
    batches of loss(w + e) - loss(w), and sam_norm_mean, the mean of the perturbation's gradient norm ||t * g||; both stay on the
    device until the epoch's one read."""
    from .device_loader import DevicePatchLoader
    from .input_pipeline import DeviceFeeder
    step.model.train()
    recs, norms, mined, lov, bnd = [], [], [], [], []
    clip = step.max_grad_norm is not None
    sam = [] if step.sam_rho is not None else None
    topk = getattr(step.criterion, 'topk', None) is not None      # hard-pixel mining: K and the threshold of every batch, read back with the losses
    boundary = step.criterion is not None and step.criterion.has_boundary    # the boundary term of every batch (terms[-1]), read back with the losses
    lovasz = getattr(step.criterion, 'w_lovasz', 0.0) > 0.0        # the Lovasz-Softmax term of every batch (the last term in front of the boundary one)
    lov_at = -2 if boundary else -1
    if not isinstance(loader, DevicePatchLoader):
        feeder = feeder or DeviceFeeder(dev)
    with torch.cuda.stream(step.stream()):                # the loop lives on the step's own stream: no joins per step
        for i, (b1, b2, labels) in enumerate(_device_batches(loader, dev, feeder)):
            if schedule is not None:
                schedule.apply(step, schedule.position(epoch, i, len(loader), step.accumulate))
            loss = step.step(b1, b2, labels)
            recs.append((loss, step.last_counts.clone(), labels.shape[0]))
            if topk:
                mined.append(step.last_terms.clone())
            if lovasz:
                lov.append(step.last_terms[lov_at:][:1].clone())
            if boundary:
                bnd.append(step.last_terms[-1:].clone())
            if sam is not None:
                sam.append(torch.stack((step.last_sam_loss - loss, step.last_sam_norm)))
            if clip and step.micro == 0:                  # this call ended with an update
                norms.append((step.last_grad_norm.clone(), step.last_clip_coef.clone()))
        if step.flush() and clip:                         # --accumulate: the batches left over at the end of the epoch
            norms.append((step.last_grad_norm.clone(), step.last_clip_coef.clone()))
    torch.cuda.current_stream(dev).wait_stream(step.stream())
    metrics = initialize_metrics()
    for loss, counts, n in recs:
        c = counts.cpu()
        metrics = set_metrics(metrics, loss.item(), batch_accuracy(c, n * patch_size ** 2), batch_prf_from_counts(c))
    out = get_mean_metrics(metrics) if recs else {}
    if mined:                                             # --loss_topk: kept / valid pixels over the epoch, and the mean K-th largest term
        cs = torch.stack([r[1] for r in recs]).cpu().double()
        out.update(topk_kept_frac=float(cs[:, 5].sum() / cs[:, 4].sum()) if float(cs[:, 4].sum()) else 0.0,
                   topk_threshold_mean=float(torch.stack(mined)[:, 2].double().mean()))
    if lov:                                               # a criterion with a Lovasz-Softmax term: its unweighted mean over the epoch
        out.update(lovasz_mean=float(torch.cat(lov).double().mean()))
    if bnd:                                               # --boundary_weight: the unweighted boundary term's mean over the epoch
        out.update(boundary_mean=float(torch.cat(bnd).double().mean()))
    if norms:                                             # --max_grad_norm: read back once per epoch, beside the losses
        nc = torch.stack([torch.stack(v) for v in norms]).cpu()
        out.update(grad_norm_mean=float(nc[:, 0].mean()), grad_norm_max=float(nc[:, 0].max()), clipped_frac=float((nc[:, 1] < 1).float().mean()))
    if sam:                                               # --sam_rho: read back once per epoch, beside the losses
        sn = torch.stack(sam).cpu().double()
        out.update(sam_sharpness_mean=float(sn[:, 0].mean()), sam_norm_mean=float(sn[:, 1].mean()))
    if step.optim.kind in ('lamb', 'lars'):               # --optimizer lamb / lars: the adapted tensors' trust ratios at the last update
        ratios = list(step.trust_ratios(adapted_only=True).values())
        if ratios:
            out.update(trust_min=min(ratios), trust_max=max(ratios))
    return out


@torch.no_grad()
def validate(model, loader, dev, patch_size, criterion, feeder=None, ignore_index=None, curve=None, world=1):
    """train.py:125-172: eval-mode forward, the SAME criterion the run optimises (train.py:137), per-batch accuracy / P / R / F1,
    mean over batches.  Batches arrive through the feeder's copy stream when one is given.  ignore_index: the run's ignore label --
    the counts, and with them accuracy / P / R / F1, are taken over the other pixels.
    curve: a fabric_amd.utils.metrics.ScoreCurve (--val_curve_bins): it is reset, fed the logits of every batch (one launch each, no host
    sync), summed over the `world` ranks and read once after the pass; the result gains best_f1, best_threshold and ap -- over ALL
    validation pixels, not a mean over batches.  None: exactly the calls above."""
    from .utils.metrics import confusion_counts
    model.eval()
    metrics = initialize_metrics()
    if curve is not None:
        curve.reset()
    for b1, b2, labels in _device_batches(loader, dev, feeder):
        logits = model(b1, b2)
        loss = criterion(logits, labels.long())
        if curve is not None:
            curve.update(logits, labels)
        c = confusion_counts(logits, labels, ignore_index).cpu()
        metrics = set_metrics(metrics, loss.item(), batch_accuracy(c, labels.shape[0] * patch_size ** 2), batch_prf_from_counts(c))
    out = get_mean_metrics(metrics)
    if curve is not None:
        if world > 1:
            curve.all_reduce()
        c = curve.compute()
        out.update(best_f1=c['best_f1'], best_threshold=c['best_threshold'], ap=c['ap'])
    return out


def train_epoch_autograd(model, criterion, optimizer, loader, dev, patch_size, world=1, feeder=None):
    """The reference loop itself (train.py:83-101) for dice / jaccard / focal without --fused_step true (the routing as it always was):
    autograd through the one-node BiDateNet function, a torch.optim optimizer (make_torch_optimizer), gradients averaged over the
    ranks after backward."""
    from .parallel import allreduce_mean_grads
    from .utils.metrics import batch_prf_from_counts, confusion_counts
    model.train()
    metrics = initialize_metrics()
    for b1, b2, labels in _device_batches(loader, dev, feeder):
        optimizer.zero_grad()
        logits = model(b1, b2)
        loss = criterion(logits, labels.long())
        loss.backward()
        allreduce_mean_grads(model.parameters(), world)     # a few 16 MB buckets, not 74 blocking per-tensor calls
        optimizer.step()
        model.engine().invalidate_weights()
        c = confusion_counts(logits.detach(), labels).cpu()
        metrics = set_metrics(metrics, loss.item(), 100.0 * int(c[3]) / (labels.shape[0] * patch_size ** 2), batch_prf_from_counts(c))
        del logits, loss                                    # the graph (and its workspace lease) dies before the next forward
    return get_mean_metrics(metrics)


def optimizer_kwargs(opt):
    """The update rule of the --optimizer / --momentum / --nesterov / --weight_decay / --betas / --adam_eps flags as TrainStep keywords."""
    kw = dict(optimizer=opt.optimizer, momentum=opt.momentum, nesterov=opt.nesterov, weight_decay=opt.weight_decay,
              betas=tuple(opt.betas), adam_eps=opt.adam_eps)
    if opt.optimizer in ('lamb', 'lars'):                 # the layer-wise rules' own flags (the fused step only)
        kw.update(layerwise_kwargs(opt))
    return kw


def layerwise_kwargs(opt):
    """--trust_coef / --lars_eps / --max_trust / --adapt_1d as OptimConfig / TrainStep keywords."""
    return dict(trust_coef=opt.trust_coef, lars_eps=opt.lars_eps, max_trust=opt.max_trust, adapt_1d=opt.adapt_1d)


def sam_kwargs(opt):
    """--sam_rho / --sam_adaptive as TrainStep keywords: {} when neither is given.  Raises ValueError for flags that cannot be honoured:
    without --fused_step true (the two passes, the perturbation and the restore live inside the fused step), --sam_adaptive without a
    radius, or a radius fabric_amd.optim.check_sam refuses."""
    if opt.sam_rho is None and not opt.sam_adaptive:
        return {}
    given = ' / '.join(f for f, on in (('--sam_rho', opt.sam_rho is not None), ('--sam_adaptive', opt.sam_adaptive)) if on)
    if not opt.fused_step:
        raise ValueError(f'{given} perturb the weights inside the fused step: add --fused_step true')
    from .optim import check_sam
    try:
        check_sam(opt.sam_rho, opt.sam_adaptive)
    except ValueError as e:
        raise ValueError(f'{given}: {e}')
    return dict(sam_rho=opt.sam_rho, sam_adaptive=opt.sam_adaptive)


def make_torch_optimizer(params, lr, optimizer='sgd', momentum=0.0, nesterov=False, weight_decay=None, betas=(0.9, 0.999), adam_eps=1e-8):
    """The torch.optim optimizer of the autograd route for the same flags (validated by fabric_amd.optim.OptimConfig like the fused
    step's).  The defaults give train.py:55's optim.SGD(lr)."""
    from .optim import OptimConfig
    c = OptimConfig(optimizer, lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=weight_decay, betas=betas, eps=adam_eps)
    if c.kind == 'sgd':
        return torch.optim.SGD(params, lr=c.lr, momentum=c.momentum, nesterov=c.nesterov, weight_decay=c.weight_decay)
    cls = torch.optim.AdamW if c.kind == 'adamw' else torch.optim.Adam
    return cls(params, lr=c.lr, betas=c.betas, eps=c.eps, weight_decay=c.weight_decay)


def fine_tune_groups(model, lr, weight_decay, freeze=(), no_decay_norm_bias=False, lr_scale=()):
    """--freeze / --no_decay_norm_bias / --lr_scale as TrainStep's `param_groups`.  Sets requires_grad=False on every parameter whose
    state-dict name starts with one of the `freeze` prefixes (TrainStep freezes those), and returns the groups of the others by name --
    one per (lr factor, decays or not) combination in use: `lr_scale` is [(prefix, factor)] (the first matching prefix counts, others
    get factor 1), and with no_decay_norm_bias every 1-D tensor (BatchNorm weights and biases, conv biases) has weight_decay 0.  None
    when the flags ask for nothing (no groups: the ungrouped step).  A prefix that matches no parameter, or more than 8 groups,
    raises ValueError."""
    freeze, lr_scale = tuple(freeze), list(lr_scale)
    named = list(model.named_parameters())
    for pre in freeze + tuple(q for q, _ in lr_scale):
        if not any(k.startswith(pre) for k, _ in named):
            raise ValueError(f'prefix {pre!r} matches no parameter (names start with inc, down1..4, up1..4, outc)')
    for k, p in named:
        if k.startswith(freeze):
            p.requires_grad_(False)
    if not (no_decay_norm_bias or lr_scale):
        return None
    groups = {}
    for k, p in named:
        if not p.requires_grad:
            continue
        factor = next((f for q, f in lr_scale if k.startswith(q)), 1.0)
        decay = not (no_decay_norm_bias and p.dim() == 1)
        g = groups.setdefault((factor, decay), {'params': [], 'lr': lr * factor})
        if not decay:
            g['weight_decay'] = 0.0
        elif weight_decay is not None:
            g['weight_decay'] = weight_decay
        g['params'].append(k)
    if len(groups) > 8:
        raise ValueError(f'{len(groups)} parameter groups (lr factors x decay): the fused step takes at most 8')
    return list(groups.values())


def _lr_scale(text):
    prefix, _, factor = text.partition('=')
    if not prefix or not factor:
        raise argparse.ArgumentTypeError(f'{text!r}: expected PREFIX=FACTOR')
    return prefix, float(factor)


_CKPT = re.compile(r'checkpoint_epoch_(\d+)\.state_dict\.pt$')


def resolve_fusion(flag, checkpoint=None, resume=False):
    """The run's date fusion from --fusion (None when the flag was not given) and the fusion the --resume / --init_from checkpoint's
    metadata names (None: no checkpoint, or one without the entry = 'product' for a checkpoint, since older runs knew no other).
    Returns (fusion, note): --resume continues the run it names, so another explicit --fusion is an error (ValueError); --init_from only
    takes weights, so an explicit --fusion wins and `note` is the one line that says the encoder was trained under the other fusion."""
    if flag is None:
        return checkpoint or 'product', None
    if checkpoint is None or checkpoint == flag:
        return flag, None
    if resume:
        raise ValueError(f'--resume continues a run trained with --fusion {checkpoint}; --fusion {flag} would change the network')
    return flag, f'--init_from: the checkpoint was trained with fusion {checkpoint!r}; fine-tuning it under fusion {flag!r}'


def resume_from(path, device=None, precision=None):
    """--resume DIR/checkpoint_epoch_N.state_dict.pt: (model, optimizer state or None, first epoch N + 1).  The weights and BatchNorm
    buffers come through load_checkpoint; the optimizer state is the sibling optimizer_epoch_N.pt save_if_better wrote, in
    torch.optim's state_dict() format (absent for a stateless optimizer).  The date fusion comes back from metadata_epoch_N.json."""
    from .utils.helpers import load_checkpoint
    m = _CKPT.search(os.path.basename(path))
    if not m:
        raise SystemExit(f'--resume {path}: expected a checkpoint_epoch_N.state_dict.pt written by this program')
    epoch = int(m.group(1))
    model = load_checkpoint(path, device=device, precision=precision, allow_pickle=False)
    opt_path = os.path.join(os.path.dirname(path), f'optimizer_epoch_{epoch}.pt')
    opt_sd = torch.load(opt_path, map_location='cpu', weights_only=True) if os.path.exists(opt_path) else None
    return model, opt_sd, epoch + 1


def save_if_better(model, mean_val_metrics, best_metrics, metadata, epoch, out_dir, optimizer_state=None, ema_state=None):
    """train.py:207-227: when validation precision, recall OR F1 improved, write `checkpoint_epoch_N.pt` (the pickled
    module, as the reference does with torch.save(model, ...)) and `metadata_epoch_N.json` (the run's metadata plus
    `validation_metrics`), and, when `optimizer_state` (torch.optim's state_dict() format) holds any state, `optimizer_epoch_N.pt`,
    and, when `ema_state` (TrainStep.ema_state_dict()'s output, torch.optim.swa_utils.AveragedModel's format, or a callable that returns
    it, called only when something is written) is given, `ema_epoch_N.pt`, which
    load_checkpoint reads as a BiDateNet on the averaged weights.  The upload to the outputs store / comet is out of scope.  Returns the
    new best metrics."""
    keys = ('cd_precisions', 'cd_recalls', 'cd_f1scores')
    if not any(mean_val_metrics[k] > best_metrics[k] for k in keys):
        return best_metrics
    os.makedirs(out_dir, exist_ok=True)
    metadata = dict(metadata)
    metadata['validation_metrics'] = {k: float(v) for k, v in mean_val_metrics.items()}
    with open(os.path.join(out_dir, f'metadata_epoch_{epoch}.json'), 'w') as fout:
        json.dump(metadata, fout)
    torch.save(model, os.path.join(out_dir, f'checkpoint_epoch_{epoch}.pt'))
    # ... and, for the way back, the parameters + BatchNorm buffers under the keys the REFERENCE's nn.DataParallel(BiDateNet) has
    # (utils/helpers.py:335): the pickle above names fabric_amd's classes, which a reference checkout cannot import; this file loads there
    # with model.load_state_dict(torch.load(path)) and here with fabric_amd.utils.helpers.load_checkpoint
    torch.save({'module.' + k: v.detach().cpu() for k, v in model.state_dict().items()},
               os.path.join(out_dir, f'checkpoint_epoch_{epoch}.state_dict.pt'))
    if optimizer_state is not None and optimizer_state['state']:
        torch.save(_to_cpu(optimizer_state), os.path.join(out_dir, f'optimizer_epoch_{epoch}.pt'))
    if ema_state is not None:
        ema_state = ema_state() if callable(ema_state) else ema_state
        torch.save(_to_cpu(ema_state), os.path.join(out_dir, f'ema_epoch_{epoch}.pt'))
    return mean_val_metrics


def _to_cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    return obj


def scene_scores(mask, label):
    """Counts of a full-scene change mask against the city's label map (class 1 positive) and the precision / recall / F1 they give
    (batch_prf_from_counts: 0 where a ratio has no denominator)."""
    m, l = np.asarray(mask) == 1, np.asarray(label) != 0
    counts = np.array([(m & l).sum(), (m & ~l).sum(), (~m & l).sum()])
    pr, rc, f1 = batch_prf_from_counts(counts)
    return {'tp': int(counts[0]), 'fp': int(counts[1]), 'fn': int(counts[2]), 'precision': pr, 'recall': rc, 'f1': f1}


def check_curve_flags(val_curve_bins, scene_threshold, scene_stride):
    """--val_curve_bins / --scene_threshold / --scene_stride together, without a device: returns 'argmax', 'val' or the float threshold;
    raises ValueError with the reason otherwise."""
    n = val_curve_bins
    if n != 0 and (n < 2 or n > 4096 or n & (n - 1)):
        raise ValueError(f'--val_curve_bins {n}: 0 (off) or a power of two in 2..4096')
    if scene_threshold in ('argmax', 'val'):
        thr = scene_threshold
    else:
        try:
            thr = float(scene_threshold)
        except ValueError:
            thr = float('nan')
        if not 0.0 <= thr <= 1.0:
            raise ValueError(f'--scene_threshold {scene_threshold}: argmax, val or a number in [0, 1]')
    if thr == 'val' and n == 0:
        raise ValueError('--scene_threshold val applies the best-F1 threshold of the validation pass: add --val_curve_bins N')
    if thr != 'argmax' and scene_stride <= 0:
        raise ValueError(f'--scene_threshold {scene_threshold} thresholds the blended scene probabilities: add --scene_stride N > 0')
    return thr


def check_object_flags(scene_min_area, scene_objects, scene_connectivity, scene_stride):
    """--scene_min_area / --scene_objects / --scene_connectivity / --scene_stride together, without a device: returns the min_area for
    predict_scene_blended (None: no filtering); raises ValueError with the reason otherwise."""
    if scene_min_area < 0:
        raise ValueError(f'--scene_min_area {scene_min_area}: 0 (off) or the smallest object kept, in pixels')
    if scene_connectivity not in (4, 8):
        raise ValueError(f'--scene_connectivity {scene_connectivity}: 4 or 8')
    if (scene_min_area > 0 or scene_objects) and scene_stride <= 0:
        raise ValueError('--scene_min_area / --scene_objects work on the blended scene masks: add --scene_stride N > 0')
    return scene_min_area if scene_min_area > 0 else None


def check_cleanup_flags(scene_hysteresis, scene_close, scene_fill_holes, scene_open, scene_threshold, scene_connectivity, scene_stride):
    """--scene_hysteresis / --scene_close / --scene_fill_holes / --scene_open with --scene_threshold (as check_curve_flags returns it) /
    --scene_connectivity / --scene_stride, without a device: returns None when all four are off, else the keyword arguments of
    predict_scene_blended {hysteresis_low, close_radius2, fill_holes, open_radius2} (None = off); raises ValueError with the reason
    otherwise.  With --scene_threshold val the high threshold is known only after the validation pass: predict_scene_blended refuses a
    low threshold above it then."""
    if scene_hysteresis is None and scene_close is None and scene_open is None and scene_fill_holes == 0:
        return None
    if scene_stride <= 0:
        raise ValueError('--scene_hysteresis / --scene_close / --scene_fill_holes / --scene_open clean the blended scene masks: add --scene_stride N > 0')
    if scene_fill_holes < -1:
        raise ValueError(f'--scene_fill_holes {scene_fill_holes}: 0 (off), -1 (every hole) or the largest hole filled, in pixels')
    if scene_hysteresis is not None and scene_threshold == 'argmax':
        raise ValueError('--scene_hysteresis LOW keeps weak change that hangs on change above --scene_threshold: add --scene_threshold val|FLOAT')
    from .utils.morphology import check_cleanup_args
    fill = None if scene_fill_holes == 0 else True if scene_fill_holes == -1 else scene_fill_holes
    high = 1.0 if scene_threshold == 'val' else None if scene_threshold == 'argmax' else scene_threshold
    try:
        check_cleanup_args(high, scene_hysteresis, scene_close, fill, scene_open, scene_connectivity)
    except ValueError as e:
        raise ValueError(f'--scene_hysteresis / --scene_close / --scene_fill_holes / --scene_open: {e}')
    return {'hysteresis_low': scene_hysteresis, 'close_radius2': scene_close, 'fill_holes': fill, 'open_radius2': scene_open}


def checkpoint_entry(path, key):
    """The `key` entry of the metadata_epoch_N.json beside a checkpoint file of this program, or None."""
    m = _CKPT.search(os.path.basename(path)) if path else None
    meta = os.path.join(os.path.dirname(path), f'metadata_epoch_{m.group(1)}.json') if m else None
    if meta is None or not os.path.exists(meta):
        return None
    with open(meta) as fh:
        return json.load(fh).get(key)


def check_auto_threshold_flags(scene_auto_threshold, scene_mad_baseline, scene_mad_iters, scene_threshold, scene_stride, checkpoint=None):
    """--scene_auto_threshold / --scene_mad_baseline / --scene_mad_iters with --scene_threshold (as check_curve_flags returns it) and
    --scene_stride, without a device.  checkpoint: the {'scene_auto_threshold', 'scene_mad_baseline'} entries of the metadata of the run
    --resume continues (or None): a resumed run keeps them unless the flag is given again.  Returns (the method of predict_scene_blended's
    auto_threshold or None, {'method', 'iters'} of the baseline or None); raises ValueError with the reason otherwise."""
    from .utils.mad import MAX_ITERS
    from .utils.thresholds import METHODS
    kept = checkpoint or {}
    auto = scene_auto_threshold if scene_auto_threshold is not None else kept.get('scene_auto_threshold')
    if auto is not None:
        if auto not in METHODS:
            raise ValueError(f'--scene_auto_threshold {auto}: one of {", ".join(METHODS)}')
        if scene_stride <= 0:
            raise ValueError('--scene_auto_threshold thresholds the blended scene probabilities: add --scene_stride N > 0')
        if scene_threshold != 'argmax':
            raise ValueError(f'--scene_auto_threshold selects the threshold on the device, --scene_threshold {scene_threshold} gives one: '
                             f'leave --scene_threshold at argmax')
    old = kept.get('scene_mad_baseline') or {}
    method = scene_mad_baseline if scene_mad_baseline is not None else old.get('method')
    if method is None:
        if scene_mad_iters is not None:
            raise ValueError('--scene_mad_iters counts the iterations of a baseline that is not on: add --scene_mad_baseline METHOD')
        return auto, None
    if method not in METHODS:
        raise ValueError(f'--scene_mad_baseline {method}: one of {", ".join(METHODS)}')
    if scene_stride <= 0:
        raise ValueError('--scene_mad_baseline adds to the scene line of the blended scenes: add --scene_stride N > 0')
    iters = scene_mad_iters if scene_mad_iters is not None else old.get('iters', 30)
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= MAX_ITERS:
        raise ValueError(f'--scene_mad_iters {iters}: an integer in 1..{MAX_ITERS}')
    return auto, {'method': method, 'iters': iters}


def cleaned_scores(mask, label, ignore_label=None):
    """scene_scores of the cleaned mask that is written, the pixels with label == ignore_label left out."""
    m, l = np.asarray(mask) == 1, np.asarray(label)
    keep = np.ones(l.shape, bool) if ignore_label is None else l != ignore_label
    pos = (l != 0) & keep
    counts = np.array([(m & pos).sum(), (m & ~pos & keep).sum(), (~m & pos).sum()])
    pr, rc, f1 = batch_prf_from_counts(counts)
    return {'tp': int(counts[0]), 'fp': int(counts[1]), 'fn': int(counts[2]), 'precision': pr, 'recall': rc, 'f1': f1}


def check_boundary_flags(boundary_weight, boundary_classes, boundary_max_dist, fused_step, scene_boundary_tol, scene_stride):
    """--boundary_weight / --boundary_classes / --boundary_max_dist / --fused_step and --scene_boundary_tol / --scene_stride together,
    without a device: returns the tolerance for boundary_scores (None: the scene line stays as it is); raises ValueError with the reason
    otherwise."""
    if boundary_weight is not None:
        if not boundary_weight > 0.0:
            raise ValueError(f'--boundary_weight {boundary_weight}: a weight > 0 (leave the flag out for no boundary term)')
        if not fused_step:
            raise ValueError(f'--boundary_weight {boundary_weight} is a term of the criterion of the fused step: add --fused_step true')
    elif boundary_classes != 'foreground' or boundary_max_dist is not None:
        raise ValueError('--boundary_classes / --boundary_max_dist shape a term that is not on: add --boundary_weight W')
    if boundary_classes not in ('foreground', 'all'):
        raise ValueError(f"--boundary_classes {boundary_classes}: 'foreground' or 'all'")
    if boundary_max_dist is not None and not 0.0 < boundary_max_dist < float('inf'):
        raise ValueError(f'--boundary_max_dist {boundary_max_dist}: a positive number of pixels')
    if scene_boundary_tol is None:
        return None
    from .utils.distance import check_boundary_tolerance
    try:
        check_boundary_tolerance(scene_boundary_tol)
    except ValueError as e:
        raise ValueError(f'--scene_boundary_tol: {e}')
    if scene_stride <= 0:
        raise ValueError('--scene_boundary_tol scores the blended scene masks: add --scene_stride N > 0')
    return scene_boundary_tol


def check_coregister_flags(coregister, cells, bands, min_ncc, band_ids=None, n_bands=13, synthetic_misreg=(0, 0), synthetic=False):
    """--coregister / --coregister_cells / --coregister_bands / --coregister_min_ncc and --synthetic_misreg together, without a device:
    returns None (off) or the keyword arguments of coregister_cities; raises ValueError with the reason otherwise.  A band is named by its
    id in the run's band_ids or by its index."""
    from .utils import registration as RG
    if len(synthetic_misreg) != 2 or any(not isinstance(v, int) or isinstance(v, bool) for v in synthetic_misreg):
        raise ValueError(f'--synthetic_misreg {synthetic_misreg}: two integers DY DX')
    if tuple(synthetic_misreg) != (0, 0) and not synthetic:
        raise ValueError('--synthetic_misreg shifts date 2 of the synthetic cities: add --synthetic')
    if not isinstance(coregister, int) or isinstance(coregister, bool) or not 0 <= coregister <= RG.MAX_SHIFT:
        raise ValueError(f'--coregister {coregister}: 0 (off) or the search radius in pixels, 1..{RG.MAX_SHIFT}')
    if coregister == 0:
        if tuple(cells) != (1, 1) or bands is not None or min_ncc != 0.0:
            raise ValueError('--coregister_cells / --coregister_bands / --coregister_min_ncc shape an alignment that is not on: add --coregister R')
        return None
    if len(cells) != 2 or any(not 1 <= v <= RG.MAX_CELLS for v in cells):
        raise ValueError(f'--coregister_cells {list(cells)}: NY NX, 1..{RG.MAX_CELLS} each')
    if not -1.0 <= min_ncc <= 1.0:
        raise ValueError(f'--coregister_min_ncc {min_ncc}: a correlation in [-1, 1]')
    n = len(band_ids) if band_ids else n_bands
    idx = None
    if bands is not None:
        idx = []
        for b in bands:
            if band_ids and str(b) in list(band_ids):
                idx.append(list(band_ids).index(str(b)))
            elif str(b).lstrip('-').isdigit() and 0 <= int(b) < n:
                idx.append(int(b))
            else:
                raise ValueError(f'--coregister_bands {b}: neither one of the band ids {list(band_ids or [])} nor an index in [0, {n})')
    if not 1 <= (len(idx) if idx is not None else n) <= RG.MAX_BANDS:
        raise ValueError(f'--coregister_bands: 1..{RG.MAX_BANDS} bands (the run has {n}: name a subset)')
    return dict(max_shift=coregister, cells=(int(cells[0]), int(cells[1])), bands=idx, min_ncc=float(min_ncc))


def coregister_loaded(full_load, coreg, ignore_label, device, log=True):
    """--coregister: align date 2 of every loaded city to its date 1, in place, once, before any loader or scene pass sees the stacks; one
    `coreg` log line per city.  Returns the per-city reports."""
    from .utils.registration import coregister_cities, report_line
    reports = coregister_cities(full_load, ignore_label=ignore_label, device=device, **coreg)
    if log:
        for city, rep in reports.items():
            print('coreg ' + json.dumps(report_line(city, rep)), flush=True)
    return reports


def check_radiometric_flags(radiometric, knots=None, value_range=None, bands=None, band_ids=None, n_bands=13, synthetic_radiometry=None,
                            synthetic=False, checkpoint=None):
    """--radiometric / --radiometric_knots / --radiometric_range / --radiometric_bands and --synthetic_radiometry together, without a
    device: returns None (off) or the keyword arguments of normalize_cities; raises ValueError with the reason otherwise.  A flag that
    was not given is None; `checkpoint` is the `radiometric` entry of the metadata of the run --resume continues (or None): with no
    --radiometric flag the run keeps the checkpoint's settings, since its weights were trained on pairs matched that way.  A band is
    named by its id in the run's band_ids or by its index."""
    from .utils import radiometry as RM
    if synthetic_radiometry is not None:
        if len(synthetic_radiometry) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float('inf')
                                                 for v in synthetic_radiometry):
            raise ValueError(f'--synthetic_radiometry {synthetic_radiometry}: two finite numbers GAIN BIAS')
        if not synthetic:
            raise ValueError('--synthetic_radiometry changes date 2 of the synthetic cities: add --synthetic')
    if radiometric is None and checkpoint is not None:
        if knots is not None or value_range is not None or bands is not None:
            raise ValueError('--radiometric_knots / --radiometric_range / --radiometric_bands would change how the resumed run matches its '
                             'pairs: give --radiometric too, or none of them')
        out = dict(checkpoint)
        if out.get('method') not in ('histogram', 'range'):
            raise ValueError(f'--resume: the checkpoint metadata holds an unknown radiometric entry {checkpoint!r}')
        return dict(method=out['method'], knots=int(out.get('knots', 256)), lower=float(out.get('lower', 0.02)),
                    upper=float(out.get('upper', 0.98)), bands=out.get('bands'))
    if radiometric not in (None, 'none', 'histogram', 'range'):
        raise ValueError(f"--radiometric {radiometric}: 'none', 'histogram' or 'range'")
    if radiometric in (None, 'none'):
        if knots is not None or value_range is not None or bands is not None:
            raise ValueError('--radiometric_knots / --radiometric_range / --radiometric_bands shape a matching that is not on: add '
                             '--radiometric histogram or --radiometric range')
        return None
    if radiometric == 'histogram' and value_range is not None:
        raise ValueError('--radiometric_range names the two quantiles of --radiometric range; --radiometric histogram takes --radiometric_knots')
    if radiometric == 'range' and knots is not None:
        raise ValueError('--radiometric_knots counts the knots of --radiometric histogram; --radiometric range takes --radiometric_range LO HI')
    knots = 256 if knots is None else knots
    if not isinstance(knots, int) or isinstance(knots, bool) or not 2 <= knots <= RM.MAX_KNOTS:
        raise ValueError(f'--radiometric_knots {knots}: the number of knots, 2..{RM.MAX_KNOTS}')
    lo, hi = (0.02, 0.98) if value_range is None else value_range
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError(f'--radiometric_range {lo} {hi}: two quantiles with 0 <= LO < HI <= 1')
    n = len(band_ids) if band_ids else n_bands
    idx = None
    if bands is not None:
        idx = []
        for b in bands:
            if band_ids and str(b) in list(band_ids):
                idx.append(list(band_ids).index(str(b)))
            elif str(b).lstrip('-').isdigit() and 0 <= int(b) < n:
                idx.append(int(b))
            else:
                raise ValueError(f'--radiometric_bands {b}: neither one of the band ids {list(band_ids or [])} nor an index in [0, {n})')
        if len(set(idx)) != len(idx):
            raise ValueError(f'--radiometric_bands {list(bands)}: a band is named twice')
    if not 1 <= (len(idx) if idx is not None else n) <= RM.MAX_BANDS:
        raise ValueError(f'--radiometric_bands: 1..{RM.MAX_BANDS} bands (the run has {n}: name a subset)')
    return dict(method=radiometric, knots=knots, lower=float(lo), upper=float(hi), bands=idx)


def check_mad_flags(invariant=None, iters=None, tol=None, invariant_min=None, radiom=None, checkpoint=None, explicit=False):
    """--radiometric_invariant / --mad_iters / --mad_tol / --mad_invariant_min, without a device: returns {} (off) or the extra keyword
    arguments of normalize_cities (invariant, invariant_min, mad_iters, mad_tol); raises ValueError with the reason otherwise.  `radiom` is
    what check_radiometric_flags returned, `checkpoint` the `radiometric` entry of the run --resume continues; `explicit`: --radiometric
    was given.  Like the matching itself, a resumed run keeps the checkpoint's settings unless --radiometric is given again."""
    from .utils import mad as MAD
    given = [n for n, v in (('--mad_iters', iters), ('--mad_tol', tol), ('--mad_invariant_min', invariant_min)) if v is not None]
    if invariant is None and not given and radiom is not None and not explicit and checkpoint and checkpoint.get('invariant') is not None:
        if checkpoint.get('invariant') != 'mad':
            raise ValueError(f'--resume: the checkpoint metadata holds an unknown radiometric invariant {checkpoint.get("invariant")!r}')
        return dict(invariant='mad', invariant_min=float(checkpoint.get('invariant_min', 0.95)), mad_iters=int(checkpoint.get('mad_iters', 30)),
                    mad_tol=float(checkpoint.get('mad_tol', 1e-3)))
    if invariant not in (None, 'mad'):
        raise ValueError(f"--radiometric_invariant {invariant}: 'mad'")
    if invariant is None:
        if given:
            raise ValueError(f'{" / ".join(given)} shape the invariant-pixel selection: add --radiometric_invariant mad')
        return {}
    if radiom is None or not explicit:
        raise ValueError('--radiometric_invariant selects the pixels --radiometric fits its transfer on: add --radiometric histogram or '
                         '--radiometric range')
    iters = 30 if iters is None else iters
    if not isinstance(iters, int) or isinstance(iters, bool) or not 1 <= iters <= MAD.MAX_ITERS:
        raise ValueError(f'--mad_iters {iters}: the largest number of iterations, 1..{MAD.MAX_ITERS}')
    tol = 1e-3 if tol is None else tol
    if not isinstance(tol, (int, float)) or isinstance(tol, bool) or not 0.0 <= tol < float('inf'):
        raise ValueError(f'--mad_tol {tol}: a finite number >= 0 (0 never stops early)')
    p = 0.95 if invariant_min is None else invariant_min
    if not isinstance(p, (int, float)) or isinstance(p, bool) or not 0.0 < p <= 1.0:
        raise ValueError(f'--mad_invariant_min {p}: a probability in (0, 1]')
    n = len(radiom['bands']) if radiom.get('bands') is not None else None
    if n is not None and n > MAD.MAX_BANDS:
        raise ValueError(f'--radiometric_invariant mad takes 1..{MAD.MAX_BANDS} bands: name a subset with --radiometric_bands')
    return dict(invariant='mad', invariant_min=float(p), mad_iters=iters, mad_tol=float(tol))


def checkpoint_radiometric(path):
    """The `radiometric` entry of the metadata_epoch_N.json beside a checkpoint file of this program, or None."""
    return checkpoint_entry(path, 'radiometric')


def checkpoint_label_smoothing(path):
    """The `label_smoothing` entry of the metadata_epoch_N.json beside a checkpoint file of this program, or None."""
    return checkpoint_entry(path, 'label_smoothing')


def resolve_label_smoothing(flag, fused_step, loss_topk, checkpoint=None):
    """--label_smoothing E (None when the flag was not given) with --fused_step / --loss_topk and the `label_smoothing` entry of the
    metadata of the run --resume continues (or None) -> the run's value (0.0: none).  A resumed run keeps the checkpoint's value unless
    the flag is given again.  ValueError names what does not fit: the smoothed targets live in the criterion of the fused step
    (bdn_criterion_soft), and --loss_topk ranks a hard-label term."""
    e = flag if flag is not None else checkpoint
    if e is None:
        return 0.0
    if isinstance(e, bool) or not isinstance(e, (int, float)) or not 0.0 <= float(e) < 1.0:
        raise ValueError(f'--label_smoothing {e}: a number in [0, 1)')
    e = float(e)
    if e > 0.0 and not fused_step:
        raise ValueError(f'--label_smoothing {e} is built into the criterion of the fused step (its soft-target kernels): add --fused_step true')
    if e > 0.0 and loss_topk is not None:
        raise ValueError(f'--label_smoothing {e} and --loss_topk {loss_topk}: top-k mining ranks a hard-label focal term and takes no '
                         f'soft targets; give one of them')
    return e


def normalize_loaded(full_load, radiom, ignore_label, device, log=True):
    """--radiometric: match date 2 of every loaded city to its date 1, in place, once, after --coregister and before any loader or scene
    pass sees the stacks; one `radiom` log line per city.  Returns the per-city reports."""
    from .utils.radiometry import mad_line, normalize_cities, report_line
    reports = normalize_cities(full_load, ignore_label=ignore_label, device=device, **radiom)
    if log:
        for city, rep in reports.items():
            if 'mad' in rep:                               # --radiometric_invariant mad: what the fit of the next line was restricted to
                print('mad ' + json.dumps(mad_line(city, rep)), flush=True)
            print('radiom ' + json.dumps(report_line(city, rep)), flush=True)
    return reports


def main(argv=None):
    ap = argparse.ArgumentParser(description='Training change detection network (HIP path)')
    for k, v in DEFAULTS.items():
        if isinstance(v, bool):
            ap.add_argument(f'--{k}', type=lambda s: s.lower() in ('1', 'true', 'yes'), default=v)
        elif isinstance(v, list):
            ap.add_argument(f'--{k}', nargs='*', default=v)
        else:
            ap.add_argument(f'--{k}', type=type(v), default=v)
    ap.add_argument('--synthetic', action='store_true', help='use fabric_amd.utils.dataloaders.synthetic_onera()')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'bf16x3', 'bf16x3-fast', 'fp32'])
    ap.add_argument('--fusion', default=None, choices=['product', 'absdiff'],
                    help="how the two dates' encoder features meet in the skips: product = relu(x_d2 * x_d1) (the default), absdiff = "
                         '|x_d2 - x_d1| (FC-Siam-diff); no parameters, same checkpoints.  Recorded in the checkpoint metadata: --resume '
                         'restores it, --init_from takes it unless the flag is given')
    ap.add_argument('--seed', type=int, default=0, help='seeds the shard permutation, the augmentation draws and the initial weights identically on every rank')
    ap.add_argument('--focal_gamma', type=float, default=None, help='required by --loss_function focal (utils/helpers.py:291)')
    ap.add_argument('--focal_alpha', type=float, default=None, help='focal class weights [a, 1 - a] (utils/metrics.py:13-14); --fused_step true only')
    ap.add_argument('--fused_step', type=lambda s: s.lower() in ('1', 'true', 'yes'), default=False,
                    help='true: every --loss_function trains on the fused step (and --freeze / --frozen_bn / --no_decay_norm_bias / --lr_scale '
                         'work with all of them), and the compound criteria focal+dice / focal+jaccard / focal+tversky are available; '
                         'false: tversky on the fused step, dice / jaccard / focal on the autograd route')
    ap.add_argument('--loss_weights', type=float, nargs=2, default=[1.0, 1.0], metavar=('W_FOCAL', 'W_OVERLAP'),
                    help='weights of the two terms of a compound --loss_function (focal+lovasz: W_FOCAL W_LOVASZ)')
    ap.add_argument('--lovasz_classes', default='present', choices=['present', 'all'],
                    help='--loss_function lovasz / focal+lovasz: average the Lovasz-Softmax term over the classes present among the labelled '
                         'pixels of the batch, or over all classes (Criterion(lovasz_classes=)); the epoch record gains train_lovasz_mean')
    ap.add_argument('--boundary_weight', type=float, default=None, metavar='W',
                    help='--fused_step true only: adds W * the boundary term of Kervadec et al. (softmax weighted by the signed distance to the '
                         'contour of the labels, computed on the device every step) to any --loss_function (Criterion(w_boundary=W)); the '
                         'epoch record gains train_boundary_mean')
    ap.add_argument('--boundary_classes', default='foreground', choices=['foreground', 'all'],
                    help='--boundary_weight: the classes of the boundary term, 1.. (foreground) or every class')
    ap.add_argument('--boundary_max_dist', type=float, default=None, metavar='D', help='--boundary_weight: clamp the signed distance to [-D, D] pixels')
    ap.add_argument('--scene_boundary_tol', type=int, default=None, metavar='T',
                    help='--scene_stride N > 0: the scene line gains boundary_precision, boundary_recall, boundary_f1 (boundary pixels within T '
                         'pixels of the other contour), hausdorff and boundary_tol (boundary_scores on the mask that is written; --ignore_label '
                         'pixels make no contour)')
    ap.add_argument('--ignore_label', type=int, default=None, metavar='V',
                    help='--fused_step true only: pixels labelled V (0..255, e.g. 255 for nodata / unlabelled) are left out of the loss, '
                         'its gradient and the accuracy / precision / recall / F1 (Criterion(ignore_index=V))')
    ap.add_argument('--label_smoothing', type=float, default=None, metavar='E',
                    help='--fused_step true only, not with --loss_topk: label smoothing, 0 <= E < 1 -- the target of the overlap and focal '
                         'terms is (1 - E) + E / ncls at the label\'s class and E / ncls elsewhere (torch.nn.CrossEntropyLoss(label_smoothing=); '
                         'bdn_criterion_soft).  Recorded in the checkpoint metadata; --resume keeps the value of the run it continues')
    ap.add_argument('--loss_topk', type=float, default=None, metavar='F',
                    help='--fused_step true only, a --loss_function with a focal term: hard-pixel mining, the focal term is averaged over the '
                         'hardest fraction F (0 < F <= 1) of the valid pixels of every batch (Criterion(topk=F)); the epoch record gains '
                         'train_topk_kept_frac and train_topk_threshold_mean')
    ap.add_argument('--synthetic_ignore_frac', type=float, default=0.1,
                    help='--synthetic with --ignore_label V: the fraction of every label raster painted with V')
    ap.add_argument('--optimizer', default='sgd', choices=['sgd', 'adam', 'adamw', 'lamb', 'lars'],
                    help='sgd is train.py:55 (optim.SGD); adam / adamw the torch.optim rules (train.py:56 is a commented-out Adam); lamb / '
                         'lars the layer-wise adaptive rules for large batches (fused step only: there is no autograd route for them)')
    ap.add_argument('--trust_coef', type=float, default=1e-3, help='lars: the trust coefficient')
    ap.add_argument('--lars_eps', type=float, default=1e-8, help='lars: the epsilon in the denominator of the local rate')
    ap.add_argument('--max_trust', type=float, default=None, metavar='X', help='lamb / lars: clamp every trust ratio at X (default: no clamp)')
    ap.add_argument('--adapt_1d', action='store_true', help='lamb / lars: adapt biases and BatchNorm weights / biases too (default: ratio 1)')
    ap.add_argument('--lr_warmup_updates', type=int, default=0, metavar='N',
                    help='fused step: ramp the learning rate linearly from lr/N to lr over the first N updates')
    ap.add_argument('--lr_schedule', default='constant', choices=['constant', 'cosine'],
                    help='fused step: cosine decays the learning rate to --lr_min at the last update of the run')
    ap.add_argument('--lr_min', type=float, default=0.0, help='--lr_schedule cosine: the learning rate of the last update')
    ap.add_argument('--momentum', type=float, default=0.0, help='sgd only')
    ap.add_argument('--nesterov', action='store_true', help='sgd only, needs --momentum')
    ap.add_argument('--weight_decay', type=float, default=None, help="default: torch's (0 for sgd and adam, 1e-2 for adamw)")
    ap.add_argument('--betas', type=float, nargs=2, default=[0.9, 0.999], help='adam / adamw')
    ap.add_argument('--adam_eps', type=float, default=1e-8, help='adam / adamw')
    ap.add_argument('--accumulate', type=int, default=1, metavar='K',
                    help='fused step: update on every K-th batch with the mean gradient of the K batches (one gradient exchange per update)')
    ap.add_argument('--max_grad_norm', type=float, default=None, metavar='X',
                    help='fused step: clip the gradients to a global L2 norm of X (torch.nn.utils.clip_grad_norm_); inf: measure only')
    ap.add_argument('--sam_rho', type=float, default=None, metavar='F',
                    help='--fused_step true only: sharpness-aware minimisation (SAM) with neighbourhood radius F > 0: every batch runs a second '
                         'forward / backward at the perturbed weights; the epoch record gains train_sam_sharpness_mean and train_sam_norm_mean')
    ap.add_argument('--sam_adaptive', action='store_true', help='--sam_rho: the scale-invariant ASAM perturbation (radii of 0.5 .. 2 are usual)')
    ap.add_argument('--ema_decay', type=float, default=None, metavar='D',
                    help='--fused_step true only: keep an exponential moving average of the weights (decay D in [0, 1), '
                         'torch.optim.swa_utils.AveragedModel); validation and the full scenes run on it, and ema_epoch_N.pt is written')
    ap.add_argument('--swa', action='store_true', help='--fused_step true only: the equal-weight running mean of the weights (SWA) instead; no --ema_decay')
    ap.add_argument('--ema_every', type=int, default=1, metavar='N', help='average on every N-th update')
    ap.add_argument('--ema_start', type=int, default=0, metavar='N', help='start averaging after the first N updates of the run (a --resume that loads a running average does not wait again)')
    ap.add_argument('--ema_buffers', type=lambda s: s.lower() in ('1', 'true', 'yes'), default=True,
                    help='true: running_mean / running_var are averaged too (use_buffers=True); false: the averaged model uses the live ones')
    ap.add_argument('--resume', default=None, help='DIR/checkpoint_epoch_N.state_dict.pt (and its siblings optimizer_epoch_N.pt, '
                                                   'ema_epoch_N.pt): continue at epoch N + 1 of --epochs')
    ap.add_argument('--init_from', default=None, help='a checkpoint load_checkpoint reads (the reference\'s pickles and module.-prefixed '
                                                      'state dicts included): weights and BatchNorm buffers only, training starts at epoch 0 '
                                                      'with a fresh optimizer -- the fine-tuning start')
    ap.add_argument('--freeze', nargs='+', default=[], metavar='PREFIX',
                    help='state-dict name prefixes whose parameters are not trained, e.g. inc down1 down2 down3 down4 (the encoder)')
    ap.add_argument('--frozen_bn', action='store_true', help='BatchNorm on its running statistics, which stay as loaded')
    ap.add_argument('--no_decay_norm_bias', action='store_true', help='no weight decay on BatchNorm weights / biases and conv biases')
    ap.add_argument('--lr_scale', nargs='+', default=[], type=_lr_scale, metavar='PREFIX=FACTOR',
                    help='learning rate x FACTOR for the parameters under PREFIX, e.g. inc=0.1 down1=0.1')
    ap.add_argument('--device_patches', type=lambda s: s.lower() in ('1', 'true', 'yes'), default=False,
                    help='cut and augment the patch pairs on the device from city stacks kept in HBM (fabric_amd.device_loader) '
                         'instead of on the host; --num_workers does not apply then')
    ap.add_argument('--aug_jitter', type=int, default=0, metavar='N',
                    help='--device_patches true: move every crop origin by up to N pixels on either axis, off the stride grid (clamped into '
                         'the city).  Any --aug_* flag switches the training loader to the counter-based draws of fabric_amd.augment')
    ap.add_argument('--aug_gain', type=float, default=0.0, metavar='F', help='per date and band: x *= 1 + F u, u uniform in [-1, 1)')
    ap.add_argument('--aug_bias', type=float, default=0.0, metavar='F', help='per date and band: x += F u, u uniform in [-1, 1)')
    ap.add_argument('--aug_shared_dates', action='store_true', help='one --aug_gain / --aug_bias draw per band for both dates')
    ap.add_argument('--aug_noise', type=float, default=0.0, metavar='F', help='additive Gaussian noise of standard deviation F')
    ap.add_argument('--aug_erase_p', type=float, default=0.0, metavar='F',
                    help='probability that a sample loses a rectangle (--aug_erase_size) on every band of both dates; its labels become '
                         '--ignore_label when that is set and are kept otherwise')
    ap.add_argument('--aug_erase_size', type=int, nargs=2, default=None, metavar=('LO', 'HI'), help='sides of the erased rectangle, drawn in LO..HI pixels')
    ap.add_argument('--aug_seed', type=int, default=None, metavar='N', help='seed of the augmentation draws (default: --seed)')
    ap.add_argument('--aug_rotate', type=float, default=0.0, metavar='DEG',
                    help='--device_patches true: rotate every patch pair by an angle uniform in [-DEG, DEG] (bilinear taps; fabric_amd.augment.'
                         'PatchWarp).  Label pixels whose source lies outside the city become --ignore_label when that is set')
    ap.add_argument('--aug_scale', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                    help='zoom every patch pair by a factor log-uniform in [LO, HI], 1/8 <= LO <= HI <= 8; above 1 magnifies')
    ap.add_argument('--aug_misreg', type=float, default=0.0, metavar='PX',
                    help='misregistration: sample date 2 shifted against date 1 by up to PX pixels on either axis; the labels follow date 1')
    ap.add_argument('--mix_p', type=float, default=0.0, metavar='F',
                    help='--device_patches true: probability that a training sample takes pixels of another one (a donor) on both dates '
                         'and in the labels (fabric_amd.augment.PatchMix); the epoch record gains train_mix_frac')
    ap.add_argument('--mix_mode', default='box', choices=['box', 'object'],
                    help='box: a rectangle of the donor (CutMix; --mix_box); object: the donor\'s change pixels (label 1), dilated by --mix_margin')
    ap.add_argument('--mix_box', type=int, nargs=2, default=None, metavar=('LO', 'HI'), help='sides of the pasted rectangle, drawn in LO..HI pixels')
    ap.add_argument('--mix_margin', type=int, default=0, metavar='M', help='--mix_mode object: paste a ring of M pixels (0..16) around the change pixels too')
    ap.add_argument('--mix_donors', default='all', choices=['all', 'change'],
                    help='the donor pool: every training patch, or those with at least --mix_min_pixels change pixels at their grid position')
    ap.add_argument('--mix_min_pixels', type=int, default=1, metavar='K', help='--mix_donors change: the fewest change pixels a donor holds')
    ap.add_argument('--scene_stride', type=int, default=0,
                    help='full validation scenes: 0 = the reference\'s non-overlapping argmax masks (predict_scene); N > 0 = tiles every N px, '
                         'softmax probabilities blended (predict_scene_blended), also writes {city}_epoch_{e}_proba.png and a scene F1 line')
    ap.add_argument('--scene_window', default='gaussian', choices=['gaussian', 'flat'], help='blending weights of --scene_stride N > 0')
    ap.add_argument('--scene_tta', type=int, default=1, choices=[1, 2, 4, 8],
                    help='symmetries of the square averaged per tile with --scene_stride N > 0: codes (0,), (0,1), (0,1,2,3), 0..7')
    ap.add_argument('--val_curve_bins', type=int, default=0, metavar='N',
                    help='0: off; a power of two in 2..4096: the validation pass also builds the precision / recall curve of class 1 over N '
                         'score bins on the device (ScoreCurve) and the epoch record and the checkpoint metadata gain validate_best_f1, '
                         'validate_best_threshold and validate_ap; with --scene_stride N > 0 the scene line gains ap, best_f1, best_threshold')
    ap.add_argument('--scene_threshold', default='argmax', metavar='argmax|val|FLOAT',
                    help='--scene_stride N > 0: the full-scene masks are the argmax (default), or P(change) >= the best-F1 threshold of '
                         'this epoch\'s validation pass (val; needs --val_curve_bins), or >= a fixed FLOAT in [0, 1]')
    ap.add_argument('--scene_min_area', type=int, default=0, metavar='N',
                    help='--scene_stride N > 0: connected components of the scene mask below N pixels are removed on the device before the '
                         'PNG is written (remove_small_objects); 0: off')
    ap.add_argument('--scene_objects', type=lambda s: s.lower() in ('1', 'true', 'yes'), default=False,
                    help='--scene_stride N > 0: the scene line gains objects_pred, objects_true, object_precision, object_recall, object_f1 '
                         'and min_area (object_scores on the unfiltered mask with min_area = --scene_min_area; --ignore_label pixels are cut out '
                         'before the areas are measured)')
    ap.add_argument('--scene_connectivity', type=int, default=8, choices=[4, 8],
                    help='connectivity of --scene_min_area / --scene_objects / --scene_hysteresis / --scene_fill_holes')
    ap.add_argument('--scene_hysteresis', type=float, default=None, metavar='LOW',
                    help='--scene_stride N > 0 with --scene_threshold val|FLOAT: P(change) >= LOW is kept where its connected component reaches '
                         'P(change) >= the threshold (hysteresis_mask, on the device); LOW <= the threshold')
    ap.add_argument('--scene_close', type=int, default=None, metavar='R2',
                    help='--scene_stride N > 0: the scene mask is closed with the disc dy^2 + dx^2 <= R2 on the device (binary_closing)')
    ap.add_argument('--scene_fill_holes', type=int, default=0, metavar='N',
                    help='--scene_stride N > 0: holes of the scene mask are filled on the device (fill_holes): -1 every hole, N > 0 the holes '
                         'of at most N pixels; 0: off')
    ap.add_argument('--scene_open', type=int, default=None, metavar='R2',
                    help='--scene_stride N > 0: the scene mask is opened with the disc dy^2 + dx^2 <= R2 on the device (binary_opening).  Order: '
                         'threshold or hysteresis, closing, hole filling, opening, --scene_min_area; the scene line gains cleanup and cleaned')
    ap.add_argument('--scene_auto_threshold', type=str, default=None, metavar='METHOD',
                    help='--scene_stride N > 0 with --scene_threshold argmax: the scene masks are P(change) >= a threshold selected on the device '
                         'from the histogram of the scene probabilities, by otsu, kittler, rosin or em (utils/thresholds.py: no labels, no '
                         'validation pass); the scene line gains auto_threshold {method, value, bin, ok}')
    ap.add_argument('--scene_mad_baseline', type=str, default=None, metavar='METHOD',
                    help='--scene_stride N > 0: the scene line gains mad_baseline, the counts of the label-free baseline on the scene pair: IR-MAD '
                         '(utils/mad.py) and its chi2 thresholded by otsu, kittler, rosin or em (auto_change_mask); --ignore_label pixels are '
                         'left out of the statistic and of the counts')
    ap.add_argument('--scene_mad_iters', type=int, default=None, metavar='N',
                    help='the iterations of --scene_mad_baseline (default 30)')
    ap.add_argument('--coregister', type=int, default=0, metavar='R',
                    help='align date 2 of every city to its date 1 once after loading, on the device (utils/registration.py): the shift is '
                         'searched over +-R pixels (1..16) by normalised cross-correlation and date 2 is resampled bilinearly; 0: off.  '
                         'With --ignore_label V, label pixels whose date-2 taps fall outside the scene become V')
    ap.add_argument('--coregister_cells', type=int, nargs=2, default=[1, 1], metavar=('NY', 'NX'),
                    help='--coregister: estimate one shift per cell of an NY x NX grid (1..64 each) and interpolate between the cell centres')
    ap.add_argument('--coregister_bands', nargs='+', default=None, metavar='BAND', help='--coregister: the bands correlated, by id or index (default: all)')
    ap.add_argument('--coregister_min_ncc', type=float, default=0.0, metavar='F',
                    help='--coregister: a cell whose peak correlation is below F takes the whole-scene shift')
    ap.add_argument('--synthetic_misreg', type=int, nargs=2, default=[0, 0], metavar=('DY', 'DX'),
                    help='--synthetic: shift date 2 of every city by DY DX pixels (integers, replicated edge)')
    ap.add_argument('--radiometric', default=None, choices=['none', 'histogram', 'range'],
                    help='match the radiometry of date 2 of every city to its date 1 once after loading (and after --coregister), on the '
                         'device (utils/radiometry.py): histogram = quantile transfer through --radiometric_knots knots per band; range = '
                         'the line that carries the two --radiometric_range quantiles of date 2 onto those of date 1; none (default): off.  '
                         '--ignore_label pixels take no part in the fit; --resume keeps the setting of the run it continues')
    ap.add_argument('--radiometric_knots', type=int, default=None, metavar='K', help='--radiometric histogram: knots per band, 2..1024 (default 256)')
    ap.add_argument('--radiometric_range', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                    help='--radiometric range: the two quantiles matched (default 0.02 0.98)')
    ap.add_argument('--radiometric_bands', nargs='+', default=None, metavar='BAND', help='--radiometric: the bands matched, by id or index (default: all)')
    ap.add_argument('--radiometric_invariant', default=None, choices=['mad'],
                    help='--radiometric: fit the transfer on invariant pixels only, found without labels by IR-MAD on the device '
                         '(utils/mad.py): the pixels whose no-change probability reaches --mad_invariant_min.  One `mad` log line per city; '
                         'recorded in the checkpoint metadata and taken back by --resume')
    ap.add_argument('--mad_iters', type=int, default=None, metavar='N', help='--radiometric_invariant mad: at most N iterations, 1..1000 (default 30)')
    ap.add_argument('--mad_tol', type=float, default=None, metavar='F',
                    help='--radiometric_invariant mad: stop once the canonical correlations move by less than F (default 1e-3; 0: never)')
    ap.add_argument('--mad_invariant_min', type=float, default=None, metavar='P',
                    help='--radiometric_invariant mad: the no-change probability from which a pixel counts as invariant (default 0.95)')
    ap.add_argument('--synthetic_radiometry', type=float, nargs=2, default=None, metavar=('GAIN', 'BIAS'),
                    help='--synthetic: date 2 of every city becomes GAIN * x + BIAS')
    ap.add_argument('--metadata', default=None, help="JSON in the reference's metadata.json schema (band_ids, band_means, "
                                                     "band_stds, ...): its entries become defaults like utils/parser.py:7-10")
    pre, _ = ap.parse_known_args(argv)
    meta = {}
    if pre.metadata:
        with open(pre.metadata) as fh:
            meta = json.load(fh)
        ap.set_defaults(**{k: v for k, v in meta.items() if k in DEFAULTS})
    opt = ap.parse_args(argv)
    for k in ('band_ids', 'band_means', 'band_stds'):
        setattr(opt, k, meta.get(k))
    from .criterion import COMPOUND, LOVASZ_NAMES
    if opt.loss_function in COMPOUND and not opt.fused_step:
        raise SystemExit(f'--loss_function {opt.loss_function} is a compound criterion of the fused step: add --fused_step true')
    if opt.loss_function in LOVASZ_NAMES and not opt.fused_step:
        raise SystemExit(f'--loss_function {opt.loss_function} is a criterion of the fused step (the Lovasz-Softmax term): add --fused_step true')
    if opt.loss_function not in ('tversky', 'dice', 'jaccard', 'focal') + COMPOUND + LOVASZ_NAMES:
        raise SystemExit(f'--loss_function {opt.loss_function}: the reference offers bce / focal / dice / jaccard / tversky '
                         f"(utils/helpers.py:288-314); its bce branch cannot run on BiDateNet's logits and is not built")
    if 'focal' in opt.loss_function.split('+') and opt.focal_gamma is None:
        raise SystemExit(f'--loss_function {opt.loss_function} needs --focal_gamma')
    if opt.ignore_label is not None:
        if not opt.fused_step:
            raise SystemExit(f'--ignore_label {opt.ignore_label} is built into the criterion of the fused step: add --fused_step true')
        if not 0 <= opt.ignore_label <= 255:
            raise SystemExit(f'--ignore_label {opt.ignore_label}: a label byte 0..255')
        if not 0.0 <= opt.synthetic_ignore_frac < 1.0:
            raise SystemExit(f'--synthetic_ignore_frac {opt.synthetic_ignore_frac}: a fraction in [0, 1)')
    if opt.loss_topk is not None:
        if 'focal' not in opt.loss_function.split('+'):
            raise SystemExit(f'--loss_topk {opt.loss_topk} ranks the focal term: --loss_function {opt.loss_function} has none '
                             f'(focal, focal+dice, focal+jaccard, focal+tversky, focal+lovasz)')
        if not opt.fused_step:
            raise SystemExit(f'--loss_topk {opt.loss_topk} is built into the criterion of the fused step: add --fused_step true')
        if not 0.0 < opt.loss_topk <= 1.0:
            raise SystemExit(f'--loss_topk {opt.loss_topk}: a fraction 0 < F <= 1')
    try:
        opt.label_smoothing = resolve_label_smoothing(opt.label_smoothing, opt.fused_step, opt.loss_topk,
                                                      checkpoint_label_smoothing(opt.resume) if opt.resume else None)
    except ValueError as e:
        raise SystemExit(str(e))
    try:
        scene_boundary_tol = check_boundary_flags(opt.boundary_weight, opt.boundary_classes, opt.boundary_max_dist, opt.fused_step,
                                                  opt.scene_boundary_tol, opt.scene_stride)
    except ValueError as e:
        raise SystemExit(str(e))
    step_criterion = None                                  # --fused_step true: ONE Criterion for the step and for validation
    if opt.fused_step:
        from .utils.helpers import criterion_from_opt
        try:
            step_criterion = criterion_from_opt(opt)
        except ValueError as e:
            raise SystemExit(f'--loss_function {opt.loss_function}: {e}')
    from .optim import OptimConfig
    try:
        OptimConfig(opt.optimizer, lr=opt.learning_rate, momentum=opt.momentum, nesterov=opt.nesterov, weight_decay=opt.weight_decay,
                    betas=opt.betas, eps=opt.adam_eps, **layerwise_kwargs(opt))
    except ValueError as e:
        raise SystemExit(f'--optimizer {opt.optimizer}: {e}')
    layerwise = opt.optimizer in ('lamb', 'lars')
    scheduled = opt.lr_warmup_updates != 0 or opt.lr_schedule != 'constant' or opt.lr_min != 0.0
    if (layerwise or scheduled) and opt.loss_function != 'tversky' and not opt.fused_step:
        raise SystemExit(f'--optimizer lamb / lars and --lr_warmup_updates / --lr_schedule / --lr_min are built into the fused step, which '
                         f'runs --loss_function tversky only (got {opt.loss_function}) unless --fused_step true is given')
    grouped = bool(opt.freeze or opt.frozen_bn or opt.no_decay_norm_bias or opt.lr_scale)
    if grouped and opt.loss_function != 'tversky' and not opt.fused_step:
        raise SystemExit(f'--freeze / --frozen_bn / --no_decay_norm_bias / --lr_scale are built into the fused step, which runs '
                         f'--loss_function tversky only (got {opt.loss_function}) unless --fused_step true is given')
    from .optim import check_accumulate, check_max_grad_norm
    try:
        check_accumulate(opt.accumulate)
        check_max_grad_norm(opt.max_grad_norm)
    except ValueError as e:
        raise SystemExit(f'--accumulate / --max_grad_norm: {e}')
    if (opt.accumulate != 1 or opt.max_grad_norm is not None) and opt.loss_function != 'tversky' and not opt.fused_step:
        raise SystemExit(f'--accumulate / --max_grad_norm are built into the fused step, which runs --loss_function tversky only '
                         f'(got {opt.loss_function}) unless --fused_step true is given')
    try:
        sam = sam_kwargs(opt)
    except ValueError as e:
        raise SystemExit(str(e))
    from .optim import check_ema
    try:
        averaging =check_ema(opt.ema_decay, 'swa' if opt.swa else 'ema', opt.ema_every, opt.ema_start)[0]
    except ValueError as e:
        raise SystemExit(f'--ema_decay / --swa / --ema_every / --ema_start: {e}')
    if (averaging or opt.ema_every != 1 or opt.ema_start != 0 or not opt.ema_buffers) and not opt.fused_step:
        raise SystemExit('--ema_decay / --swa / --ema_every / --ema_start / --ema_buffers are built into the fused step: add --fused_step true')
    if not averaging and (opt.ema_every != 1 or opt.ema_start != 0 or not opt.ema_buffers):
        raise SystemExit('--ema_every / --ema_start / --ema_buffers shape an average that is not on: add --ema_decay D or --swa')
    try:
        scene_thr = check_curve_flags(opt.val_curve_bins, opt.scene_threshold, opt.scene_stride)
        scene_min_area = check_object_flags(opt.scene_min_area, opt.scene_objects, opt.scene_connectivity, opt.scene_stride)
        scene_cleanup = check_cleanup_flags(opt.scene_hysteresis, opt.scene_close, opt.scene_fill_holes, opt.scene_open, scene_thr,
                                            opt.scene_connectivity, opt.scene_stride)
        kept = {k: checkpoint_entry(opt.resume, k) for k in ('scene_auto_threshold', 'scene_mad_baseline')} if opt.resume else None
        scene_auto, scene_mad = check_auto_threshold_flags(opt.scene_auto_threshold, opt.scene_mad_baseline, opt.scene_mad_iters, scene_thr,
                                                           opt.scene_stride, kept)
    except ValueError as e:
        raise SystemExit(str(e))
    try:
        coreg = check_coregister_flags(opt.coregister, opt.coregister_cells, opt.coregister_bands, opt.coregister_min_ncc, opt.band_ids, 13,
                                       opt.synthetic_misreg, opt.synthetic)
    except ValueError as e:
        raise SystemExit(str(e))
    try:
        radiom = check_radiometric_flags(opt.radiometric, opt.radiometric_knots, opt.radiometric_range, opt.radiometric_bands, opt.band_ids, 13,
                                         opt.synthetic_radiometry, opt.synthetic, checkpoint_radiometric(opt.resume) if opt.resume else None)
        mad_kw = check_mad_flags(opt.radiometric_invariant, opt.mad_iters, opt.mad_tol, opt.mad_invariant_min, radiom,
                                 checkpoint_radiometric(opt.resume) if opt.resume else None, explicit=opt.radiometric not in (None, 'none'))
        if mad_kw:                                         # without the flag the dict, and with it every call, stays what it was
            radiom = dict(radiom, **mad_kw)
    except ValueError as e:
        raise SystemExit(str(e))
    if opt.init_from and opt.resume:
        raise SystemExit('--init_from starts a run from given weights, --resume continues one: give one of them')
    from .utils.helpers import checkpoint_fusion
    ckpt = opt.resume or opt.init_from
    try:
        fusion, fusion_note = resolve_fusion(opt.fusion, (checkpoint_fusion(ckpt) or 'product') if ckpt else None, resume=bool(opt.resume))
    except ValueError as e:
        raise SystemExit(str(e))
    try:
        patch_augment = augment_from_opt(opt)
        patch_warp = warp_from_opt(opt) if patch_augment is not None else None
        patch_mix = mix_from_opt(opt) if patch_augment is not None else None
    except ValueError as e:
        raise SystemExit(str(e))

    # one process per GPU (launched by torch.distributed.run): RANK / LOCAL_RANK / WORLD_SIZE from the environment
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(dev)                            # the library's stream / workspace helpers follow the current device
    if world > 1:
        import torch.distributed as dist
        from .parallel import init_rccl
        init_rccl(rank, world, dev)

    import random
    random.seed(opt.seed)                                  # same dataset order / initial weights on every rank; augmentation draws
    torch.manual_seed(opt.seed)                            # (global `random`, utils/dataloaders.py:150-156) are re-seeded per rank below
    scenes = None
    if opt.synthetic:
        data = synthetic_onera(n_cities=6, bands=13, size=(360, 360), **(
            {} if opt.ignore_label is None else dict(ignore_frac=opt.synthetic_ignore_frac, ignore_value=opt.ignore_label)),
            **({} if tuple(opt.synthetic_misreg) == (0, 0) else dict(misreg=tuple(opt.synthetic_misreg))),
            **({} if opt.synthetic_radiometry is None else dict(radiometry=tuple(opt.synthetic_radiometry))))
        if coreg is not None:
            coregister_loaded(data, coreg, opt.ignore_label, dev, log=rank == 0)
        if radiom is not None:                             # after the alignment: resampling moves the histogram slightly
            normalize_loaded(data, radiom, opt.ignore_label, dev, log=rank == 0)
        val_cities = ['city4', 'city5']
    else:
        if not opt.band_ids:
            raise SystemExit('real data needs --metadata with band_ids / band_means / band_stds (the reference keeps them in '
                             'metadata.json); or use --synthetic')
        from .utils import ingest
        scenes = ingest.full_onera_loader(opt.dataset_dir, opt, device=dev)      # city stacks stay in HBM for the scene pass
        if coreg is not None:                              # before the loaders' views and copies of the stacks are made
            coregister_loaded(scenes, coreg, opt.ignore_label, dev, log=rank == 0)
        if radiom is not None:
            normalize_loaded(scenes, radiom, opt.ignore_label, dev, log=rank == 0)
        if opt.device_patches:                            # the patch sampler reads the same HBM stacks: no round trip through the host
            data = {c: {'images': d['images'], 'labels': d['labels']} for c, d in scenes.items()}
        else:
            data = {c: {'images': d['images'].cpu().numpy(), 'labels': d['labels']} for c, d in scenes.items()}
        val_cities = [c for c in opt.validation_cities if c in data]
    stride = opt.stride // 2 if opt.synthetic else opt.stride
    if opt.device_patches:
        train_loader, val_loader = make_device_loaders(data, val_cities, opt.patch_size, stride, opt.batch_size, opt.augmentation,
                                                       rank=rank, world_size=world, seed=opt.seed, device=dev,
                                                       **({} if patch_augment is None else dict(augment=patch_augment)),
                                                       **({} if patch_warp is None else dict(warp=patch_warp)),
                                                       **({} if patch_mix is None else dict(mix=patch_mix)))
        if patch_mix is not None and opt.mix_donors == 'change':      # the pool: training patches that hold change at their grid position
            try:
                train_loader.mix = patch_mix.donors_from(train_loader.label_counts(1), opt.mix_min_pixels)
            except ValueError as e:
                raise SystemExit(str(e))
    else:
        train_loader, val_loader = make_loaders(data, val_cities, opt.patch_size, stride, opt.batch_size, opt.augmentation,
                                                num_workers=opt.num_workers, rank=rank, world_size=world, seed=opt.seed)
    random.seed(opt.seed * 7919 + rank)                    # different augmentation draws per rank from here on
    model = BiDateNet(len(opt.band_ids) if opt.band_ids else 13, 2, precision=opt.precision, fusion=fusion).to(dev)
    opt_sd, first_epoch = None, 0
    if opt.resume:
        model, opt_sd, first_epoch = resume_from(opt.resume, dev, opt.precision)      # the fusion comes back from the metadata
    elif opt.init_from:
        from .utils.helpers import load_checkpoint
        model = load_checkpoint(opt.init_from, device=dev, precision=opt.precision, fusion=fusion)
        if fusion_note and rank == 0:
            print(fusion_note, flush=True)
    fused = opt.fused_step or opt.loss_function == 'tversky'
    from .input_pipeline import DeviceFeeder
    from .utils.helpers import get_criterion
    # ONE feeder (copy stream, staging threads, device slots) for the whole run; device-sampled batches need none
    feeder = None if opt.device_patches else DeviceFeeder(dev)
    if step_criterion is not None:
        from .utils.metrics import CompoundLoss
        criterion = CompoundLoss(step_criterion)           # the step's own Criterion, through its autograd module
    else:
        criterion = get_criterion(opt)                     # validation reports the criterion the run optimises (train.py:137)
    if fused:
        try:
            groups = fine_tune_groups(model, opt.learning_rate, opt.weight_decay, opt.freeze, opt.no_decay_norm_bias, opt.lr_scale)
            step = TrainStep(model, lr=opt.learning_rate, tversky_alpha=opt.tversky_alpha, tversky_beta=opt.tversky_beta,
                             param_groups=groups, bn='frozen' if opt.frozen_bn else 'batch', criterion=step_criterion,
                             accumulate=opt.accumulate, max_grad_norm=opt.max_grad_norm, ema_decay=opt.ema_decay,
                             average='swa' if opt.swa else 'ema', ema_every=opt.ema_every, ema_start=opt.ema_start,
                             ema_buffers=opt.ema_buffers, **optimizer_kwargs(opt), **sam)
        except ValueError as e:
            raise SystemExit(f'parameter groups: {e}')
        if opt_sd is not None:
            step.load_optimizer_state_dict(opt_sd)
        if averaging and opt.resume:                       # the averaged weights of the epoch resumed from, when that run kept them
            ema_path = os.path.join(os.path.dirname(opt.resume), f'ema_epoch_{first_epoch - 1}.pt')
            if os.path.exists(ema_path):
                step.load_ema_state_dict(torch.load(ema_path, map_location='cpu', weights_only=True))
        if world > 1:
            # measure (and, if it is the slow one, repair) the placement of RCCL's collective stream BEFORE the loop adopts the chain's stream
            rep = step.guard_collectives(opt.batch_size, opt.patch_size, opt.patch_size)
            if rank == 0:
                print(json.dumps({'collectives_guard': rep}), flush=True)
    else:
        optimizer = make_torch_optimizer(model.parameters(), opt.learning_rate, **optimizer_kwargs(opt))      # train.py:55
        if opt_sd is not None:
            optimizer.load_state_dict(opt_sd)
        if world > 1:
            for p in model.parameters():
                dist.broadcast(p.data, src=0)
    best = {'cd_f1scores': -1, 'cd_recalls': -1, 'cd_precisions': -1}              # train.py:62
    val_curve = None
    if opt.val_curve_bins:
        from .utils.metrics import ScoreCurve
        val_curve = ScoreCurve(opt.val_curve_bins, 1, opt.ignore_label)
    run_meta = dict(meta, **{k: getattr(opt, k) for k in DEFAULTS}, precision=opt.precision, fusion=model.fusion, world_size=world)
    if coreg is not None:                                  # a checkpoint says how its training pairs were aligned
        run_meta['coregister'] = dict(coreg, cells=list(coreg['cells']))
    if radiom is not None:                                 # ... and how date 2 was matched: --resume reads it back
        run_meta['radiometric'] = dict(radiom)
    if opt.label_smoothing:                                # the criterion's smoothed targets: --resume reads it back
        run_meta['label_smoothing'] = opt.label_smoothing
    if scene_cleanup is not None:                          # how the scene masks written beside this checkpoint were cleaned
        run_meta['scene_cleanup'] = dict(scene_cleanup, connectivity=opt.scene_connectivity)
    if scene_auto is not None:                             # the label-free threshold of the scene masks: --resume reads it back
        run_meta['scene_auto_threshold'] = scene_auto
    if scene_mad is not None:
        run_meta['scene_mad_baseline'] = dict(scene_mad)
    schedule = None
    if scheduled:                                          # host floats only; its position comes from (epoch, batch), so --resume continues it
        from .schedule import LRSchedule
        try:
            schedule = LRSchedule(opt.learning_rate, opt.epochs * LRSchedule.updates_per_epoch(len(train_loader), opt.accumulate),
                                  opt.lr_warmup_updates, opt.lr_schedule, opt.lr_min,
                                  None if groups is None else [g['lr'] for g in groups])      # the flags' values, not a resumed state's
        except ValueError as e:
            raise SystemExit(f'--lr_warmup_updates / --lr_schedule / --lr_min: {e}')
    for epoch in range(first_epoch, opt.epochs):
        train_loader.sampler.set_epoch(epoch)
        if fused and schedule is not None:
            tr = train_epoch(step, train_loader, dev, opt.patch_size, feeder, schedule, epoch)
        elif fused:
            tr = train_epoch(step, train_loader, dev, opt.patch_size, feeder)
        else:
            tr = train_epoch_autograd(model, criterion, optimizer, train_loader, dev, opt.patch_size, world, feeder)
        if patch_mix is not None:                              # this rank's share of mixed samples: host counts of the loader's plans
            tr['mix_frac'] = train_loader.mixed / max(train_loader.seen, 1)
        with step.ema_weights() if averaging else contextlib.nullcontext():       # --ema_decay / --swa: evaluate the averaged weights
            if val_curve is None:
                va = validate(model, val_loader, dev, opt.patch_size, criterion, feeder, ignore_index=opt.ignore_label)
            else:
                va = validate(model, val_loader, dev, opt.patch_size, criterion, feeder, ignore_index=opt.ignore_label, curve=val_curve,
                              world=world)
            if rank == 0:
                print(json.dumps({'epoch': epoch, **{'train_' + k: float(v) for k, v in tr.items()},
                                  **{'validate_' + k: float(v) for k, v in va.items()},
                                  **({'ema_n_averaged': step.n_averaged} if averaging else {})}), flush=True)
            if scenes is not None and rank == 0:               # train.py:182-205: full validation images
                _predict_scenes(model, scenes, val_cities, opt, epoch, va['best_threshold'] if scene_thr == 'val' else
                                None if scene_thr == 'argmax' else scene_thr, min_area=scene_min_area,
                                **({} if scene_boundary_tol is None else {'boundary_tol': scene_boundary_tol}),
                                **({} if scene_cleanup is None else {'cleanup': scene_cleanup}),
                                **({} if scene_auto is None else {'auto_threshold': scene_auto}),
                                **({} if scene_mad is None else {'mad_baseline': scene_mad}))
        if rank == 0:                                          # replica 0's BatchNorm buffers, like DataParallel
            best = save_if_better(model, va, best, run_meta, epoch, opt.log_dir,
                                  step.optimizer_state_dict() if fused else optimizer.state_dict(),
                                  step.ema_state_dict if averaging else None)
    if feeder is not None:
        feeder.close()
    if world > 1:
        dist.destroy_process_group()


def mad_baseline_scores(d1, d2, label, ignore_label, device, method, iters):
    """The label-free baseline of one scene pair: irmad + auto_change_mask(method) on the device, scored against the label raster like the
    `cleaned` entry.  Pixels with label == ignore_label take no part in the statistic, the histogram or the counts."""
    from .utils.mad import auto_change_mask, irmad
    g1 = torch.as_tensor(d1).to(device=device, dtype=torch.float32).contiguous()
    g2 = torch.as_tensor(d2).to(device=device, dtype=torch.float32).contiguous()
    exclude = None if ignore_label is None else torch.as_tensor(np.asarray(label)).to(device=device, dtype=torch.uint8).contiguous()
    res = irmad(g1, g2, exclude=exclude, exclude_value=ignore_label, iters=iters)
    mask, table = auto_change_mask(res, method)
    d = table.read()[method]
    return dict({'method': method, 'threshold': d['value'] if d['ok'] else None, 'iters': res.read()['iters']},
                **cleaned_scores(mask.cpu().numpy(), label, ignore_label))


def _predict_scenes(model, scenes, val_cities, opt, epoch, threshold=None, min_area=None, boundary_tol=None, cleanup=None,
                    auto_threshold=None, mad_baseline=None):
    """train.py:182-205: the full validation scenes of one epoch, written as PNG masks (and, blended, as probabilities with a scene F1 line).
    threshold (--scene_threshold): None = the argmax masks, else the masks are P(change) >= threshold.  With --val_curve_bins the scene
    line of every city comes from a ScoreCurve over its probabilities and label raster (the run's --ignore_label left out), on the device:
    ap, best_f1, best_threshold, and tp / fp / fn / precision / recall / f1 at the applied threshold (0.5 for the argmax masks),
    rounded down to a bin edge.
    min_area (--scene_min_area, from check_object_flags): the components of the mask below that many pixels are removed before the PNG is
    written and the pixel counts are taken.  With --scene_objects the objects are scored on the unfiltered mask by
    object_scores(mask, truth, ignore_index=--ignore_label, min_area=min_area): the ignore pixels are cut out BEFORE the areas are
    measured, so a component held above min_area only by pixels inside the ignore region is no object, although the PNG keeps it.
    boundary_tol (--scene_boundary_tol, from check_boundary_flags): the scene line gains boundary_precision, boundary_recall, boundary_f1,
    hausdorff and boundary_tol from boundary_scores(the mask that is written, truth, boundary_tol, ignore_index=--ignore_label).
    cleanup (--scene_hysteresis / --scene_close / --scene_fill_holes / --scene_open, from check_cleanup_flags): the keyword arguments of
    predict_scene_blended that clean the mask on the device, before the area filter: --scene_objects then scores the mask after the
    opening.  The scene line gains cleanup (the settings) and cleaned = {tp, fp, fn, precision, recall, f1} of the mask that is written
    against the labels (--ignore_label left out): with --val_curve_bins the other counts come from the probabilities.
    auto_threshold (--scene_auto_threshold, from check_auto_threshold_flags): the method of predict_scene_blended's auto_threshold; the
    scene line gains auto_threshold = {method, value, bin, ok} (value None when the rule found no split: the mask is then empty), and its
    tp / fp / fn / precision / recall / f1 are those of the mask that is written (--ignore_label left out).
    mad_baseline (--scene_mad_baseline, from check_auto_threshold_flags): {'method', 'iters'}; the scene line gains mad_baseline =
    {method, threshold, iters, tp, fp, fn, precision, recall, f1} of irmad + auto_change_mask on the scene pair, the label's
    --ignore_label pixels excluded from the statistic and from the counts (iters: the iterations IR-MAD ran before it converged)."""
    from .utils import ingest
    from .utils.inference import predict_scene, predict_scene_blended, TTA_SYMMETRIES
    os.makedirs(opt.log_dir, exist_ok=True)
    model.eval()
    scene_counts = {}
    conn = getattr(opt, 'scene_connectivity', 8)
    objects = getattr(opt, 'scene_objects', False)
    for city in val_cities:
        st = scenes[city]['images']
        selected = {}
        if opt.scene_stride > 0:
            proba, mask = predict_scene_blended(model, st[0], st[1], patch_size=opt.patch_size, stride=opt.scene_stride,
                                                window=opt.scene_window, symmetries=TTA_SYMMETRIES[opt.scene_tta],
                                                batch_size=opt.batch_size, **({} if threshold is None else {'threshold': threshold}),
                                                **({} if min_area is None or objects else {'min_area': min_area}),
                                                **({} if (min_area is None or objects) and cleanup is None else {'connectivity': conn}),
                                                **(cleanup or {}),
                                                **({} if auto_threshold is None else {'auto_threshold': auto_threshold, 'threshold_out': selected}))
            raw = mask
            if min_area is not None and objects:             # the unfiltered mask is scored below; the same launches as min_area= above
                from .utils.objects import remove_small_objects
                mask = remove_small_objects(raw, min_area, conn)
            ingest.write_png_gray(os.path.join(opt.log_dir, f'{city}_epoch_{epoch}_proba.png'),
                                  torch.round(proba[1] * 255).to(torch.uint8).cpu().numpy())
            if getattr(opt, 'val_curve_bins', 0):
                from .utils.metrics import ScoreCurve
                sc = ScoreCurve(opt.val_curve_bins, 1, getattr(opt, 'ignore_label', None))
                sc.update_proba(proba, torch.as_tensor(scenes[city]['labels']).to(proba.device))
                c = sc.compute()
                scene_counts[city] = dict(sc.at(0.5 if threshold is None else threshold), ap=c['ap'], best_f1=c['best_f1'],
                                          best_threshold=c['best_threshold'], threshold='argmax' if threshold is None else threshold)
            else:
                scene_counts[city] = scene_scores(mask.cpu().numpy(), scenes[city]['labels'])
            if objects:
                from .utils.objects import object_scores
                truth = torch.as_tensor(scenes[city]['labels']).to(device=mask.device, dtype=torch.uint8).contiguous()
                obj = object_scores(raw, truth, 1, getattr(opt, 'ignore_label', None), conn, min_area or 1)
                scene_counts[city].update({k: obj[k] for k in ('objects_pred', 'objects_true', 'object_precision', 'object_recall',
                                                               'object_f1')})
            if min_area is not None or objects:
                scene_counts[city]['min_area'] = min_area or 1
            if cleanup is not None:
                scene_counts[city]['cleanup'] = dict(cleanup)
                scene_counts[city]['cleaned'] = cleaned_scores(mask.cpu().numpy(), scenes[city]['labels'], getattr(opt, 'ignore_label', None))
            if auto_threshold is not None:
                d = selected['table'].read()[auto_threshold]
                scene_counts[city].update(cleaned_scores(mask.cpu().numpy(), scenes[city]['labels'], getattr(opt, 'ignore_label', None)))
                scene_counts[city]['auto_threshold'] = {'method': auto_threshold, 'value': d['value'] if d['ok'] else None, 'bin': d['bin'],
                                                        'ok': d['ok']}
            if mad_baseline is not None:
                scene_counts[city]['mad_baseline'] = mad_baseline_scores(st[0], st[1], scenes[city]['labels'], getattr(opt, 'ignore_label', None),
                                                                         proba.device, **mad_baseline)
            if boundary_tol is not None:
                from .utils.distance import boundary_scores
                truth = torch.as_tensor(scenes[city]['labels']).to(device=mask.device, dtype=torch.uint8).contiguous()
                bs = boundary_scores(mask.contiguous(), truth, boundary_tol, 1, getattr(opt, 'ignore_label', None))
                scene_counts[city].update({k: bs[k] for k in ('boundary_precision', 'boundary_recall', 'boundary_f1', 'hausdorff', 'boundary_tol')})
        else:
            mask = predict_scene(model, st[0], st[1], patch_size=opt.patch_size, batch_size=opt.batch_size)
        ingest.write_png_gray(os.path.join(opt.log_dir, f'{city}_epoch_{epoch}.png'), (mask * 255).cpu().numpy())
    if opt.scene_stride > 0:
        print(json.dumps({'epoch': epoch, 'scene': scene_counts}), flush=True)


if __name__ == '__main__':
    main()
