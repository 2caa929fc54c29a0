"""Glue with the reference's names and semantics (utils/helpers.py:24-89, 288-337) for the parts the
train step needs: running-mean metric dicts, criterion factory, model factory."""
import os

import numpy as np
import torch

from ..models.bidate_model import BiDateNet
from .metrics import CompoundLoss, FocalLoss, TverskyLoss, dice_loss, jaccard_loss


def initialize_metrics():
    """reference utils/helpers.py:24-42"""
    return {'cd_losses': [], 'cd_corrects': [], 'cd_precisions': [], 'cd_recalls': [], 'cd_f1scores': []}


def get_mean_metrics(metric_dict):
    """reference utils/helpers.py:45-59: arithmetic mean of the per-batch values (val F1 = mean of per-batch F1)."""
    return {k: np.mean(v) for k, v in metric_dict.items()}


def set_metrics(metric_dict, cd_loss, cd_corrects, cd_report):
    """reference utils/helpers.py:62-89"""
    metric_dict['cd_losses'].append(float(cd_loss))
    metric_dict['cd_corrects'].append(float(cd_corrects))
    metric_dict['cd_precisions'].append(cd_report[0])
    metric_dict['cd_recalls'].append(cd_report[1])
    metric_dict['cd_f1scores'].append(cd_report[2])
    return metric_dict


def get_criterion(opt):
    """reference utils/helpers.py:288-314.  `focal` reads opt.focal_gamma exactly like the reference (absent from
    metadata.json there, so it raises AttributeError unless the caller adds it); `bce` cannot run on BiDateNet's
    [B,2,H,W] logits with [B,H,W] labels in the reference either (shape mismatch inside BCEWithLogitsLoss)."""
    if '+' in str(opt.loss_function):                        # focal+dice / focal+jaccard / focal+tversky: one compound criterion
        return CompoundLoss(criterion_from_opt(opt))
    if opt.loss_function == 'focal':
        return FocalLoss(opt.focal_gamma)
    if opt.loss_function == 'dice':
        return dice_loss
    if opt.loss_function == 'jaccard':
        return jaccard_loss
    if opt.loss_function == 'tversky':
        return TverskyLoss(alpha=opt.tversky_alpha, beta=opt.tversky_beta)
    raise NotImplementedError(f'fabric_amd: loss_function={opt.loss_function!r}: the reference\'s BCEWithLogitsLoss '
                              f'branch fails on [B,2,H,W] logits vs [B,H,W] labels and is not built')


def criterion_from_opt(opt):
    """fabric_amd.criterion.Criterion of the --loss_function / --tversky_alpha / --tversky_beta / --focal_gamma / --focal_alpha /
    --loss_weights (W_FOCAL W_OVERLAP; focal+lovasz: W_FOCAL W_LOVASZ) / --ignore_label / --loss_topk / --lovasz_classes /
    --boundary_weight / --boundary_classes / --boundary_max_dist / --label_smoothing options; ValueError as Criterion.parse raises it."""
    from ..criterion import Criterion
    return Criterion.parse(opt.loss_function, tversky_alpha=getattr(opt, 'tversky_alpha', 0.5), tversky_beta=getattr(opt, 'tversky_beta', 0.5),
                           focal_gamma=getattr(opt, 'focal_gamma', None), focal_alpha=getattr(opt, 'focal_alpha', None),
                           weights=tuple(getattr(opt, 'loss_weights', None) or (1, 1)), ignore_index=getattr(opt, 'ignore_label', None),
                           topk=getattr(opt, 'loss_topk', None), lovasz_classes=getattr(opt, 'lovasz_classes', 'present'),
                           w_boundary=getattr(opt, 'boundary_weight', None) or 0.0,
                           boundary_classes=getattr(opt, 'boundary_classes', 'foreground'),
                           boundary_max_dist=getattr(opt, 'boundary_max_dist', None),
                           label_smoothing=getattr(opt, 'label_smoothing', None) or 0.0)


def get_loaders(opt):
    """reference utils/helpers.py:211-258, same signature and return value: (train_loader, val_loader) over OneraPreloader datasets
    built from `opt.dataset_dir` (OSCD layout), `opt.validation_cities`, `opt.patch_size`, `opt.stride`, `opt.augmentation`,
    `opt.batch_size`, `opt.num_workers` (+ `opt.band_ids / band_means / band_stds` for the ingest).  One process, no sharding: this is
    the reference's loader for the reference's loop; the data-parallel loop of fabric_amd.train uses make_loaders (per-rank shards)."""
    from . import ingest
    from .dataloaders import OneraPreloader
    train_samples, val_samples = ingest.get_train_val_metadata(opt.dataset_dir, opt.validation_cities, opt.patch_size, opt.stride)
    print('train samples : ', len(train_samples))
    print('val samples : ', len(val_samples))
    full_load = ingest.full_onera_loader(opt.dataset_dir, opt)
    train_dataset = OneraPreloader(opt.dataset_dir, train_samples, full_load, opt.patch_size, opt.augmentation)
    val_dataset = OneraPreloader(opt.dataset_dir, val_samples, full_load, opt.patch_size, False)
    train_loader = torch.utils.data.DataLoader(train_dataset, batch_size=opt.batch_size, shuffle=True, num_workers=opt.num_workers)
    val_loader = torch.utils.data.DataLoader(val_dataset, batch_size=opt.batch_size, shuffle=False, num_workers=opt.num_workers)
    return train_loader, val_loader


def load_model(opt, device, precision=None):
    """reference utils/helpers.py:317-337 builds nn.DataParallel(BiDateNet(13, 2)); here one process drives one
    GPU and gradients are exchanged by fabric_amd.parallel (RCCL), so the bare module is returned.  `opt.fusion`
    ('product' / 'absdiff'), when present, selects the date fusion."""
    return BiDateNet(13, 2, precision=precision, fusion=getattr(opt, 'fusion', None) or 'product').to(device)


def checkpoint_fusion(path):
    """The date fusion a checkpoint file of fabric_amd.train was trained with: the `fusion` entry of the metadata_epoch_N.json
    beside checkpoint_epoch_N.pt / checkpoint_epoch_N.state_dict.pt / ema_epoch_N.pt, or None (not such a file, no metadata,
    or metadata from before the entry existed)."""
    import json
    import re
    if not isinstance(path, (str, bytes)) and not hasattr(path, '__fspath__'):
        return None
    path = os.fsdecode(path)
    m = re.match(r'(?:checkpoint|ema)_epoch_(\d+)(?:\.state_dict)?\.pt$', os.path.basename(path))
    meta = os.path.join(os.path.dirname(path), f'metadata_epoch_{m.group(1)}.json') if m else None
    if meta is None or not os.path.exists(meta):
        return None
    with open(meta) as fh:
        return json.load(fh).get('fusion')


def strip_module_prefix(state_dict):
    """State dict saved from the reference's nn.DataParallel wrapper (utils/helpers.py:335): every key carries `module.`.
    Returns a dict with the prefix removed from the keys that have it (a bare-module state dict passes through unchanged)."""
    return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state_dict.items()}


def load_checkpoint(src, device=None, precision=None, allow_pickle=True, fusion=None):
    """A usable BiDateNet from anything the reference (or fabric_amd.train) leaves behind.

    `src` is a path / file object for torch.load, or an object already loaded:
      * the whole-module pickle of train.py:222 -- nn.DataParallel(BiDateNet) or a bare BiDateNet (the class paths
        `models.bidate_model.BiDateNet`, `models.unet_parts.*` resolve through the repo-root shims; run with the repo root on
        sys.path).  The DataParallel wrapper is dropped: here one process drives one GPU (fabric_amd.parallel);
      * a state dict, with or without the `module.` prefix of a DataParallel save, optionally nested under 'state_dict' / 'model';
      * the state dict of a torch.optim.swa_utils.AveragedModel of a BiDateNet (TrainStep.ema_state_dict(), the `ema_epoch_N.pt`
        fabric_amd.train writes): a dict whose keys are all `module.`-prefixed except an integer scalar `n_averaged`, which is dropped
        -- the result is a BiDateNet on the averaged weights.
    The result is always a fresh fabric_amd BiDateNet carrying the checkpoint's parameters AND BatchNorm buffers; the channel
    counts come from the tensors.  Mismatched / missing / unexpected keys raise (load_state_dict(strict=True)).
    The date fusion has no parameters, so no tensor records it: `fusion` when given, else the `fusion` attribute of a pickled BiDateNet,
    else what checkpoint_fusion() finds in the metadata beside a file fabric_amd.train wrote, else 'product' (the reference's).

    Trust: a file is first read with torch.load(weights_only=True) -- tensors and plain containers only, no code runs; that covers
    every state-dict form (incl. the `*.state_dict.pt` fabric_amd.train writes for interchange).  Only when that loader refuses the
    file (a whole-module pickle, train.py:222) is it unpickled in full, which EXECUTES whatever the pickle holds: pass
    allow_pickle=False to refuse such files when the checkpoint does not come from a trusted source."""
    obj = src
    if fusion is None:
        fusion = checkpoint_fusion(src)
    if isinstance(src, (str, bytes)) or hasattr(src, 'read') or hasattr(src, '__fspath__'):
        import pickle
        pos = src.tell() if hasattr(src, 'tell') else None
        try:
            obj = torch.load(src, map_location='cpu', weights_only=True)
        except (pickle.UnpicklingError, RuntimeError, AttributeError) as e:
            # a whole-module pickle needs the unpickler, not the tensors-only loader
            if not allow_pickle:
                raise RuntimeError('fabric_amd: this checkpoint is a whole-module pickle (train.py:222); loading it executes the pickle -- '
                                   'pass allow_pickle=True for files from a trusted source') from e
            if pos is not None:
                src.seek(pos)
            obj = torch.load(src, map_location='cpu', weights_only=False)
    if isinstance(obj, torch.nn.DataParallel) or (isinstance(obj, torch.nn.Module) and hasattr(obj, 'module')
                                                  and not isinstance(obj, BiDateNet)):
        obj = obj.module
    if isinstance(obj, torch.nn.Module):
        sd = obj.state_dict()
        if fusion is None:
            fusion = getattr(obj, 'fusion', None)
    elif isinstance(obj, dict):
        sd = obj
        for nest in ('state_dict', 'model'):
            if nest in sd and isinstance(sd[nest], dict):
                sd = sd[nest]
            elif nest in sd and isinstance(sd[nest], torch.nn.Module):
                return load_checkpoint(sd[nest], device, precision, allow_pickle, fusion)
    else:
        raise TypeError(f'fabric_amd: cannot load a checkpoint from {type(obj).__name__}')
    from ..optim import AVG_COUNT, is_averaged_state
    if is_averaged_state(sd):
        sd = {k: v for k, v in sd.items() if k != AVG_COUNT}
    sd = strip_module_prefix(sd)
    try:
        n_channels = int(sd['inc.conv.conv.0.weight'].shape[1])
        n_classes = int(sd['outc.conv.weight'].shape[0])
    except KeyError as e:
        raise RuntimeError(f'fabric_amd: not a BiDateNet checkpoint (missing {e.args[0]!r})') from None
    model = BiDateNet(n_channels, n_classes, precision=precision, fusion=fusion or 'product')
    model.load_state_dict(sd, strict=True)
    return model.to(device) if device is not None else model
