"""The augmentation policy of device-cut patches (bdn_sample_patches_aug; DevicePatchLoader(augment=...)).

A policy is a handful of scalars.  Every draw of a sample comes from Philox4x32-10 keyed by (seed, sample key), where the sample key is
epoch << 32 | dataset index: what a sample looks like does not depend on the batch split, the rank count or the process's `random`
state, and a resumed epoch repeats it.  The stages and their draws are specified in include/bidate_hip.h and DESIGN.md; a stage at its
default is off and does no arithmetic.

    policy = PatchAugment(seed=3, jitter=8, gain=0.1, bias=0.05, noise_std=0.02, erase_p=0.25, erase_size=(8, 32), erase_label=255)
    loader = DevicePatchLoader(train_ds, stacks, 64, sampler=sampler, drop_last=True, augment=policy)

PatchWarp is the second policy, for what no permutation of pixels expresses (rotation, zoom, misregistration between the dates;
bdn_sample_patches_warp).  It rides on a PatchAugment and leaves that class, its ABI and its draws as they are.

PatchMix is the third, for augmentation ACROSS samples (bdn_mix_plan, bdn_mix_patches): a rectangle (CutMix) or the changed regions
(copy-paste) of a donor sample replace the recipient's pixels on both dates and in the labels.  It rides on a PatchAugment too.
"""
import math
import operator

import numpy as np

FLAG_SYMMETRY, FLAG_PER_DATE = 1, 2          # AUG_SYMMETRY, AUG_PER_DATE of csrc/scene.hip
MAX_JITTER = 1 << 24


def _integer(name, v):
    if isinstance(v, bool):
        raise ValueError(f'PatchAugment: {name} must be an integer, got {v!r}')
    try:
        return operator.index(v)
    except TypeError:
        raise ValueError(f'PatchAugment: {name} must be an integer, got {v!r}')


def _finite(name, v):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f'PatchAugment: {name} must be finite, got {v}')
    return v


class PatchAugment:
    """seed: 64-bit key of every draw.  jitter: J >= 0, the crop origin moves by up to J pixels on either axis (clamped into the city).
    symmetry: draw one of the eight symmetries of the square per sample.  gain, bias: per band, out = g x + b with g in
    [1 - gain, 1 + gain] and b in [-bias, bias]; per_date: the two dates draw their own (g, b) (False: one pair per band for both).
    noise_std: sigma of additive Gaussian noise.  erase_p: the probability that a sample loses a rectangle of erase_size = (lo, hi)
    pixels a side (each side drawn in lo..hi, hi at most the patch size) on every band of both dates, set to erase_fill; erase_label:
    the byte the rectangle of the label patch becomes (the criterion's ignore_index), None to keep the labels."""

    def __init__(self, seed=0, jitter=0, symmetry=True, gain=0.0, bias=0.0, per_date=True, noise_std=0.0, erase_p=0.0,
                 erase_size=(1, 1), erase_label=None, erase_fill=0.0):
        seed, jitter = _integer('seed', seed), _integer('jitter', jitter)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f'PatchAugment: seed {seed} outside [0, 2^64)')
        if not 0 <= jitter <= MAX_JITTER:
            raise ValueError(f'PatchAugment: jitter {jitter} outside [0, 2^24]')
        self.seed, self.jitter = seed, jitter
        self.symmetry, self.per_date = bool(symmetry), bool(per_date)
        self.gain, self.bias, self.erase_fill = _finite('gain', gain), _finite('bias', bias), _finite('erase_fill', erase_fill)
        self.noise_std = _finite('noise_std', noise_std)
        if self.noise_std < 0.0:
            raise ValueError(f'PatchAugment: noise_std {noise_std} must be >= 0')
        self.erase_p = float(erase_p)
        if not 0.0 <= self.erase_p <= 1.0:
            raise ValueError(f'PatchAugment: erase_p {erase_p} outside [0, 1]')
        try:
            lo, hi = erase_size
        except (TypeError, ValueError):
            raise ValueError(f'PatchAugment: erase_size must be (lo, hi), got {erase_size!r}')
        lo, hi = _integer('erase_size', lo), _integer('erase_size', hi)
        if not 1 <= lo <= hi:
            raise ValueError(f'PatchAugment: erase_size needs integers 1 <= lo <= hi, got {erase_size!r}')
        self.erase_size = (lo, hi)
        if erase_label is not None and not 0 <= _integer('erase_label', erase_label) <= 255:
            raise ValueError(f'PatchAugment: erase_label {erase_label!r}: a label byte 0..255, or None to keep the labels')
        self.erase_label = None if erase_label is None else int(erase_label)

    @property
    def flags(self):
        return (FLAG_SYMMETRY if self.symmetry else 0) | (FLAG_PER_DATE if self.per_date else 0)

    def check_patch_size(self, S):
        if self.erase_p > 0.0 and self.erase_size[1] > S:
            raise ValueError(f'PatchAugment: erase_size {self.erase_size} exceeds the patch size {S}')

    @staticmethod
    def sample_key(epoch, index):
        """The 64-bit key of dataset item `index` in epoch `epoch`: epoch << 32 | index."""
        epoch, index = int(epoch), int(index)
        if not 0 <= epoch < 1 << 32 or not 0 <= index < 1 << 32:
            raise ValueError(f'PatchAugment.sample_key: epoch {epoch} and index {index} must fit 32 bits')
        return epoch << 32 | index

    def abi_args(self):
        """The policy as bdn_sample_patches_aug takes it: (seed, J, flags, gain, bias, sigma, erase_p, lo, hi, erase_label, erase_fill)."""
        return (self.seed, self.jitter, self.flags, self.gain, self.bias, self.noise_std, self.erase_p, self.erase_size[0],
                self.erase_size[1], -1 if self.erase_label is None else self.erase_label, self.erase_fill)

    def __repr__(self):
        return (f'PatchAugment(seed={self.seed}, jitter={self.jitter}, symmetry={self.symmetry}, gain={self.gain}, bias={self.bias}, '
                f'per_date={self.per_date}, noise_std={self.noise_std}, erase_p={self.erase_p}, erase_size={self.erase_size}, '
                f'erase_label={self.erase_label}, erase_fill={self.erase_fill})')


MAX_ROTATE, MIN_SCALE, MAX_SCALE, MAX_MISREG = 180.0, 0.125, 8.0, 64.0          # the bounds bdn_sample_patches_warp checks


class PatchWarp:
    """The geometric policy no permutation of pixels can express (bdn_sample_patches_warp; DevicePatchLoader(augment=..., warp=...)):
    the patch is gathered through an affine map with bilinear taps.  It rides on a PatchAugment, whose seed and sample keys its draws use.
    rotate: R >= 0 degrees (at most 180), the angle is uniform in [-R, R].  scale: (lo, hi) with 1/8 <= lo <= hi <= 8, the zoom s is
    log-uniform in [lo, hi]; s > 1 magnifies (the source footprint shrinks).  misreg: M >= 0 pixels (at most 64), date 2 is sampled at
    date 1's coordinates plus (t_i, t_j), each uniform in [-M, M]; the labels follow date 1.  oob_label: None, or the byte 0..255 a label
    pixel becomes when its source centre lies outside the city (the criterion's ignore_index); image taps outside replicate the border.

        warp = PatchWarp(rotate=30, scale=(0.8, 1.25), misreg=0.75, oob_label=255)
        loader = DevicePatchLoader(train_ds, stacks, 64, sampler=sampler, drop_last=True, augment=policy, warp=warp)
    """

    def __init__(self, rotate=0.0, scale=(1.0, 1.0), misreg=0.0, oob_label=None):
        self.rotate = self._finite('rotate', rotate)
        if not 0.0 <= self.rotate <= MAX_ROTATE:
            raise ValueError(f'PatchWarp: rotate {rotate} outside [0, 180] degrees')
        try:
            lo, hi = scale
        except (TypeError, ValueError):
            raise ValueError(f'PatchWarp: scale must be (lo, hi), got {scale!r}')
        lo, hi = self._finite('scale', lo), self._finite('scale', hi)
        if not MIN_SCALE <= lo <= hi <= MAX_SCALE:
            raise ValueError(f'PatchWarp: scale needs 1/8 <= lo <= hi <= 8, got {scale!r}')
        self.scale = (lo, hi)
        self.misreg = self._finite('misreg', misreg)
        if not 0.0 <= self.misreg <= MAX_MISREG:
            raise ValueError(f'PatchWarp: misreg {misreg} outside [0, 64] pixels')
        if oob_label is not None:
            try:
                ok = not isinstance(oob_label, bool) and 0 <= operator.index(oob_label) <= 255
            except TypeError:
                ok = False
            if not ok:
                raise ValueError(f'PatchWarp: oob_label {oob_label!r}: a label byte 0..255, or None to keep the clamped labels')
        self.oob_label = None if oob_label is None else int(oob_label)

    @staticmethod
    def _finite(name, v):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f'PatchWarp: {name} must be a number, got {v!r}')
        if not math.isfinite(v):
            raise ValueError(f'PatchWarp: {name} must be finite, got {v}')
        return v

    @property
    def off(self):
        """True when the policy maps every patch onto itself: such a loader takes the bdn_sample_patches_aug path."""
        return self.rotate == 0.0 and self.scale == (1.0, 1.0) and self.misreg == 0.0

    def abi_args(self):
        """The policy as bdn_sample_patches_warp takes it: (rotate_rad, log2_lo, log2_hi, misreg, oob_label or -1)."""
        return (math.radians(self.rotate), math.log2(self.scale[0]), math.log2(self.scale[1]), self.misreg,
                -1 if self.oob_label is None else self.oob_label)

    def __repr__(self):
        return f'PatchWarp(rotate={self.rotate}, scale={self.scale}, misreg={self.misreg}, oob_label={self.oob_label})'


MIX_MODES = {'box': 0, 'object': 1}          # MIX_BOX, MIX_OBJECT of csrc/mix.hip
MAX_MIX_MARGIN = 16


class PatchMix:
    """Augmentation across samples (bdn_mix_plan, bdn_mix_patches; DevicePatchLoader(augment=..., mix=...)).  With probability p a sample,
    the recipient, takes every band of both dates and the label byte of ONE donor wherever a mask is set; bits are moved, never computed.
    The donor is another dataset item, cut and augmented exactly as the loader would yield it in that epoch (its own jitter, symmetry,
    gain / bias, noise, erase rectangle and warp); it is never itself mixed and may equal the recipient.  It rides on a PatchAugment,
    whose seed and the recipient's sample key key its draws.
    mode='box' (CutMix): the mask is a rectangle whose sides are drawn in box_size = (lo, hi), 1 <= lo <= hi <= the patch size, placed
    uniformly inside the patch.  mode='object' (copy-paste): the mask is (donor labels == paste_label) dilated by a (2 margin + 1)
    square, margin in 0..16; the ring carries the donor's labels, and both dates switch source at the same pixels, so the seam is not
    change.  donors: None (any dataset item) or a sorted, non-empty 1-D integer array of dataset indices, the donor pool.

        mix = PatchMix(p=0.5, mode='object', margin=2).donors_from(loader.label_counts(1))
    """

    def __init__(self, p=0.0, mode='box', box_size=(1, 1), paste_label=1, margin=0, donors=None):
        try:
            self.p = float(p)
        except (TypeError, ValueError):
            raise ValueError(f'PatchMix: p must be a number, got {p!r}')
        if not 0.0 <= self.p <= 1.0:
            raise ValueError(f'PatchMix: p {p} outside [0, 1]')
        if mode not in MIX_MODES:
            raise ValueError(f"PatchMix: mode must be 'box' or 'object', got {mode!r}")
        self.mode = mode
        try:
            lo, hi = box_size
        except (TypeError, ValueError):
            raise ValueError(f'PatchMix: box_size must be (lo, hi), got {box_size!r}')
        lo, hi = self._integer('box_size', lo), self._integer('box_size', hi)
        if not 1 <= lo <= hi:
            raise ValueError(f'PatchMix: box_size needs integers 1 <= lo <= hi, got {box_size!r}')
        self.box_size = (lo, hi)
        self.paste_label, self.margin = self._integer('paste_label', paste_label), self._integer('margin', margin)
        if not 0 <= self.paste_label <= 255:
            raise ValueError(f'PatchMix: paste_label {paste_label!r}: a label byte 0..255')
        if not 0 <= self.margin <= MAX_MIX_MARGIN:
            raise ValueError(f'PatchMix: margin {margin} outside 0..{MAX_MIX_MARGIN}')
        if donors is not None:
            pool = np.asarray(donors)
            if pool.ndim != 1 or pool.size == 0 or pool.dtype.kind not in 'iu':
                raise ValueError('PatchMix: donors must be a non-empty 1-D integer array of dataset indices, or None')
            if int(pool.min()) < 0 or int(pool.max()) >= 1 << 31 or (np.diff(pool.astype(np.int64)) < 0).any():
                raise ValueError('PatchMix: donors must be sorted dataset indices in [0, 2^31)')
            donors = np.ascontiguousarray(pool, dtype=np.int32)
        self.donors = donors

    @staticmethod
    def _integer(name, v):
        if isinstance(v, bool):
            raise ValueError(f'PatchMix: {name} must be an integer, got {v!r}')
        try:
            return operator.index(v)
        except TypeError:
            raise ValueError(f'PatchMix: {name} must be an integer, got {v!r}')

    @property
    def off(self):
        """True when no sample is ever mixed: such a loader issues the calls it issues without the policy."""
        return self.p == 0.0

    def check(self, S, n_items):
        """What only the loader knows: the box fits the patch, and every donor is an item of the dataset."""
        if self.box_size[1] > S:
            raise ValueError(f'PatchMix: box_size {self.box_size} exceeds the patch size {S}')
        if self.donors is not None and int(self.donors[-1]) >= n_items:
            raise ValueError(f'PatchMix: donor {int(self.donors[-1])} is no item of a dataset of {n_items}')

    def donors_from(self, counts, min_pixels=1):
        """A copy of the policy whose pool is the dataset indices with counts[i] >= min_pixels (counts: loader.label_counts(value), a
        device tensor, or any integer array): the one host read.  A pool only: jitter and warp may move a donor's content."""
        counts = counts.cpu().numpy() if hasattr(counts, 'cpu') else np.asarray(counts)
        pool = np.flatnonzero(counts.reshape(-1) >= self._integer('min_pixels', min_pixels))
        if pool.size == 0:
            raise ValueError(f'PatchMix: no dataset item has {min_pixels} or more such pixels: the donor pool is empty')
        return PatchMix(self.p, self.mode, self.box_size, self.paste_label, self.margin, pool)

    def __repr__(self):
        donors = None if self.donors is None else f'<{self.donors.size} indices>'
        return (f'PatchMix(p={self.p}, mode={self.mode!r}, box_size={self.box_size}, paste_label={self.paste_label}, margin={self.margin}, '
                f'donors={donors})')
