"""Training patch pairs cut out of HBM-resident city stacks (bdn_sample_patches) instead of on the host.

The host path (reference utils/dataloaders.py:148-198 + utils/helpers.py:250-257) crops every patch pair with numpy, collates the
batch, pins it and copies it over PCIe.  `DevicePatchLoader` keeps the city stacks on the device and sends only the batch's
descriptors, (city, row, col, symmetry) as int32, through a pinned ring; one launch on the current stream then writes the batch.
It yields what `DataLoader(dataset, batch_size, sampler=sampler, drop_last=drop_last, num_workers=0)` yields, moved to the device,
bit for bit: the same index order and batch boundaries, and the same `_draw_symmetry()` calls from the global `random`, in the same
order, when `dataset.aug`.

    loader = DevicePatchLoader(train_ds, stacks, batch_size=64, sampler=ShardSampler(len(train_ds), rank, world, seed))
    for x1, x2, y in loader:            # device tensors; valid until the next iteration (the contract of DeviceFeeder)
        loss = step.step(x1, x2, y)

With `augment=PatchAugment(...)` (fabric_amd.augment) the batch is cut by bdn_sample_patches_aug instead: crop jitter, a drawn symmetry,
per-date per-band gain / bias, Gaussian noise and erasing, every draw from a counter-based generator keyed by (policy seed, epoch,
dataset index).  The host then draws nothing from `random` and `dataset.aug` is ignored for that loader: descriptors carry sym = 0 and a
pinned ring of 64-bit sample keys travels beside them.  Index order and batch boundaries are unchanged.

With `warp=PatchWarp(...)` beside the policy the batch is cut by bdn_sample_patches_warp: the same draws, and the patch gathered through
a drawn rotation, zoom and between-date shift with bilinear taps.  A PatchWarp that is `off` changes nothing: the loader then issues the
calls it issues without one.

With `mix=PatchMix(...)` beside the policy a sample takes, with probability p, a rectangle or the changed regions of a donor sample
(bdn_mix_plan on the host, bdn_mix_patches on the device).  The donors of a batch are cut by the same call as its n recipients, behind
them, each exactly as the loader would yield it in that epoch; the slots therefore hold 2 * batch_size rows, and the first n are
yielded.  A PatchMix that is `off` changes nothing.
"""
import numpy as np
import torch
import torch.utils.data

from . import _lib
from .augment import MIX_MODES, PatchAugment, PatchMix, PatchWarp
from .utils.dataloaders import _draw_symmetry


def symmetry_code(sym):
    """(transpose, reverse rows, reverse columns) -> the `sym` field 4 t + 2 rr + rc of a descriptor."""
    t, rr, rc = sym
    return 4 * int(t) + 2 * int(rr) + int(rc)


def plan_descriptors(dataset, indices, city_index, out=None):
    """Host half of one batch, no device needed: int32 [len(indices)][4] = (city, row, col, sym) for items `indices` of the
    OneraPreloader `dataset`, drawing one symmetry per item from the global `random` exactly as `dataset[i]` does (only when
    `dataset.aug`).  `city_index`: {city name: row of the city table}.  `out`: an int32 array to fill (a view of it is returned)."""
    n = len(indices)
    table = np.empty((n, 4), np.int32) if out is None else out[:n]
    for k, idx in enumerate(indices):
        city, i, j = dataset.imgs[idx]
        table[k] = (city_index[city], i, j, symmetry_code(_draw_symmetry()) if dataset.aug else 0)
    return table


def batch_sampler(dataset, batch_size, sampler=None, drop_last=False):
    """The batches of indices that DataLoader(dataset, batch_size, sampler=sampler, drop_last=drop_last) visits."""
    return torch.utils.data.BatchSampler(sampler if sampler is not None else torch.utils.data.SequentialSampler(dataset),
                                         batch_size, drop_last)


def plan_epoch(dataset, city_index, batch_size, sampler=None, drop_last=False):
    """The descriptor tables of one pass of DevicePatchLoader, planned on the host alone (no device): one int32 [n][4] per batch."""
    for indices in batch_sampler(dataset, batch_size, sampler, drop_last):
        yield plan_descriptors(dataset, indices, city_index)


def device_stacks(stacks, device):
    """{city: {'images': float32 [2,C,H,W], 'labels': uint8 [H,W]}} on `device`: device tensors are kept as they are (no copy),
    numpy arrays and CPU tensors are uploaded.  Share the result between loaders to upload once."""
    device = torch.device(device)
    out = {}
    for city, d in stacks.items():
        e = {}
        for key, dtype in (('images', torch.float32), ('labels', torch.uint8)):
            t = d[key] if torch.is_tensor(d[key]) else torch.from_numpy(np.asarray(d[key]))
            if t.dtype != dtype or not t.is_contiguous():
                raise RuntimeError(f'fabric_amd: city {city!r}: {key} must be contiguous {dtype}, got {t.dtype}'
                                   f'{"" if t.is_contiguous() else " (not contiguous)"}')
            e[key] = t if t.device == device else t.to(device)
        out[city] = e
    return out


def plan_keys(indices, epoch, out=None):
    """Host half of an augmented batch, no device needed: uint64 [len(indices)] sample keys epoch << 32 | dataset index."""
    n = len(indices)
    keys = np.empty(n, np.uint64) if out is None else out[:n]
    for k, idx in enumerate(indices):
        keys[k] = PatchAugment.sample_key(epoch, idx)
    return keys


class _Slot:
    def __init__(self, batch_size, C, S, device, keys=False, export=False, warp=False, mix=False):
        if mix:                   # the plan of the batch, under the same `done` discipline; its donors are cut behind the recipients
            self.plan_pin = torch.empty((batch_size, 8), dtype=torch.int32, pin_memory=True)
            self.plan_np = self.plan_pin.numpy()
            self.plan_dev = torch.empty((batch_size, 8), dtype=torch.int32, device=device)
            batch_size = 2 * batch_size
        if keys:                  # the ring of sample keys: rewritten and read under the same `done` discipline as the descriptors
            self.keys_pin = torch.empty((batch_size,), dtype=torch.int64, pin_memory=True)
            self.keys_np = self.keys_pin.numpy().view(np.uint64)
            self.keys_dev = torch.empty((batch_size,), dtype=torch.int64, device=device)
        if export:
            self.geom = torch.empty((batch_size, 8), dtype=torch.int32, device=device)
            self.radio = torch.empty((batch_size, 2, C, 2), dtype=torch.float32, device=device)
            if warp:
                self.warp = torch.empty((batch_size, 2, 6), dtype=torch.float32, device=device)
        self.desc_pin = torch.empty((batch_size, 4), dtype=torch.int32, pin_memory=True)
        self.desc_np = self.desc_pin.numpy()
        self.desc_dev = torch.empty((batch_size, 4), dtype=torch.int32, device=device)
        self.d1 = torch.empty((batch_size, C, S, S), dtype=torch.float32, device=device)
        self.d2 = torch.empty_like(self.d1)
        self.labels = torch.empty((batch_size, S, S), dtype=torch.uint8, device=device)
        self.done = None          # recorded after the launch: the copy out of desc_pin is over once it has completed


class DevicePatchLoader:
    """Batches of `dataset` (an OneraPreloader: its `imgs`, `input_size` and `aug` are used) sampled on the device from `stacks`
    ({city: {'images', 'labels'}}; see device_stacks).  `depth` (>= 2) slots of pinned descriptors and device outputs are cycled;
    a slot's pinned table is rewritten only after the launch that read it `depth` batches ago has completed.
    `augment`: a PatchAugment; the batches are then augmented on the device (module docstring) and `dataset.aug` is ignored.  The epoch
    half of a sample key is `sampler.epoch` when the sampler has one, else the number of passes begun so far; set_epoch(e) overrides
    both.  `export_drawn=True` (with a policy): `last_drawn` = (int32 [n][8] (row, col, sym, erased, top, left, eh, ew), float32
    [n][2][C][2] (g, b)) of the batch yielded last, valid as long as the batch is.
    `warp`: a PatchWarp (needs `augment`, whose seed and keys its draws use); unless it is `off` the batches are cut by
    bdn_sample_patches_warp and `last_drawn` gains a third element, the float32 [n][2][6] warp records.
    `mix`: a PatchMix (needs `augment` too); unless it is `off` the batches are mixed across samples (module docstring), `last_drawn`
    keeps its elements for the n yielded rows and gains the device int32 [n][8] plan (on, donor_index, donor_row, top, left, h, w, 0)
    as its last one, and `mixed` / `seen` count the samples mixed / yielded in the pass begun last."""

    def __init__(self, dataset, stacks, batch_size, sampler=None, drop_last=False, device=None, depth=3, augment=None,
                 export_drawn=False, warp=None, mix=None):
        if augment is not None:
            if not isinstance(augment, PatchAugment):
                raise TypeError(f'fabric_amd: augment must be a PatchAugment, got {type(augment).__name__}')
            augment.check_patch_size(int(dataset.input_size))
        elif export_drawn:
            raise ValueError('fabric_amd: export_drawn needs an augment policy')
        if warp is not None:
            if not isinstance(warp, PatchWarp):
                raise TypeError(f'fabric_amd: warp must be a PatchWarp, got {type(warp).__name__}')
            if augment is None:
                raise ValueError('fabric_amd: warp needs an augment policy (its seed and sample keys key the warp draws)')
        if mix is not None:
            if not isinstance(mix, PatchMix):
                raise TypeError(f'fabric_amd: mix must be a PatchMix, got {type(mix).__name__}')
            if augment is None:
                raise ValueError('fabric_amd: mix needs an augment policy (its seed and sample keys key the mix draws)')
            mix.check(int(dataset.input_size), len(dataset))
        self.augment, self.export_drawn = augment, bool(export_drawn)
        self.mix = mix if mix is not None and not mix.off else None               # an `off` mix: the calls of a loader without one
        self.mixed = self.seen = 0                # samples mixed / yielded in the pass begun last (host counts: the plan is made here)
        self.warp = warp if warp is not None and not warp.off else None          # an `off` warp: the bdn_sample_patches_aug path, call for call
        self.last_drawn = None
        self._epoch, self._passes = None, 0
        self.dataset = dataset
        self.batch_sampler = batch_sampler(dataset, batch_size, sampler, drop_last)
        self.sampler = self.batch_sampler.sampler
        self.batch_size, self.drop_last, self.S = int(batch_size), drop_last, int(dataset.input_size)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.type != 'cuda':
            raise RuntimeError('fabric_amd: DevicePatchLoader needs a ROCm device')
        self.stacks = device_stacks(stacks, self.device)          # held: the table below points into these tensors
        self.cities = sorted(self.stacks)
        self.city_index = {c: k for k, c in enumerate(self.cities)}          # row of the city table: cities in sorted order
        shapes = []
        for c in self.cities:
            im, lb = self.stacks[c]['images'], self.stacks[c]['labels']
            if im.dim() != 4 or im.shape[0] != 2 or lb.dim() != 2 or tuple(im.shape[2:]) != tuple(lb.shape):
                raise RuntimeError(f'fabric_amd: city {c!r}: need images [2,C,H,W] and labels [H,W], got {tuple(im.shape)} and {tuple(lb.shape)}')
            shapes.append(tuple(im.shape[1:]))
        if len({s[0] for s in shapes}) != 1:
            raise RuntimeError(f'fabric_amd: all cities need the same number of bands, got {sorted({s[0] for s in shapes})}')
        self.C = shapes[0][0]
        self.city_hw = np.ascontiguousarray([s[1:] for s in shapes], dtype=np.int32)
        rec = np.zeros((len(self.cities), 3), np.int64)           # { const float* images; const uint8_t* labels; int32 H, W; }
        for k, c in enumerate(self.cities):
            h, w = (int(v) for v in self.city_hw[k])
            rec[k] = (self.stacks[c]['images'].data_ptr(), self.stacks[c]['labels'].data_ptr(), h | (w << 32))
        self.city_table = torch.from_numpy(rec).to(self.device)
        self.depth = max(2, int(depth))
        self.slots = [_Slot(self.batch_size, self.C, self.S, self.device, keys=augment is not None, export=self.export_drawn,
                            warp=self.warp is not None, mix=self.mix is not None)
                      for _ in range(self.depth)]
        torch.cuda.synchronize(self.device)                       # uploads and allocations are complete before any stream reads them
        self._k = 0
        self._streams = set()

    def _long_lived(self):
        yield self.city_table
        for city in self.stacks.values():
            yield from (city['images'], city['labels'])
        for slot in self.slots:
            yield from (slot.desc_dev, slot.d1, slot.d2, slot.labels)
            if self.augment is not None:
                yield slot.keys_dev
            if self.export_drawn:
                yield from (slot.geom, slot.radio)
                if self.warp is not None:
                    yield slot.warp
            if self.mix is not None:
                yield slot.plan_dev

    def __len__(self):
        return len(self.batch_sampler)

    def set_epoch(self, epoch):
        """The epoch half of the sample keys of every pass from now on (None: back to the sampler's epoch / the pass counter)."""
        self._epoch = None if epoch is None else int(epoch)

    def __iter__(self):
        if self.augment is None:
            for indices in self.batch_sampler:
                yield self._sample(indices)
            return
        epoch = self._epoch if self._epoch is not None else getattr(self.sampler, 'epoch', self._passes)
        self._passes += 1
        self.mixed = self.seen = 0
        for indices in self.batch_sampler:
            yield self._sample_aug(indices, int(epoch))

    def _sample_aug(self, indices, epoch):
        """_sample with a policy: sym = 0 descriptors (no draw from `random`) and the sample keys through the pinned slot."""
        slot = self.slots[self._k % self.depth]
        self._k += 1
        if slot.done is not None:
            slot.done.synchronize()                               # the copies that read desc_pin and keys_pin `depth` batches ago have run
        n = len(indices)
        for k, idx in enumerate(indices):
            city, i, j = self.dataset.imgs[idx]
            slot.desc_np[k] = (self.city_index[city], i, j, 0)
        plan_keys(indices, epoch, out=slot.keys_np)
        rows = n if self.mix is None else self._plan_mix(slot, n, epoch)          # the donors' descriptors and keys follow the recipients'
        cur = torch.cuda.current_stream(self.device)
        desc_dev, keys_dev = slot.desc_dev[:rows], slot.keys_dev[:rows]
        desc_dev.copy_(slot.desc_pin[:rows], non_blocking=True)
        keys_dev.copy_(slot.keys_pin[:rows], non_blocking=True)
        d1, d2, labels = slot.d1[:rows], slot.d2[:rows], slot.labels[:rows]
        geom, radio = (slot.geom[:rows], slot.radio[:rows]) if self.export_drawn else (None, None)
        args = (self.city_table.data_ptr(), _lib.host_int32(self.city_hw), len(self.cities), self.C,
                _lib.host_int32(slot.desc_pin.data_ptr()), desc_dev.data_ptr(), rows, self.S, d1.data_ptr(), d2.data_ptr(),
                labels.data_ptr(), keys_dev.data_ptr(), *self.augment.abi_args(), _lib.ptr(geom), _lib.ptr(radio))
        if self.warp is None:
            _lib.call('bdn_sample_patches_aug', *args, cur.cuda_stream)
        else:
            records = slot.warp[:rows] if self.export_drawn else None
            _lib.call('bdn_sample_patches_warp', *args, *self.warp.abi_args(), None, None, _lib.ptr(records), cur.cuda_stream)
        if self.mix is not None:
            plan_dev = slot.plan_dev[:n]
            plan_dev.copy_(slot.plan_pin[:n], non_blocking=True)
            _lib.call('bdn_mix_patches', _lib.host_int32(slot.plan_pin.data_ptr()), plan_dev.data_ptr(), n, rows, self.C, self.S,
                      MIX_MODES[self.mix.mode], self.mix.paste_label, self.mix.margin, d1.data_ptr(), d2.data_ptr(), labels.data_ptr(),
                      None, cur.cuda_stream)
            d1, d2, labels = d1[:n], d2[:n], labels[:n]
        if cur.cuda_stream not in self._streams:
            self._streams.add(cur.cuda_stream)
            for t in self._long_lived():
                t.record_stream(cur)
        slot.done = torch.cuda.Event()
        slot.done.record(cur)
        if self.export_drawn:
            drawn = (geom, radio) if self.warp is None else (geom, radio, records)
            self.last_drawn = drawn if self.mix is None else tuple(t[:n] for t in drawn) + (plan_dev,)
        else:
            self.last_drawn = None
        return d1, d2, labels

    def _plan_mix(self, slot, n, epoch):
        """Host half of a mixed batch: the plan of the n recipients in the pinned slot (bdn_mix_plan on their keys), then the descriptor
        and the sample key of every mixed sample's donor behind the recipients'.  Returns the number of rows to cut, n + donors."""
        mix = self.mix
        _lib.call('bdn_mix_plan', self.augment.seed, _lib.host_uint64(slot.keys_pin.data_ptr()), n, self.S, mix.p, MIX_MODES[mix.mode],
                  *mix.box_size, _lib.host_int32(mix.donors), len(self.dataset) if mix.donors is None else len(mix.donors),
                  _lib.host_int32(slot.plan_pin.data_ptr()))
        rows = n
        for on, donor in slot.plan_np[:n, :2].tolist():
            if on:
                city, i, j = self.dataset.imgs[donor]
                slot.desc_np[rows] = (self.city_index[city], i, j, 0)
                slot.keys_np[rows] = PatchAugment.sample_key(epoch, donor)
                rows += 1
        self.mixed += rows - n
        self.seen += n
        return rows

    def label_counts(self, value=1, chunk=4096):
        """Device int32 [len(dataset)]: how many label bytes of every dataset item's window, at its grid position (no jitter), equal
        `value` (bdn_patch_label_counts, in chunks of `chunk` descriptors on the current stream).  PatchMix.donors_from turns it into
        a donor pool."""
        counts = torch.empty((len(self.dataset),), dtype=torch.int32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        for a in range(0, len(self.dataset), chunk):
            desc = np.array([(self.city_index[city], i, j, 0) for city, i, j in self.dataset.imgs[a:a + chunk]], np.int32).reshape(-1, 4)
            desc_dev = torch.from_numpy(desc).to(self.device)          # from pageable memory: the copy has read `desc` when it returns
            _lib.call('bdn_patch_label_counts', self.city_table.data_ptr(), _lib.host_int32(self.city_hw), len(self.cities),
                      _lib.host_int32(desc), desc_dev.data_ptr(), len(desc), self.S, int(value), counts[a:a + len(desc)].data_ptr(),
                      cur.cuda_stream)
            desc_dev.record_stream(cur)
        return counts

    def _sample(self, indices):
        """Plan the batch on the host, copy its descriptors through the next pinned slot and launch on the current stream."""
        slot = self.slots[self._k % self.depth]
        self._k += 1
        if slot.done is not None:
            slot.done.synchronize()                               # the copy that read desc_pin `depth` batches ago has run
        n = len(indices)
        plan_descriptors(self.dataset, indices, self.city_index, out=slot.desc_np)
        cur = torch.cuda.current_stream(self.device)
        desc_dev = slot.desc_dev[:n]
        desc_dev.copy_(slot.desc_pin[:n], non_blocking=True)
        d1, d2, labels = slot.d1[:n], slot.d2[:n], slot.labels[:n]
        _lib.call('bdn_sample_patches', self.city_table.data_ptr(), self.city_hw.ctypes.data, len(self.cities), self.C,
                  slot.desc_pin.data_ptr(), desc_dev.data_ptr(), n, self.S, d1.data_ptr(), d2.data_ptr(), labels.data_ptr(),
                  cur.cuda_stream)
        if cur.cuda_stream not in self._streams:                 # memory allocated at construction, read and written on this stream
            self._streams.add(cur.cuda_stream)
            for t in self._long_lived():
                t.record_stream(cur)
        slot.done = torch.cuda.Event()
        slot.done.record(cur)
        return d1, d2, labels
