"""numpy restatement of cross-sample mixing (bdn_mix_plan, bdn_mix_patches), written from the specification in include/bidate_hip.h and
DESIGN.md 19c, not from the kernel.  The draws are built on tests/augment_ref.draw; every one is an integer except the comparison
u(w0) < p, which is a float32 comparison of exactly representable values, so this file reproduces the library element for element."""
import numpy as np

from tests import augment_ref as R

MIX = 0x4D495820          # the stream 'MIX '
BOX, OBJECT = 0, 1
MODES = {'box': BOX, 'object': OBJECT}


def plan(seed, keys, S, p, mode, lo, hi, pool=None, n_items=None):
    """int32 [n][8] = (on, donor_index, donor_row, top, left, h, w, 0) for the recipients' sample keys `keys`.  pool: the sorted donor
    indices, or None for range(n_items)."""
    mode = MODES.get(mode, mode)
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    a = R.draw(seed, keys, MIX, 0)                                   # one row of four words per key
    on = R.u(a[:, 0]) < np.float32(p)
    pick = R.rng(a[:, 1], len(pool) if pool is not None else int(n_items)).astype(np.int64)
    h, w = lo + R.rng(a[:, 2], hi - lo + 1).astype(np.int64), lo + R.rng(a[:, 3], hi - lo + 1).astype(np.int64)
    if mode == BOX:
        b = R.draw(seed, keys, MIX, 1)
        top = (b[:, 0].astype(np.uint64) * (S - h + 1).astype(np.uint64)) >> np.uint64(32)
        left = (b[:, 1].astype(np.uint64) * (S - w + 1).astype(np.uint64)) >> np.uint64(32)
    else:
        top, left, h, w = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, S), np.full(n, S)
    donor = np.asarray(pool, np.int64)[pick] if pool is not None else pick
    row = n + np.cumsum(on) - on                                     # n + the number of mixed samples before this one
    out = np.stack([on, donor, row, top, left, h, w, np.zeros(n)], -1).astype(np.int32)
    out[~on] = (0, 0, -1, 0, 0, 0, 0, 0)
    return out


def mask(plan_row, donor_labels, mode, paste_label=1, margin=0):
    """uint8 [S][S]: 1 where the recipient takes the donor.  donor_labels: the donor's uint8 [S][S] label patch."""
    mode = MODES.get(mode, mode)
    S = donor_labels.shape[0]
    out = np.zeros((S, S), np.uint8)
    on, _, _, top, left, h, w, _ = (int(v) for v in plan_row)
    if not on:
        return out
    if mode == BOX:
        out[top:top + h, left:left + w] = 1
        return out
    hit = np.zeros((S + 2 * margin, S + 2 * margin), bool)          # donor labels outside the patch count as unset
    hit[margin:margin + S, margin:margin + S] = donor_labels == paste_label
    for di in range(2 * margin + 1):                                # the (2 margin + 1) square, confined to the patch
        for dj in range(2 * margin + 1):
            out |= hit[di:di + S, dj:dj + S]
    return out


def mix(recipients, donors, masks):
    """select(mask, donor, recipient) per sample, on whole arrays of any dtype: recipients, donors [n][...][S][S], masks uint8 [n][S][S]."""
    m = np.asarray(masks).astype(bool)
    m = m.reshape(m.shape[:1] + (1,) * (recipients.ndim - 3) + m.shape[1:])
    return np.where(m, donors, recipients)
