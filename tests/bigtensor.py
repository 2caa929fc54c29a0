"""Big twins of the launch-shape rows: the same kernels on tensors of 2 to 4 GB, where a byte offset uses the sign bit and then the top of
its 32-bit range.  Host logic only: the functions work on tensors of whatever device they are given, and tests/test_bigtensor_cpu.py proves
them on the CPU; the launches are in tests/test_gpu_bigtensor.py.

The MFMA kernels address an activation tensor as one uniform base + a 32-bit byte offset, and their entry points refuse a tensor that reaches
4 GB.  A twin keeps a row's precision, channels, modes and map (so the tile class and the instantiation stay) and raises N:

  blocks   G = 2 statistic groups where the row has groups (eval rows: 1; the two dates of an eval_pair operand are two blocks as well)
  period   P images, P even (two-image tiles pair n and n + 1: a pair never straddles a period); a block is N / (G P) copies of its period
  N_cross  the smallest multiple of G P at which the widest tensor the entry point bounds passes 2^31 bytes by at least one whole period
  N_top    the largest multiple of G P the entry point accepts (the widest tensor stays below 2^32 bytes)

At N_top every tensor of half the widest width crosses 2^31 too, which is why two sizes do.  One period is built on the host exactly as the
sibling test builds its row (at N = G P) and tiled on the device; outputs are born 0xFF.  Every period of an output must equal period 0 of
its block bit for bit (period_findings, every byte of the tensor), and period 0 is held against the sibling's float64 reference at the
sibling's bar.  A wrapped or sign-extended offset lands in another period's place or outside the payload (the guard bands): periods differ
in position only, so this detects it unless the wrap distance (2^31 or 2^32 bytes) is a multiple of the period's byte size -- the chooser
picks P so that it is not, for every tensor of the launch.

Reductions over all images take integer-valued data (int_values): float32 accumulation is then exact in any order while the sum of |terms|
stays below 2^24 (exact_in_f32), and the expected result is (N / P) x the period's integers, compared with equality.
"""
from collections import namedtuple

import numpy as np
import torch

TWO31, TWO32 = 1 << 31, 1 << 32
MEM_CAP = 24 << 30                 # no twin holds more device memory than this
GUARD_MIN = 64 * 1024              # tests/guard.py: each guard is max(64 KiB, one image) bytes
SLAB_BYTES = 128 << 20             # period_findings compares this many bytes at a time
GROUPED = ('fwd', 'dgrad', 'dgrad_bs', 'dgrad_bb', 'x3', 'x3src', 'wgrad', 'wgrad_bnbwd')

# one activation-sized tensor of a twin: bytes per pixel, pixels per image (pooled maps have fewer), images per unit of N (2: both dates of N pairs)
Tensor = namedtuple('Tensor', 'name bpp pix imgs')
Twin = namedtuple('Twin', 'row size G P N bound_bytes period_bytes step_bytes mem_bytes tensors')


def blocks(r):
    """Statistic groups of the twin of row r."""
    return 2 if r.op in GROUPED else 1


def bound_widths(r):
    """Bytes per pixel of the tensors the row's entry point bounds below 4 GB, as its own check states them (conv3x3.hip: conv3x3_impl,
    bdn_conv3x3_x3src, conv3x3_eval_impl, bdn_conv3x3_eval_pair), and the images per unit of N those checks count."""
    es, oes = (4 if r.prec == 'fp32' else 2), (2 if r.prec == 'bf16' else 4)
    if r.op in ('fwd', 'dgrad', 'dgrad_bs', 'dgrad_bb'):
        return [max(r.C0, r.C1) * es, r.Cout * oes], 1
    if r.op == 'x3':                                       # ld0 = 2 C0 bf16 (hi | lo), float32 outputs
        return [2 * r.C0 * 2, r.Cout * 4], 1
    if r.op == 'x3src':
        return [r.C0 * 4, r.Cout * 4], 1
    if r.op in ('eval', 'eval_cls'):
        return [max(r.C0, r.C1) * es, r.Cout * es], 1
    if r.op == 'eval_pair':                                # npix = 2 B H W
        return [r.C0 * es, r.Cout * es], 2
    raise ValueError(r.op)


def tensors(r):
    """Every activation-sized tensor the twin's test holds (operands and outputs of tests/test_gpu_bigtensor.py's launch of the row)."""
    es, oes = (4 if r.prec == 'fp32' else 2), (2 if r.prec == 'bf16' else 4)
    hw, phw = r.H * r.W, (r.H // 2) * (r.W // 2)
    T = Tensor
    if r.op == 'fwd':
        out = [T('in0', r.C0 * es, hw, 1), T('out', r.Cout * oes, hw, 1)]
        return out + ([T('in1', r.C1 * es, hw, 1)] if r.C1 else [])
    if r.op == 'dgrad':
        return [T('dz', r.C0 * es, hw, 1), T('dA', r.Cout * oes, hw, 1)]
    if r.op == 'dgrad_bs':
        return [T('dz', r.C0 * es, hw, 1), T('z_prev', r.Cout * es, hw, 1), T('plain', r.Cout * oes, hw, 1), T('dA', r.Cout * oes, hw, 1)]
    if r.op == 'dgrad_bb':                                 # bf16: g, z and the dz by-product of C0 channels; z_prev and the two gradients of Cout
        return [T('dA', r.C0 * 2, hw, 1), T('z', r.C0 * 2, hw, 1), T('dz', r.C0 * 2, hw, 1), T('z_prev', r.Cout * 2, hw, 1),
                T('dA_prev', r.Cout * 2, hw, 1), T('dA_prev masked', r.Cout * 2, hw, 1)]
    if r.op == 'x3':
        return [T('split', 2 * r.C0 * 2, hw, 1), T('out', r.Cout * 4, hw, 1)]
    if r.op == 'x3src':
        return [T('in', r.C0 * 4, hw, 1), T('out', r.Cout * 4, hw, 1)] + ([T('x3_split', 2 * r.C0 * 2, hw, 1)] if r.stats else [])
    if r.op == 'eval':
        out = [T('in0', r.C0 * es, hw, 1), T('out', r.Cout * es, hw, 1), T('pool', r.Cout * es, phw, 1)]
        return out + ([T('in1', r.C1 * es, hw, 1)] if r.C1 else [])
    if r.op == 'eval_pair':
        return [T('in', r.C0 * es, hw, 2), T('f', r.Cout * es, hw, 1), T('pool', r.Cout * es, phw, 2)]
    if r.op == 'eval_cls':
        return [T('in0', r.C0 * es, hw, 1), T('a_out', r.Cout * es, hw, 1), T('logits', 2 * 4, hw, 1), T('mask', 1, hw, 1)]
    raise ValueError(r.op)


def _guard(image_bytes):
    return max(GUARD_MIN, image_bytes) + 256


def memory_bytes(r, N):
    """Device bytes a twin of N images holds at once: its guarded tensors, the comparator's slab temporaries (a mask and an int32 copy of
    it per slab) and 1 GiB for everything small (filters, tables, partials, the period's upload)."""
    total = 6 * SLAB_BYTES + (1 << 30)
    for t in tensors(r):
        if r.op == 'dgrad_bb' and t.name in ('dz', 'dA_prev'):
            continue                                       # the twin runs in two phases; these belong to the smaller first one
        total += N * t.imgs * t.pix * t.bpp + 2 * _guard(t.pix * t.bpp)
    return total


def period_for(ts):
    """The smallest even period P for which neither 2^31 nor 2^32 bytes is a whole number of periods of any tensor in ts (2^31 | 2^32, so
    one test does): 2 wherever the map has an odd factor; power-of-two maps take 6."""
    for P in range(2, 64, 2):
        if all(TWO32 % (P * t.pix * t.bpp) != 0 for t in ts):
            return P
    raise AssertionError(f'no period for {ts}')


def n_reaching(nbytes, per_image, step):
    """The smallest multiple of `step` images whose tensor of per_image bytes per image holds at least nbytes."""
    return -(-(-(-nbytes // per_image)) // step) * step


def n_below(nbytes, per_image, step):
    """The largest multiple of `step` images whose tensor stays below nbytes."""
    return (nbytes - 1) // per_image // step * step


def wrap_safe(r, P):
    """Neither 2^31 nor 2^32 bytes is a whole number of periods of any tensor of the twin (2^31 | 2^32, so one test does)."""
    return all(TWO32 % (P * t.pix * t.bpp) != 0 for t in tensors(r))


def period(r):
    """The smallest even period for which wrap_safe holds (2 wherever the map has an odd factor; power-of-two maps take 6)."""
    return period_for(tensors(r))


def small_row(r, P=None):
    """The row at N = G P, P images per statistic group: what the sibling test builds, one period per block."""
    P = P or period(r)
    return r._replace(N=blocks(r) * P, ipg=P)


def twin_row(r, N):
    """The row at N images in G groups: what the library is asked about (instantiation) and launched with."""
    return r._replace(N=N, ipg=N // blocks(r))


def choose(r, size):
    """The twin of row r at size 'cross' or 'top' (module docstring)."""
    G, P = blocks(r), period(r)
    widths, imgs = bound_widths(r)
    per_image = imgs * r.H * r.W * max(widths)             # bytes of the widest bounded tensor per unit of N
    step, pbytes = G * P, P * per_image // imgs            # a period of that tensor: P images
    if size == 'cross':
        N = n_reaching(TWO31 + pbytes, per_image, step)
    elif size == 'top':
        N = n_below(TWO32, per_image, step)
    else:
        raise ValueError(size)
    return Twin(r, size, G, P, N, N * per_image, pbytes, step * per_image, memory_bytes(r, N), tensors(r))


def next_refused(tw):
    """The next valid N above N_top: the entry point must refuse it."""
    assert tw.size == 'top'
    return tw.N + tw.G * tw.P


def entry_call(r, N):
    """(entry point, arguments) of the row's launch at N images with fake non-null pointers: for the refusal tests only -- the entry points
    check the shape before anything is launched or dereferenced (conv3x3.hip: the 4 GB tests of conv3x3_impl, bdn_conv3x3_x3src,
    conv3x3_eval_impl and bdn_conv3x3_eval_pair stand in front of the plan and the dispatch)."""
    from fabric_amd._lib import IN_BNRELU, IN_PLAIN
    from tests import launch_cases as lc
    p, dt, ipg = 16, lc.DTYPE[r.prec], N // blocks(r)
    mode, bn = (IN_BNRELU, p) if r.bnrelu else (IN_PLAIN, None)
    tail = (N, r.H, r.W, r.Cout, None)
    if r.op in ('fwd', 'dgrad', 'x3'):
        return 'bdn_conv3x3', (dt, p, r.C0, p if r.C1 else None, r.C1, mode, bn, ipg, p, None, p, None) + tail
    if r.op == 'dgrad_bs':
        return 'bdn_conv3x3_dgrad_bs', (dt, p, r.C0, p, p, p, p, ipg, p) + tail
    if r.op == 'dgrad_bb':
        return 'bdn_conv3x3_dgrad_bb', (dt, p, r.C0, p, p, p, ipg, p, p, None, None, None, None) + tail
    if r.op == 'x3src':
        return 'bdn_conv3x3_x3src', (dt, p, r.C0, mode, bn, ipg, p, None, p, None, None) + tail
    if r.op == 'eval':
        return 'bdn_conv3x3_eval', (dt, p, r.C0, p if r.C1 else None, r.C1, p, p, p, p, None, None) + tail
    if r.op == 'eval_pair':
        return 'bdn_conv3x3_eval_pair', (dt, p, r.C0, p, p, p, p, None) + tail
    if r.op == 'eval_cls':
        return 'bdn_conv3x3_eval_cls', (dt, p, r.C0, p, p, p, p, p, p, 2, p, None, None, 0, 0) + tail
    raise ValueError(r.op)


TWIN_OPS = ('fwd', 'dgrad', 'dgrad_bs', 'dgrad_bb', 'x3', 'x3src', 'eval', 'eval_pair', 'eval_cls')
Case = namedtuple('Case', 'row twin inst')


def twin_id(t):
    from tests import launch_cases as lc
    return f'{lc.row_id(t.row)}-{t.twin.size}-N{t.twin.N}'


def twins(ops=TWIN_OPS):
    """[(row, twin, instantiation the twin runs)] at both sizes: one per (op, precision, instantiation, modes), in table order.  The
    instantiation is the library's answer for the raised N -- the row's own, except across the BN = 64 / 128 threshold of conv_plan."""
    from tests import launch_cases as lc
    out, seen = [], set()
    for r in lc.ROWS:
        if r.op not in ops:
            continue
        tws = [choose(r, size) for size in ('cross', 'top')]
        insts = {lc.instantiation(twin_row(r, tw.N)) for tw in tws}
        assert len(insts) == 1 and '' not in insts, (r, insts)
        inst = insts.pop()
        key = (r.op, r.prec, inst, r.bnrelu, bool(r.C1), r.stats)
        if key in seen:
            continue
        seen.add(key)
        out += [Case(r, tw, inst) for tw in tws]
    return out


# ------------------------------------------------------------------ weight-gradient twins
# bdn_conv3x3_wgrad_ex has no 4 GB refusal: its kernels form 64-bit pixel addresses (wgrad_kernel) or a 64-bit base per 8 x 16 tile plus
# offsets inside the tile (wgrad7 / wgrad7x, which the plan leaves at 2^31 elements = 4 GB of bf16).  Three sizes: 'cross' and 'top' as above
# (top: the last N below 2^32 bytes = the last N of the pipelined kernels) and 'far', the first N at or past 2^32 bytes.
WG_SIZES = ('cross', 'top', 'far')
WgTwin = namedtuple('WgTwin', 'row size G P N inst widest_bytes period_bytes step_bytes mem_bytes')


def wg_tensors(r):
    x3 = r.prec in ('bf16x3', 'bf16x2')
    es, k = (4 if r.prec == 'fp32' else 2), (2 if x3 else 1)                 # split operands: [hi | lo], twice the channels
    hw = r.H * r.W
    out = [Tensor('dz', k * r.Cout * es, hw, 1), Tensor('in0', k * r.C0 * es, hw, 1)]
    return out + ([Tensor('in1', r.C1 * es, hw, 1)] if r.C1 else [])


def wg_expected_inst(r, size):
    """The GEMM a weight-gradient twin runs: the row's, except that the pipelined kernels hand over to wgrad_kernel past 2^31 elements."""
    if size != 'far' or not r.inst.startswith('wgrad7'):
        return r.inst
    return 'wgrad_kernel<bf16,8,16,1,false>' + ('+wgrad_x3_combine_kernel' if r.inst.startswith('wgrad7x') else '')


def wg_choose(r, size):
    G = 2
    ts = wg_tensors(r)
    P = period_for(ts)
    per_image = max(t.pix * t.bpp for t in ts)
    step, pbytes = G * P, P * per_image
    if size == 'cross':
        N = n_reaching(TWO31 + pbytes, per_image, step)
    elif size == 'top':
        N = n_below(TWO32, per_image, step)
    elif size == 'far':
        N = n_reaching(TWO32, per_image, step)
    else:
        raise ValueError(size)
    mem = 6 * SLAB_BYTES + (1 << 30) + sum(N * t.pix * t.bpp + 2 * _guard(t.pix * t.bpp) for t in ts)
    return WgTwin(r, size, G, P, N, wg_expected_inst(r, size), N * per_image, pbytes, step * per_image, mem)


def wg_twins():
    from tests import launch_cases as lc
    return [wg_choose(r, size) for r in lc.ROWS if r.op == 'wgrad' for size in WG_SIZES]


def wg_twin_id(tw):
    from tests import launch_cases as lc
    return f'{lc.row_id(tw.row)}-{tw.size}-N{tw.N}'


LO = 2.0 ** -9            # grid of the lo halves of split operands: below half a bf16 step of 1 and of 2, so hi = the integer part exactly


def wg_density(r, n_images, mean_abs=1.5):
    """Fraction of non-zero dz elements so that the sum of |dz a| over all n_images x H x W pixels is about 2^22 units per filter element
    (a quarter of the float32 exactness bound, which wg_case then asserts from the data): units are 1, or LO for split operands, whose
    terms are multiples of LO up to about |a| / LO units -- few terms each, so their sums scatter more: an eighth of the bound."""
    x3 = r.prec in ('bf16x3', 'bf16x2')
    units_per_term = mean_abs / LO if x3 else mean_abs
    return min(1.0, (1 << (21 if x3 else 22)) / (n_images * r.H * r.W * units_per_term))


def wg_case(rs, n_images):
    """One period per group of integer-valued weight-gradient operands for the small row rs (N = G P), their exact per-period result and
    the data's own exactness bound for a tensor of n_images images.  Activations from {-2..2} (split operands: {-2, -1, 1, 2} + {-1, 0, 1}
    LO, so the lo half is non-zero), dz = +-1 (+ {-1, 0, 1} LO) at wg_density of the pixels; BatchNorm tables with scales 1, 2, -1 and
    shifts -1, 0, 1."""
    import torch.nn.grad
    N, H, W, C0, C1, Cout = rs.N, rs.H, rs.W, rs.C0, rs.C1, rs.Cout
    G, P = N // rs.ipg, rs.ipg
    x3 = rs.prec in ('bf16x3', 'bf16x2')
    d = wg_density(rs, n_images)
    if x3:
        x0 = int_values((N, C0, H, W), 21, values=(-2, -1, 1, 2))
        x0_lo = int_values((N, C0, H, W), 25, values=(-1, 0, 1), scale=LO)
        dz = int_values((N, Cout, H, W), 23, values=(-1, 1), density=d)
        dz_lo = int_values((N, Cout, H, W), 26, values=(-1, 0, 1), scale=LO) * (dz != 0)
    else:
        x0 = int_values((N, C0, H, W), 21)
        dz = int_values((N, Cout, H, W), 23, values=(-1, 1), density=d)
    x1 = int_values((N, C1, H, W), 22) if C1 else None
    bn = None
    a0 = x0
    if rs.bnrelu:
        r = np.random.default_rng(24)
        scale = r.choice(np.asarray([1.0, 2.0, -1.0], dtype=np.float32), size=(G, C0))
        shift = r.choice(np.asarray([-1.0, 0.0, 1.0], dtype=np.float32), size=(G, C0))
        bn = torch.from_numpy(np.stack([np.zeros_like(scale), np.ones_like(scale), scale, shift], 1))      # mean, invstd, scale, shift
        a0 = torch.cat([torch.relu(x0[g * P:(g + 1) * P] * bn[g, 2][None, :, None, None] + bn[g, 3][None, :, None, None]) for g in range(G)])
    a = torch.cat([a0, x1], 1) if C1 else a0
    shape = (Cout, C0 + C1, 3, 3)

    def cw(act, grad):
        return torch.nn.grad.conv2d_weight(act.double(), shape, grad.double(), padding=1)
    if x3:                                                 # hi x hi + lo x hi (+ hi x lo: three terms); the lo x lo product is left out
        ref = cw(a, dz) + cw(x0_lo, dz) + (cw(a, dz_lo) if rs.prec == 'bf16x3' else 0)
        bound = cw(a.abs() + x0_lo.abs(), dz.abs() + dz_lo.abs())
        unit = LO
    else:
        ref, bound, unit = cw(a, dz), cw(a.abs(), dz.abs()), 1.0
    reps = n_images // N
    abs_sum = bound.max().item()
    assert exact_in_f32(abs_sum, reps, unit), f'sum of |terms| = {abs_sum * reps / unit:.3g} units reaches 2^24'
    assert (ref / unit == (ref / unit).round()).all() and (ref != 0).float().mean() > 0.5, 'degenerate integer data'
    return {'x0': x0 + x0_lo if x3 else x0, 'x1': x1, 'dz': dz + dz_lo if x3 else dz, 'bn': bn, 'ref': ref, 'abs_sum': abs_sum, 'unit': unit,
            'density': d}


# ------------------------------------------------------------------ tiling a period, and the comparator
def tile(small, nblocks, N, alloc):
    """[nblocks * P, ...] (one period per block) -> [N, ...] on the device, block b = N / (nblocks P) copies of period b.  `alloc(shape,
    dtype)` makes the big tensor (a guarded one); no host copy of it exists."""
    P = small.shape[0] // nblocks
    assert small.shape[0] == nblocks * P and N % (nblocks * P) == 0
    reps = N // (nblocks * P)
    big = alloc((N,) + tuple(small.shape[1:]), small.dtype)
    src = small.to(big.device).reshape((nblocks, 1, P) + tuple(small.shape[1:]))
    big.view((nblocks, reps, P) + tuple(small.shape[1:])).copy_(src.expand((nblocks, reps, P) + tuple(small.shape[1:])))
    return big


def period0(t, nblocks, reps):
    """Period 0 of every block of t [rows, ...] (rows = nblocks * reps * rows per period), as one contiguous [nblocks * rows per period, ...]."""
    rows = t.shape[0] // (nblocks * reps)
    assert t.shape[0] == nblocks * reps * rows
    return t.reshape((nblocks, reps, rows) + tuple(t.shape[1:]))[:, 0].reshape((nblocks * rows,) + tuple(t.shape[1:])).clone()


_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NONE = 1 << 62


def period_findings(t, nblocks, reps, slab_bytes=SLAB_BYTES):
    """Compare every period of the contiguous tensor t with period 0 of its block, element by element as raw bits, and look for elements
    that still hold the 0xFF bytes they were born with.  Slabs on the device, one host read-back.  Returns
    {'differ': count, 'first_differ': (block, period, byte offset inside the period) or None, 'unwritten': count, 'first_unwritten': ...}."""
    es = t.element_size()
    v = t.reshape(-1).view(_VIEW[es])
    per = v.numel() // (nblocks * reps)
    assert per * nblocks * reps == v.numel(), 'the tensor is not a whole number of periods'
    v = v.view(nblocks, reps, per)
    marker = 255 if es == 1 else -1
    rows = max(1, slab_bytes // (per * es))
    acc = torch.tensor([0, _NONE, 0, _NONE], dtype=torch.int64, device=t.device)       # differ, first, unwritten, first
    big = torch.tensor(_NONE, dtype=torch.int64, device=t.device)
    for b in range(nblocks):
        base = v[b, :1]
        for r0 in range(0, reps, rows):
            blk = v[b, r0:r0 + rows]
            origin = (b * reps + r0) * per
            for slot, m in ((0, blk != base), (2, blk == marker)):
                f = m.reshape(-1)
                n = f.sum()
                first = torch.where(n > 0, f.to(torch.int32).argmax() + origin, big)   # argmax: the first of equal maxima
                acc[slot] += n
                acc[slot + 1] = torch.minimum(acc[slot + 1], first)
    nd, fd, nu, fu = acc.tolist()

    def where(i):
        return None if i == _NONE else (i // (reps * per), i // per % reps, i % per * es)
    return {'differ': nd, 'first_differ': where(fd), 'unwritten': nu, 'first_unwritten': where(fu)}


def assert_periodic(name, t, nblocks, reps):
    f = period_findings(t, nblocks, reps)
    assert f['unwritten'] == 0, (f'{name}: {f["unwritten"]} elements still hold the 0xFF they were born with; the first at (block, period, '
                                 f'byte in period) = {f["first_unwritten"]}')
    assert f['differ'] == 0, (f'{name}: {f["differ"]} elements differ from period 0 of their block; the first at (block, period, byte in '
                              f'period) = {f["first_differ"]}')


# ------------------------------------------------------------------ integer-valued data for the reductions
def int_values(shape, seed, values=(-2, -1, 0, 1, 2), density=1.0, scale=1.0):
    """float32 tensor drawn from `values` (small integers: exact in bf16) times `scale` (a power of two), zero with probability
    1 - density."""
    r = np.random.default_rng(seed)
    x = r.choice(np.asarray(values, dtype=np.float32), size=shape)
    if density < 1.0:
        x = x * (r.uniform(0, 1, shape) < density)
    return torch.from_numpy((x * scale).astype(np.float32))


def exact_in_f32(abs_sum_period, reps, unit=1.0):
    """Whether a float32 sum of the whole tensor's terms is exact in any order: the terms are multiples of `unit` (a power of two) and the
    sum of their magnitudes over all `reps` periods stays below 2^24 units, so every partial sum is an integer below 2^24 units."""
    return abs_sum_period * reps / unit < (1 << 24)


# ------------------------------------------------------------------ stage-boundary kernels
# bdn_bnrelu, bdn_bnrelu_pool, bdn_fuse_product, bdn_product_pool, bdn_upsample2x and bdn_split_pack index pixels in int (far below 2^31 here) and form every
# address in size_t: no 4 GB bound of their own, so their twins also pass 2^32 bytes.  Shapes: the engine's deepest and shallowest levels.
BN_EXTRA, SKIP_EXTRA = 16, 32
STAGE_KERNELS = ('bnrelu', 'bnrelu_pool', 'fuse_product', 'product_pool', 'upsample2x', 'split_pack', 'product_pool_split', 'upsample2x_split')
SPLIT_KERNELS = ('split_pack', 'product_pool_split', 'upsample2x_split')     # float32 sources, [hi | lo] bf16 outputs
STAGE_SHAPES = ((8, 8, 512), (64, 64, 64))
STAGE_SIZES = ('cross', 'far')            # the widest tensor passes 2^31, resp. 2^32, bytes by at least one period
Stage = namedtuple('Stage', 'kernel prec H W C size P N tensors widest_bytes period_bytes step_bytes mem_bytes')


def stage_tensors(kernel, prec, H, W, C):
    """Activation-sized tensors of a stage twin of N images (fuse_product / product_pool: N = 2 B, both dates)."""
    es = 4 if prec == 'fp32' else 2
    hw, phw = H * W, (H // 2) * (W // 2)
    z = Tensor('z', C * es, hw, 1)
    if kernel == 'bnrelu':
        return [z, Tensor('out', C * es, hw, 1)]
    if kernel == 'bnrelu_pool':
        return [z, Tensor('pool', C * es, phw, 1)]
    if kernel == 'fuse_product':
        return [z, Tensor('f', C * es, hw, 0.5)]
    if kernel == 'product_pool':
        return [z, Tensor('f', C * es, hw, 0.5), Tensor('pool', C * es, phw, 1)]
    if kernel == 'product_pool_split':
        return [Tensor('z', C * 4, hw, 1), Tensor('f_split', 2 * C * 2, hw, 0.5), Tensor('pool_split', 2 * C * 2, phw, 1)]
    if kernel == 'upsample2x_split':
        return [Tensor('src', C * 4, hw, 1), Tensor('out_split', 2 * C * 2, 4 * hw, 1)]
    if kernel == 'upsample2x':             # [N,H,W,C] -> [N,2H,2W,C], BatchNorm+ReLU of the source on load
        return [Tensor('src', C * es, hw, 1), Tensor('out', C * es, 4 * hw, 1)]
    if kernel == 'outc':                   # classifier forward and backward: z, float32 logits and their gradient [N,2,H,W], dA
        return [z, Tensor('logits', 2 * 4, hw, 1), Tensor('dlogits', 2 * 4, hw, 1), Tensor('dA', C * es, hw, 1)]
    if kernel == 'enc_skip_bwd':           # N = 2 B: z and dA hold both dates, dF (a slice of a tensor SKIP_EXTRA channels wider) one
        return [z, Tensor('dF', (C + SKIP_EXTRA) * es, hw, 0.5), Tensor('dP', C * es, phw, 1), Tensor('dA', C * es, hw, 1)]
    if kernel == 'upsample2x_bwd':         # dU = channels [BN_EXTRA, BN_EXTRA + C) of the wider [dF | dU] gradient at twice the map
        return [Tensor('dU', (C + BN_EXTRA) * es, 4 * hw, 1), Tensor('dsrc', C * es, hw, 1)]
    if kernel == 'bn_bwd':                 # dA = channels [BN_EXTRA, BN_EXTRA + C) of a wider tensor
        return [Tensor('dA', (C + BN_EXTRA) * es, hw, 1), z, Tensor('dz', C * es, hw, 1)]
    if kernel == 'split_pack':             # float32 source, [hi | lo] bf16 operand
        return [Tensor('src', C * 4, hw, 1), Tensor('split', 2 * C * 2, hw, 1)]
    raise ValueError(kernel)


def stage_choose(kernel, prec, H, W, C, size):
    ts = stage_tensors(kernel, prec, H, W, C)
    P = period_for(ts)
    per_image = max(int(t.pix * t.bpp * t.imgs) for t in ts)
    step, pbytes = 2 * P, P * per_image                    # two blocks: statistic groups, or the two dates
    edge = {'cross': TWO31, 'far': TWO32}[size]
    N = n_reaching(edge + pbytes, per_image, step)
    mem = 6 * SLAB_BYTES + (1 << 30) + sum(int(N * t.imgs) * t.pix * t.bpp + 2 * _guard(t.pix * t.bpp) for t in ts)
    return Stage(kernel, prec, H, W, C, size, P, N, ts, N * per_image, pbytes, step * per_image, mem)


STAGE_BACKWARD = ('enc_skip_bwd', 'upsample2x_bwd')


def outc_twins():
    return [stage_choose('outc', p, 64, 64, 64, s) for p in ('bf16', 'fp32') for s in STAGE_SIZES]


def stage_backward_twins():
    return [stage_choose(k, p, H, W, C, s) for k in STAGE_BACKWARD for p in ('bf16', 'fp32') for (H, W, C) in STAGE_SHAPES for s in STAGE_SIZES]


def bn_bwd_twins():
    return [stage_choose('bn_bwd', p, H, W, C, s) for p in ('bf16', 'fp32') for (H, W, C) in STAGE_SHAPES for s in STAGE_SIZES]


def bn_bwd_case(C, H, W, P, n_images):
    """Integer-valued BatchNorm-backward operands for two groups of P images: dA (C + BN_EXTRA channels, the last C are the layer's) from
    {-1, 0, 1}, z from {-2..2}, a table with mean 0, invstd 1 (so xhat = z), scales 1, 2, -1 and shifts -1, 0, 1.  The sums of g and g xhat
    over a group are integers and exact in float32 (asserted from the data for n_images images); dz = scale (g - s0/M - xhat s1/M) is the
    same for every period because s0/M and s1/M are (float64 reference for period 0, bit-equality for the rest)."""
    dA = int_values((2 * P, C + BN_EXTRA, H, W), 32, values=(-1, 0, 1))
    z = int_values((2 * P, C, H, W), 31)
    r = np.random.default_rng(33)
    scale = r.choice(np.asarray([1.0, 2.0, -1.0], dtype=np.float32), size=(2, C))
    shift = r.choice(np.asarray([-1.0, 0.0, 1.0], dtype=np.float32), size=(2, C))
    bn = torch.from_numpy(np.stack([np.zeros_like(scale), np.ones_like(scale), scale, shift], 1))
    g64 = dA[:, BN_EXTRA:].double()
    sums, dz = torch.empty(2, 2, C, dtype=torch.float64), torch.empty(2 * P, C, H, W, dtype=torch.float64)
    bound = 0.0
    for g in range(2):
        sl = slice(g * P, (g + 1) * P)
        sc, sh = bn[g, 2].double()[None, :, None, None], bn[g, 3].double()[None, :, None, None]
        gm = g64[sl] * (z[sl].double() * sc + sh > 0)
        s0, s1 = gm.sum((0, 2, 3)), (gm * z[sl].double()).sum((0, 2, 3))
        sums[g, 0], sums[g, 1] = s0, s1
        bound = max(bound, gm.abs().sum((0, 2, 3)).max().item(), (gm * z[sl].double()).abs().sum((0, 2, 3)).max().item())
        M = P * H * W
        dz[sl] = sc * (gm - s0[None, :, None, None] / M - z[sl].double() * s1[None, :, None, None] / M)
    reps = n_images // (2 * P)
    assert exact_in_f32(bound, reps), f'sum of |terms| = {bound * reps:.3g} reaches 2^24'
    assert (sums != 0).float().mean() > 0.9
    return {'dA': dA, 'z': z, 'bn': bn, 'sums': sums, 'dz': dz, 'abs_sum': bound}


def stage_twins():
    return [stage_choose(k, p, H, W, C, s) for k in STAGE_KERNELS for p in (('fp32',) if k in SPLIT_KERNELS else ('bf16', 'fp32'))
            for (H, W, C) in STAGE_SHAPES for s in STAGE_SIZES]


def stage_id(s):
    return f'{s.kernel}-{s.prec}-{s.H}x{s.W}x{s.C}-{s.size}-N{s.N}'


# ------------------------------------------------------------------ the first layer's weight gradient (bdn_conv3x3_wgrad_bnbwd)
# Supported while N H W 64 < 2^31 (bdn_conv3x3_wgrad_bnbwd_supported); pixel addresses are 64-bit.  dA arrives as channels [0, 64) of a
# wider tensor (ldA = 80, the sibling's), so at the top of the supported range dA passes 2^32 bytes while z stays just below.
WB_LDA, WB_CREAL = 80, 13
WbTwin = namedtuple('WbTwin', 'row size G P N widest_bytes period_bytes step_bytes mem_bytes')


def wb_tensors(r):
    es = 2 if r.prec == 'bf16' else 4                      # bf16x3 / bf16x2: float32 dA and z, the split operand [hi(16) | lo(16)] bf16
    hw = r.H * r.W
    return [Tensor('dA', WB_LDA * es, hw, 1), Tensor('z', 64 * es, hw, 1), Tensor('x', (16 if r.prec == 'bf16' else 32) * 2, hw, 1)]


def wb_choose(r, size):
    G, ts = 2, wb_tensors(r)
    P = period_for(ts)
    per_image = max(t.pix * t.bpp for t in ts)
    step, pbytes = G * P, P * per_image
    if size == 'cross':
        N = n_reaching(TWO31 + pbytes, per_image, step)
    elif size == 'top':                                    # the largest N the entry point supports
        N = n_below(TWO31, r.H * r.W * 64, step)
    else:
        raise ValueError(size)
    mem = 6 * SLAB_BYTES + (1 << 30) + sum(N * t.pix * t.bpp + 2 * _guard(t.pix * t.bpp) for t in ts)
    return WbTwin(r, size, G, P, N, N * per_image, pbytes, step * per_image, mem)


def wb_twins():
    from tests import launch_cases as lc
    return [wb_choose(r, size) for r in lc.ROWS if r.op == 'wgrad_bnbwd' for size in ('cross', 'top')]


def wb_case(rs, n_images):
    """Integer-valued operands of the first layer's fused weight gradient for the small row rs: dA (ldA channels, the first 64 are the
    layer's) = +-1 at a density that keeps the sums exact, z from {-2..2}, x from {-2..2} in 13 real channels, a BatchNorm table with
    scales 1, 2, -1 and shifts -1, 0, 1 (split operand: x = +-1 + {-1, 0, 1} LO and scales +-1 -- a term costs up to |x dz| / LO units of
    the 2^24, so small magnitudes keep the gradient from getting too sparse), and zero sums: dz = scale g exactly, with
    g = dA [scale z + shift > 0].  Returns the exact per-period dW as well."""
    import torch.nn.grad
    N, H, W = rs.N, rs.H, rs.W
    G, P = N // rs.ipg, rs.ipg
    x3 = rs.prec != 'bf16'
    units = 1.0 / LO if x3 else 1.5 * 2                    # |x| |scale| on average, roughly, in units
    d = min(1.0, (1 << 22) / (n_images * H * W * units))
    dA = int_values((N, WB_LDA, H, W), 301, values=(-1, 1), density=d)
    z = int_values((N, 64, H, W), 302)
    x = int_values((N, 16, H, W), 303, values=(-1, 1) if x3 else (-2, -1, 0, 1, 2))
    if x3:
        x = x + int_values((N, 16, H, W), 305, values=(-1, 0, 1), scale=LO)
    x[:, WB_CREAL:] = 0
    r = np.random.default_rng(304)
    scale = r.choice(np.asarray([1.0, -1.0] if x3 else [1.0, 2.0, -1.0], dtype=np.float32), size=(G, 64))
    shift = r.choice(np.asarray([-1.0, 0.0, 1.0], dtype=np.float32), size=(G, 64))
    bn = torch.from_numpy(np.stack([np.zeros_like(scale), np.ones_like(scale), scale, shift], 1))
    dz = torch.cat([dA[g * P:(g + 1) * P, :64] * bn[g, 2][None, :, None, None]
                    * (z[g * P:(g + 1) * P] * bn[g, 2][None, :, None, None] + bn[g, 3][None, :, None, None] > 0) for g in range(G)])
    shape = (64, WB_CREAL, 3, 3)
    ref = torch.nn.grad.conv2d_weight(x[:, :WB_CREAL].double(), shape, dz.double(), padding=1)
    bound = torch.nn.grad.conv2d_weight(x[:, :WB_CREAL].abs().double(), shape, dz.abs().double(), padding=1).max().item()
    unit = LO if x3 else 1.0
    assert exact_in_f32(bound, n_images // N, unit), f'sum of |terms| = {bound * (n_images // N) / unit:.3g} units reaches 2^24'
    assert (ref != 0).float().mean() > 0.5, 'degenerate integer data'
    return {'dA': dA, 'z': z, 'x': x, 'bn': bn, 'ref': ref, 'abs_sum': bound, 'unit': unit, 'density': d}


def wb_twin_id(tw):
    from tests import launch_cases as lc
    return f'{lc.row_id(tw.row)}-{tw.size}-N{tw.N}'


# ------------------------------------------------------------------ integer-valued cases for the reductions over N x tiles rows
def int_bn(G, C, seed):
    """[G][4][C] BatchNorm table with mean 0, invstd 1 (xhat = z), scales 1, 2, -1 and shifts -1, 0, 1: integers stay integers."""
    r = np.random.default_rng(seed)
    scale = r.choice(np.asarray([1.0, 2.0, -1.0], dtype=np.float32), size=(G, C))
    shift = r.choice(np.asarray([-1.0, 0.0, 1.0], dtype=np.float32), size=(G, C))
    return torch.from_numpy(np.stack([np.zeros_like(scale), np.ones_like(scale), scale, shift], 1))


def _groups(t, G):
    n = t.shape[0] // G
    return [t[g * n:(g + 1) * n] for g in range(G)]


def _bn_apply(x, bn, G):
    return torch.cat([xg * bn[g, 2][None, :, None, None] + bn[g, 3][None, :, None, None] for g, xg in enumerate(_groups(x, G))])


def int_forward_case(rs):
    """Integer operands of a 'fwd' row at N = G P (fields as tests/test_gpu_launch_shapes.forward_case) and, per group, the exact
    sum z and sum z^2 of the convolution output: what the tile partials of a launch must add up to."""
    from types import SimpleNamespace
    import torch.nn.functional as F
    N, H, W, C0, C1, Cout = rs.N, rs.H, rs.W, rs.C0, rs.C1, rs.Cout
    G = N // rs.ipg
    x0 = int_values((N, C0, H, W), 1)
    x1 = int_values((N, C1, H, W), 2) if C1 else None
    w = int_values((Cout, C0 + C1, 3, 3), 3, values=(-1, 1), density=0.05)
    b = int_values((Cout,), 4, values=(-1, 0, 1))
    bn_in = int_bn(G, C0, 5) if rs.bnrelu else None
    a0 = torch.relu(_bn_apply(x0, bn_in, G)) if rs.bnrelu else x0
    a = torch.cat([a0, x1], 1) if C1 else a0
    z = F.conv2d(a.double(), w.double(), b.double(), padding=1)
    assert z.abs().max() <= 256 and torch.equal(z, z.round()), 'the outputs must be integers that bf16 holds exactly'
    totals = torch.stack([torch.stack([zg.sum((0, 2, 3)), (zg * zg).sum((0, 2, 3))]) for zg in _groups(z, G)])      # [G][2][Cout]
    return SimpleNamespace(x0=x0, x1=x1, w=w, b=b, bn_in=bn_in, ref=z, totals=totals)


def int_dgrad_bs_case(rs):
    """Integer operands of a 'dgrad_bs' row at N = G P (fields as dgrad_bs_case) and, per group, the exact sum g and sum g z of the
    masked gradient g = dA [scale z + shift > 0]."""
    from types import SimpleNamespace
    import torch.nn.grad
    N, H, W, C0, Cout = rs.N, rs.H, rs.W, rs.C0, rs.Cout
    G = N // rs.ipg
    dz = int_values((N, C0, H, W), 51, values=(-1, 1), density=0.2)
    w = int_values((C0, Cout, 3, 3), 52, values=(-1, 1), density=0.05)
    dA = torch.nn.grad.conv2d_input((N, Cout, H, W), w.double(), dz.double(), padding=1)
    zprev = int_values((N, Cout, H, W), 53)
    bnp = int_bn(G, Cout, 54)
    assert dA.abs().max() <= 256 and torch.equal(dA, dA.round())
    g = dA * (_bn_apply(zprev, bnp, G).double() > 0)
    sums = torch.stack([torch.stack([gg.sum((0, 2, 3)), (gg * zz.double()).sum((0, 2, 3))]) for gg, zz in zip(_groups(g, G), _groups(zprev, G))])
    return SimpleNamespace(dz=dz, w=w, ref=dA, zprev=zprev, bnp=bnp, sums=sums)


def int_enc_skip_case(C, H, W, P):
    """Integer operands of bdn_enc_skip_bwd without pooling for P pairs (z [2P], dF [P, C + SKIP_EXTRA]) and the exact per-date sums of
    the stored gradient g = dF a_other [scale z + shift > 0] and of g z."""
    z = int_values((2 * P, C, H, W), 51)
    bn = int_bn(2, C, 52)
    dF = int_values((P, C + SKIP_EXTRA, H, W), 53, values=(-1, 0, 1))
    pre = _bn_apply(z, bn, 2).double()
    a = torch.relu(pre)
    d = dF[:, :C].double()
    g = torch.cat([d * a[P:], d * a[:P]]) * (pre > 0)
    assert g.abs().max() <= 256
    sums = torch.stack([torch.stack([gg.sum((0, 2, 3)), (gg * zz.double()).sum((0, 2, 3))]) for gg, zz in zip(_groups(g, 2), _groups(z, 2))])
    return {'z': z, 'bn': bn, 'dF': dF, 'g': g, 'sums': sums}


def int_outc_case(C, H, W, P, n_images, ncls=2):
    """Integer operands of the classifier's backward for 2 P images (one statistic group): z, an integer table, w from {-1, 0, 1}, dlogits
    = +-1 at a density that keeps every sum over n_images images exact in float32 (asserted from the data).  Exact per-period dw, db,
    sum g and sum g z, and the float64 dz = scale (g - s0/M - z s1/M) of the BatchNorm backward on those sums."""
    npix = n_images * H * W
    d = min(1.0, (1 << 22) / (npix * 3.0))
    z = int_values((2 * P, C, H, W), 61)
    bn = int_bn(1, C, 62)
    w = int_values((ncls, C), 63, values=(-1, 0, 1))
    dl = int_values((2 * P, ncls, H, W), 65, values=(-1, 1), density=d)
    pre = _bn_apply(z, bn, 1).double()
    a = torch.relu(pre)
    dA = torch.einsum('nkhw,kc->nchw', dl.double(), w.double())
    g = dA * (pre > 0)
    dw, db = torch.einsum('nkhw,nchw->kc', dl.double(), a), dl.double().sum((0, 2, 3))
    sums = torch.stack([g.sum((0, 2, 3)), (g * z.double()).sum((0, 2, 3))])[None]                    # [1][2][C]
    reps = n_images // (2 * P)
    bound = max(torch.einsum('nkhw,nchw->kc', dl.abs().double(), a).max().item(), dl.abs().sum((0, 2, 3)).max().item(),
                g.abs().sum((0, 2, 3)).max().item(), (g * z.double()).abs().sum((0, 2, 3)).max().item())
    assert exact_in_f32(bound, reps), f'sum of |terms| = {bound * reps:.3g} reaches 2^24'
    assert (dw != 0).float().mean() > 0.5
    M = 2 * P * H * W
    sc = bn[0, 2].double()[None, :, None, None]
    dz = sc * (g - sums[0, 0][None, :, None, None] / M - z.double() * sums[0, 1][None, :, None, None] / M)
    return {'z': z, 'bn': bn, 'w': w, 'dl': dl, 'dw': dw, 'db': db, 'sums': sums, 'dz': dz, 'density': d}
