"""Ill-conditioned test data and plain float64 references for tests/test_gpu_conditioning.py (pinned without a GPU by
tests/test_illcond_cpu.py).  Four families:

  offsets      pre-BatchNorm maps whose per-channel |mean| / std is driven to 0, 4, 16, 64, 256 (plus exactly constant channels), the
               float64 BatchNorm of such a map, torch's float32 arithmetic on it, and a float32 restatement of the library's documented
               one-pass contract (include/bidate_hip.h: per-tile float32 sum and sum of squares, combined in double);
  planted      maps and tables on a coarse dyadic grid: every pre-activation scale * z + shift is exact in float32 and bf16, many are
               exactly 0 and most 2x2 windows hold a tie for their maximum; first-maximum-wins references written as plain loops;
  loss edges   saturated / shifted logits, degenerate label maps, labels >= ncls;
  bf16 edges   float32 bit patterns at the round-to-nearest-even ties of the bf16 conversion, binade carries, subnormals, signed zeros.

Nothing here imports the library.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
RATIOS = (0.0, 4.0, 16.0, 64.0, 256.0)
# Largest per-channel |mean| / std of any pre-BatchNorm map in a training forward of the reference network on the committed
# fixture tests/golden/g2_c13_b2_s128.npz (CPU oracle): down3.mpconv.1.conv.1.
R0 = 4.0926
REQUIRED_RATIO = max(4.0, 2.0 * R0)
CONST_BIASES = (100.25, 0.0)          # the two exactly constant channels (weights zero)


def _rng(seed):
    return np.random.default_rng(seed)


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a.astype(dtype)))


def rnd(precision, t):
    return t.to(torch.bfloat16).float() if precision == 'bf16' else t.float()


# ================================================================= offsets: forward statistics
def channel_ratios(C):
    """Nominal |mean| / std of channel c: RATIOS in turn over channels [0, C - 2); NaN marks the two constant channels at the end."""
    r = np.array([RATIOS[c % len(RATIOS)] for c in range(C)])
    r[C - 2:] = np.nan
    return r


def offset_conv_case(precision, N, Cin, Cout, spatial, seed=0):
    """Operands of a 3x3 (len(spatial) == 2) or 3x3x3 convolution whose output channel c has |mean| / std close to channel_ratios(Cout)[c]:
    a constant positive input plane (1.0) under Gaussian noise on every input channel but the first, which holds the plane alone; a filter
    whose noise part sums to zero over the noisy channels of every tap and reads the first channel through its centre tap only (so the
    plane reaches the output as one constant, the same at border pixels as inside); half of the offset is carried by that tap, half by the
    bias.  The last two output channels are exactly constant: zero filter, bias CONST_BIASES.
    Returns (x, w, b, z64): x [N,Cin,*spatial] and w [Cout,Cin,3,..] rounded to the storage type, b float32, z64 the float64 convolution of
    exactly these operands -- the achieved ratio is the one measured on z64 (achieved_ratio)."""
    r = _rng(seed)
    nd = len(spatial)
    conv = F.conv2d if nd == 2 else F.conv3d
    x = rnd(precision, _t(1.0 + 0.5 * r.standard_normal((N, Cin) + tuple(spatial))))
    x[:, 0] = 1.0
    wn = r.standard_normal((Cout, Cin) + (3,) * nd) * (2.0 / (3 ** nd * Cin)) ** 0.5
    wn[:, 1:] -= wn[:, 1:].mean(1, keepdims=True)
    wn[:, 0] = 0.0
    wn[Cout - 2:] = 0.0
    wn_t = rnd(precision, _t(wn))
    s = conv(x.double(), wn_t.double(), None, padding=1).std(dim=(0,) + tuple(range(2, 2 + nd)), unbiased=False).numpy()     # noise std per channel
    nominal = channel_ratios(Cout)
    off = np.where(np.isnan(nominal), 0.0, nominal) * s
    centre = (slice(None), 0) + (1,) * nd
    w = wn.copy()
    w[centre] = 0.5 * off
    w[Cout - 2:] = 0.0
    b = 0.5 * off
    b[Cout - 2:] = CONST_BIASES
    w_t, b_t = rnd(precision, _t(w)), _t(b)
    z64 = conv(x.double(), w_t.double(), b_t.double(), padding=1)
    return x, w_t, b_t, z64


def achieved_ratio(z64_group):
    """|mean| / std per channel of one statistic group [n, C, ...] in float64 (inf for a constant channel)."""
    dims = (0,) + tuple(range(2, z64_group.dim()))
    m, s = z64_group.mean(dims), z64_group.std(dims, unbiased=False)
    return torch.where(s > 0, m.abs() / s.clamp_min(1e-300), torch.full_like(m, float('inf')))


def _bshape(t, like):
    return t.reshape((1, -1) + (1,) * (like.dim() - 2))


def bn_train64(z64_group, gamma, beta, eps=BN_EPS):
    """float64 training BatchNorm of one group: (y, mean, biased var)."""
    dims = (0,) + tuple(range(2, z64_group.dim()))
    mean = z64_group.mean(dims)
    var = ((z64_group - _bshape(mean, z64_group)) ** 2).mean(dims)
    inv = 1.0 / torch.sqrt(var + eps)
    y = (z64_group - _bshape(mean, z64_group)) * _bshape(inv * gamma.double(), z64_group) + _bshape(beta.double(), z64_group)
    return y, mean, var


def running64(means, variances, count, rm0, rv0, momentum=0.1):
    """Running buffers after the groups' updates in order (unbiased variance), float64."""
    rm, rv = rm0.double(), rv0.double()
    for mean, var in zip(means, variances):
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * count / max(count - 1, 1)
    return rm, rv


def bn_torch32(z64_groups, gamma, beta, rm0, rv0, eps=BN_EPS, momentum=0.1):
    """The reference's arithmetic: torch.native_batch_norm in float32 on the CPU, group after group on shared running buffers.
    Returns ([y per group], running_mean, running_var)."""
    rm, rv = rm0.clone().float(), rv0.clone().float()
    ys = []
    for zg in z64_groups:
        y, _, _ = torch.native_batch_norm(zg.float(), gamma.float(), beta.float(), rm, rv, True, momentum, eps)
        ys.append(y)
    return ys, rm, rv


def tile_sums_f32(v_f32, rows):
    """The documented contract of the statistics epilogue, restated: the group's values v [count, C] (float32) fall into `rows` tiles of
    consecutive values; each tile keeps a float32 sum and a float32 sum of squares, accumulated one value after the other
    (s += v; q = fma(v, v, q)).  Returns float32 [rows, 2, C].  The fused multiply-add is formed in float64 (the product of two float32
    values is exact there) and rounded once to float32."""
    count, C = v_f32.shape
    per = -(-count // rows)
    pad = np.zeros((rows * per, C), np.float32)
    pad[:count] = v_f32
    t = pad.reshape(rows, per, C)
    s = np.zeros((rows, C), np.float32)
    q = np.zeros((rows, C), np.float32)
    for i in range(per):
        v = t[:, i]
        s = (s + v).astype(np.float32)
        q = (v.astype(np.float64) * v.astype(np.float64) + q.astype(np.float64)).astype(np.float32)
    return np.stack([s, q], 1)


def finalize_contract(partials, count, gamma, beta, eps=BN_EPS):
    """bdn_bn_finalize's documented arithmetic on float32 partial rows [rows, 2, C]: rows added in double, mean = s0 / count,
    var = s1 / count - mean^2 clamped at 0, invstd rounded to float32, scale = gamma * invstd and shift = beta - mean * scale in float32.
    Returns (table [4, C] float32: mean, invstd, scale, shift; var float64)."""
    S = partials.astype(np.float64).sum(0)
    mean = S[0] / count
    var = np.maximum(S[1] / count - mean * mean, 0.0)
    inv = (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)
    g, b = gamma.numpy().astype(np.float32), beta.numpy().astype(np.float32)
    scale = (g * inv).astype(np.float32)
    shift = (b - (mean.astype(np.float32) * scale).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(np.stack([mean.astype(np.float32), inv, scale, shift])), torch.from_numpy(var)


def onepass_contract(z64_group, rows, gamma, beta, eps=BN_EPS):
    """tile_sums_f32 + finalize_contract on one group [n, C, ...] (values taken in image-major, pixel-major order)."""
    C = z64_group.shape[1]
    v = z64_group.float().movedim(1, -1).reshape(-1, C).numpy()
    return finalize_contract(tile_sums_f32(v, rows), v.shape[0], gamma, beta, eps)


def affine_error(z64_group, scale, shift, y64):
    """e = max |z * scale + shift - y64| / max |y64| per channel (float64 arithmetic on the given per-channel scale / shift)."""
    dims = (0,) + tuple(range(2, z64_group.dim()))
    y = z64_group * _bshape(scale.double(), z64_group) + _bshape(shift.double(), z64_group)
    return (y - y64).abs().amax(dims) / y64.abs().amax(dims)


def output_error(y, y64):
    dims = (0,) + tuple(range(2, y64.dim()))
    return (y.double() - y64).abs().amax(dims) / y64.abs().amax(dims)


# ================================================================= offsets: backward
def offset_map(precision, N, C, H, W, seed=0):
    """[N,C,H,W] map, rounded to the storage type, whose channel c has mean = RATIOS[c % 5] * std (std between 0.5 and 2)."""
    r = _rng(seed)
    std = r.uniform(0.5, 2.0, C)
    ratio = np.array([RATIOS[c % len(RATIOS)] for c in range(C)])
    z = (ratio * std)[None, :, None, None] + std[None, :, None, None] * r.standard_normal((N, C, H, W))
    return rnd(precision, _t(z))


def true_table(z, ipg, gamma, beta, eps=BN_EPS):
    """[G,4,C] float32 table (mean, invstd, scale, shift) from the float64 batch statistics of z [N,C,H,W] itself."""
    G = z.shape[0] // ipg
    bn = torch.empty(G, 4, z.shape[1])
    for g in range(G):
        _, mean, var = bn_train64(z[g * ipg:(g + 1) * ipg].double(), gamma, beta, eps)
        inv = 1.0 / torch.sqrt(var + eps)
        bn[g, 0], bn[g, 1] = mean.float(), inv.float()
        bn[g, 2] = (gamma.double() * inv).float()
        bn[g, 3] = (beta.double() - mean * gamma.double() * inv).float()
    return bn


def bn_relu_backward(z, dA, gamma, beta, ipg, dtype=torch.float64, eps=BN_EPS):
    """Autograd of relu(batch_norm(z)) per statistic group in `dtype` (float64: the yardstick, test_bn_bwd's construction; float32:
    torch's own arithmetic on the CPU).  Returns (dz [N,C,H,W], dgamma [C], dbeta [C]) in `dtype`; the parameter gradients are
    accumulated over the groups."""
    zs = z.to(dtype).clone().requires_grad_(True)
    gs, bs = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    ys = [torch.relu(F.batch_norm(zs[i:i + ipg], None, None, gs, bs, True, 0.0, eps)) for i in range(0, z.shape[0], ipg)]
    torch.cat(ys).backward(dA.to(dtype))
    return zs.grad, gs.grad, bs.grad


def bn_bwd_contract64(z, g_masked, bn, ipg):
    """The documented BatchNorm-backward arithmetic (include/bidate_hip.h) in float64 on a GIVEN table bn [G,4,C] and an already masked
    gradient g: s0 = sum g, s1 = sum g * xhat with xhat = (z - mean) * invstd, dz = scale * (g - s0 / M - xhat * s1 / M);
    dgamma = sum over groups of s1, dbeta = of s0.  Returns (dz, dgamma, dbeta, sums [G,2,C])."""
    N, C, H, W = z.shape
    G, M = N // ipg, ipg * H * W
    dz = torch.empty(N, C, H, W, dtype=torch.float64)
    sums = torch.empty(G, 2, C, dtype=torch.float64)
    for g in range(G):
        sl = slice(g * ipg, (g + 1) * ipg)
        mean, inv, scale = (bn[g, i].double()[None, :, None, None] for i in range(3))
        xhat = (z[sl].double() - mean) * inv
        gg = g_masked[sl].double()
        s0, s1 = gg.sum((0, 2, 3)), (gg * xhat).sum((0, 2, 3))
        sums[g, 0], sums[g, 1] = s0, s1
        dz[sl] = scale * (gg - s0[None, :, None, None] / M - xhat * s1[None, :, None, None] / M)
    return dz, sums[:, 1].sum(0), sums[:, 0].sum(0), sums


def per_channel_error(got, ref):
    """max |got - ref| over (N,H,W) per channel, relative to that channel's max |ref|."""
    got, ref = got.double(), ref.double()
    return (got - ref).abs().amax((0, 2, 3)) / ref.abs().amax((0, 2, 3)).clamp_min(1e-300)


def regime_max(err, ratios, lo, hi):
    """Largest entry of err over the channels whose achieved ratio lies in [lo, hi) (0 when there is none)."""
    sel = (ratios >= lo) & (ratios < hi)
    return err[sel].max().item() if sel.any() else 0.0


# ================================================================= planted grids: ties and exact zeros
Z_GRID = (-1.0, -0.5, 0.0, 0.5, 1.0, 1.5)
# (scale, shift) pairs exact in float32 and bf16 for which some grid value gives scale * z + shift == 0 exactly
TABLE_PAIRS = ((0.5, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.5, -0.25), (0.5, 0.5), (1.0, 0.5), (-1.0, 0.5))


def planted_table(G, C, seed=0, neg_zero_shift=False):
    """[G,4,C] table with (scale, shift) from TABLE_PAIRS per (group, channel), mean 0 and invstd 1 (so xhat = z).  neg_zero_shift:
    every other zero shift is stored as -0.0."""
    r = _rng(seed)
    pick = r.integers(0, len(TABLE_PAIRS), (G, C))
    pairs = np.array(TABLE_PAIRS, np.float32)
    bn = np.zeros((G, 4, C), np.float32)
    bn[:, 1] = 1.0
    bn[:, 2], bn[:, 3] = pairs[pick, 0], pairs[pick, 1]
    if neg_zero_shift:
        z = bn[:, 3] == 0
        z[:, ::2] = False
        bn[:, 3][z] = -0.0
    return torch.from_numpy(bn)


def planted_preact(z, bn, ipg):
    """scale * z + shift per group: exact in float32 for planted data (every value a multiple of 1/4 below 4)."""
    out = torch.empty_like(z)
    for g in range(bn.shape[0]):
        s = slice(g * ipg, (g + 1) * ipg)
        out[s] = z[s] * bn[g, 2][None, :, None, None] + bn[g, 3][None, :, None, None]
    return out


def planted_map(N, C, H, W, bn, ipg, seed=0, zero_share=0.12, tie_share=0.75, neg_zero=False):
    """z [N,C,H,W] on Z_GRID.  A share of the pixels is set to the channel's zero point -shift / scale (pre-activation exactly 0), and in
    a share of the 2x2 pooling windows the value at the window's (first) maximum is copied to one more position of the window (a tie for
    the maximum).  neg_zero: a quarter of the zeros of z are stored as -0.0."""
    r = _rng(seed)
    z = np.array(Z_GRID, np.float32)[r.integers(0, len(Z_GRID), (N, C, H, W))]
    bn_n = bn.numpy()
    grp = np.arange(N) // ipg
    scale, shift = bn_n[grp, 2][:, :, None, None], bn_n[grp, 3][:, :, None, None]
    z0 = np.broadcast_to(-shift / scale, z.shape)
    plant = r.uniform(0, 1, z.shape) < zero_share
    z[plant] = z0[plant]
    Hp, Wp = H // 2, W // 2
    if Hp and Wp:
        pre = scale * z + shift
        win = pre[:, :, :2 * Hp, :2 * Wp].reshape(N, C, Hp, 2, Wp, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, Hp, Wp, 4)
        zwin = z[:, :, :2 * Hp, :2 * Wp].reshape(N, C, Hp, 2, Wp, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, Hp, Wp, 4).copy()
        am = win.argmax(-1)
        other = (am + r.integers(1, 4, am.shape)) % 4
        do = r.uniform(0, 1, am.shape) < tie_share
        src = np.take_along_axis(zwin, am[..., None], -1)[..., 0]
        cur = np.take_along_axis(zwin, other[..., None], -1)[..., 0]
        np.put_along_axis(zwin, other[..., None], np.where(do, src, cur)[..., None], -1)
        z[:, :, :2 * Hp, :2 * Wp] = zwin.reshape(N, C, Hp, Wp, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Hp, 2 * Wp)
    z = z + 0.0                                                   # no -0.0 unless asked for
    if neg_zero:
        flip = (z == 0) & (r.uniform(0, 1, z.shape) < 0.25)
        z[flip] = -0.0
    return torch.from_numpy(z.astype(np.float32))


def windows(a):
    """[N,C,H,W] -> [N,C,H//2,W//2,4]: the 2x2 windows of floor-mode pooling in row-major order."""
    N, C, H, W = a.shape
    Hp, Wp = H // 2, W // 2
    return a[:, :, :2 * Hp, :2 * Wp].reshape(N, C, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Hp, Wp, 4)


def zero_share(pre):
    return (pre == 0).double().mean().item()


def positive_tie_share(a):
    """Share of the 2x2 windows whose maximum is positive and attained more than once."""
    w = windows(a)
    m = w.amax(-1, keepdim=True)
    return (((w == m).sum(-1) > 1) & (m[..., 0] > 0)).double().mean().item()


def grid_values(shape, seed, step=0.125, lim=2.0):
    """Values on a `step` grid in [-lim, lim] (exact in float32 and bf16)."""
    n = int(round(lim / step))
    return _t(_rng(seed).integers(-n, n + 1, shape) * step)


def maxpool_first(a):
    """nn.MaxPool2d(2), floor mode, as a plain loop: (values, index 0..3 of the FIRST maximum in row-major window order)."""
    w = windows(a)
    best = w[..., 0].clone()
    idx = torch.zeros_like(best, dtype=torch.int64)
    for k in range(1, 4):
        better = w[..., k] > best                  # strictly greater: an equal later value does not take over
        best = torch.where(better, w[..., k], best)
        idx = torch.where(better, torch.full_like(idx, k), idx)
    return best, idx


def unpool_first(a, dP):
    """Gradient of maxpool_first's values wrt a for the upstream gradient dP: each dP goes to the first maximum of its window."""
    N, C, H, W = a.shape
    Hp, Wp = H // 2, W // 2
    _, idx = maxpool_first(a)
    out = torch.zeros(N, C, H, W, dtype=dP.dtype)
    for k in range(4):
        dy, dx = divmod(k, 2)
        out[:, :, dy:2 * Hp:2, dx:2 * Wp:2] = torch.where(idx == k, dP, torch.zeros_like(dP))
    return out


def enc_skip_bwd_ref(a, dF, dP, B):
    """bdn_enc_skip_bwd's contract on the activations a [2B,C,H,W] (date 1 first): dA_d1 = dF * a_d2 + unpool(dP_d1),
    dA_d2 = dF * a_d1 + unpool(dP_d2), first maximum wins.  Float64; exact for planted data."""
    a, dF = a.double(), dF.double()
    out = torch.cat([dF * a[B:], dF * a[:B]])
    return out + unpool_first(a, dP.double()) if dP is not None else out


# ================================================================= argmax ties
def tied_logits(shape, seed, tie_share=0.2):
    """[n,ncls,H,W] float32 logits on {-2,-1,0,1}: a share of the pixels has ALL classes equal, and half of the zeros are stored as
    -0.0 (so +0.0 meets -0.0 in some pixels).  The tie rate for the maximum is measured by max_tie_share."""
    r = _rng(seed)
    n, ncls, H, W = shape
    lg = r.integers(-2, 2, shape).astype(np.float32)
    alleq = r.uniform(0, 1, (n, 1, H, W)) < tie_share
    lg = np.where(alleq, lg[:, :1], lg)
    lg = lg + 0.0
    flip = (lg == 0) & (r.uniform(0, 1, shape) < 0.5)
    lg[flip] = -0.0
    return torch.from_numpy(lg)


def max_tie_share(logits):
    m = logits.amax(1, keepdim=True)
    return ((logits == m).sum(1) > 1).double().mean().item()


def first_argmax(logits):
    """torch.max(logits, 1) on the CPU: the index of the first maximum."""
    return torch.max(logits.cpu(), 1)[1]


def argmax_counts(logits, labels):
    """{TP, FP, FN, correct} of the first-maximum class map against the labels, class 1 positive."""
    pred = first_argmax(logits)
    lab = labels.reshape(labels.shape[0], *labels.shape[-2:]).long()
    return [int(((pred == 1) & (lab == 1)).sum()), int(((pred == 1) & (lab != 1)).sum()),
            int(((pred != 1) & (lab == 1)).sum()), int((pred == lab).sum())]


# ================================================================= loss extremes
def saturated_logits(shape, seed):
    return _t(40.0 * _rng(seed).standard_normal(shape))


def quarter_grid_logits(shape, seed):
    """Logits on a 1/4 grid in [-4, 4]; adding 8192 to them is exact in float32."""
    return _t(_rng(seed).integers(-16, 17, shape) * 0.25)


def mixed_labels(shape, ncls, seed):
    B, _, H, W = shape
    return torch.from_numpy(_rng(seed).integers(0, ncls, (B, H, W)).astype(np.uint8))


def degenerate_labels(shape, ncls, kind, seed=0):
    """uint8 [B,H,W]: 'zeros', 'ones', 'columns' (a third of the columns hold no positive pixel, a third only positives, the rest mixed),
    'image' (image 0 entirely class 1, the others mixed)."""
    B, _, H, W = shape
    lab = mixed_labels(shape, ncls, seed)
    if kind == 'zeros':
        lab[:] = 0
    elif kind == 'ones':
        lab[:] = 1
    elif kind == 'columns':
        lab[:, :, 0::3] = 0
        lab[:, :, 1::3] = 1
    elif kind == 'image':
        lab[0] = 1
    else:
        raise ValueError(kind)
    return lab


def void_labels(shape, ncls, seed, share=0.1):
    """Mixed labels with `share` of the pixels set to a value >= ncls: 255 (the OSCD masks are {0, 255}), ncls itself (the usual
    ignore = ncls convention) and 7 (the last index of the kernels' class arrays), a third of them each."""
    lab = mixed_labels(shape, ncls, seed)
    r = _rng(seed + 1)
    void = torch.from_numpy(r.uniform(0, 1, tuple(lab.shape)) < share)
    values = torch.tensor([255, ncls, 7], dtype=torch.uint8)[torch.from_numpy(r.integers(0, 3, tuple(lab.shape)))]
    return torch.where(void, values, lab)


# ================================================================= bf16 rounding edges
def bf16_edge_values(n, seed=0, subnormals=True):
    """n float32 values built from bit patterns: round-to-nearest-even ties of the bf16 conversion (low half 0x8000) above even and odd
    bf16 mantissas, their neighbours 0x7fff / 0x8001, mantissas 0x7f.... that carry into the next binade, magnitudes log-uniform over
    2^-100 .. 2^100, float32 subnormals (optional), +0.0 and -0.0, both signs.  All finite, the largest magnitude below 2^101.
    Returns (values float32 [n], kind int8 [n]: 0 tie-even, 1 tie-odd, 2 below tie, 3 above tie, 4 carry, 5 random, 6 subnormal, 7 zero)."""
    r = _rng(seed)
    kind = r.integers(0, 8 if subnormals else 7, n)
    if not subnormals:
        kind[kind == 6] = 7
    sign = r.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    exp = r.integers(27, 228, n).astype(np.uint32) << np.uint32(23)          # biased exponents of 2^-100 .. 2^100
    man7 = r.integers(0, 128, n).astype(np.uint32)
    low = r.integers(0, 1 << 16, n).astype(np.uint32)
    man7 = np.where(kind == 0, man7 & ~np.uint32(1), man7)
    man7 = np.where(kind == 1, man7 | np.uint32(1), man7)
    man7 = np.where(kind == 4, np.uint32(0x7f), man7)
    low = np.where((kind == 0) | (kind == 1), np.uint32(0x8000), low)
    low = np.where(kind == 2, np.uint32(0x7fff), low)
    low = np.where(kind == 3, np.uint32(0x8001), low)
    low = np.where(kind == 4, np.uint32(0x8000) + (r.integers(0, 2, n).astype(np.uint32)), low)       # the tie and just above it
    bits = sign | exp | (man7 << np.uint32(16)) | low
    sub = sign | (r.integers(1, 1 << 23, n).astype(np.uint32))
    bits = np.where(kind == 6, sub, bits)
    bits = np.where(kind == 7, sign, bits)
    return torch.from_numpy(bits.astype(np.uint32).view(np.float32).copy()), torch.from_numpy(kind.astype(np.int8))


def split_ref(t):
    """hi = bf16(x), lo = bf16(x - hi) of a float32 tensor, on the CPU (round to nearest even): (hi, lo) bf16."""
    hi = t.to(torch.bfloat16)
    return hi, (t - hi.float()).to(torch.bfloat16)


def bits16(t):
    return t.contiguous().view(torch.int16)
