"""Float64 reference of BiDateNet evaluated AT A RECORDED FORWARD STATE (CPU only; fabric_amd is never imported here).

tests/test_gpu_model.py and tests/test_gpu_autograd.py compare the engine with a float32 / float64 oracle whose forward is a different
forward: ReLU masks, batch statistics and pooling winners move on bf16-sized activation differences, so their bounds (bf16: 0.8 per
tensor) are forward-divergence allowances.  This module removes that term.  After a training-layout forward the engine's workspace holds
every layer's raw output z and its [G][4][C] table {mean, invstd, scale, shift} (and, outside bf16x3, x0, the skips f, the pooled maps and
the upsampled maps).  Every stage of the network is re-evaluated in float64 on operands rebuilt from the engine's own STORED predecessors:

  audit_forward(state)     per stage, the deviation of what the engine stored from the float64 op on the engine's stored inputs: one
                           stage's rounding, nothing upstream of it
  forced_backward(state)   float64 gradients of every parameter (and of the two images) with every local derivative evaluated at the
                           stored values: ReLU masks from the engine's own scale*z+shift, BatchNorm backward from the table's mean and
                           invstd, unpooling to the first maximum of the stored activations, fusion partners = stored activations

The same graph code, free-running in float32 with the roundings applied (emulate()), is a CPU stand-in for the engine: it supplies a state
and "engine" gradients for tests/test_forced_ref_cpu.py (noise floor, sensitivity to wiring mutations).  With precision 'exact' (no
rounding, float64) the state of oracle.bidate_oracle itself can be fed in, and forced_backward must equal plain autograd of the oracle.

Where the engine rounds (read off the kernels; q_store = the storage type, q_gemm = what a GEMM operand is rounded to):

  * pack_input: the images are rounded to the storage type, channels padded with zeros to a multiple of 16
    (csrc/head.hip:24-25); bf16x3: split into hi = bf16(x), lo = bf16(x - hi) (csrc/head.hip:43-49).
  * IN_BNRELU consumers (the second conv of every double_conv, the classifier, upsample2x, product_pool / fuse_*): the operand is
    a = q_store(relu(fma(z, scale, shift))): ONE float32 fused multiply-add on the STORED z and the float32 table, ReLU, then one rounding
    to the storage type (csrc/common.hpp:146-153 bnrelu_unit, :160-168 bnrelu_pair; csrc/fuse.hip:15-18 act1; csrc/head.hip:267).
    bf16x3: a stays float32 and is split hi / lo where the GEMM stages it (csrc/x3.hip:12-20, :38).
  * product_pool / fuse_*: the fusion of two ROUNDED activations in float32, one rounding on store (csrc/fuse.hip:126-129, :152-153,
    :214-218): a1*a2 of two bf16 values is exact in float32, |a2 - a1| is one float32 subtraction.  The pooled map is the maximum of
    rounded activations: exact, no rounding of its own (csrc/fuse.hip:215, :223-224).
  * upsample2x: BatchNorm+ReLU with the storage rounding first (csrc/fuse.hip:316 act1, :349 bnrelu_unit), then four taps blended in
    float32 with float32 tap weights -- lam = scale*d - floor(scale*d), scale = float((n-1)/(2n-1)) (csrc/fuse.hip:283-289) -- and
    one rounding on store (:319, :377).  The float32 lam is up to 2^-23*n_in away from the exact one: that is in the stage's bound.
  * weight packing: bf16: bf16(w); fp32: w; bf16x3: [hi(w) | hi(w) | lo(w)] against operand channels [a_hi | a_lo | a_hi]
    (csrc/x3.hip:82-93, :104-110), so a product keeps a_hi*w_hi + a_lo*w_hi + a_hi*w_lo and DROPS a_lo*w_lo (csrc/x3.hip:3-4): the
    reference convolution is conv(a_hi + a_lo, w_hi + w_lo) - conv(a_lo, w_lo).
  * convolution epilogue: v = accumulator + bias in float32; the per-tile BatchNorm sums (sum v, sum v*v) are taken from v, the float32
    ACCUMULATORS, before z = q_store(v) is stored (csrc/conv3x3.hip:838-848: `s += v; q = fmaf(v, v, q)` precede `from_f<TO>(v)`).  The
    tiles are reduced in float64, var = E[v^2] - mean^2 clamped at 0, invstd = float(1/sqrt(var + eps)), scale = gamma*invstd,
    shift = beta - float(mean)*scale in float32 (csrc/bn.hip:145-153).  So in bf16 the table is that of the unrounded v while every
    consumer (forward and backward) applies it to the rounded z.  Running-statistics tables: invstd = 1/sqrtf(rv + eps) (csrc/bn.hip:197).
  * classifier: a = q_store(relu(fma(z, scale, shift))) of the last layer, float32 weights, float32 fmaf chain (csrc/head.hip:267-268).

Design choices of the backward that are modelled, not flagged: gradients are stored under the landing layer's ReLU mask
(csrc/conv3x3.hip:874-883) -- the same function; the folded three-constant dz = a g + b z + c (engine.folds_bn_bwd) is the explicit
BatchNorm backward with the sums pulled out -- the same function; statistics from the accumulators (above): the table is taken as stored.
Rounding steps pass the gradient straight through; weight gradients are with respect to the float32 master weight, through q_gemm.
"""
import torch
import torch.nn.functional as F

from oracle import bidate_oracle as O

ENC_CH = (64, 128, 256, 512, 512)
DEC_OUT = (256, 128, 64, 64)
BN_EPS = 1e-5
PRECISIONS = ('fp32', 'bf16x3', 'bf16x3-fast', 'bf16')
# unit roundoff of the STORED type: bf16 keeps 8 significand bits, float32 24 (the figures the audit's bounds are written in)
U_STORE = {'bf16': 2.0 ** -8, 'fp32': 2.0 ** -23, 'bf16x3': 2.0 ** -23, 'bf16x3-fast': 2.0 ** -23, 'exact': 0.0}


def build_layers(n_channels):
    """The 18 3x3 convolutions in forward order: dict(name, conv, bn, cin, cout, level, enc) -- fabric_amd.engine.build_layers restated
    (tests/test_gpu_forced.py asserts the two agree)."""
    out, prev = [], n_channels
    for k in range(1, 6):
        base = 'inc.conv.conv' if k == 1 else f'down{k - 1}.mpconv.1.conv'
        co = ENC_CH[k - 1]
        out.append(dict(name=f'e{k}a', conv=f'{base}.0', bn=f'{base}.1', cin=prev, cout=co, level=k, enc=True))
        out.append(dict(name=f'e{k}b', conv=f'{base}.3', bn=f'{base}.4', cin=co, cout=co, level=k, enc=True))
        prev = co
    cprev = ENC_CH[4]
    for j in range(1, 5):
        k = 5 - j
        base = f'up{j}.conv.conv'
        co = DEC_OUT[j - 1]
        out.append(dict(name=f'd{j}a', conv=f'{base}.0', bn=f'{base}.1', cin=ENC_CH[k - 1] + cprev, cout=co, level=k, enc=False))
        out.append(dict(name=f'd{j}b', conv=f'{base}.3', bn=f'{base}.4', cin=co, cout=co, level=k, enc=False))
        cprev = co
    return out


# ---------------------------------------------------------------- roundings
def _bf16(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def hi_lo(t):
    """bdn_split_pack's split of float32 values: hi = bf16(x), lo = bf16(x - hi) (the difference is exact in float32)."""
    f = t.float()
    hi = f.to(torch.bfloat16).float()
    return hi.to(t.dtype), (f - hi).to(torch.bfloat16).float().to(t.dtype)


class Rounding:
    """q_store / q_gemm of one numerics setting, on tensors of any float dtype holding float32-representable values."""

    def __init__(self, precision):
        if precision not in PRECISIONS + ('exact',):
            raise ValueError(precision)
        self.precision = precision
        self.exact = precision == 'exact'
        self.x3 = precision in ('bf16x3', 'bf16x3-fast')
        self.u = U_STORE[precision]

    def store(self, t):
        if self.exact:
            return t
        return _bf16(t) if self.precision == 'bf16' else t.float().to(t.dtype)

    def gemm(self, t):
        if self.exact:
            return t
        if self.precision == 'bf16':
            return _bf16(t)
        if self.x3:
            hi, lo = hi_lo(t)
            return hi + lo
        return t.float().to(t.dtype)

    def gemm_lo(self, t):
        return hi_lo(t)[1] if self.x3 else None

    def fma(self, z, sc, sh):
        """fmaf(z, sc, sh) of float32 values: the product is exact in float64, one rounding there, one to float32."""
        if self.exact:
            return z * sc + sh
        return (z.double() * sc.double() + sh.double()).float().to(z.dtype)


class _Subst(torch.autograd.Function):
    """Value `val`, derivative of `ref`: a rounding (or the engine's stored result) with the gradient passed straight through."""

    @staticmethod
    def forward(ctx, ref, val):
        return val.to(ref.dtype).clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _st(t, fn):
    return _Subst.apply(t, fn(t.detach()))


class _GradRound(torch.autograd.Function):
    """Identity whose backward rounds the gradient to the storage type: the emulated engine stores dA and dz in it."""

    @staticmethod
    def forward(ctx, t, fn):
        ctx.fn = fn
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


class _BN(torch.autograd.Function):
    """scale*z + shift of one statistic group with the explicit backward at the GIVEN table:
        batch    dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)),  xhat = (z - mean)*invstd,  dgamma = sum g*xhat,  dbeta = sum g
        running  dz = scale*g (the statistics are constants), dgamma and dbeta as above
    dg_mean / dg_inv: the mean / invstd dgamma is finalized with (a wiring mutation of the sensitivity tests; normally the group's own).
    With batch statistics sum(dz) = -gamma*invstd^2*dgamma*(mean(z) - mean): the conv bias in front gets exactly 0 only where the table's
    mean IS the mean of the z it is applied to.  The engine's table is that of the float32 accumulators and z is stored rounded, so at a
    device state the formula leaves a rounding-sized residual there (forced_backward's `residual`)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, mean, inv, scale, shift, rnd, running, dg_mean, dg_inv, tag):
        ctx.save_for_backward(z, gamma, mean, inv, scale, dg_mean, dg_inv)
        ctx.running, ctx.tag = running, tag
        c = lambda v: v[None, :, None, None]
        return rnd.fma(z, c(scale), c(shift))

    @staticmethod
    def backward(ctx, g):
        z, gamma, mean, inv, scale, dg_mean, dg_inv = ctx.saved_tensors
        c = lambda v: v[None, :, None, None]
        m = g.numel() // g.shape[1]
        xhat = (z - c(mean)) * c(inv)
        dbeta = g.sum(dim=(0, 2, 3))
        dgamma = (g * xhat).sum(dim=(0, 2, 3))
        dz = c(scale) * g if ctx.running else c(gamma * inv) * (g - c(dbeta / m) - xhat * c(dgamma / m))
        dgamma_out = (g * ((z - c(dg_mean)) * c(dg_inv))).sum(dim=(0, 2, 3))
        if ctx.tag is not None:                          # (probe dict, key): the group's own dgamma, for the conv-bias residual
            ctx.tag[0][ctx.tag[1]] = dgamma.detach()
        return dz, dgamma_out, dbeta, None, None, None, None, None, None, None, None, None


def maxpool_first(a, last=False):
    """O.maxpool2's values with the gradient routed to the FIRST maximum in row-major window order (last=True: to the last -- a mutation)."""
    n, c, h, w = a.shape
    ho, wo = h // 2, w // 2
    xw = a[:, :, :2 * ho, :2 * wo].reshape(n, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, ho, wo, 4)
    eq = xw.detach() == xw.detach().max(dim=-1, keepdim=True).values
    if last:
        eq = eq.flip(-1)
    pick = eq & (eq.cumsum(-1) == 1)
    if last:
        pick = pick.flip(-1)
    return torch.where(pick, xw, torch.zeros_like(xw)).sum(-1)


def fuse(a1, a2, fusion):
    """'product' = torch.relu(x_d2 * x_d1) (models/bidate_model.py:35-38), 'absdiff' = |x_d2 - x_d1| with sign 0 at equality."""
    if fusion == 'product':
        return torch.relu(a2 * a1)
    if fusion == 'absdiff':
        return (a2 - a1).abs()
    raise ValueError(fusion)


def absdiff(a1, a2):
    return fuse(a1, a2, 'absdiff')


def _dev(got, ref):
    d = (got - ref).abs()
    return float(d.max()), float(ref.abs().max())


# ---------------------------------------------------------------- the graph
def _run(params, x1, x2, cfg, state=None, dtype=torch.float64, audit=None, c_conv=0.0, mutate=None, grad_round=False, probe=None):
    """BiDateNet's training-layout forward as the engine composes it.

    state None: free-running (the emulated engine): every stage consumes what the previous one produced, the roundings applied, and the
    recorded state is returned beside the logits.  state given: forced -- every stage's OUTPUT is replaced by the engine's stored value
    (derivative kept), so each stage sees only stored predecessors.  audit: dict that receives the per-stage deviations (forced only)."""
    rnd = Rounding(cfg['precision'])
    fusion, running = cfg['fusion'], cfg['bn_mode'] == 'running'
    mutate = mutate or {}
    forced = state is not None
    rec = None if forced else dict(z={}, bn={}, f={}, pool={}, U={})
    B, C = x1.shape[:2]
    u = rnd.u
    cast = lambda t: t.to(dtype)

    def stored(group, key, ref, rfn, kind='elementwise', tol=None):
        """The stage result q(ref), q = rfn: free-running -> rounded here and recorded; forced -> the engine's stored tensor where it
        exists, audited against the UNROUNDED float64 ref (bound tol(ref): one rounding of the stored type), else q(ref) itself."""
        if not forced:
            out = _st(ref, rfn)
            if key is None:
                rec[group] = out.detach()
            else:
                rec[group][key] = out.detach()
            return out
        src = state.get(group)
        val = src if key is None or src is None else src.get(key)
        if val is None:                                  # bf16x3: never a tensor -- derived
            return _st(ref, rfn)
        val = cast(val)
        if audit is not None:
            r = ref.detach()
            d = (val - r).abs()
            ent = dict(kind=kind, dev=float(d.max()), scale=float(r.abs().max()))
            if not rnd.exact:
                t = tol(r)
                ent['ratio'] = float(torch.where(d == 0, torch.zeros_like(d), d / t.clamp_min(1e-300)).max())
            audit[group if key is None else f'{group}[{key}]'] = ent
        return _Subst.apply(ref, val)

    def table(L, z_acc, g0):
        """[4][C] rows of one statistic group: forced -> the stored table; free-running -> what bn_finalize / bn_eval would write."""
        gam, bet = params[f"{L['bn']}.weight"], params[f"{L['bn']}.bias"]
        if forced:
            return [cast(state['bn'][L['name']][g0][i]) for i in range(4)]
        if rnd.exact:
            if running:
                mean, inv = params[f"{L['bn']}.running_mean"].detach(), torch.rsqrt(params[f"{L['bn']}.running_var"].detach() + BN_EPS)
            else:
                zd = z_acc.detach()
                mean = zd.mean(dim=(0, 2, 3))
                inv = torch.rsqrt(((zd - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3)) + BN_EPS)
            scale = gam.detach() * inv
            return [mean, inv, scale, bet.detach() - mean * scale]
        if running:
            mean = params[f"{L['bn']}.running_mean"].detach().float()
            inv = 1.0 / torch.sqrt(params[f"{L['bn']}.running_var"].detach().float() + BN_EPS)
        else:
            zd = z_acc.detach().double()
            m = zd.mean(dim=(0, 2, 3))
            var = ((zd * zd).mean(dim=(0, 2, 3)) - m * m).clamp_min(0.0)
            mean, inv = m.float(), (1.0 / torch.sqrt(var + BN_EPS)).float()
        scale = gam.detach().float() * inv
        shift = bet.detach().float() - mean * scale
        return [cast(t) for t in (mean, inv, scale, shift)]

    def conv_stage(L, a_in, groups):
        """conv3x3 + bias + the BatchNorm table(s); returns (z as stored, [table per group])."""
        name = L['name']
        w, b = params[f"{L['conv']}.weight"], params[f"{L['conv']}.bias"]
        aq, wq = _st(a_in, rnd.gemm), _st(w, rnd.gemm)
        z_acc = F.conv2d(aq, wq, b, padding=1)
        if rnd.x3:                                       # the dropped a_lo*w_lo term
            z_acc = z_acc - F.conv2d(rnd.gemm_lo(a_in.detach()), rnd.gemm_lo(w.detach()), None, padding=1)
        n = a_in.shape[0]
        ipg = n // groups
        tabs = [table(L, z_acc[g * ipg:(g + 1) * ipg], g) for g in range(groups)]
        if not forced:
            rec['bn'][name] = torch.stack([torch.stack(t) for t in tabs]).detach()
            z = _st(z_acc, rnd.store)
            rec['z'][name] = z.detach()
            if grad_round:
                z = _GradRound.apply(z, rnd.store)
            return z, tabs
        zs = cast(state['z'][name])
        if audit is not None:
            zr = z_acc.detach()
            A = F.conv2d(aq.detach().abs(), wq.detach().abs(), b.detach().abs(), padding=1)
            if rnd.x3:
                A = A + F.conv2d(rnd.gemm_lo(a_in.detach()).abs(), rnd.gemm_lo(w.detach()).abs(), None, padding=1)
            d = (zs - zr).abs()
            ent = dict(kind='conv', dev=float(d.max()), scale=float(zr.abs().max()), K=9 * _round16(a_in.shape[1]))
            if not rnd.exact:
                ent['c'] = float(((d - u * zr.abs()).clamp_min(0.0) / A.clamp_min(1e-300)).max())
            audit[f'z[{name}]'] = ent
            audit[f'bn[{name}]'] = _audit_table(L, params, zr, A, [[t.detach() for t in tb] for tb in tabs], ipg, running, rnd, c_conv)
        return _Subst.apply(z_acc, zs), tabs

    def act(L, z, tabs):
        """a = q_store(relu(fma(z, scale, shift))) per statistic group, with the forced BatchNorm backward."""
        name = L['name']
        gam, bet = params[f"{L['bn']}.weight"], params[f"{L['bn']}.bias"]
        ipg = z.shape[0] // len(tabs)
        outs = []
        for g, tb in enumerate(tabs):
            dg = tabs[0] if mutate.get('dgamma_joint') == name else tb
            outs.append(_BN.apply(z[g * ipg:(g + 1) * ipg], gam, bet, tb[0], tb[1], tb[2], tb[3], rnd, running, dg[0], dg[1],
                                  None if probe is None else (probe, (name, g))))
        pre = torch.cat(outs) if len(outs) > 1 else outs[0]
        a = _st(torch.relu(pre), rnd.store)
        if grad_round:
            a = _GradRound.apply(a, rnd.store)
        return a

    by = {L['name']: L for L in build_layers(C)}
    # ---- packed input
    x = torch.cat([x1, x2])
    # (bf16x3: the float32 values; every operand is split ONCE, by the convolution that consumes it -- the split is not idempotent: hi + lo
    # can sit in the binade below hi, where bf16(hi + lo) != hi)
    x0 = stored('x0', None, x, rnd.store, tol=lambda r: u * r.abs())
    # ---- shared encoder, both dates as one batch of 2B images with two statistic groups
    skips, a_in = {}, x0
    for k in range(1, 6):
        La, Lb = by[f'e{k}a'], by[f'e{k}b']
        za, ta = conv_stage(La, a_in, 2)
        zb, tb = conv_stage(Lb, act(La, za, ta), 2)
        ab = act(Lb, zb, tb)
        skips[k] = stored('f', k, fuse(ab[:B], ab[B:], fusion), rnd.store, tol=lambda r: u * r.abs())
        if k < 5:
            pooled = maxpool_first(ab, last=mutate.get('unpool_last') == k)
            a_in = stored('pool', k + 1, pooled, rnd.store, kind='pool', tol=lambda r: r * 0)
    # ---- decoder on the fused skips
    prev = skips[5]
    for j in range(1, 5):
        k = 5 - j
        La, Lb = by[f'd{j}a'], by[f'd{j}b']
        up = O.pad_to(O.upsample2x_align(prev), skips[k])
        n_in, amax = max(prev.shape[2:]), prev.detach().abs().amax(dim=(2, 3), keepdim=True)
        U = stored('U', j, up, rnd.store, kind='upsample', tol=lambda r: u * r.abs() + 2.0 ** -21 * n_in * amax)
        za, ta = conv_stage(La, torch.cat([skips[k], U], dim=1), 1)
        zb, tb = conv_stage(Lb, act(La, za, ta), 1)
        prev = act(Lb, zb, tb)
    wc, bc = params['outc.conv.weight'], params['outc.conv.bias']
    logits = F.conv2d(prev, wc, bc)
    if forced and audit is not None and 'logits' in state:
        Ac = F.conv2d(prev.detach().abs(), wc.detach().abs(), bc.detach().abs())
        got = cast(state['logits'])
        dev, scale = _dev(got, logits.detach())
        audit['logits'] = dict(kind='classifier', dev=dev, scale=scale,
                               ratio=None if rnd.exact else float(((got - logits.detach()).abs() / ((prev.shape[1] + 2) * 2.0 ** -24 * Ac)).max()))
    if not forced:
        rec['logits'] = logits.detach()
    return logits, rec


def _round16(v):
    return (v + 15) // 16 * 16


def _audit_table(L, params, zr, A, tabs, ipg, running, rnd, c_conv):
    """The stored table against float64 statistics of the quantity the kernel sums (v = accumulator + bias; here its float64 value zr):
    dict(dev, scale, ratio) with ratio = the worst |deviation| / bound over the four rows and the groups.  Bounds:
      mean    c*mean(A) [accumulation order of v] + 2^-15*mean|v| [float32 sums of tiles of <= 512 pixels] + 2^-24*|mean| [the store]
      invstd  between (var +- tol_var + eps)^-1/2, tol_var = 2c*mean(A|v|) + 2^-15*mean(v^2) + 2|mean|*tol_mean + tol_mean^2, and 2^-23 relative
      scale   gamma*invstd OF THE TABLE, one float32 rounding;  shift  beta - mean*scale OF THE TABLE, two float32 roundings
      running mean = running_mean exactly, invstd = 1/sqrtf(rv + eps) within 4 float32 roundings"""
    gam, bet = params[f"{L['bn']}.weight"].detach().double(), params[f"{L['bn']}.bias"].detach().double()
    worst, dev, scale_ = 0.0, 0.0, 0.0
    for g, tb in enumerate(tabs):
        mean, inv, sc, sh = (t.double() for t in tb)
        if running:
            rm, rv = params[f"{L['bn']}.running_mean"].detach().double(), params[f"{L['bn']}.running_var"].detach().double()
            mref, iref = rm, torch.rsqrt(rv + BN_EPS)
            r_mean = (mean - mref).abs() / (2.0 ** -24 * mref.abs()).clamp_min(1e-300) if not rnd.exact else (mean - mref).abs()
            r_inv = (inv - iref).abs() / (4 * 2.0 ** -24 * iref) if not rnd.exact else (inv - iref).abs()
            r_mean = torch.where((mean - mref) == 0, torch.zeros_like(r_mean), r_mean)
        else:
            v = zr[g * ipg:(g + 1) * ipg].double()
            a = A[g * ipg:(g + 1) * ipg].double()
            mref = v.mean(dim=(0, 2, 3))
            m2 = (v * v).mean(dim=(0, 2, 3))
            var = (m2 - mref * mref).clamp_min(0.0)
            iref = torch.rsqrt(var + BN_EPS)
            if rnd.exact:
                r_mean, r_inv = (mean - mref).abs(), (inv - iref).abs()
            else:
                tol_mean = c_conv * a.mean(dim=(0, 2, 3)) + 2.0 ** -15 * v.abs().mean(dim=(0, 2, 3)) + 2.0 ** -24 * mref.abs()
                tol_var = 2 * c_conv * (a * v.abs()).mean(dim=(0, 2, 3)) + 2.0 ** -15 * m2 + 2 * mref.abs() * tol_mean + tol_mean ** 2
                lo = torch.rsqrt(var + tol_var + BN_EPS) * (1 - 2.0 ** -23)
                hi = torch.rsqrt((var - tol_var).clamp_min(0.0) + BN_EPS) * (1 + 2.0 ** -23)
                r_mean = (mean - mref).abs() / tol_mean
                r_inv = torch.nan_to_num(torch.maximum((inv - iref) / (hi - iref), (iref - inv) / (iref - lo)), nan=0.0)
        dev = max(dev, float((mean - mref).abs().max()), float((inv - iref).abs().max()))
        scale_ = max(scale_, float(mref.abs().max()), float(iref.abs().max()))
        if rnd.exact:
            d_sc, d_sh = (sc - gam * inv).abs(), (sh - (bet - mean * sc)).abs()
            dev = max(dev, float(d_sc.max()), float(d_sh.max()))
            worst = max(worst, float(r_mean.max()), float(r_inv.max()), float(d_sc.max()), float(d_sh.max()))
            continue
        r_sc = (sc - gam * inv).abs() / (2.0 ** -24 * (gam * inv).abs())
        r_sh = (sh - (bet - mean * sc)).abs() / (2.0 ** -23 * (bet.abs() + (mean * sc).abs()))
        worst = max(worst, float(r_mean.max()), float(r_inv.max()), float(r_sc.max()), float(r_sh.max()))
    return dict(kind='table', dev=dev, scale=scale_, ratio=worst)


# ---------------------------------------------------------------- public surface
def _cfg(state):
    return dict(precision=state['precision'], fusion=state['fusion'], bn_mode=state['bn_mode'])


def _leaves(state, want_dx, dtype=torch.float64):
    params = {k: (v.to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in state['params'].items()}
    names = [k for k, v in params.items() if v.is_floating_point() and 'running_' not in k]
    for k in names:
        params[k].requires_grad_(True)
    x1, x2 = state['x_d1'].to(dtype).clone(), state['x_d2'].to(dtype).clone()
    if want_dx:
        x1.requires_grad_(True)
        x2.requires_grad_(True)
    return params, names, x1, x2


def audit_forward(state, c_conv=0.0):
    """{stage: dict(kind, dev, scale[, c | ratio])}: the deviation of every stored stage result from the float64 op on the engine's stored
    predecessors.  Stages: x0; z[L] and bn[L] of the 18 layers; f[1..5]; pool[2..5]; U[1..4]; logits (bf16x3: z, bn and logits only).
    conv stages report c = max (|z_engine - z_ref| - u|z_ref|)+ / A, A = conv(|a|,|w|) + |b|; the others ratio = max |dev| / bound
    (elementwise stages: one rounding of the stored type, u*|ref|; pooled maps: 0, exact; tables: _audit_table with c_conv)."""
    params, _, x1, x2 = _leaves(state, False)
    out = {}
    with torch.no_grad():
        _run(params, x1, x2, _cfg(state), state=state, audit=out, c_conv=c_conv)
    return out


def forced_backward(state, dlogits, want_dx=True, audit=None, c_conv=0.0, mutate=None, residual=None):
    """Float64 gradients {state-dict key: tensor} (+ 'dx1', 'dx2' with want_dx) of sum(logits*dlogits) with every local derivative at the
    stored values.  audit: a dict that receives audit_forward's result from the same pass.  residual: a dict that receives, per conv bias
    in front of a batch-statistics BatchNorm, what the explicit BatchNorm backward leaves there because the table's mean is not the mean
    of the stored z: -sum_g gamma*invstd_g^2*dgamma_g*(mean(z_g) - mean_g) (0 at an exact state).  The gradient itself is analytically 0."""
    params, names, x1, x2 = _leaves(state, want_dx)
    probe = {}
    logits, _ = _run(params, x1, x2, _cfg(state), state=state, audit=audit, c_conv=c_conv, mutate=mutate, probe=probe)
    wrt = [params[k] for k in names] + ([x1, x2] if want_dx else [])
    g = torch.autograd.grad(logits, wrt, dlogits.to(logits.dtype), allow_unused=True)
    out = {k: (v if v is not None else torch.zeros_like(p)) for k, v, p in zip(names, g, wrt)}
    if want_dx:
        out['dx1'], out['dx2'] = g[-2], g[-1]
    if residual is not None and state['bn_mode'] == 'batch':
        for L in build_layers(x1.shape[1]):
            z, bn = state['z'][L['name']].double(), state['bn'][L['name']].double()
            ipg, r = z.shape[0] // bn.shape[0], 0.0
            for gi in range(bn.shape[0]):
                gap = z[gi * ipg:(gi + 1) * ipg].mean(dim=(0, 2, 3)) - bn[gi, 0]
                r = r - params[f"{L['bn']}.weight"].detach() * bn[gi, 1] ** 2 * probe[L['name'], gi] * gap
            residual[f"{L['conv']}.bias"] = r
    return out


def emulate(sd, x_d1, x_d2, precision, fusion='product', bn_mode='batch', dlogits_fn=None, want_dx=True, mutate=None):
    """The CPU stand-in for the engine: the same graph free-running in float32 (float64 for 'exact') with the roundings applied and
    straight-through gradients; the gradient of every stored tensor (dz, dA) is rounded to the storage type like the engine's.
    Returns (state, grads): the state in state_from_workspace's format, the "engine" gradients of sum(logits*dlogits_fn(logits))."""
    dtype = torch.float64 if precision == 'exact' else torch.float32
    st = dict(precision=precision, fusion=fusion, bn_mode=bn_mode, params={k: v.clone() for k, v in sd.items()},
              x_d1=x_d1.clone(), x_d2=x_d2.clone())
    params, names, x1, x2 = _leaves(st, want_dx, dtype)
    logits, rec = _run(params, x1, x2, _cfg(st), dtype=dtype, mutate=mutate, grad_round=precision != 'exact')
    st.update(rec)
    if Rounding(precision).x3:                           # the engine keeps these as split GEMM operands only
        for k in ('x0', 'f', 'pool', 'U'):
            st.pop(k)
    if dlogits_fn is None:
        return st, None
    dl = dlogits_fn(logits.detach())
    wrt = [params[k] for k in names] + ([x1, x2] if want_dx else [])
    g = torch.autograd.grad(logits, wrt, dl.to(dtype), allow_unused=True)
    grads = {k: (v if v is not None else torch.zeros_like(p)).detach() for k, v, p in zip(names, g, wrt)}
    if want_dx:
        grads['dx1'], grads['dx2'] = g[-2].detach(), g[-1].detach()
    return st, grads


def tversky_dlogits(logits, labels, alpha=0.1, beta=0.9):
    """The float64 gradient of oracle.tversky_loss(alpha, beta) at the given logits, as float32: the realistic, tiny dlogits."""
    lg = logits.detach().double().clone().requires_grad_(True)
    O.tversky_loss(lg, labels.long(), alpha, beta).backward()
    return lg.grad.float()


def state_from_workspace(eng, ws, P, x_d1, x_d2, logits, bn_mode='batch'):
    """The engine's stored forward state as CPU tensors (call after a training=True or frozen=True forward, synchronised): NCHW float64
    copies of ws.z[*], the tables ws.bn[*], x0 / f / pool / U where the setting stores them, the logits, the master parameters, the
    images, and precision / fusion / bn_mode."""
    nchw = lambda t: t.float().cpu().double().permute(0, 3, 1, 2).contiguous()
    st = dict(precision=eng.precision, fusion=eng.fusion, bn_mode=bn_mode,
              x_d1=x_d1.detach().cpu().double(), x_d2=x_d2.detach().cpu().double(), logits=logits.detach().cpu().double(),
              params={k: v.detach().cpu().clone() for k, v in P.items()},
              z={L.name: nchw(ws.z[L.name]) for L in eng.layers}, bn={L.name: ws.bn[L.name].cpu().double() for L in eng.layers})
    if not eng.x3:
        c = x_d1.shape[1]
        x0 = nchw(ws.x0)
        assert bool((x0[:, c:] == 0).all()), 'x0: the padding channels are not zero'
        st.update(x0=x0[:, :c].contiguous(), f={k: nchw(ws.f[k]) for k in range(1, 6)},
                  pool={k: nchw(ws.pool[k]) for k in range(2, 6)}, U={j: nchw(ws.U[j]) for j in range(1, 5)})
    return st


def state_from_oracle(sd, x_d1, x_d2, fusion='product', bn_mode='batch'):
    """The exact state (precision 'exact': q = identity): oracle.bidate_oracle's own float64 forward -- bidate_forward itself for
    'product', its encoder / up_stage / classifier around |x_d2 - x_d1| for 'absdiff' -- with every conv3x3 output recorded on the way
    (the oracle's leaf op is wrapped for the duration of the call), the tables from O.bn_batch_stats of those outputs (or the running
    buffers), and the oracle's logits.  The skips, pooled and upsampled maps are left to be derived, as in the bf16x3 setting."""
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    x1, x2 = x_d1.double(), x_d2.double()
    training = bn_mode == 'batch'
    rec, orig = [], O.conv3x3

    def recording(x, w, b=None):
        rec.append(orig(x, w, b).detach())
        return rec[-1]
    O.conv3x3 = recording
    try:
        with torch.no_grad():
            if fusion == 'product':
                logits, _ = O.bidate_forward(sd, x1, x2, training=training)
            else:
                s = O.State(sd)
                f1, f2 = O.encoder(s, x1, training), O.encoder(s, x2, training)
                fused = [fuse(a, b, fusion) for a, b in zip(f1, f2)]
                x = O.up_stage(s, 'up1', fused[4], fused[3], training)
                for j, k in ((2, 2), (3, 1), (4, 0)):
                    x = O.up_stage(s, f'up{j}', x, fused[k], training)
                logits = O.conv1x1(x, s.p('outc.conv.weight'), s.p('outc.conv.bias'))
    finally:
        O.conv3x3 = orig
    assert len(rec) == 28
    z, bn = {}, {}
    for i, L in enumerate(build_layers(x1.shape[1])):
        groups = [rec[i], rec[10 + i]] if L['enc'] else [rec[20 + i - 10]]
        z[L['name']] = torch.cat(groups)
        rows = []
        for zg in groups:
            if training:
                mean, var = O.bn_batch_stats(zg)
            else:
                mean, var = sd[f"{L['bn']}.running_mean"], sd[f"{L['bn']}.running_var"]
            inv = torch.rsqrt(var + BN_EPS)
            scale = sd[f"{L['bn']}.weight"] * inv
            rows.append(torch.stack([mean, inv, scale, sd[f"{L['bn']}.bias"] - mean * scale]))
        bn[L['name']] = torch.stack(rows)
    return dict(precision='exact', fusion=fusion, bn_mode=bn_mode, params=sd, x_d1=x1, x_d2=x2, z=z, bn=bn, logits=logits)


def compare(got, ref, zero_keys=(), residual=None):
    """{key: (relative L2, cosine, gain)} of got against ref, gain = <got, ref> / <ref, ref> (a coherent scale error moves it where
    incoherent rounding noise averages out); keys in zero_keys (conv biases in front of a batch-statistics BatchNorm, analytically
    zero) are reported as (|got|, |ref - residual|) instead, residual = forced_backward's (absent: 0)."""
    out = {}
    for k, r in ref.items():
        g, r = got[k].detach().double().cpu().reshape(-1), r.detach().double().reshape(-1)
        if k in zero_keys:
            out[k] = (float(g.norm()), float((r - residual[k].reshape(-1)).norm() if residual else r.norm()))
            continue
        out[k] = (float((g - r).norm() / r.norm()), float((g * r).sum() / (g.norm() * r.norm())), float((g * r).sum() / (r * r).sum()))
    return out


# ---------------------------------------------------------------- the bounds of the device audit (tests/test_gpu_forced.py), kept here so
# that the CPU sensitivity tests (tests/test_forced_ref_cpu.py) judge the SAME numbers.  Measured values: that file's docstring.
# conv stages: |z_engine - z_ref| <= u*|z_ref| + C_CONV*A, A = conv(|a|,|w|) + |b|: 4 x the largest c measured on the device per setting
C_CONV = {'fp32': 4 * 5.16e-7, 'bf16x3': 4 * 1.34e-6, 'bf16x3-fast': 4 * 1.34e-6, 'bf16': 4 * 4.08e-8}
C_CEILING = 9 * 16 * 2.0 ** -24          # K*2^-24 at the shortest reduction of the network (the first layer: 9 taps x 16 padded channels)
# gradients: per tensor relative L2, 1 - cosine and |gain - 1| of the engine against forced_backward: 2 x the largest measured per setting
# (box-to-box and summation-order spread)
GRAD_REL = {'fp32': 2 * 5.21e-6, 'bf16x3': 2 * 1.91e-5, 'bf16x3-fast': 2 * 9.24e-3, 'bf16': 2 * 1.32e-2}
GRAD_1MCOS = {'fp32': 2 * 1.36e-11, 'bf16x3': 2 * 1.81e-10, 'bf16x3-fast': 2 * 4.26e-5, 'bf16': 2 * 8.25e-5}
# |gain - 1|, gain = <engine, ref> / <ref, ref>: what a coherent scale error moves (rounding noise is incoherent and averages out of it)
GRAD_GAIN = {'fp32': 2 * 8.44e-7, 'bf16x3': 2 * 4.41e-6, 'bf16x3-fast': 2 * 5.01e-3, 'bf16': 2 * 4.40e-3}


def bn_fed_conv_biases(n_channels=3):
    """Conv biases in front of a BatchNorm: with batch statistics their gradient is analytically zero."""
    return [f"{L['conv']}.bias" for L in build_layers(n_channels)]
