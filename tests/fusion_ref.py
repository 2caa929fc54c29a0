"""Float64 reference of BiDateNet under a date fusion, and restatements of the three training fusion kernels' contracts.

The network reference is NOT a second model: it recomposes oracle.bidate_oracle's own `encoder`, `up_stage` and `conv1x1` (imported, unchanged)
around the one line of `bidate_forward` that fuses the dates (models/bidate_model.py:35-38), so that with 'product' it must equal
`bidate_forward` bit for bit (tests/test_fusion_cpu.py pins that before the 'absdiff' reference is trusted).

The kernel contracts work on GIVEN rounded activations a = [a_d1 ; a_d2] (NCHW, 2B images, date 1 first) -- what tests/gpu_util.bnrelu_ref
forms exactly as the kernels do -- so a comparison with a kernel sees the fusion arithmetic alone.
"""
import torch

from oracle import bidate_oracle as O

FUSIONS = ('product', 'absdiff')


def fuse(a1, a2, fusion):
    """The date fusion of two feature maps: 'product' is the reference's torch.relu(x_d2 * x_d1), 'absdiff' is |x_d2 - x_d1|."""
    if fusion == 'product':
        return torch.relu(a2 * a1)
    if fusion == 'absdiff':
        return (a2 - a1).abs()
    raise ValueError(fusion)


# ---------------------------------------------------------------- the network
def forward(sd, x_d1, x_d2, fusion, training=True, return_skips=False):
    """oracle.bidate_forward with the fusion as an argument: (logits, new_buffers[, skips])."""
    st = O.State(sd)
    f1 = O.encoder(st, x_d1, training)
    f2 = O.encoder(st, x_d2, training)
    fused = [fuse(a, b, fusion) for a, b in zip(f1, f2)]
    x = O.up_stage(st, 'up1', fused[4], fused[3], training)
    x = O.up_stage(st, 'up2', x, fused[2], training)
    x = O.up_stage(st, 'up3', x, fused[1], training)
    x = O.up_stage(st, 'up4', x, fused[0], training)
    logits = O.conv1x1(x, st.p('outc.conv.weight'), st.p('outc.conv.bias'))
    return (logits, st.new_buffers, fused) if return_skips else (logits, st.new_buffers)


def to_f64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def step(sd, x_d1, x_d2, labels, fusion, training=True, lr=None, alpha=0.1, beta=0.9, input_grads=False):
    """Forward + Tversky loss + autograd in float64 on a copy of `sd` (float tensors are promoted): dict(logits, loss, grads{name},
    new_buffers, and with lr the state after one plain SGD step as new_sd, and with input_grads dx1 / dx2).  training=False is the
    frozen-BatchNorm graph: running statistics as constants."""
    sd = to_f64(sd)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running_' not in k}
    full = dict(sd)
    full.update(params)
    x1, x2 = x_d1.double(), x_d2.double()
    if input_grads:
        x1, x2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    logits, new_buf = forward(full, x1, x2, fusion, training)
    loss = O.tversky_loss(logits, labels.long(), alpha, beta)
    names = list(params)
    wrt = [params[k] for k in names] + ([x1, x2] if input_grads else [])
    g = torch.autograd.grad(loss, wrt)
    out = dict(logits=logits.detach(), loss=loss.detach(), grads={k: v.detach() for k, v in zip(names, g)},
               new_buffers={k: v.detach() for k, v in new_buf.items()})
    if input_grads:
        out['dx1'], out['dx2'] = g[-2].detach(), g[-1].detach()
    if lr is not None:
        new_sd = {k: v.clone() for k, v in sd.items()}
        for k in names:
            new_sd[k] = sd[k] - lr * out['grads'][k]
        new_sd.update(out['new_buffers'])
        out['new_sd'] = new_sd
    return out


# ---------------------------------------------------------------- the kernels' contracts, on given rounded activations
def fuse_ref(a, B, fusion):
    """bdn_fuse_dates: f [B,C,H,W] of a [2B,C,H,W] in float64 (the caller rounds to the storage type, or splits)."""
    a = a.double()
    return fuse(a[:B], a[B:], fusion)


def fuse_pool_ref(a, B, fusion):
    """bdn_fuse_dates_pool: (f, MaxPool2d(2) of both dates, floor mode)."""
    return fuse_ref(a, B, fusion), O.maxpool2(a.double())


def split_hi_lo(t):
    """bdn_split_pack's [hi | lo] split of float32 values: hi = bf16(x), lo = bf16(x - hi); both returned as float32."""
    t = t.float()
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def enc_skip_bwd_ref(a, dF, dP, B, fusion):
    """bdn_enc_skip_bwd_fusion WITHOUT bs_partial, in float64: dA [2B,C,H,W] = fusion part + unpooled dP (first maximum of a window wins),
    returned as (fusion part, pool part).  The fusion part is the kernel's contract, not autograd of relu(a2 * a1): the product hands
    dF * a_other to a dead ReLU too (the producer's own mask follows); absdiff is dF * sign(a1 - a2) and its exact negation, 0 at a tie."""
    a, dF = a.double(), dF.double()
    a1, a2 = a[:B], a[B:]
    if fusion == 'product':
        part = torch.cat([dF * a2, dF * a1])
    else:
        s = torch.sign(a1 - a2)
        part = torch.cat([dF * s, -(dF * s)])
    pool = torch.zeros_like(a)
    if dP is not None:
        ar = a.clone().requires_grad_(True)
        (O.maxpool2(ar) * dP.double()).sum().backward()
        pool = ar.grad
    return part, pool
