"""float64 restatement of the layer-wise adaptive rules (include/bidate_hip.h: bdn_lamb_step, bdn_lars_step), in the style of
tests/optim_ref.py: shared by tests/test_layerwise_cpu.py (which pins it against CPU torch.optim with every ratio forced to 1, and on
hand examples) and the GPU tests (which hold the HIP kernels to it).

Both rules work on LISTS with one entry per tensor: parameters, gradients, state, and the tensor's own lr / weight_decay (its group's).
They return the new parameters and state, the two norms and the ratio of every tensor, and a magnitude per output: the same expression
on the absolute values of its inputs, every subtraction an addition (tests/optim_ref.py).  `ratios`: None (the rule's own), or a list that
replaces them -- all ones (the torch.optim pins), or what a kernel reported in trust_out (the element check).  `frozen`: indices that are
skipped: their outputs are their inputs, their norms and ratio 0.

Roundings, counted from fabric_amd/csrc/optim.hip with every float32 hyperparameter (float(lr), float(1 - beta1), float(bc1), ...)
counted as one rounding of its own:

  LAMB  g = s*grad (1; one more when s is the product grad_scale * *dev_scale).  m = m + w1*(g - m): g, w1, the difference, the product,
        the sum: 5.  v = beta2*v + c2*g*g: g twice (its error doubles in g*g), c2, beta2, three products, one sum: 8.  den = sqrt(v)/
        sqrt(bc2) + eps: half of v's 8, the sqrt, float(sqrt(bc2)), the division, float(eps), the sum: 9.  r = (m / bc1) / den: m's 5,
        float(bc1), two divisions, den's 9: 17.  u = fma(wd, p, r): float(wd) and one rounding: 19 -> ULPS_U = 20.
        p - (lr*ratio)*u: float(lr), two products, the difference on top of u's: 23 -> ULPS_P = 24.  The ratio is the kernel's own
        float32 and enters exactly.  The moments are Adam's statements: optim_ref.ULPS.
  LARS  the summed value is float32(s*grad): ULPS_G = 2 (s as above).  d = local*(g + wd*p): g's 2, float(wd), a product, a sum, the
        product with the reported ratio: 6.  buf = momentum*buf + (1 - dampening)*d: two hyperparameters, two products, a sum: 11 with
        d's.  Nesterov d + momentum*buf: a product and a sum more, 13 and d's 6 beside buf's: below 16.  p - lr*(...): float(lr), a
        product, a difference: below 20 -> ULPS_LARS = 20 for the parameters, 12 for the buffer.

Norms: ||p_t|| is formed in double from the float32 parameters and rounded once: within EPS32 * ||p_t|| of the float64 norm.  The second
norm is of float32 values each within ULPS * EPS32 * mag of the twin's, so by the triangle inequality it lies within ULPS * EPS32 *
||mag||_2 of the twin's norm, plus the one rounding to float32.
"""
import math

import torch

from tests.optim_ref import EPS32, ULPS

ULPS_U, ULPS_P = 20, 24
ULPS_G, ULPS_LARS, ULPS_BUF = 2, 20, 12


def _ratio(wn, xn, formula, max_trust, adapt):
    r = formula(wn, xn) if wn > 0 and xn > 0 else 1.0
    if max_trust and max_trust > 0:
        r = min(r, max_trust)
    return r if adapt else 1.0


def lamb_ratio(wn, un, max_trust=0.0, adapt=True):
    """The LAMB trust ratio of one tensor from its two norms."""
    return _ratio(wn, un, lambda a, b: a / b, max_trust, adapt)


def lars_ratio(wn, gn, trust_coef, wd, lars_eps, max_trust=0.0, adapt=True):
    """The LARS local rate of one tensor from its two norms."""
    return _ratio(wn, gn, lambda a, b: trust_coef * a / (b + wd * a + lars_eps), max_trust, adapt)


def lamb(ps, gs, ms, vs, step, lrs, wds, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, max_trust=0.0, adapt=None, ratios=None, frozen=()):
    """-> dict of lists, one entry per tensor: p, m, v (new values), u, wn, xn (= ||u||), ratio, p_mag, m_mag, v_mag, u_mag.
    step is 1-based (after the increment); lrs / wds: per tensor."""
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    out = {k: [] for k in ('p', 'm', 'v', 'u', 'wn', 'xn', 'ratio', 'p_mag', 'm_mag', 'v_mag', 'u_mag')}
    for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs)):
        p, m, v = p.double(), m.double(), v.double()
        if i in frozen:
            for k, val in (('p', p), ('m', m), ('v', v), ('u', torch.zeros_like(p)), ('wn', 0.0), ('xn', 0.0), ('ratio', 0.0),
                           ('p_mag', p.abs()), ('m_mag', m.abs()), ('v_mag', v.abs()), ('u_mag', torch.zeros_like(p))):
                out[k].append(val)
            continue
        g = g.double() * grad_scale
        m_new = m + (1 - b1) * (g - m)
        mm = b1 * m.abs() + (1 - b1) * g.abs()
        v_new = b2 * v + (1 - b2) * g * g
        vm = b2 * v.abs() + (1 - b2) * g * g
        den = v_new.sqrt() / math.sqrt(bc2) + eps
        u = (m_new / bc1) / den + wds[i] * p
        um = (mm / bc1) / den + wds[i] * p.abs()
        wn, un = float(p.norm()), float(u.norm())
        r = lamb_ratio(wn, un, max_trust, True if adapt is None else adapt[i]) if ratios is None else float(ratios[i])
        for k, val in (('p', p - lrs[i] * r * u), ('m', m_new), ('v', v_new), ('u', u), ('wn', wn), ('xn', un), ('ratio', r),
                       ('p_mag', p.abs() + lrs[i] * r * um), ('m_mag', mm), ('v_mag', vm), ('u_mag', um)):
            out[k].append(val)
    return out


def lars(ps, gs, bufs, lrs, wds, grad_scale=1.0, momentum=0.0, dampening=0.0, nesterov=False, first=True, trust_coef=1e-3, lars_eps=1e-8,
         max_trust=0.0, adapt=None, ratios=None, frozen=()):
    """-> dict of lists, one entry per tensor: p, buf (None without momentum), g (the scaled gradient), wn, xn (= ||g||), ratio, p_mag,
    buf_mag, g_mag.  bufs: a list (entries may be None when momentum == 0 or on the first step)."""
    out = {k: [] for k in ('p', 'buf', 'g', 'wn', 'xn', 'ratio', 'p_mag', 'buf_mag', 'g_mag')}
    for i, (p, g) in enumerate(zip(ps, gs)):
        p = p.double()
        buf = None if bufs is None or bufs[i] is None else bufs[i].double()
        if i in frozen:
            for k, val in (('p', p), ('buf', buf), ('g', torch.zeros_like(p)), ('wn', 0.0), ('xn', 0.0), ('ratio', 0.0), ('p_mag', p.abs()),
                           ('buf_mag', None if buf is None else buf.abs()), ('g_mag', torch.zeros_like(p))):
                out[k].append(val)
            continue
        g = g.double() * grad_scale
        wn, gn = float(p.norm()), float(g.norm())
        r = lars_ratio(wn, gn, trust_coef, wds[i], lars_eps, max_trust, True if adapt is None else adapt[i]) if ratios is None \
            else float(ratios[i])
        d, dm = r * (g + wds[i] * p), r * (g.abs() + wds[i] * p.abs())
        bm = None
        if momentum:
            if first:
                buf, bm = d.clone(), dm.clone()
            else:
                buf, bm = momentum * buf + (1 - dampening) * d, momentum * buf.abs() + (1 - dampening) * dm
            if nesterov:
                d, dm = d + momentum * buf, dm + momentum * bm
            else:
                d, dm = buf, bm
        else:
            buf = None
        for k, val in (('p', p - lrs[i] * d), ('buf', buf), ('g', g), ('wn', wn), ('xn', gn), ('ratio', r), ('p_mag', p.abs() + lrs[i] * dm),
                       ('buf_mag', bm), ('g_mag', g.abs())):
            out[k].append(val)
    return out


def check_norms(got, wn_ref, xn_ref, x_mag, ulps, what):
    """One tensor's reported norms (float32) against the twin's: ||p|| within one float32 rounding, the second norm within
    ulps * EPS32 * ||x_mag||_2 (triangle inequality) plus one float32 rounding."""
    wn, xn = float(got[0]), float(got[1])
    assert abs(wn - wn_ref) <= EPS32 * wn_ref + 1e-38, f'{what}: ||p|| = {wn!r}, float64 {wn_ref!r}'
    bound = ulps * EPS32 * float(x_mag.double().norm()) + EPS32 * xn_ref + 1e-38
    assert abs(xn - xn_ref) <= bound, f'{what}: second norm {xn!r}, float64 {xn_ref!r}, error / bound {abs(xn - xn_ref) / bound:.2f}'


def expected_ratio(kind, hyper, wn, xn, wd, adapt):
    """The rule's ratio from two norms (the twin's branches: zero norms, the clamp, the adapt flag)."""
    if kind == 'lamb':
        return lamb_ratio(wn, xn, hyper.get('max_trust', 0.0), adapt)
    return lars_ratio(wn, xn, hyper.get('trust_coef', 1e-3), wd, hyper.get('lars_eps', 1e-8), hyper.get('max_trust', 0.0), adapt)


def check_update(kind, hyper, it, ps, gs, state_in, p_out, state_out, trust, lrs, wds, adapt, frozen=(), what='update', zero=None):
    """One update of a kernel against the twin, from the kernel's own float32 inputs.  Everything is a per-tensor list (CPU): ps / gs the
    parameters and RAW gradients before the update, state_in / state_out dicts of lists ('m', 'v' for lamb; 'buf' for lars with
    momentum), trust the [n_tensors, 3] tensor the kernel wrote, lrs / wds / adapt per tensor.  hyper: grad_scale, betas, eps, max_trust,
    momentum, dampening, nesterov, trust_coef, lars_eps.  it: the 0-based update index (LAMB's step is it + 1, LARS's first step is
    it == 0).  zero: the index of a tensor known to be all zero (only checked at it == 0).

    Three parts: the reported norms against the twin's own (check_norms); the reported ratio against the rule's formula on the reported
    norms, each of which lies within half an epsilon of the double the kernel used, as do float(trust_coef), float(wd) and float(lars_eps)
    and the final rounding: below 6 epsilons; and, with the reported ratio, every element (optim_ref.check).  A frozen tensor keeps its
    bits and reports {0, 0, 0}."""
    from tests.optim_ref import check
    n_t = len(ps)
    trust = trust.detach().cpu()
    reported = trust[:, 2].double().tolist()
    lamb_rule = kind == 'lamb'
    bits = lambda t: t.detach().contiguous().view(torch.int32)
    if lamb_rule:
        kw = dict(step=it + 1, lrs=lrs, wds=wds, grad_scale=hyper.get('grad_scale', 1.0), betas=hyper.get('betas', (0.9, 0.999)),
                  eps=hyper.get('eps', 1e-8), max_trust=hyper.get('max_trust', 0.0), adapt=adapt, frozen=frozen)
        args = (ps, gs, state_in['m'], state_in['v'])
        own, ref = lamb(*args, **kw), lamb(*args, ratios=reported, **kw)
        x_mag, ulps_x = own['u_mag'], ULPS_U
    else:
        bufs = state_in['buf'] if 'buf' in state_in and it > 0 else None
        kw = dict(lrs=lrs, wds=wds, grad_scale=hyper.get('grad_scale', 1.0), momentum=hyper.get('momentum', 0.0),
                  dampening=hyper.get('dampening', 0.0), nesterov=hyper.get('nesterov', False), first=it == 0,
                  trust_coef=hyper.get('trust_coef', 1e-3), lars_eps=hyper.get('lars_eps', 1e-8), max_trust=hyper.get('max_trust', 0.0),
                  adapt=adapt, frozen=frozen)
        own, ref = lars(ps, gs, bufs, **kw), lars(ps, gs, bufs, ratios=reported, **kw)
        x_mag, ulps_x = own['g_mag'], ULPS_G
    for i in range(n_t):
        w = f'{what} update {it} tensor {i} (n={ps[i].numel()})'
        if i in frozen:
            assert trust[i].tolist() == [0.0, 0.0, 0.0], f'{w}: frozen, trust_out {trust[i].tolist()}'
            assert torch.equal(bits(p_out[i]), bits(ps[i])), f'{w}: a frozen parameter changed'
            assert all(torch.equal(bits(state_out[k][i]), bits(state_in[k][i])) for k in state_out), f'{w}: frozen state changed'
            continue
        check_norms(trust[i], own['wn'][i], own['xn'][i], x_mag[i], ulps_x, w)
        want = expected_ratio(kind, hyper, float(trust[i, 0]), float(trust[i, 1]), wds[i], bool(adapt[i]))
        assert abs(reported[i] - want) <= 6 * EPS32 * want, f'{w}: ratio {reported[i]!r}, formula on the reported norms {want!r}'
        if zero == i and it == 0:                            # (the first update moves it off zero)
            mt = hyper.get('max_trust', 0.0)
            one = 1.0 if not adapt[i] or not mt else float(torch.tensor(min(1.0, mt), dtype=torch.float32))
            assert reported[i] == one and float(trust[i, 0]) == 0.0, f'{w}: an all-zero tensor takes ratio 1 (then the clamp)'
        if not adapt[i]:
            assert reported[i] == 1.0, f'{w}: adapt = 0 takes ratio 1'
        check(p_out[i], ref['p'][i], ref['p_mag'][i], w + ' params', ulps=ULPS_P if lamb_rule else ULPS_LARS)
        if lamb_rule:
            check(state_out['m'][i], ref['m'][i], ref['m_mag'][i], w + ' exp_avg')
            check(state_out['v'][i], ref['v'][i], ref['v_mag'][i], w + ' exp_avg_sq')
        elif 'buf' in state_out:
            check(state_out['buf'][i], ref['buf'][i], ref['buf_mag'][i], w + ' momentum_buffer', ulps=ULPS_BUF)
