"""-m "not gpu": the forced reference (tests/forced_ref.py) is right before it judges the engine.

1. At an EXACT state -- oracle.bidate_oracle's own float64 forward, q = identity -- forced_backward equals torch.autograd.grad of the oracle
   to 1e-10 relative L2 per tensor and audit_forward reports deviations <= 1e-12 of scale: both fusions, both bn_modes, a ragged size
   (2 x 3 x 36 x 44: maps 18x22, 9x11, 4x5, 2x2).
2. A CPU emulation of the bf16 and bf16x3 engines (the same graph free-running in float32, q at the rounding points, straight-through
   gradients, stored gradients rounded to the storage type) supplies a state and "engine" gradients: the forced-vs-emulated distance per
   tensor is the CPU estimate of the backward-rounding floor, printed, and held under the device bound (an input on which the EMULATION
   already exceeds the bound would be too ill-conditioned to audit the device with).
3. Sensitivity: four wiring mutations of the emulated bf16 engine must push the comparison over the bound tests/test_gpu_forced.py uses
   (forced_ref.GRAD_REL / GRAD_1MCOS / GRAD_GAIN): a weight gradient scaled by 1.02, a BatchNorm dgamma finalized over both statistic
   groups together, an unpool routed to the last maximum, a `cat` half zeroed in a decoder weight gradient.

Figures on these inputs (2 x 3 x 36 x 44), emulated engine against the forced reference, worst tensor: relative L2 1.1e-6 (fp32, bf16x3),
9.7e-3 (bf16; the device gives 9.6e-3 ... 1.3e-2); 1 - cosine 6e-13 / 4.6e-5; |gain - 1| 9e-7 / 1.7e-3.  Mutations in bf16 (relative L2,
1 - cosine, |gain - 1|): 1.02 scaling 2.0e-2 ... 2.2e-2, <= 4e-5, 2.0e-2 on every layer -- under the relative-L2 bound (2.64e-2) and the
cosine's, rejected by |gain - 1| (8.8e-3); dgamma at e1a / e3a / e5b 0.62 / 5.9e-2 / 0.20; unpool-last at levels 1 / 2 7.4e-2 / 6.8e-2 on
the level's second conv weight; a dropped `cat` half 0.82 / 0.58.
"""
import functools

import pytest
import torch

from oracle import filler
from tests import forced_ref as R
from tests import fusion_ref as FR

C, SHAPE = 3, (2, 36, 44)


@functools.lru_cache(maxsize=None)
def _sd(c=C):
    """The filler's state dict without building a model: shapes from the layer table."""
    sd = {}
    for L in R.build_layers(c):
        sd[f"{L['conv']}.weight"] = torch.empty(L['cout'], L['cin'], 3, 3)
        sd[f"{L['conv']}.bias"] = torch.empty(L['cout'])
        for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
            sd[f"{L['bn']}.{leaf}"] = torch.empty(L['cout'])
        sd[f"{L['bn']}.num_batches_tracked"] = torch.empty((), dtype=torch.int64)
    sd['outc.conv.weight'], sd['outc.conv.bias'] = torch.empty(2, 64, 1, 1), torch.empty(2)
    return {k: torch.from_numpy(filler.fill_tensor(k, v)).to(v.dtype) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _inputs(shape=SHAPE, c=C):
    b, h, w = shape
    x1, x2, lbl = filler.make_inputs(b, c, h, seed=0, different_dates=True, size_w=w)
    return torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(lbl)


def _oracle_grads(sd, x1, x2, fusion, training, dlogits):
    """Plain autograd of the oracle (tests/fusion_ref.forward: bidate_forward with the fusion as an argument) in float64."""
    sd = FR.to_f64(sd)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running_' not in k}
    full = dict(sd)
    full.update(params)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    logits, _ = FR.forward(full, a, b, fusion, training)
    names = list(params)
    g = torch.autograd.grad(logits, [params[k] for k in names] + [a, b], dlogits)
    return dict(zip(names, g[:-2]), dx1=g[-2], dx2=g[-1]), logits.detach()


@pytest.mark.parametrize('bn_mode', ['batch', 'running'])
@pytest.mark.parametrize('fusion', ['product', 'absdiff'])
def test_forced_equals_plain_autograd_at_an_exact_state(fusion, bn_mode):
    x1, x2, _ = _inputs()
    st = R.state_from_oracle(_sd(), x1, x2, fusion, bn_mode)
    dl = torch.randn(st['logits'].shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref, logits = _oracle_grads(_sd(), x1, x2, fusion, bn_mode == 'batch', dl)
    assert torch.equal(logits, st['logits'])
    audit = {}
    got = R.forced_backward(st, dl, True, audit=audit)
    assert len(got) == 76 and set(got) == set(ref)
    zero = R.bn_fed_conv_biases(C) if bn_mode == 'batch' else ()
    for k, v in R.compare(got, ref, zero).items():
        if k in zero:
            assert max(v) < 1e-9 * float(dl.norm()), (k, v)
        else:
            assert v[0] <= 1e-10, (k, v)
    assert len([s for s in audit if s.startswith('z[')]) == 18 and len([s for s in audit if s.startswith('bn[')]) == 18 and 'logits' in audit
    for stage, a in audit.items():
        assert a['dev'] <= 1e-12 * max(a['scale'], 1.0), (stage, a)


def test_audit_lists_every_stage_and_the_pool_rule_matches_the_oracle():
    """The emulated fp32 engine stores every stage: 1 + 18 + 18 + 5 + 4 + 4 + 1 audited entries; maxpool_first has O.maxpool2's values and
    routes a tied window's gradient to its first (last=True: last) maximum."""
    from oracle import bidate_oracle as O
    x1, x2, _ = _inputs()
    st, _ = R.emulate(_sd(), x1, x2, 'fp32')
    audit = R.audit_forward(st, c_conv=R.C_CEILING)
    kinds = [a['kind'] for a in audit.values()]
    assert len(audit) == 51 and kinds.count('conv') == 18 and kinds.count('table') == 18 and kinds.count('pool') == 4
    assert kinds.count('upsample') == 4 and kinds.count('elementwise') == 6 and kinds.count('classifier') == 1
    a = torch.tensor([[1., 3., 3., 0.], [3., 2., 0., 0.]]).reshape(1, 1, 2, 4).requires_grad_(True)
    for last, want in ((False, [[0., 1., 1., 0.], [0., 0., 0., 0.]]), (True, [[0., 0., 1., 0.], [1., 0., 0., 0.]])):
        p = R.maxpool_first(a, last=last)
        assert torch.equal(p.detach(), O.maxpool2(a.detach()))
        g, = torch.autograd.grad(p.sum(), a)
        assert g.reshape(2, 4).tolist() == want


@functools.lru_cache(maxsize=None)
def _emulated(prec, mutate=None):
    x1, x2, lbl = _inputs()
    st, g = R.emulate(_sd(), x1, x2, prec, dlogits_fn=lambda lg: R.tversky_dlogits(lg, lbl), mutate=dict(mutate) if mutate else None)
    return st, g


@functools.lru_cache(maxsize=None)
def _forced(prec):
    st, _ = _emulated(prec)
    _, _, lbl = _inputs()
    return R.forced_backward(st, R.tversky_dlogits(st['logits'], lbl), True)


def _worst(got, ref):
    cmp = R.compare(got, ref, R.bn_fed_conv_biases(C))
    live = {k: v for k, v in cmp.items() if k not in R.bn_fed_conv_biases(C)}
    rel = max((v[0], k) for k, v in live.items())
    cos = max((1 - v[1], k) for k, v in live.items())
    gain = max((abs(v[2] - 1), k) for k, v in live.items())
    return rel, cos, gain


@pytest.mark.parametrize('prec', ['fp32', 'bf16x3', 'bf16'])
def test_emulated_engine_noise_floor_is_under_the_device_bound(prec):
    st, g = _emulated(prec)
    audit = R.audit_forward(st, c_conv=R.C_CEILING)
    c = max(a['c'] for a in audit.values() if a['kind'] == 'conv')
    ratio = max((a['ratio'], s) for s, a in audit.items() if a['kind'] != 'conv')
    rel, cos, gain = _worst(g, _forced(prec))
    print(f'\n[{prec}] emulated engine: c {c:.3e}; worst non-conv stage {ratio}; gradient relative L2 {rel}, 1 - cosine {cos}, |gain - 1| {gain}')
    assert c <= R.C_CEILING and ratio[0] <= 1.0, (c, ratio)
    assert rel[0] <= R.GRAD_REL[prec] and cos[0] <= R.GRAD_1MCOS[prec] and gain[0] <= R.GRAD_GAIN[prec], (rel, cos, gain)


def _rejected(got, ref, keys):
    """Does the device test's bf16 bound reject `got` on one of `keys`?  Prints the figures."""
    cmp = R.compare(got, ref, R.bn_fed_conv_biases(C))
    fig = {k: (cmp[k][0], 1 - cmp[k][1], abs(cmp[k][2] - 1)) for k in keys}
    print('   ', {k: tuple('%.3e' % x for x in v) for k, v in fig.items()})
    return any(v[0] > R.GRAD_REL['bf16'] or v[1] > R.GRAD_1MCOS['bf16'] or v[2] > R.GRAD_GAIN['bf16'] for v in fig.values())


def test_bound_rejects_a_weight_gradient_scaled_by_1_02():
    """EVERY layer's weight gradient, one at a time."""
    _, g = _emulated('bf16')
    for L in R.build_layers(C):
        k = f"{L['conv']}.weight"
        assert _rejected(dict(g, **{k: 1.02 * g[k]}), _forced('bf16'), [k]), k


def test_bound_rejects_a_dgamma_finalized_over_both_groups():
    """Group 1's dgamma finalized with group 0's mean and invstd, at layers whose two tables differ (e1a: the dates' own statistics; e3a, e5b:
    gaps of 4 % and 20 % of a standard deviation).  At e1b and e2b the two groups' tables coincide to 1 % on these inputs and the mutation
    moves dgamma by 1.3e-2 / 2.2e-2, the rounding floor itself: no gradient bound can see it there."""
    for name in ('e1a', 'e3a', 'e5b'):
        L = {l['name']: l for l in R.build_layers(C)}[name]
        _, g = _emulated('bf16', (('dgamma_joint', name),))
        assert _rejected(g, _forced('bf16'), [f"{L['bn']}.weight"]), name


def test_bound_rejects_an_unpool_to_the_last_maximum():
    for k in (1, 2):
        _, g = _emulated('bf16', (('unpool_last', k),))
        L = {l['name']: l for l in R.build_layers(C)}[f'e{k}b']
        assert _rejected(g, _forced('bf16'), [f"{L['conv']}.weight", f"{L['bn']}.weight", f"{L['bn']}.bias"]), k


def test_bound_rejects_a_cat_half_dropped_from_a_weight_gradient():
    _, g = _emulated('bf16')
    for j, half in ((2, 0), (4, 1)):
        L = {l['name']: l for l in R.build_layers(C)}[f'd{j}a']
        k, ck = f"{L['conv']}.weight", R.ENC_CH[4 - j]
        w = g[k].clone()
        if half == 0:
            w[:, :ck] = 0
        else:
            w[:, ck:] = 0
        assert _rejected(dict(g, **{k: w}), _forced('bf16'), [k]), (j, half)


def test_bounds_meet_the_conditions():
    """The device bounds sit under the forward-divergence allowances they replace, and c under its derivable ceiling."""
    assert R.GRAD_REL['bf16'] < 0.8 and R.GRAD_REL['fp32'] < 2e-2 and R.GRAD_REL['bf16x3'] < 6e-2 and R.GRAD_REL['bf16x3-fast'] < 6e-2
    assert all(0 < c <= R.C_CEILING for c in R.C_CONV.values())
