"""-m gpu: the layer-wise adaptive update kernels (include/bidate_hip.h: bdn_lamb_step, bdn_lars_step) on guard-banded buffers.

Every step is checked from the kernel's own float32 inputs against the float64 twin (tests/layerwise_ref.py, pinned in
tests/test_layerwise_cpu.py), in two parts so that every bound is derived and none is measured: the norms the kernel reports against the
twin's (one rounding for ||p||, the triangle inequality for the second norm), the ratio against the rule's formula on the reported norms,
and -- with the ratio the kernel reported -- every parameter and state element against the float64 evaluation.  The rounding counts are
those of the twin's docstring.  Then the bit-level properties: frozen tensors and guards, NaN pads, poisoned workspace, repeats,
dev_scale = 1, LAMB without adaptation against AdamW's kernel, and one schedule-stress case."""
import pytest
import torch

from fabric_amd import _lib
from tests import guard
from tests import layerwise_ref as L
from tests import optim_ref as R
from tests import sched_stress as ss
from tests.guard import guarded

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)
EPS = R.EPS32

_B = [2, 64, 3, 16384, 16388, 100003, 5]
_LAYOUTS = {
    'one_1': dict(sizes=[1]), 'one_3': dict(sizes=[3]), 'one_4': dict(sizes=[4]), 'one_1023': dict(sizes=[1023]),
    # many tensors in one block, one exactly a partial chunk long, one a vector past it, one over several blocks; pads of 2, 1 and 3 floats
    'mixed': dict(sizes=_B, zero=2),
    # the same around the partial pass's own chunk of 1024 vectors: exactly one chunk, a vector past it, chunks that start inside a tensor
    'chunk_edges': dict(sizes=[4096, 4100, 12, 4092, 8192, 3], zero=2),
    'many_small': dict(sizes=[4 + (7 * i) % 9 for i in range(256)], zero=5),
    'frozen_groups': dict(sizes=_B, zero=2, groups=[0, -1, 1, 0, -1, 1, 0], adapt=[1, 1, 1, 0, 1, 1, 0], lrs=[0.01, 0.03], wds=[0.01, 0.0]),
    # 4096 + 1024 + 256 + 5 vectors, five tensors (three pad entries in the staged table): a 16-vector one, one that ends 3 vectors into
    # a block of 256, a frozen one, and the last end 5 vectors short of n / 4 -- those hold NaN and are neither read nor written
    'short_table': dict(sizes=[61, 4042, 7997, 1199, 8195], groups=[0, 1, -1, 0, 1], lrs=[0.01, 0.03], wds=[0.01, 0.0], slack=20),
}
_RULES = {
    'lamb': dict(kind='lamb', wd=0.01),
    'lamb_clamp': dict(kind='lamb', wd=0.0, max_trust=0.5, betas=(0.8, 0.99), gs=0.5),
    'lars_nesterov': dict(kind='lars', wd=0.01, momentum=0.9, nesterov=True, trust_coef=0.02),
    'lars_damp_clamp': dict(kind='lars', wd=0.0, momentum=0.8, dampening=0.1, trust_coef=0.5, max_trust=0.2, gs=0.5),
    'lars_plain': dict(kind='lars', wd=0.01, trust_coef=0.02),
}


class Lay:
    """A flat layout of `sizes` (every tensor padded to a float4) and its per-tensor table."""

    def __init__(self, sizes, zero=None, groups=None, adapt=None, lrs=None, wds=None, slack=0):
        self.sizes, self.zero, self.slack = list(sizes), zero, slack       # slack: floats (whole vectors) behind the table's last end
        self.offs, off = [], 0
        for s in self.sizes:
            self.offs.append(off)
            off += (s + 3) // 4 * 4
        self.n, self.nt = off + slack, len(self.sizes)
        self.ends = [(o + (s + 3) // 4 * 4) // 4 for o, s in zip(self.offs, self.sizes)]
        self.groups = list(groups) if groups is not None else [0] * self.nt
        self.adapt = list(adapt) if adapt is not None else [1] * self.nt
        self.lrs, self.wds = lrs, wds
        self.frozen = {i for i, g in enumerate(self.groups) if g < 0}
        real = torch.zeros(self.n, dtype=torch.bool)
        for o, s in zip(self.offs, self.sizes):
            real[o:o + s] = True
        self.real = real

    def split(self, flat):
        flat = flat.detach().cpu()
        return [flat[o:o + s] for o, s in zip(self.offs, self.sizes)]

    def table(self):
        as32 = lambda v: guard.guard(torch.tensor(v, dtype=torch.int64).to(torch.int32), dev)
        return as32(self.ends), as32(self.sizes), as32(self.groups), as32(self.adapt)

    def inputs(self, seed, steps=3, pad=0.0):
        """(p, [grads]) on the CPU: some parameters scaled by 1e-3, tensor `zero` all zero, some zero gradients; pads hold `pad`."""
        gen = torch.Generator(device='cpu').manual_seed(seed)
        p = torch.randn(self.n, generator=gen)
        p[::7] *= 1e-3
        if self.zero is not None:
            o, s = self.offs[self.zero], self.sizes[self.zero]
            p[o:o + s] = 0.0
        grads = [torch.randn(self.n, generator=gen) * (0.3 + it) for it in range(steps)]
        if steps > 1:
            grads[1][::5] = 0.0
        for t in [p] + grads:
            t[~self.real] = pad
            t[self.n - self.slack:] = float('nan')            # behind the table: a read poisons a norm
        return p, grads


def _bits(t):
    return t.detach().view(torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hyper(rule, lay):
    lrs = lay.lrs or [0.01]
    wds = lay.wds if lay.wds is not None else [rule['wd']]
    return lrs, wds


def _call(rule, lay, tab, p, g, state, it, ws, trust, ds=None):
    lrs, wds = _hyper(rule, lay)
    st = _lib.stream_ptr()
    table = tuple(t.data_ptr() for t in tab) + (lay.nt, len(lrs))
    gs = rule.get('gs', 1.0)
    if rule['kind'] == 'lamb':
        b1, b2 = rule.get('betas', (0.9, 0.999))
        _lib.call('bdn_lamb_step', p.data_ptr(), g.data_ptr(), state['m'].data_ptr(), state['v'].data_ptr(), *table, _lib.floats(lrs),
                  _lib.floats(wds), gs, _lib.ptr(ds), b1, b2, 1e-8, rule.get('max_trust', 0.0), it + 1, ws.data_ptr(), trust.data_ptr(),
                  lay.n, st)
    else:
        _lib.call('bdn_lars_step', p.data_ptr(), g.data_ptr(), _lib.ptr(state.get('buf')), *table, _lib.floats(lrs), _lib.floats(wds), gs,
                  _lib.ptr(ds), rule.get('momentum', 0.0), rule.get('dampening', 0.0), int(rule.get('nesterov', False)), int(it == 0),
                  rule.get('trust_coef', 1e-3), 1e-8, rule.get('max_trust', 0.0), ws.data_ptr(), trust.data_ptr(), lay.n, st)


def _run(rule, lay, p0, grads, pad=0.0, ws_zero=False, ds=None):
    """len(grads) steps on fresh guarded buffers -> [(p_in, state_in, p_out, state_out, trust)] (clones), one per step."""
    tab = lay.table()
    p = guard.guard(p0, dev)
    gbufs = [guard.guard(g, dev) for g in grads]
    if rule['kind'] == 'lamb':
        state = {'m': guard.zeros(lay.n, device=dev), 'v': guard.zeros(lay.n, device=dev)}
        for t in state.values():
            t[~lay.real.to(dev)] = pad
    else:
        state = {'buf': guard.full((lay.n,), float('nan'), device=dev)} if rule.get('momentum', 0.0) else {}   # the first step must not read it
    ws = guard.alloc_bytes(_lib.load().bdn_layerwise_workspace_bytes(lay.n, lay.nt), dev)       # born 0xFF
    trust = guard.empty(lay.nt, 3, device=dev)
    if ws_zero:
        ws.zero_()
        trust.zero_()
    dsb = None if ds is None else guard.guard(torch.tensor([ds], dtype=torch.float32), dev)
    hist = []
    for it, g in enumerate(gbufs):
        before = (p.clone(), {k: v.clone() for k, v in state.items()})
        _call(rule, lay, tab, p, g, state, it, ws, trust, dsb)
        hist.append(before + (p.clone(), {k: v.clone() for k, v in state.items()}, trust.clone()))
    return hist


def _check_step(name, rule, lay, it, g, rec):
    """One recorded step against the twin (tests/layerwise_ref.py: check_update), on the real elements of every tensor."""
    p_in, s_in, p_out, s_out, trust = rec
    lrs, wds = _hyper(rule, lay)
    hyper = dict({k: v for k, v in rule.items() if k not in ('kind', 'wd', 'gs')}, grad_scale=rule.get('gs', 1.0))
    L.check_update(rule['kind'], hyper, it, lay.split(p_in), lay.split(g), {k: lay.split(v) for k, v in s_in.items()}, lay.split(p_out),
                   {k: lay.split(v) for k, v in s_out.items()}, trust, [lrs[max(gid, 0)] for gid in lay.groups],
                   [wds[max(gid, 0)] for gid in lay.groups], lay.adapt, lay.frozen, name, lay.zero)
    assert bool((p_out != p_in).any()), 'the step changed nothing'
    if lay.slack:
        tail = slice(lay.n - lay.slack, lay.n)
        assert _same(p_out[tail], p_in[tail]) and all(_same(s_out[k][tail], s_in[k][tail]) for k in s_in), \
            f'{name}: a vector behind the table\'s end was written'


@pytest.mark.parametrize('layout', list(_LAYOUTS))
@pytest.mark.parametrize('name', list(_RULES))
@guarded
def test_layerwise_kernel_matches_float64_twin(name, layout):
    """Three steps (LARS's first-step branch, LAMB's bias corrections), each checked from the kernel's own inputs: norms, ratio, elements;
    frozen tensors keep their bits and report {0, 0, 0}; the guards stay 0xFF (@guarded)."""
    rule, lay = _RULES[name], Lay(**_LAYOUTS[layout])
    p0, grads = lay.inputs(len(name) * 131 + lay.n)
    hist = _run(rule, lay, p0, grads)
    torch.cuda.synchronize()
    for it, rec in enumerate(hist):
        _check_step(f'{name}/{layout}', rule, lay, it, grads[it], rec)


def _final(hist, lay):
    """What a run leaves, as comparable bits: the real elements of the parameters and the state after every step, and trust_out."""
    real = lay.real.to(dev)
    out = []
    for _, _, p, s, trust in hist:
        out += [_bits(p[real])] + [_bits(v[real]) for v in s.values()] + [_bits(trust)]
    return out


def _equal_runs(a, b, lay, what):
    fa, fb = _final(a, lay), _final(b, lay)
    assert len(fa) == len(fb) and all(torch.equal(x, y) for x, y in zip(fa, fb)), what


@pytest.mark.parametrize('name', ['lamb', 'lars_nesterov'])
@guarded
def test_bits_do_not_depend_on_pads_workspace_or_repeats(name):
    """On the frozen / grouped layout: a repeat run is bit-identical; NaN in the pads of parameters, gradients and state changes no real
    element and no norm; a workspace and a trust_out born 0xFF give the bits of zeroed ones; dev_scale pointing at 1.0f gives the
    bits of NULL."""
    rule, lay = _RULES[name], Lay(**_LAYOUTS['frozen_groups'])
    p0, grads = lay.inputs(77)
    base = _run(rule, lay, p0, grads)
    _equal_runs(base, _run(rule, lay, p0, grads), lay, 'a repeat run differs')
    _equal_runs(base, _run(rule, lay, p0, grads, ws_zero=True), lay, 'the result depends on what the workspace or trust_out held')
    _equal_runs(base, _run(rule, lay, p0, grads, ds=1.0), lay, 'dev_scale -> 1.0f differs from NULL')
    pn, gn = lay.inputs(77, pad=float('nan'))
    assert _same(pn[lay.real], p0[lay.real]) and bool(torch.isnan(pn[~lay.real]).all())
    _equal_runs(base, _run(rule, lay, pn, gn, pad=float('nan')), lay, 'NaN pads reached a real element or a norm')
    torch.cuda.synchronize()
    assert not bool(torch.isnan(base[-1][2][lay.real.to(dev)]).any())


@guarded
def test_lamb_dev_scale_is_multiplied_in():
    """dev_scale = 0.25 with grad_scale 2 gives the bits of grad_scale 0.5 (both products are exact)."""
    lay = Lay(**_LAYOUTS['mixed'])
    p0, grads = lay.inputs(5, steps=2)
    for name in ('lamb', 'lars_nesterov'):
        a = _run(dict(_RULES[name], gs=2.0), lay, p0, grads, ds=0.25)
        b = _run(dict(_RULES[name], gs=0.5), lay, p0, grads)
        _equal_runs(a, b, lay, f'{name}: dev_scale is not a factor on the gradient')


@guarded
def test_lamb_without_adaptation_is_adamw():
    """One tensor, adapt = 0, one group: the moments are bdn_adam_step_grouped's bit for bit, and the parameters agree with its decoupled
    rule within the sum of the two kernels' element bounds (the two rules are the same real-number expression)."""
    n = 70001
    lay = Lay([n], adapt=[0])
    p0, grads = lay.inputs(9)
    rule = dict(kind='lamb', wd=0.01)
    hist = _run(rule, lay, p0, grads)
    p = guard.guard(p0, dev)
    m, v = guard.zeros(lay.n, device=dev), guard.zeros(lay.n, device=dev)
    ends = guard.guard(torch.tensor([lay.n // 4], dtype=torch.int32), dev)
    ids = guard.guard(torch.tensor([0], dtype=torch.int32), dev)
    st = _lib.stream_ptr()
    for it, g in enumerate(grads):
        gb = guard.guard(g, dev)
        p_in, m_in, v_in = p.clone(), m.clone(), v.clone()
        _lib.call('bdn_adam_step_grouped', p.data_ptr(), gb.data_ptr(), m.data_ptr(), v.data_ptr(), ends.data_ptr(), ids.data_ptr(), 1, 1,
                  _lib.floats([0.01]), _lib.floats([0.01]), 1.0, 0.9, 0.999, 1e-8, 1, it + 1, lay.n, st)
        _, s_in, lp, ls, trust = hist[it]
        assert trust[0, 2].item() == 1.0
        assert _same(ls['m'][:n], m[:n]) and _same(ls['v'][:n], v[:n]), f'step {it}: LAMB\'s moments are not Adam\'s bits'
        if it == 0:                                          # the same inputs still: the two parameter results bound each other
            ref = L.lamb([p_in[:n].cpu()], [g[:n]], [m_in[:n].cpu()], [v_in[:n].cpu()], 1, [0.01], [0.01], ratios=[1.0])
            ap = R.adam(p_in[:n].cpu(), g[:n], m_in[:n].cpu(), v_in[:n].cpu(), 1, 0.01, weight_decay=0.01, decoupled=True)
            assert float((ref['p'][0] - ap[0]).abs().max()) <= 1e-12 * float(ap[3].max())
            err = (lp[:n].double().cpu() - p[:n].double().cpu()).abs()
            tol = EPS * (L.ULPS_P * ref['p_mag'][0] + R.ULPS * ap[3]) + 1e-38
            assert not bool((err > tol).any()), f'LAMB vs AdamW parameters: worst error / bound {float((err / tol).max()):.2f}'
        p.copy_(lp)                                          # go on from LAMB's parameters: the moments do not depend on them


def test_layerwise_bits_do_not_depend_on_launch_timing():
    """random(seed, 0.5) delays in front of the launches against a synchronize() in front of each: the same bits (the three launches of
    an update are ordered by their stream alone)."""
    lay = Lay(**_LAYOUTS['mixed'])
    p0, grads = lay.inputs(21, steps=2)
    for name in ('lamb', 'lars_nesterov'):
        with ss.Perturb(ss.sync()):
            a = _run(_RULES[name], lay, p0, grads)
        with ss.Perturb(ss.random(3, 0.5), short=200_000) as h:
            b = _run(_RULES[name], lay, p0, grads)
        torch.cuda.synchronize()
        assert h.log, 'no launch was delayed'
        _equal_runs(a, b, lay, f'{name}: launch timing changed the result')
