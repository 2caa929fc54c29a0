"""-m gpu: the sharpness-aware kernels (include/bidate_hip.h: bdn_sam_perturb, bdn_sam_restore) on guard-banded buffers.

Every perturbation is checked from the kernel's own float32 inputs against the float64 twin (tests/sam_ref.py, pinned in
tests/test_sam_cpu.py) with the bounds of check_perturb, which are derived from the kernel's arithmetic and not measured: the reported
norm is one rounding of a double sum, an element carries six float32 roundings in e and one in the sum.  Then the bit-level properties:
NaN pads, a frozen tensor with NaN gradients, huge, zero and NaN gradients, perturb + restore = identity, poisoned workspaces, launch
delays."""
import pytest
import torch

from fabric_amd import BiDateNet, _lib
from fabric_amd import optim as O
from fabric_amd.engine import param_order
from fabric_amd.parallel import FlatLayout
from tests import guard
from tests import sam_ref as S
from tests import sched_stress as ss
from tests.guard import guarded

pytestmark = pytest.mark.gpu
dev = torch.device('cuda', 0)

CHUNK = 4096 * 4          # floats per partial sum (include/bidate_hip.h: one double per 4096 vectors)

_LAYOUTS = {
    'one_short': dict(sizes=[1023]),                                          # a single tensor shorter than one reduction chunk
    'primes': dict(sizes=[1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41], groups=[0] * 6 + [-1] + [0] * 7),   # many tensors sharing a chunk
    # more than three partial-sum blocks with a ragged last one; tensor boundaries inside chunks, one tensor over several chunks
    'blocks': dict(sizes=[5, CHUNK, 3, 2 * CHUNK + 6, 4099, 70, 9001], groups=[0, 0, 1, 0, -1, 2, 0]),
    'model': None,                                                            # BiDateNet(3, 2)'s real table, the first block frozen
    # 4096 + 1024 + 256 + 5 vectors, five tensors (three pad entries in the staged table): a 16-vector one, one that ends 3 vectors into
    # a block of 256, a frozen one, and the last end 5 vectors short of n / 4 -- those hold NaN and are neither read nor written
    'short_table': dict(sizes=[61, 4042, 7997, 1199, 8195], groups=[0, 1, -1, 0, 1], slack=20),
}


class Lay:
    """A flat layout of `sizes` (every tensor padded to a float4) and its per-tensor table; group -1 is frozen."""

    def __init__(self, sizes, groups=None, slack=0):
        self.sizes, self.slack = list(sizes), slack                 # slack: floats (whole vectors) behind the table's last end
        self.offs, off = [], 0
        for s in self.sizes:
            self.offs.append(off)
            off += (s + 3) // 4 * 4
        self.n, self.nt = off + slack, len(self.sizes)
        self.ends = [(o + (s + 3) // 4 * 4) // 4 for o, s in zip(self.offs, self.sizes)]
        self.groups = list(groups) if groups is not None else [0] * self.nt
        self.frozen = {i for i, g in enumerate(self.groups) if g < 0}
        self.real = torch.zeros(self.n, dtype=torch.bool)
        self.live = torch.zeros(self.n, dtype=torch.bool)           # whole float4s of the trainable tensors: what the kernels may touch
        for i, (o, s) in enumerate(zip(self.offs, self.sizes)):
            self.real[o:o + s] = True
            if i not in self.frozen:
                self.live[o:o + (s + 3) // 4 * 4] = True

    @classmethod
    def of_model(cls):
        model = BiDateNet(3, 2)
        named = list(model.named_parameters())
        layout = FlatLayout([(k, p.shape) for k, p in named], param_order(3))
        frozen = {k for k, _ in named if k.startswith('inc.')}
        ends, lens, ids, _ = O.tensor_table(layout, O.ParamGroups(O.OptimConfig(), [k for k, _ in named], None, frozen))
        lay = cls(lens.tolist(), ids.tolist())
        assert lay.ends == ends.tolist() and lay.n == layout.total and lay.frozen          # the product's own table
        return lay

    def split(self, flat):
        flat = flat.detach().cpu()
        return [flat[o:o + s] for o, s in zip(self.offs, self.sizes)]

    def table(self):
        as32 = lambda v: guard.guard(torch.tensor(v, dtype=torch.int64).to(torch.int32), dev)
        return as32(self.ends), as32(self.sizes), as32(self.groups)

    def inputs(self, seed, pad=0.0):
        """(p, g) on the CPU: some parameters scaled by 1e-3, some exactly zero (also -0.0), some zero gradients; pads hold `pad`."""
        gen = torch.Generator(device='cpu').manual_seed(seed)
        p = torch.randn(self.n, generator=gen)
        p[::7] *= 1e-3
        p[3::11] = 0.0
        p[5::13] = -0.0
        g = torch.randn(self.n, generator=gen) * 0.3
        g[::5] = 0.0
        for t in (p, g):
            t[~self.real] = pad
            t[self.n - self.slack:] = float('nan')            # behind the table: a read poisons the norm
        return p, g


_CACHE = {}


def _lay(name):
    if name not in _CACHE:
        _CACHE[name] = Lay.of_model() if name == 'model' else Lay(**_LAYOUTS[name])
    return _CACHE[name]


def _bits(t):
    return t.detach().view(torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run(lay, p0, g0, adaptive, rho=0.05, eps=1e-12, ws_fill=None, restore=True):
    """perturb (and restore) on fresh guarded buffers -> dict of clones: p1 (perturbed), saved, out, p2 (restored)."""
    ends, lens, ids = lay.table()
    p, g = guard.guard(p0, dev), guard.guard(g0, dev)
    saved = guard.empty(lay.n, device=dev)                                   # born 0xFF: NaN wherever the kernel does not write
    ws = guard.alloc_bytes(_lib.load().bdn_sam_workspace_bytes(lay.n, lay.nt), dev)
    out = guard.empty(2, device=dev)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    st = _lib.stream_ptr()
    _lib.call('bdn_sam_perturb', p.data_ptr(), saved.data_ptr(), g.data_ptr(), ends.data_ptr(), lens.data_ptr(), ids.data_ptr(), lay.nt,
              rho, int(adaptive), eps, ws.data_ptr(), out.data_ptr(), lay.n, st)
    res = dict(p1=p.clone(), saved=saved.clone(), out=out.clone(), g=g.clone())
    if restore:
        _lib.call('bdn_sam_restore', p.data_ptr(), saved.data_ptr(), ends.data_ptr(), ids.data_ptr(), lay.nt, lay.n, st)
        res['p2'] = p.clone()
    return res


def _untouched(lay, r, p0, g0, what):
    """Nothing outside the float4s of the trainable tensors was written: params and grads keep their bits there, saved its 0xFF."""
    dead = ~lay.live
    assert _same(r['p1'].cpu()[dead], p0[dead]) and _same(r['g'].cpu(), g0), f'{what}: a frozen tensor or the gradient was written'
    assert bool((_bits(r['saved'])[dead] == -1).all()), f'{what}: saved was written outside the trainable tensors'
    assert _same(r['saved'].cpu()[lay.live], p0[lay.live]), f'{what}: saved is not the parameters'


@pytest.mark.parametrize('adaptive', [0, 1])
@pytest.mark.parametrize('layout', list(_LAYOUTS))
@guarded
def test_perturb_matches_the_twin_and_restore_is_the_identity(layout, adaptive):
    lay = _lay(layout)
    p0, g0 = lay.inputs(17 + lay.n)
    rho = 0.5 if adaptive else 0.05
    r = _run(lay, p0, g0, adaptive, rho)
    torch.cuda.synchronize()
    nrm = S.check_perturb(lay.split(p0), lay.split(g0), lay.split(r['p1']), r['out'][0].item(), rho, bool(adaptive), frozen=lay.frozen,
                          what=f'{layout}/{adaptive}')
    assert nrm > 0 and r['out'][1].item() == (torch.tensor(rho) / (r['out'][0].cpu() + torch.tensor(1e-12))).item()      # float32, from the reported norm
    _untouched(lay, r, p0, g0, layout)
    assert _same(r['p1'].cpu()[~lay.real], p0[~lay.real]), 'a pad element moved'
    assert bool((r['p1'].cpu()[lay.live & lay.real] != p0[lay.live & lay.real]).any()), 'the perturbation changed nothing'
    assert _same(r['p2'], p0), 'perturb + restore is not the identity in bits'


@pytest.mark.parametrize('adaptive', [0, 1])
@guarded
def test_bits_do_not_depend_on_pads_or_workspace(adaptive):
    lay = _lay('blocks')
    p0, g0 = lay.inputs(5)
    base = _run(lay, p0, g0, adaptive, ws_fill=0x00)
    other = _run(lay, p0, g0, adaptive, ws_fill=0xFF)
    assert _same(base['p1'], other['p1']) and _same(base['out'], other['out']), 'the result depends on what the workspace held'
    pn, gn = lay.inputs(5, pad=float('nan'))
    assert _same(pn[lay.real], p0[lay.real]) and bool(torch.isnan(pn[~lay.real]).all()) and bool(torch.isnan(gn[~lay.real]).all())
    nan = _run(lay, pn, gn, adaptive)
    real = lay.real.to(dev)
    assert _same(nan['p1'][real], base['p1'][real]) and _same(nan['out'], base['out']), 'NaN pads reached a real element or the norm'
    assert _same(nan['p1'][~real], pn.to(dev)[~real]) and _same(nan['p2'], pn), 'a pad lost its bits'
    torch.cuda.synchronize()
    assert bool(torch.isfinite(base['p1'][real]).all()) and bool(torch.isfinite(base['out']).all())


@pytest.mark.parametrize('adaptive', [0, 1])
@guarded
def test_a_frozen_tensor_with_nan_gradients_is_neither_read_nor_written(adaptive):
    lay = _lay('blocks')
    p0, g0 = lay.inputs(9)
    base = _run(lay, p0, g0, adaptive)
    k = 4                                                                        # the frozen tensor in the middle
    assert k in lay.frozen
    gn = g0.clone()
    gn[lay.offs[k]:lay.ends[k] * 4] = float('nan')
    r = _run(lay, p0, gn, adaptive)
    assert _same(r['out'], base['out']) and _same(r['p1'], base['p1']), 'a frozen tensor\'s gradient was read'
    _untouched(lay, r, p0, gn, 'frozen NaN')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(r['out']).all())


@pytest.mark.parametrize('adaptive', [0, 1])
@guarded
def test_huge_zero_and_nan_gradients(adaptive):
    lay = _lay('primes')
    p0, g0 = lay.inputs(3)
    live_real = lay.live & lay.real
    # 1e30: the squares overflow float32, not the double sums (the elements are not held to the twin's bound here: with rho / norm near
    # 1e-32 the adaptive products pass through float32's subnormals)
    big = torch.where(g0 != 0, torch.full_like(g0, 1e30) * g0.sign(), g0)
    r = _run(lay, p0, big, adaptive)
    nrm = S.norm(lay.split(p0), lay.split(big), bool(adaptive), lay.frozen)
    assert bool(torch.isfinite(r['out']).all()) and abs(r['out'][0].item() - nrm) <= 2.0 ** -23 * nrm and nrm > 1e27
    assert bool(torch.isfinite(r['p1'].cpu()[live_real]).all()) and _same(r['p2'], p0)
    # zero: norm 0, the parameters keep their bits (-0.0 included) and stay finite
    z = _run(lay, p0, torch.zeros_like(g0), adaptive)
    assert z['out'][0].item() == 0.0 and _same(z['p1'], p0) and _same(z['p2'], p0)
    assert bool(torch.isfinite(z['p1'].cpu()[lay.real]).all()) and bool(torch.isfinite(z['out']).all())
    # one NaN in a trainable gradient: the norm is NaN, and the restore still returns every bit
    gn = g0.clone()
    gn[lay.offs[9]] = float('nan')
    pn = p0.clone()
    pn[~lay.real] = float('nan')
    n = _run(lay, pn, gn, adaptive)
    assert n['out'][0].item() != n['out'][0].item(), 'a NaN gradient must give a NaN norm'
    assert bool(torch.isnan(n['p1'].cpu()[live_real]).any())
    assert _same(n['p2'], pn), 'the restore did not return every bit'


def test_bits_do_not_depend_on_launch_timing():
    """random(seed, 0.5) delays in front of the launches against a synchronize() in front of each: the same bits (the launches of the
    perturbation and the restore are ordered by their stream alone)."""
    lay = _lay('blocks')
    p0, g0 = lay.inputs(21)
    for adaptive in (0, 1):
        with ss.Perturb(ss.sync()):
            a = _run(lay, p0, g0, adaptive)
        with ss.Perturb(ss.random(3, 0.5), short=200_000) as h:
            b = _run(lay, p0, g0, adaptive)
        torch.cuda.synchronize()
        assert h.log, 'no launch was delayed'
        assert all(_same(a[k], b[k]) for k in ('p1', 'saved', 'out', 'p2')), 'launch timing changed the result'
