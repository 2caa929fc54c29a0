"""-m "not gpu": sharpness-aware minimisation without a device -- the float64 twin (tests/sam_ref.py) against the papers' formulas written
with torch autograd on a two-layer MLP, fabric_amd.optim.check_sam, the C ABI rows and argument errors of bdn_sam_perturb /
bdn_sam_restore (they come before any launch), and train.py's flags."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from fabric_amd import _lib
from fabric_amd import optim as O
from tests import sam_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_VP = ctypes.c_void_p
_CTYPES = {'float*': _VP, 'const float*': _VP, 'void*': _VP, 'const uint32_t*': _VP, 'const int32_t*': _VP, 'float': ctypes.c_float,
           'int': ctypes.c_int, 'size_t': ctypes.c_size_t}


# ------------------------------------------------------------------ the twin against autograd
def _mlp(seed=0, d=5, h=7, o=3, n=11):
    gen = torch.Generator().manual_seed(seed)
    w1 = torch.randn(h, d, generator=gen, dtype=torch.float64)
    b1 = torch.randn(h, generator=gen, dtype=torch.float64) * 0.1
    w2 = torch.randn(o, h, generator=gen, dtype=torch.float64)
    x = torch.randn(n, d, generator=gen, dtype=torch.float64)
    y = torch.randn(n, o, generator=gen, dtype=torch.float64)
    return [w1, b1, w2], x, y


def _loss(params, x, y):
    w1, b1, w2 = params
    return ((torch.relu(x @ w1.t() + b1) @ w2.t() - y) ** 2).mean()


def _grads(params, x, y):
    ps = [p.clone().requires_grad_(True) for p in params]
    return [g.detach() for g in torch.autograd.grad(_loss(ps, x, y), ps)]


@pytest.mark.parametrize('adaptive', [False, True])
def test_one_sam_step_of_the_twin_is_the_hand_rolled_step(adaptive):
    """perturb, regrad, restore, SGD -- the perturbation written out as the papers state it, on the concatenated vector."""
    params, x, y = _mlp()
    rho, lr = 0.05 if not adaptive else 0.5, 0.1
    g1 = _grads(params, x, y)
    # the papers' formula on one flat vector
    wv, gv = torch.cat([p.reshape(-1) for p in params]), torch.cat([g.reshape(-1) for g in g1])
    tv = wv.abs() if adaptive else torch.ones_like(wv)
    ev = rho * tv * tv * gv / torch.linalg.vector_norm(tv * gv)
    hand, off = [], 0
    for p in params:
        hand.append(p + ev[off:off + p.numel()].view_as(p))
        off += p.numel()
    g2_hand = _grads(hand, x, y)
    want = [p - lr * g for p, g in zip(params, g2_hand)]
    # the twin
    pert, es, saved, nrm = S.perturb(params, g1, rho, adaptive, eps=0.0)
    assert nrm == pytest.approx(float(torch.linalg.vector_norm(tv * gv)), rel=1e-14)
    assert all(torch.allclose(a, b, rtol=1e-13, atol=0) for a, b in zip(pert, hand))
    assert abs(float(torch.linalg.vector_norm(torch.cat([(e / t.clamp_min(1e-300)).reshape(-1) for e, t in
                                                         zip(es, [p.abs() if adaptive else torch.ones_like(p) for p in params])]))) - rho) < 1e-12
    g2 = _grads(pert, x, y)
    back = S.restore(saved)
    assert all(torch.equal(a, b) for a, b in zip(back, params))                        # a copy: bit for bit
    got = [p - lr * g for p, g in zip(back, g2)]
    assert all(torch.allclose(a, b, rtol=1e-12, atol=1e-15) for a, b in zip(got, want))
    assert any(not torch.equal(a, b) for a, b in zip(g2, g1))                           # the perturbation mattered
    assert float(_loss(pert, x, y)) > float(_loss(params, x, y))                         # an ascent step


def test_asam_is_invariant_under_rescaling_a_layer_and_its_successor_inversely():
    """relu is positively homogeneous: (a W1, a b1, W2 / a) is the same function.  ASAM's perturbation follows the rescaling (e1 -> a e1,
    e2 -> e2 / a), so the perturbed function, its loss and ||t g|| are the same; SAM's is not."""
    params, x, y = _mlp(seed=3)
    a = 7.5
    scaled = [params[0] * a, params[1] * a, params[2] / a]
    assert float(_loss(scaled, x, y)) == pytest.approx(float(_loss(params, x, y)), rel=1e-13)
    g, gs = _grads(params, x, y), _grads(scaled, x, y)
    pert, e, _, nrm = S.perturb(params, g, 0.5, True)
    perts, es, _, nrms = S.perturb(scaled, gs, 0.5, True)
    assert nrms == pytest.approx(nrm, rel=1e-12)
    for ek, esk, f in zip(e, es, (a, a, 1 / a)):
        assert torch.allclose(esk, ek * f, rtol=1e-11, atol=1e-18)
    assert float(_loss(perts, x, y)) == pytest.approx(float(_loss(pert, x, y)), rel=1e-11)
    plain, plains = S.perturb(params, g, 0.5, False)[0], S.perturb(scaled, gs, 0.5, False)[0]
    assert abs(float(_loss(plains, x, y)) - float(_loss(plain, x, y))) > 1e-3 * float(_loss(plain, x, y))


def test_twin_skips_frozen_tensors_and_survives_a_zero_gradient():
    params, x, y = _mlp(seed=5)
    g = _grads(params, x, y)
    pert, e, _, nrm = S.perturb(params, g, 0.05, False, frozen={1})
    assert torch.equal(pert[1], params[1]) and not bool(e[1].any())
    assert nrm == pytest.approx(float(torch.sqrt((g[0] ** 2).sum() + (g[2] ** 2).sum())), rel=1e-14)
    zero = [torch.zeros_like(p) for p in params]
    pert, e, _, nrm = S.perturb(params, zero, 0.05, True)
    assert nrm == 0.0 and all(torch.equal(a, b) for a, b in zip(pert, params))
    assert all(bool(torch.isfinite(a).all()) for a in pert)
    S.check_perturb([p.float() for p in params], [t.float() for t in zero], [p.float() for p in params], 0.0, 0.05, True, what='zero')


# ------------------------------------------------------------------ check_sam
def test_check_sam():
    assert O.check_sam() == (None, False, 1e-12)
    assert O.check_sam(0.05) == (0.05, False, 1e-12)
    assert O.check_sam(2, True, 0) == (2.0, True, 0.0)
    for bad in (0, 0.0, -0.1, float('nan'), float('inf'), True, '0.05'):
        with pytest.raises(ValueError, match='sam_rho'):
            O.check_sam(bad)
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='sam_adaptive'):
            O.check_sam(0.05, bad)
    for bad in (-1e-12, float('nan'), float('inf'), None, False):
        with pytest.raises(ValueError, match='sam_eps'):
            O.check_sam(0.05, False, bad)
    with pytest.raises(ValueError, match='give sam_rho'):
        O.check_sam(None, True)
    with pytest.raises(ValueError, match='give sam_rho'):
        O.check_sam(None, False, 1e-8)


# ------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize('name', ['bdn_sam_workspace_bytes', 'bdn_sam_perturb', 'bdn_sam_restore'])
def test_header_declaration_matches_signature_row(name):
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\b(int|size_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
    assert m, f'{name} not declared'
    params = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())).rsplit(' ', 1) for p in m.group(2).split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_size_t)
    assert [_CTYPES[ptype.strip()] for ptype, _ in params] == list(args), (params, args)
    assert hasattr(_lib.load(), name)


def _perturb_args(**kw):
    a = dict(params=32, saved=64, grads=96, ten_end=32, ten_len=32, ten_group=32, n_tensors=1, rho=0.05, adaptive=0, eps=1e-12, ws=32,
             out=32, n=16, stream=None)
    a.update(kw)
    return list(a.values())


def _restore_args(**kw):
    a = dict(params=32, saved=64, ten_end=32, ten_group=32, n_tensors=1, n=16, stream=None)
    a.update(kw)
    return list(a.values())


_REFUSED = [
    ('perturb', dict(params=None), 'null'), ('perturb', dict(saved=None), 'null'), ('perturb', dict(grads=None), 'null'),
    ('perturb', dict(ten_end=None), 'null'), ('perturb', dict(ten_len=None), 'null'), ('perturb', dict(ten_group=None), 'null'),
    ('perturb', dict(ws=None), 'null'), ('perturb', dict(out=None), 'null'), ('perturb', dict(params=40), 'aligned'),
    ('perturb', dict(saved=72), 'aligned'), ('perturb', dict(grads=100), 'aligned'), ('perturb', dict(ten_len=34), 'aligned'),
    ('perturb', dict(ws=36), 'aligned'), ('perturb', dict(out=34), 'aligned'), ('perturb', dict(saved=32), 'same buffer'),
    ('perturb', dict(n=18), 'multiple of 4'), ('perturb', dict(n_tensors=0), 'tensors'), ('perturb', dict(n_tensors=257), 'tensors'),
    ('perturb', dict(rho=0.0), 'rho'), ('perturb', dict(rho=-0.05), 'rho'), ('perturb', dict(rho=float('nan')), 'rho'),
    ('perturb', dict(eps=-1e-12), 'eps'), ('perturb', dict(eps=float('nan')), 'eps'), ('perturb', dict(adaptive=2), 'adaptive'),
    ('restore', dict(params=None), 'null'), ('restore', dict(saved=None), 'null'), ('restore', dict(ten_end=None), 'null'),
    ('restore', dict(ten_group=None), 'null'), ('restore', dict(saved=72), 'aligned'), ('restore', dict(ten_group=34), 'aligned'),
    ('restore', dict(saved=32), 'same buffer'), ('restore', dict(n=6), 'multiple of 4'), ('restore', dict(n_tensors=0), 'tensors'),
    ('restore', dict(n_tensors=300), 'tensors'),
]


@pytest.mark.parametrize('entry,kw,word', _REFUSED, ids=[f'{r}-{"-".join(k)}-{i}' for i, (r, k, _) in enumerate(_REFUSED)])
def test_argument_errors_return_before_touching_a_device(entry, kw, word):
    """Fake non-null pointers: every refusal is BDN_E_ARG from the host checks, nothing reaches a device."""
    lib = _lib.load()
    rc = lib.bdn_sam_perturb(*_perturb_args(**kw)) if entry == 'perturb' else lib.bdn_sam_restore(*_restore_args(**kw))
    msg = lib.bdn_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


def test_n_zero_launches_nothing_and_workspace_size():
    lib = _lib.load()
    assert lib.bdn_sam_perturb(*_perturb_args(n=0)) == 0 and lib.bdn_sam_restore(*_restore_args(n=0)) == 0
    # one double per chunk of 4096 vectors, rounded up to 16 bytes, whatever the table
    assert lib.bdn_sam_workspace_bytes(4 * 4096 * 3 + 4, 7) == 32
    assert lib.bdn_sam_workspace_bytes(4 * 4096 * 3 + 4, 7) == lib.bdn_sam_workspace_bytes(4 * 4096 * 3 + 4, 200)
    assert lib.bdn_sam_workspace_bytes(0, 0) == 16


# ------------------------------------------------------------------ train.py
def test_train_cli_refuses_the_sam_flags_without_the_fused_step():
    from fabric_amd import train
    for extra in (['--sam_rho', '0.05'], ['--sam_adaptive'], ['--sam_rho', '1.0', '--sam_adaptive']):
        with pytest.raises(SystemExit, match='add --fused_step true'):
            train.main(['--synthetic'] + extra)
    with pytest.raises(SystemExit, match='sam_rho'):
        train.main(['--synthetic', '--fused_step', 'true', '--sam_rho', '-1'])
    with pytest.raises(SystemExit, match='give sam_rho'):
        train.main(['--synthetic', '--fused_step', 'true', '--sam_adaptive'])


def test_without_the_flags_the_step_is_built_as_before():
    """No flag: no keyword reaches TrainStep, so the run issues today's calls and writes today's epoch record (its keys are pinned on the
    device by the existing epoch-record test; train_epoch adds the two SAM keys only for a step whose sam_rho is set)."""
    from fabric_amd import train
    assert train.sam_kwargs(argparse.Namespace(sam_rho=None, sam_adaptive=False, fused_step=False)) == {}
    assert train.sam_kwargs(argparse.Namespace(sam_rho=None, sam_adaptive=False, fused_step=True)) == {}
    assert train.sam_kwargs(argparse.Namespace(sam_rho=0.05, sam_adaptive=True, fused_step=True)) == dict(sam_rho=0.05, sam_adaptive=True)
