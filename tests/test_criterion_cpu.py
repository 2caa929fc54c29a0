"""CPU tests of the criterion layer (fabric_amd/criterion.py, bdn_criterion's argument checks and workspace size, the CLI routing of
--fused_step) and of the float64 restatement of the compound loss that tests/test_gpu_criterion.py holds the kernels to: the weighted sum
of the oracle's own terms (tests/criterion_ref.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.criterion import COMPOUND, NAMES, Criterion
from oracle import bidate_oracle as O

from tests import criterion_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'const uint8_t*': ctypes.c_void_p,
           'int32_t*': ctypes.c_void_p, 'float': ctypes.c_float, 'int': ctypes.c_int}


def test_header_declaration_matches_signature_row():
    hdr = open(os.path.join(ROOT, 'include', 'bidate_hip.h')).read()
    m = re.search(r'\bint\s+bdn_criterion\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'bdn_criterion not declared'
    types = [re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', '* ', p.strip())).rsplit(' ', 1)[0].strip() for p in m.group(1).split(',')]
    res, args = _lib.SIGNATURES['bdn_criterion']
    assert res is ctypes.c_int and [_CTYPES[t] for t in types] == list(args), (types, args)
    assert _lib.SIGNATURES['bdn_criterion_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    for ref in ('utils/metrics.py:8-48', ':51-171', 'utils/helpers.py:303-312'):
        assert ref in hdr, f'the declaration names the reference call site {ref}'


# ---------------------------------------------------------------- parsing
def test_parse_gives_the_coefficients_of_the_seven_names():
    kw = dict(tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=0.25, weights=(0.25, 2.0), eps=1e-6)
    want = {'tversky': (1.0, 0.1, 0.9, 1e-6, 0.0), 'dice': (1.0, 0.5, 0.5, 5e-7, 0.0), 'jaccard': (1.0, 1.0, 1.0, 1e-6, 0.0),
            'focal+tversky': (2.0, 0.1, 0.9, 1e-6, 0.25), 'focal+dice': (2.0, 0.5, 0.5, 5e-7, 0.25), 'focal+jaccard': (2.0, 1.0, 1.0, 1e-6, 0.25)}
    assert set(NAMES) == set(want) | {'focal'} and set(COMPOUND) == {n for n in want if '+' in n}
    for name, (wo, a, b, eps, wf) in want.items():
        c = Criterion.parse(name, **kw)
        assert (c.w_overlap, c.alpha, c.beta, c.eps, c.w_focal) == (wo, a, b, eps, wf), (name, c)
        assert c.reduce == 'columns' and c.size_average is True
        assert (c.gamma, c.class_alpha) == ((2.0, (0.25, 0.75)) if wf else (0.0, None)), (name, c)
    f = Criterion.parse('focal', **kw)
    assert (f.w_overlap, f.w_focal, f.gamma, f.class_alpha) == (0.0, 1.0, 2.0, (0.25, 0.75))     # a single term ignores `weights`
    d = Criterion.parse('dice')
    assert (d.alpha, d.beta, d.eps) == (0.5, 0.5, 0.5e-7) and Criterion.parse('jaccard').eps == 1e-7
    assert Criterion.parse('focal+dice', focal_gamma=0).w_focal == 1.0 == Criterion.parse('focal+dice', focal_gamma=0).w_overlap
    assert Criterion.parse('dice', reduce='image').reduce == 'image'


def test_parse_and_constructor_rejections():
    with pytest.raises(ValueError, match='unknown criterion'):
        Criterion.parse('bce')
    with pytest.raises(ValueError, match='unknown criterion'):
        Criterion.parse('dice+focal')
    with pytest.raises(ValueError, match='gamma'):
        Criterion.parse('focal')
    with pytest.raises(ValueError, match='gamma'):
        Criterion.parse('focal+dice')
    with pytest.raises(ValueError, match='>= 0'):
        Criterion.parse('focal+dice', focal_gamma=2, weights=(-1, 1))
    with pytest.raises(ValueError, match='>= 0'):
        Criterion(w_overlap=-0.5, w_focal=1.0)
    with pytest.raises(ValueError, match='both zero'):
        Criterion.parse('focal+tversky', focal_gamma=2, weights=(0, 0))
    with pytest.raises(ValueError, match='both zero'):
        Criterion(w_overlap=0.0, w_focal=0.0)
    with pytest.raises(ValueError, match='reduce'):
        Criterion(reduce='rows')
    with pytest.raises(ValueError, match='gamma'):
        Criterion(w_focal=1.0, gamma=-1.0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        Criterion().evaluate(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))


# ---------------------------------------------------------------- the entry point's checks
def _crit(**kw):
    a = dict(logits=16, labels=16, w_overlap=1.0, alpha=0.5, beta=0.5, eps=1e-7, reduce_w=0, w_focal=1.0, gamma=2.0, class_alpha=None,
             size_average=1, ws=16, loss=16, terms=None, counts=None, dlogits=None, B=2, ncls=2, H=8, W=8, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    lib = _lib.load()
    rc = lib.bdn_criterion(*a.values())
    return rc, lib.bdn_last_error()


def test_argument_errors_return_before_touching_a_device():
    for name in ('logits', 'labels', 'ws', 'loss'):
        rc, msg = _crit(**{name: None})
        assert rc != 0 and b'null pointer' in msg, name
    rc, msg = _crit(w_overlap=0.0, w_focal=0.0)
    assert rc != 0 and b'both weights are zero' in msg
    for kw in (dict(w_overlap=-1.0), dict(w_focal=-0.5), dict(w_overlap=float('nan'))):
        rc, msg = _crit(**kw)
        assert rc != 0 and b'negative weight' in msg, kw
    rc, msg = _crit(gamma=-1.0)
    assert rc != 0 and b'negative gamma' in msg
    for ncls in (1, 9):
        rc, msg = _crit(ncls=ncls)
        assert rc != 0 and b'ncls' in msg, ncls
    rc, msg = _crit(B=1 << 15, H=1 << 8, W=1 << 8)                                # B*H*W = 2^31
    assert rc != 0 and b'2^31' in msg
    rc, msg = _crit(B=0)
    assert rc != 0 and b'bad shape' in msg
    rc, msg = _crit(ws=24)
    assert rc != 0 and b'aligned' in msg
    with pytest.raises(RuntimeError, match='both weights are zero'):
        _lib.call('bdn_criterion', 16, 16, 0.0, 0.5, 0.5, 1e-7, 0, 0.0, 0.0, None, 1, 16, 16, None, None, None, 2, 2, 8, 8, None)


def test_workspace_size():
    lib = _lib.load()
    ws = lib.bdn_criterion_workspace_bytes
    for shape in [(64, 2, 128, 128), (3, 2, 90, 77), (1, 8, 16, 300), (2, 3, 1, 5), (2, 2, 1, 1)]:
        B, C, H, W = shape
        for reduce_w in (0, 1):
            n = ws(B, C, H, W, reduce_w)
            assert n > 0 and n >= lib.bdn_overlap_workspace_bytes(B, C, H, W, reduce_w) and n >= lib.bdn_focal_workspace_bytes(), shape
    assert ws(0, 2, 8, 8, 0) == 0 and ws(2, 1, 8, 8, 0) == 0 and ws(2, 9, 8, 8, 0) == 0 and ws(2, 2, 0, 8, 0) == 0 and ws(2, 2, 8, -1, 1) == 0
    assert ws(1 << 15, 2, 1 << 8, 1 << 8, 0) == 0                                 # B*H*W = 2^31


# ---------------------------------------------------------------- CLI routing (no step runs: every case is refused while the options are read)
def _train(*args):
    return subprocess.run([sys.executable, '-m', 'fabric_amd.train', '--synthetic', '--epochs', '1', *args], cwd=ROOT, capture_output=True,
                          text=True, timeout=600)


@pytest.mark.parametrize('name', ['focal+dice', 'focal+jaccard', 'focal+tversky'])
def test_compound_names_need_the_fused_step(name):
    r = _train('--loss_function', name, '--focal_gamma', '2')
    assert r.returncode != 0 and '--fused_step true' in r.stderr, r.stderr[-500:]


def test_cli_refusals_without_and_with_the_flag():
    r = _train('--freeze', 'inc', '--loss_function', 'dice')
    assert r.returncode != 0 and 'tversky' in r.stderr and '--fused_step' in r.stderr
    r = _train('--fused_step', 'true', '--loss_function', 'focal+dice')            # a focal term without a gamma
    assert r.returncode != 0 and '--focal_gamma' in r.stderr
    r = _train('--fused_step', 'true', '--loss_function', 'bce')
    assert r.returncode != 0 and 'bce' in r.stderr
    r = _train('--fused_step', 'true', '--loss_function', 'focal+dice', '--focal_gamma', '2', '--loss_weights', '0', '0')
    assert r.returncode != 0 and 'zero' in r.stderr


def test_get_criterion_returns_a_compound_loss_for_compound_names():
    import types
    from fabric_amd.utils import metrics as M
    from fabric_amd.utils.helpers import get_criterion
    opt = types.SimpleNamespace(loss_function='focal+tversky', tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, loss_weights=[0.25, 2.0])
    c = get_criterion(opt)
    assert isinstance(c, M.CompoundLoss) and c.last_counts is None and c.last_terms is None
    k = c.criterion
    assert (k.w_focal, k.w_overlap, k.alpha, k.beta, k.gamma) == (0.25, 2.0, 0.1, 0.9, 2.0)
    opt.loss_function = 'dice'
    assert get_criterion(opt) is M.dice_loss                                       # what it returned before, it still returns


# ---------------------------------------------------------------- the float64 yardstick
@pytest.mark.parametrize('shape', [(3, 2, 9, 7), (2, 3, 1, 5)])
def test_reference_formula_is_the_weighted_sum_of_the_oracle_terms(shape):
    B, C, H, W = shape
    r = np.random.default_rng(3)
    logits = torch.from_numpy(3 * r.standard_normal(shape))
    lbl = torch.from_numpy(r.integers(0, C, (B, H, W)))
    ca = [0.25, 0.75, 0.5][:C]
    for reduce, labels in (('columns', lbl), ('image', lbl[:, None])):
        terms = {'dice': O.dice_loss(logits, labels), 'jaccard': O.jaccard_loss(logits, labels),
                 'tversky': O.tversky_loss(logits, labels, 0.1, 0.9)}
        for name, ov in terms.items():
            for wf, wo in ((1, 1), (0.25, 2), (3, 0.5)):
                c = Criterion.parse('focal+' + name, tversky_alpha=0.1, tversky_beta=0.9, focal_gamma=2.0, focal_alpha=ca, weights=(wf, wo),
                                    reduce=reduce)
                ref = CR.reference(c, logits, lbl)
                fo = O.focal_loss(logits, lbl, 2.0, ca)
                assert ref['overlap'] == float(ov) and ref['focal'] == float(fo)
                assert ref['loss'] == pytest.approx(wo * float(ov) + wf * float(fo), rel=1e-14)
                lo = logits.clone().requires_grad_(True)
                (wo * {'dice': O.dice_loss, 'jaccard': O.jaccard_loss, 'tversky': lambda a, b: O.tversky_loss(a, b, 0.1, 0.9)}[name](lo, labels)
                 + wf * O.focal_loss(lo, lbl, 2.0, ca)).backward()
                assert torch.allclose(ref['dloss'], lo.grad, rtol=1e-12, atol=1e-15)
                assert torch.allclose(ref['dloss'], wo * ref['doverlap'] + wf * ref['dfocal'], rtol=1e-12, atol=1e-15)
    single = CR.reference(Criterion.parse('dice'), logits, lbl)
    assert single['loss'] == float(O.dice_loss(logits, lbl)) and single['focal'] == 0.0
