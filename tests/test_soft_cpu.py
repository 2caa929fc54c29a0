"""-m "not gpu": the soft-target criterion without a device -- the float64 restatement tests/soft_ref.py pinned three ways (to
tests/ignore_ref.py at one-hot targets and 0 / 1 weights, to torch's cross_entropy with label_smoothing and with probability targets),
the arguments of Criterion(label_smoothing=), the refusals of topk and of the add-on terms, the argument errors of bdn_criterion_soft
that come before any launch, and train.py's flag."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fabric_amd import _lib
from fabric_amd.criterion import Criterion
from tests import ignore_ref as IR
from tests import soft_ref as SR

SHAPES = [(3, 2, 9, 7), (2, 5, 4, 6)]


def _data(shape, seed=3, ignore_frac=0.3, ignore=255):
    B, C, H, W = shape
    r = np.random.default_rng(seed)
    logits = torch.from_numpy(3 * r.standard_normal(shape))
    labels = torch.from_numpy(r.integers(0, C, (B, H, W)).astype(np.int64))
    m = torch.from_numpy(r.random((B, H, W)) < ignore_frac)
    return logits, labels, torch.where(m, torch.full_like(labels, ignore), labels), m


def _class_alpha(C):
    return [0.25, 0.75] if C == 2 else [round(0.1 + 0.8 * k / (C - 1), 3) for k in range(C)]


def _criteria(C, reduce, **kw):
    kw = dict(reduce=reduce, **kw)
    out = [Criterion.parse('tversky', tversky_alpha=0.1, tversky_beta=0.9, **kw)]
    for g in (0.0, 2.0):
        for sa in (True, False):
            out.append(Criterion(w_overlap=0.0, w_focal=1.0, gamma=g, class_alpha=_class_alpha(C), size_average=sa, **kw))
    out.append(Criterion.parse('focal+dice', focal_gamma=2.0, weights=(0.25, 2), **kw))
    return out


# ------------------------------------------------------------------ the restatement, pinned
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('reduce', ['columns', 'image'])
def test_one_hot_targets_and_01_weights_are_the_ignore_restatement(shape, reduce):
    """Hard labels with an ignore_index, the same as 0 / 1 weights on the unpainted labels, the same as one-hot float targets with 0 / 1
    weights: all three equal tests/ignore_ref.reference to 1e-12 in loss and gradient."""
    logits, clean, painted, ignored = _data(shape)
    C = shape[1]
    w01 = (~ignored).double()
    one_hot = F.one_hot(clean, C).permute(0, 3, 1, 2).double()
    for c, plain in zip(_criteria(C, reduce, ignore_index=255), _criteria(C, reduce)):
        want = IR.reference(c, logits, painted)
        for got in (SR.reference(c, logits, painted), SR.reference(plain, logits, clean, weights=w01),
                    SR.reference(plain, logits, one_hot, weights=w01)):
            for k in ('loss', 'overlap', 'focal'):
                assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, got[k], want[k])
            for k in ('dloss', 'doverlap', 'dfocal'):
                assert (got[k] - want[k]).abs().max().item() <= 1e-12, k
        assert SR.counts(c, logits, painted) == IR.counts(logits, painted, 255)
        assert SR.counts(plain, logits, clean, weights=w01) == IR.counts(logits, painted, 255)
        assert SR.counts(plain, logits, one_hot, weights=w01) == IR.counts(logits, painted, 255)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('e', [0.0, 0.1, 0.5])
def test_smoothed_hard_labels_are_torchs_cross_entropy(shape, e):
    logits, _, painted, _ = _data(shape)
    c = Criterion(w_overlap=0.0, w_focal=1.0, gamma=0.0, ignore_index=255, label_smoothing=e)
    x = logits.clone().requires_grad_(True)
    want = F.cross_entropy(x, painted, ignore_index=255, label_smoothing=e)
    (dwant,) = torch.autograd.grad(want, x)
    want = want.detach()
    got = SR.reference(c, logits, painted)
    # (hi, lo) are float32 values: the distance of e / ncls from its float32 rounding carries into the loss
    tol = 1e-12 if e == 0.0 else 2.0 ** -23 * max(1.0, abs(float(want)))
    assert abs(got['loss'] - float(want)) <= tol * 4, (got['loss'], float(want))
    assert (got['dloss'] - dwant).abs().max().item() <= tol * 4 / max(1, int((painted != 255).sum())) + 1e-12


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_float_targets_are_torchs_cross_entropy_with_probabilities(shape):
    logits, _, _, _ = _data(shape)
    B, C, H, W = shape
    q = torch.from_numpy(np.random.default_rng(5).dirichlet([0.5] * C, (B, H, W))).permute(0, 3, 1, 2).contiguous()
    c = Criterion(w_overlap=0.0, w_focal=1.0, gamma=0.0)
    x = logits.clone().requires_grad_(True)
    want = F.cross_entropy(x, q)
    (dwant,) = torch.autograd.grad(want, x)
    want = want.detach()
    got = SR.reference(c, logits, q)
    assert abs(got['loss'] - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert (got['dloss'] - dwant).abs().max().item() <= 1e-12


def test_invalid_pixels_reach_nothing_in_the_restatement():
    logits, clean, _, ignored = _data(SHAPES[0])
    w = torch.where(ignored, torch.zeros(()), torch.rand(ignored.shape, generator=torch.Generator().manual_seed(1)) + 0.1).double()
    c = Criterion.parse('focal+dice', focal_gamma=2.0, label_smoothing=0.1)
    bad = logits.clone()
    bad[ignored[:, None].expand_as(bad)] = float('nan')
    a, b = SR.reference(c, logits, clean, weights=w), SR.reference(c, bad, clean, weights=w)
    assert a['loss'] == b['loss'] and torch.equal(a['dloss'], b['dloss'])
    assert not b['dloss'][ignored[:, None].expand_as(bad)].any()


# ------------------------------------------------------------------ Criterion
def test_criterion_label_smoothing_arguments():
    assert Criterion().label_smoothing == 0.0 and 'label_smoothing' not in repr(Criterion())
    c = Criterion.parse('focal+dice', focal_gamma=2.0, label_smoothing=0.1)
    assert c.label_smoothing == 0.1 and 'label_smoothing=0.1' in repr(c)
    assert Criterion.parse('focal+lovasz', label_smoothing=0.05, w_boundary=0.01).label_smoothing == 0.05
    for bad in (-0.1, 1.0, 1.5, float('nan'), True, 'x', None):
        with pytest.raises(ValueError, match='label_smoothing'):
            Criterion(label_smoothing=bad)
    with pytest.raises(ValueError, match='topk ranks a hard-label'):
        Criterion(w_focal=1.0, topk=0.25, label_smoothing=0.1)
    with pytest.raises(ValueError, match='topk ranks a hard-label'):
        Criterion.parse('focal+dice', focal_gamma=2.0, topk=0.25, label_smoothing=0.1)
    with pytest.raises(ValueError, match='needs one of their weights'):
        Criterion.parse('lovasz', label_smoothing=0.1)


def test_topk_and_the_add_on_terms_refuse_soft_inputs_at_the_call():
    """The refusals come before the device check: CPU tensors show them."""
    shape = (2, 2, 4, 4)
    lg, lab = torch.zeros(shape), torch.zeros(2, 4, 4, dtype=torch.uint8)
    w, q = torch.ones(2, 4, 4), torch.full(shape, 0.5)
    topk = Criterion(w_focal=1.0, topk=0.25)
    for kw in (dict(labels=lab, weights=w), dict(labels=q)):
        with pytest.raises(ValueError, match='topk ranks a hard-label'):
            topk.evaluate(lg, **kw)
    for c in (Criterion.parse('focal+lovasz'), Criterion.parse('dice', w_boundary=0.1)):
        with pytest.raises(ValueError, match='do not take float targets'):
            c.evaluate(lg, q)
    with pytest.raises(ValueError, match='needs one of their weights'):
        Criterion.parse('lovasz').evaluate(lg, lab, weights=w)
    for c in (Criterion(label_smoothing=0.1), Criterion(ignore_index=255)):
        with pytest.raises(ValueError, match='float targets are taken as given'):
            c.evaluate(lg, q)
    plain = Criterion()
    for bad in (w.double(), torch.ones(2, 4, 5), torch.ones(2, 4, 8)[:, :, ::2]):
        with pytest.raises(RuntimeError, match='weights must be a contiguous float32'):
            plain.evaluate(lg, lab, weights=bad)
    with pytest.raises(RuntimeError, match='float targets must be a contiguous float32'):
        plain.evaluate(lg, q.double())
    # what is no soft input keeps its old errors
    with pytest.raises(RuntimeError, match='no CPU path'):
        plain.evaluate(lg, lab)
    with pytest.raises(RuntimeError, match='no CPU path'):
        plain.evaluate(lg, lab, weights=w)


# ------------------------------------------------------------------ the C ABI: every BDN_E_ARG case comes before any launch
def _soft(**kw):
    """bdn_criterion_soft with plausible (never dereferenced) addresses; the keyword arguments replace one of them."""
    a = dict(logits=4096, labels=8192, targets=None, weights=None, ignore=-1, smoothing=0.0, w_o=1.0, alpha=0.5, beta=0.5, eps=1e-7,
             reduce=0, w_f=1.0, gamma=0.0, calpha=None, sa=1, ws=16384, loss=20480, terms=None, counts=None, dl=None)
    a.update(kw)
    return _lib.load().bdn_criterion_soft(a['logits'], a['labels'], a['targets'], a['weights'], a['ignore'], a['smoothing'], a['w_o'],
                                          a['alpha'], a['beta'], a['eps'], a['reduce'], a['w_f'], a['gamma'], a['calpha'], a['sa'], a['ws'],
                                          a['loss'], a['terms'], a['counts'], a['dl'], 2, 2, 4, 4, None)


def test_c_abi_argument_errors_come_before_any_launch():
    lib = _lib.load()
    E_ARG = -1
    cases = [dict(labels=None), dict(targets=4096 * 9), dict(smoothing=-0.1), dict(smoothing=1.0), dict(smoothing=float('nan')),
             dict(labels=None, targets=12288, smoothing=0.1), dict(ignore=-2), dict(ignore=256),
             dict(labels=None, targets=12288, ignore=255), dict(w_o=0.0, w_f=0.0), dict(w_o=-1.0), dict(ws=None), dict(loss=None),
             dict(logits=None), dict(ws=16392), dict(logits=4098), dict(weights=12290), dict(dl=24578), dict(loss=20482),
             dict(terms=28674), dict(counts=28674), dict(labels=None, targets=12290)]
    for kw in cases:
        assert _soft(**kw) == E_ARG, kw
        assert b'criterion_soft' in lib.bdn_last_error()
    assert lib.bdn_criterion_soft_workspace_bytes(2, 1, 4, 4, 0) == 0 and lib.bdn_criterion_soft_workspace_bytes(2, 9, 4, 4, 0) == 0
    assert lib.bdn_criterion_soft_workspace_bytes(1 << 11, 2, 1 << 10, 1 << 10, 0) == 0
    assert lib.bdn_criterion_soft_workspace_bytes(64, 2, 128, 128, 0) == lib.bdn_criterion_masked_workspace_bytes(64, 2, 128, 128, 0)


# ------------------------------------------------------------------ train.py
def test_train_cli_label_smoothing_flag(tmp_path):
    from fabric_amd import train
    assert train.resolve_label_smoothing(None, False, None) == 0.0
    assert train.resolve_label_smoothing(0.0, False, 0.25) == 0.0                    # the default value asks for nothing
    assert train.resolve_label_smoothing(0.1, True, None) == 0.1
    assert train.resolve_label_smoothing(None, True, None, checkpoint=0.05) == 0.05  # --resume keeps the run's value ...
    assert train.resolve_label_smoothing(0.2, True, None, checkpoint=0.05) == 0.2    # ... unless the flag is given again
    with pytest.raises(ValueError, match='add --fused_step true'):
        train.resolve_label_smoothing(0.1, False, None)
    with pytest.raises(ValueError, match='ranks a hard-label focal term'):
        train.resolve_label_smoothing(0.1, True, 0.25)
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match=r'a number in \[0, 1\)'):
            train.resolve_label_smoothing(bad, True, None)
    with pytest.raises(SystemExit, match='add --fused_step true'):
        train.main(['--synthetic', '--label_smoothing', '0.1'])
    with pytest.raises(SystemExit, match='ranks a hard-label focal term'):
        train.main(['--synthetic', '--fused_step', 'true', '--loss_function', 'focal+dice', '--focal_gamma', '2', '--loss_topk', '0.25',
                    '--label_smoothing', '0.1'])
    with pytest.raises(SystemExit, match=r'a number in \[0, 1\)'):
        train.main(['--synthetic', '--fused_step', 'true', '--label_smoothing', '1.0'])
    (tmp_path / 'metadata_epoch_3.json').write_text(json.dumps({'label_smoothing': 0.05}))
    assert train.checkpoint_label_smoothing(str(tmp_path / 'checkpoint_epoch_3.state_dict.pt')) == 0.05
    assert train.checkpoint_label_smoothing(str(tmp_path / 'checkpoint_epoch_4.state_dict.pt')) is None
    from fabric_amd.utils.helpers import criterion_from_opt
    import argparse
    assert criterion_from_opt(argparse.Namespace(loss_function='dice', label_smoothing=0.1)).label_smoothing == 0.1
    assert criterion_from_opt(argparse.Namespace(loss_function='dice')).label_smoothing == 0.0
