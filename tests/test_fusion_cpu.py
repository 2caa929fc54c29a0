"""CPU tests of the date-fusion option (fusion='product' | 'absdiff'): the float64 reference the GPU tests lean on (tests/fusion_ref.py) is
pinned to oracle.bidate_forward first, then its 'absdiff' properties (date symmetry, zero gradient at equal features), then the public
surface that needs no device: constructor validation, pickles from before the attribute, the CLI flag, the checkpoint-metadata round trip
and the C entry points' argument checks."""
import ctypes
import io
import json
import os
import pickle

import pytest
import torch

from fabric_amd import BiDateNet, _lib
from oracle import bidate_oracle as O
from oracle import filler
from tests import fusion_ref as R


def _case(b=2, c=3, s=16, seed=0, different=True):
    x1, x2, lbl = filler.make_inputs(b, c, s, seed=seed, different_dates=different)
    sd = {k: v.clone() for k, v in filler.fill_module(BiDateNet(c, 2)).state_dict().items()}
    return sd, torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(lbl)


@pytest.mark.parametrize('training', [True, False])
def test_product_recomposition_is_the_oracle_bit_for_bit(training):
    sd, x1, x2, _ = _case()
    want, want_buf = O.bidate_forward(sd, x1, x2, training=training)
    got, got_buf = R.forward(sd, x1, x2, 'product', training=training)
    assert torch.equal(got, want)
    assert set(got_buf) == set(want_buf) and all(torch.equal(got_buf[k], want_buf[k]) for k in want_buf)


def test_product_step_is_the_oracle_step_in_float64():
    """R.step is O.train_step's graph in float64: against the float32 oracle the loss and gradients agree to float32 rounding."""
    sd, x1, x2, lbl = _case()
    ref = O.train_step(sd, x1, x2, lbl, lr=1e-3)
    got = R.step(sd, x1, x2, lbl, 'product', lr=1e-3)
    assert abs(float(got['loss']) - float(ref['loss'])) < 1e-5
    for k, g in ref['grads'].items():
        if float(g.norm()) > 1e-6:
            assert float((got['grads'][k].float() - g).norm() / g.norm()) < 2e-2, k


@pytest.mark.parametrize('training', [True, False])
def test_absdiff_is_symmetric_in_the_dates(training):
    sd, x1, x2, _ = _case()
    a, _ = R.forward(sd, x1, x2, 'absdiff', training=training)
    b, _ = R.forward(sd, x2, x1, 'absdiff', training=training)
    assert torch.equal(a, b)
    p, _ = R.forward(sd, x1, x2, 'product', training=training)
    assert not torch.equal(a, p)


def test_absdiff_gradient_is_zero_at_equal_features():
    """torch.abs's rule: d|x|/dx = 0 at 0.  Identical dates give identical features (running statistics), every skip is exactly 0 and
    nothing reaches the encoder."""
    sd, x1, _, lbl = _case()
    logits, _, skips = R.forward(R.to_f64(sd), x1.double(), x1.double(), 'absdiff', training=False, return_skips=True)
    assert all(bool((f == 0).all()) for f in skips)
    out = R.step(sd, x1, x1, lbl, 'absdiff', training=False, input_grads=True)
    for k, g in out['grads'].items():
        if k.startswith(('inc', 'down')):
            assert bool((g == 0).all()), k
    assert bool((out['dx1'] == 0).all()) and bool((out['dx2'] == 0).all())
    assert any(float(g.abs().max()) > 0 for k, g in out['grads'].items() if k.startswith('up'))


def test_kernel_contract_restatements():
    a = torch.tensor([0.0, 0.0, 1.5, 0.25, 2.0, 2.0]).reshape(2, 3, 1, 1)           # date 1: 0, 0, 1.5; date 2: 0.25, 2, 2
    dF = torch.tensor([1.0, -3.0, 0.5]).reshape(1, 3, 1, 1)
    assert R.fuse_ref(a, 1, 'absdiff').flatten().tolist() == [0.25, 2.0, 0.5]
    assert R.fuse_ref(a, 1, 'product').flatten().tolist() == [0.0, 0.0, 3.0]
    part, pool = R.enc_skip_bwd_ref(a, dF, None, 1, 'absdiff')
    assert part.flatten().tolist() == [-1.0, 3.0, -0.5, 1.0, -3.0, 0.5] and not pool.any()
    tie = torch.tensor([0.0, 0.75, 0.0, 0.75]).reshape(2, 2, 1, 1)                   # both-dead ReLUs and a live tie
    part, _ = R.enc_skip_bwd_ref(tie, torch.ones(1, 2, 1, 1), None, 1, 'absdiff')
    assert bool((part == 0).all())
    hi, lo = R.split_hi_lo(torch.tensor([1.0 + 2.0 ** -10]))
    assert float(hi) == 1.0 and float(lo) == 2.0 ** -10


# ---------------------------------------------------------------- public surface
def test_constructor_validates_fusion():
    with pytest.raises(ValueError, match='fusion'):
        BiDateNet(13, 2, fusion='xor')
    assert BiDateNet(13, 2).fusion == 'product'
    m = BiDateNet(13, 2, fusion='absdiff')
    assert m.fusion == 'absdiff'
    assert list(m.state_dict()) == list(BiDateNet(13, 2).state_dict())              # no parameters: the same schema
    eng = m.engine()
    assert eng.fusion == 'absdiff' and eng.fm == _lib.FUSE_ABSDIFF
    m.fusion = 'product'                                                             # rebuilt at the next call, as precision is
    assert m.engine() is not eng and m.engine().fusion == 'product'
    m.fusion = 'xor'
    with pytest.raises(ValueError, match='fusion'):
        m.engine()


def test_pickle_without_the_attribute_is_product(monkeypatch):
    from fabric_amd.models.bidate_model import BiDateNet as B
    m = BiDateNet(3, 2, fusion='absdiff')
    assert pickle.loads(pickle.dumps(m)).fusion == 'absdiff'
    monkeypatch.setattr(B, '__getstate__', lambda self: {k: v for k, v in self.__dict__.items() if k not in ('fusion', '_engine')})
    blob = pickle.dumps(m)
    monkeypatch.undo()
    old = pickle.loads(blob)
    assert old.fusion == 'product' and old._engine is None


def test_load_model_reads_opt_fusion():
    from types import SimpleNamespace
    from fabric_amd.utils.helpers import load_model
    assert load_model(SimpleNamespace(), 'cpu').fusion == 'product'
    assert load_model(SimpleNamespace(fusion='absdiff'), 'cpu').fusion == 'absdiff'


def test_cli_flag_and_resolution():
    from fabric_amd import train
    with pytest.raises(SystemExit):
        train.main(['--synthetic', '--fusion', 'xor'])
    with pytest.raises(SystemExit, match='give one of them'):                        # the flag parses; the run stops at the next host check
        train.main(['--synthetic', '--fusion', 'absdiff', '--init_from', 'a.pt', '--resume', 'b.pt'])
    rf = train.resolve_fusion
    assert rf(None) == ('product', None) and rf('absdiff') == ('absdiff', None)
    assert rf(None, 'absdiff', resume=True) == ('absdiff', None)                     # --resume restores it
    assert rf(None, 'absdiff') == ('absdiff', None)                                  # --init_from takes it unless the flag is given
    fusion, note = rf('absdiff', 'product')
    assert fusion == 'absdiff' and 'product' in note and 'absdiff' in note and '\n' not in note
    assert rf('product', 'product', resume=True) == ('product', None)
    with pytest.raises(ValueError, match='--resume'):
        rf('product', 'absdiff', resume=True)


def test_checkpoint_metadata_round_trip(tmp_path):
    from fabric_amd import train
    from fabric_amd.utils.helpers import checkpoint_fusion, load_checkpoint
    model = filler.fill_module(BiDateNet(3, 2, fusion='absdiff'))
    better = {'cd_precisions': 0.5, 'cd_recalls': 0.5, 'cd_f1scores': 0.5, 'cd_losses': 1.0, 'cd_corrects': 50.0}
    best = {'cd_f1scores': -1, 'cd_recalls': -1, 'cd_precisions': -1}
    train.save_if_better(model, better, best, {'precision': 'fp32', 'fusion': model.fusion}, 3, str(tmp_path))
    assert json.load(open(tmp_path / 'metadata_epoch_3.json'))['fusion'] == 'absdiff'
    sd_path = str(tmp_path / 'checkpoint_epoch_3.state_dict.pt')
    assert checkpoint_fusion(sd_path) == 'absdiff'
    assert load_checkpoint(sd_path).fusion == 'absdiff'                              # from the metadata beside the file
    assert load_checkpoint(str(tmp_path / 'checkpoint_epoch_3.pt')).fusion == 'absdiff'
    assert load_checkpoint(sd_path, fusion='product').fusion == 'product'            # an explicit argument wins
    got, _, first = train.resume_from(sd_path)
    assert got.fusion == 'absdiff' and first == 4
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in got.state_dict().items())
    # a state dict with no metadata beside it, and a pickle alone: 'product' and the attribute
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    assert load_checkpoint(io.BytesIO(buf.getvalue())).fusion == 'product'
    os.remove(tmp_path / 'metadata_epoch_3.json')
    assert checkpoint_fusion(sd_path) is None and load_checkpoint(sd_path).fusion == 'product'
    assert load_checkpoint(str(tmp_path / 'checkpoint_epoch_3.pt')).fusion == 'absdiff'


# ---------------------------------------------------------------- C ABI
NEW = ('bdn_fuse_dates', 'bdn_fuse_dates_pool', 'bdn_fuse_dates_pool_split', 'bdn_enc_skip_bwd_fusion', 'bdn_conv3x3_eval_fusion',
       'bdn_conv3x3_eval_pair_fusion')
OLD = ('bdn_fuse_product', 'bdn_product_pool', 'bdn_product_pool_split', 'bdn_enc_skip_bwd', 'bdn_conv3x3_eval', 'bdn_conv3x3_eval_pair')


def test_new_entry_points_are_the_old_ones_plus_the_mode():
    assert (_lib.FUSE_PRODUCT, _lib.FUSE_ABSDIFF) == (0, 1) and _lib.FUSIONS == {'product': 0, 'absdiff': 1}
    for new, old in zip(NEW, OLD):
        res, args = _lib.SIGNATURES[new]
        ores, oargs = _lib.SIGNATURES[old]
        at = 0 if new == 'bdn_fuse_dates_pool_split' else 1                          # behind dtype, where there is one
        assert res is ctypes.c_int and args[at] is ctypes.c_int and args[:at] + args[at + 1:] == oargs, new


def test_bad_mode_is_refused_before_anything_touches_a_device():
    p = 4096                                                                         # fake non-null pointers: never dereferenced
    calls = {
        'bdn_fuse_dates': (0, 2, p, p, p, 1, 4, 4, 64, None),
        'bdn_fuse_dates_pool': (0, 2, p, p, p, p, 1, 4, 4, 64, None),
        'bdn_fuse_dates_pool_split': (-1, p, p, p, 128, 64, p, 1, 4, 4, 64, None),
        'bdn_enc_skip_bwd_fusion': (0, 7, p, 64, p, p, None, p, None, 1, 4, 4, 64, None),
        'bdn_conv3x3_eval_fusion': (0, 2, p, 64, None, 0, p, p, p, p, p, None, 2, 8, 8, 64, None),
        'bdn_conv3x3_eval_pair_fusion': (0, 2, p, 64, p, p, p, p, None, 1, 8, 8, 64, None),
    }
    assert set(calls) == set(NEW)
    for name, args in calls.items():
        with pytest.raises(RuntimeError, match='bad fusion mode'):
            _lib.call(name, *args)
    with pytest.raises(RuntimeError, match='null pointer'):
        _lib.call('bdn_fuse_dates', 0, 1, None, p, p, 1, 4, 4, 64, None)
    with pytest.raises(RuntimeError, match='bad shape'):
        _lib.call('bdn_enc_skip_bwd_fusion', 0, 1, p, 60, p, p, None, p, None, 1, 4, 4, 64, None)
