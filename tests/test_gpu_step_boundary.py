"""-m gpu: the fused train step with the boundary term (TrainStep(criterion=Criterion(..., w_boundary=))); tests/test_gpu_step_lovasz.py's
shapes.  The step's loss gradient is Criterion.evaluate on the step's logits, bit for bit, and the parameter gradients are those of
CompoundLoss through autograd on the module; w_boundary=0 is the step without the keyword; the weight is read per step; twin and
poisoned-allocation steps are the same bits."""
import pytest
import torch

from fabric_amd import BiDateNet
from fabric_amd.criterion import Criterion
from fabric_amd.train_step import TrainStep
from fabric_amd.utils.metrics import CompoundLoss
from oracle import filler
from tests import edt_ref as ER
from tests import stale

pytestmark = pytest.mark.gpu

dev = 'cuda'


def _inputs(b=2, c=3, s=32, seed=3, ignore=True):
    x1, x2, lbl = (torch.from_numpy(v) for v in filler.make_inputs(b, c, s, seed=seed))
    lbl = lbl.clone()
    if ignore:
        for i in range(b):
            lbl[i, 3 + 2 * i:15 + 3 * i, 5 * i:s // 2 + 4 * i] = 255
    return x1.to(dev), x2.to(dev), lbl.to(dev)


def _model():
    return filler.fill_module(BiDateNet(3, 2, precision='fp32')).to(dev).train()


def _grad_errors(got, ref):
    """tests/test_gpu_step_criterion.py's: worst per-parameter max(relative L2 error, relative error of the norm), cosine of the whole."""
    worst, worst_key, allg, allr = 0.0, None, [], []
    for k, r in ref.items():
        g, r = got[k].detach().cpu().double().reshape(-1), r.detach().cpu().double().reshape(-1)
        if float(r.norm()) < 1e-6:
            assert float(g.norm()) < 1e-6, k
            continue
        e = max(float((g - r).norm() / r.norm()), abs(float(g.norm()) - float(r.norm())) / float(r.norm()))
        allg.append(g)
        allr.append(r)
        if e > worst:
            worst, worst_key = e, k
    ag, ar = torch.cat(allg), torch.cat(allr)
    return worst, worst_key, float((ag * ar).sum() / (ag.norm() * ar.norm()))


def _criteria():
    return [('focal+dice+boundary', lambda: Criterion.parse('focal+dice', focal_gamma=2.0, w_boundary=0.05), None),
            ('boundary alone, all, ignore', lambda: Criterion(w_overlap=0.0, w_boundary=1.0, boundary_classes='all', ignore_index=255), 255),
            ('focal+lovasz+boundary clamp ignore', lambda: Criterion.parse('focal+lovasz', ignore_index=255, w_boundary=0.2, boundary_max_dist=4), 255),
            ('topk+boundary', lambda: Criterion.parse('focal+jaccard', focal_gamma=0.0, ignore_index=255, topk=0.5, w_boundary=0.1), 255)]


@pytest.mark.parametrize('name,crit,ignore', _criteria(), ids=[c[0] for c in _criteria()])
def test_step_runs_and_its_loss_gradient_is_the_criterion_on_its_logits(name, crit, ignore):
    x1, x2, lbl = _inputs(ignore=ignore is not None)
    ts = TrainStep(_model(), lr=0.0, criterion=crit())
    loss = ts.step(x1, x2, lbl)
    torch.cuda.synchronize()
    c = ts.criterion
    l2, terms, counts, dlogits = c.evaluate(ts.last_logits, lbl)
    assert torch.equal(ts.last_dlogits, dlogits) and torch.equal(ts.last_terms, terms) and torch.equal(ts.last_counts, counts)
    assert torch.equal(loss, l2) and torch.isfinite(loss) and ts.last_dlogits.any() and torch.isfinite(ts.flat_grads).all()
    if ignore is not None:
        assert not ts.last_dlogits[(lbl == 255)[:, None].expand(-1, 2, -1, -1)].any()
    # last_terms[-1] is the boundary value of the step's logits (the float64 restatement, the bar of tests/test_gpu_boundary.py)
    t64 = ER.boundary_loss_ref(ts.last_logits.cpu().numpy(), lbl.cpu().numpy().astype('uint8'), ignore, c.boundary_classes == 'all',
                               c.boundary_max_dist)[0]
    assert abs(ts.last_terms[-1].item() - t64) <= 5e-6 * max(1.0, abs(t64)) and t64 != 0.0
    # the autograd route: the module's own backward under CompoundLoss(criterion); the bars of tests/test_gpu_step_topk.py
    m = _model()
    mod = CompoundLoss(crit())
    v = mod(m(x1, x2), lbl)
    v.backward()
    torch.cuda.synchronize()
    ref = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    gerr, gkey, gcos = _grad_errors(ts.grads, ref)
    print(f'\n{name}: step loss {loss.item():.7f} autograd {v.item():.7f} worst grad err {gerr:.3e} @ {gkey} cos {gcos:.6f}')
    assert abs(loss.item() - v.item()) < 1e-5 * max(1.0, abs(v.item()))
    assert gerr < 2e-2 and gcos > 0.9999, (gkey, gerr, gcos)
    assert abs(mod.last_terms[-1].item() - ts.last_terms[-1].item()) <= 5e-6 * max(1.0, abs(t64))


def test_w_boundary_zero_is_the_step_without_the_keyword():
    x = _inputs()
    a = TrainStep(_model(), lr=1e-3, criterion=Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255))
    b = TrainStep(_model(), lr=1e-3, criterion=Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255, w_boundary=0.0))
    for _ in range(2):
        la, lb = a.step(*x), b.step(*x)
        torch.cuda.synchronize()
        stale.same_bits(dict(loss=la, terms=a.last_terms, counts=a.last_counts, dlogits=a.last_dlogits, grads=a.flat_grads, params=a.flat_params),
                        dict(loss=lb, terms=b.last_terms, counts=b.last_counts, dlogits=b.last_dlogits, grads=b.flat_grads, params=b.flat_params),
                        'w_boundary=0')
    assert 'boundary' not in repr(b.criterion)


def test_changing_the_weight_between_steps_equals_a_fresh_step_with_that_weight():
    x = _inputs()
    crit = lambda w: Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255, w_boundary=w)       # noqa: E731
    ts = TrainStep(_model(), lr=0.0, criterion=crit(0.01))
    ts.step(*x)
    ts.criterion.w_boundary = 0.5
    loss = ts.step(*x)
    fresh = TrainStep(_model(), lr=0.0, criterion=crit(0.5))
    want = fresh.step(*x)
    torch.cuda.synchronize()
    stale.same_bits(dict(loss=loss, terms=ts.last_terms, dlogits=ts.last_dlogits, grads=ts.flat_grads),
                    dict(loss=want, terms=fresh.last_terms, dlogits=fresh.last_dlogits, grads=fresh.flat_grads), 'ramped weight')


def test_twin_and_poisoned_allocation_steps_are_the_same_bits(monkeypatch):
    crit = lambda: Criterion.parse('focal+dice', focal_gamma=2.0, ignore_index=255, w_boundary=0.1, boundary_classes='all')       # noqa: E731
    x = _inputs()
    clean = TrainStep(_model(), lr=1e-3, criterion=crit())
    want = []
    for _ in range(2):
        loss = clean.step(*x)
        want.append(dict(loss=loss.clone(), terms=clean.last_terms.clone(), dlogits=clean.last_dlogits.clone(), params=clean.flat_params.clone()))
    with stale.poisoned_allocations(monkeypatch):           # every floating-point buffer the library allocates starts as NaN
        ts = TrainStep(_model(), lr=1e-3, criterion=crit())
        for i in range(2):
            loss = ts.step(*x)
            torch.cuda.synchronize()
            got = dict(loss=loss, terms=ts.last_terms, dlogits=ts.last_dlogits, params=ts.flat_params)
            stale.same_bits(got, want[i], f'poisoned allocation, step {i}')
            stale.all_finite(got, f'poisoned allocation, step {i}')


def test_train_main_runs_an_epoch_with_the_boundary_term_and_records_it(tmp_path, capsys):
    import json
    from fabric_amd import train as T
    T.main(['--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64', '--stride', '128', '--num_workers', '0', '--learning_rate',
            '0.02', '--fused_step', 'true', '--loss_function', 'focal+dice', '--focal_gamma', '2', '--boundary_weight', '0.01',
            '--boundary_classes', 'all', '--boundary_max_dist', '20', '--ignore_label', '255', '--log_dir', str(tmp_path)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['epoch'] == 0 and {'train_cd_losses', 'train_boundary_mean', 'validate_cd_f1scores', 'validate_cd_losses'} <= set(line)
    assert line['train_boundary_mean'] != 0.0 and abs(line['train_boundary_mean']) <= 20.0
    with pytest.raises(SystemExit):
        T.main(['--synthetic', '--loss_function', 'tversky', '--boundary_weight', '0.01'])              # without --fused_step true
