"""-m gpu: bdn_shift_corr / bdn_shift_peak / bdn_shift_apply (include/bidate_hip.h; fabric_amd.utils.registration) through the C ABI on
guard-banded buffers, with a workspace of exactly the queried size born as 0xFF (NaN), against tests/register_ref.py.

The table: every entry within (n - 1) 2^-53 sum |term| of the correctly rounded exact sum (the bound for adding n exact terms in any
order), the counts equal.  The peak: fed the kernel's own table, the reference must give the same integer shift, ok and field, and dy, dx,
ncc bit for bit.  The resampling: bit for bit.

Shapes: as small as the kernel can still go wrong at -- one pixel (every shift undefined), fewer rows than the radius, odd sizes below one
32 x 32 tile, uneven cells, sizes that straddle the tile in both axes with more than one tile per cell and more partial accumulators than
tiles (97 x 131: 20 tiles, 1024 partials per band), the largest radius (five shifts per thread), a band subset of a 13-band stack."""
import functools
import json

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import registration as RG
from gpu_util import dev, st
from tests import guard
from tests import register_ref as RR
from tests.guard import guarded

pytestmark = pytest.mark.gpu

#        C   H    W    R  cells   bands
CASES = [(1, 1, 1, 1, (1, 1), None),
         (1, 3, 40, 4, (1, 1), None),
         (1, 5, 7, 2, (1, 1), None),
         (3, 33, 65, 4, (2, 3), None),
         (2, 97, 131, 8, (1, 1), None),
         (2, 97, 131, 8, (3, 2), None),
         (1, 40, 48, 16, (1, 1), None),
         (13, 150, 130, 8, (1, 1), [11, 0, 7, 3])]
EXV = 9


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def _case(i, holes):
    """(d1, d2, exclude or None, bands, reference table, sums of |terms|).  Shared: never modified.  date 2 is date 1 moved by (1, -1)
    (where the scene is large enough), scaled, plus noise: a clear peak for the peak tests."""
    C, H, W, R, cells, bands = CASES[i]
    r = np.random.default_rng(1000 + i)
    d1 = r.standard_normal((C, H, W)).astype(np.float32)
    t = (1, -1) if H > 4 else (0, 1 if W > 4 else 0)
    d2 = (RR.shift_bilinear(d1, *t) * np.float32(1.3) + np.float32(0.2) + np.float32(0.3) * r.standard_normal((C, H, W)).astype(np.float32))
    d2 = d2.astype(np.float32)
    ex = None
    if holes:
        ex = np.where(r.random((H, W)) < 0.05, EXV, 0).astype(np.uint8)
        for d in (d1, d2):
            k = max(1, d.size // 50)
            d.reshape(-1)[r.choice(d.size, k, replace=False)] = r.choice([np.nan, np.inf, -np.inf], k)
    bands = list(range(C)) if bands is None else bands
    table, sabs = RR.table_ref(d1, d2, bands, R, cells[0], cells[1], ex, EXV)
    return d1, d2, ex, bands, table, sabs


def _corr(d1_d, d2_d, bands, R, cells, ex_d=None, stream=None):
    C, H, W = d1_d.shape
    nb, S = len(bands), 2 * R + 1
    bands_d = dev(torch.tensor(bands), torch.int32)
    table = guard.empty(nb, cells[0], cells[1], S, S, 6, dtype=torch.float64)
    ws = guard.alloc_bytes(_lib.load().bdn_shift_corr_workspace_bytes(nb, H, W, R, cells[0], cells[1]), label='shift_corr workspace')
    _lib.call('bdn_shift_corr', d1_d.data_ptr(), d2_d.data_ptr(), bands_d.data_ptr(), nb, _lib.ptr(ex_d), EXV if ex_d is not None else 0,
              R, cells[0], cells[1], table.data_ptr(), ws.data_ptr(), C, H, W, st() if stream is None else stream)
    return table


def _peak(table_d, R, min_ncc=0.0):
    nb, ny, nx = table_d.shape[:3]
    report = guard.empty(ny * nx + 1, 4, dtype=torch.float64)
    field = guard.empty(ny, nx, 2)
    _lib.call('bdn_shift_peak', table_d.data_ptr(), nb, R, ny, nx, float(min_ncc), report.data_ptr(), field.data_ptr(), st())
    return report, field


def _device_case(i, holes):
    d1, d2, ex, bands, table, sabs = _case(i, holes)
    return dev(torch.from_numpy(d1)), dev(torch.from_numpy(d2)), None if ex is None else dev(torch.from_numpy(ex), torch.uint8)


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize('holes', [False, True], ids=['plain', 'exclude+nonfinite'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=[f'{c[0]}x{c[1]}x{c[2]}-R{c[3]}-{c[4][0]}x{c[4][1]}' for c in CASES])
@guarded
def test_table_is_within_the_summation_bound_and_the_same_on_every_run(i, holes):
    C, H, W, R, cells, _ = CASES[i]
    d1, d2, ex, bands, ref, sabs = _case(i, holes)
    d1_d, d2_d, ex_d = _device_case(i, holes)
    got_d = _corr(d1_d, d2_d, bands, R, cells, ex_d)
    got = got_d.cpu().numpy()
    assert np.array_equal(got[..., 0], ref[..., 0]), 'the counts'
    n = ref[..., :1]
    bound = np.maximum(n - 1, 0) * 2.0 ** -53 * sabs
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
    print(f'table {CASES[i]} holes={holes}: largest error / bound = {worst:.3g}')
    assert np.isfinite(got).all() and (err <= bound).all(), (CASES[i], holes, worst)
    if holes:
        assert (ref[..., 0] < _case(i, False)[4][..., 0]).any(), "the holes take pixels out"
    # the same bits from a second NaN-born workspace, and on a side stream
    again = _corr(d1_d, d2_d, bands, R, cells, ex_d)
    assert torch.equal(got_d.view(torch.int64), again.view(torch.int64)), 'second run'
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _corr(d1_d, d2_d, bands, R, cells, ex_d, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(got_d.view(torch.int64), other.view(torch.int64)), 'side stream'


def test_an_undefined_scene_and_short_scenes():
    """The conditions the first two rows of the table stand for, on the reference."""
    _, _, _, _, t0, _ = _case(0, False)
    assert t0.shape == (1, 1, 1, 3, 3, 6) and t0[0, 0, 0, 1, 1, 0] == 1 and t0[..., 0].sum() == 1
    rep, field, _ = RR.report_ref(t0, 1)
    assert rep[-1].tolist() == [0.0, 0.0, -2.0, 0.0] and not field.any()
    _, _, _, _, t1, _ = _case(1, False)
    assert not t1[0, 0, 0, [0, 1, 7, 8], :, 0].any() and t1[0, 0, 0, 2, 4, 0] == 40      # |dy| >= 3 leaves the 3-row scene


# ---------------------------------------------------------------- the peak
@pytest.mark.parametrize('holes', [False, True], ids=['plain', 'exclude+nonfinite'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=[f'{c[0]}x{c[1]}x{c[2]}-R{c[3]}-{c[4][0]}x{c[4][1]}' for c in CASES])
@guarded
def test_peak_reproduces_the_reference_from_the_kernels_table(i, holes):
    C, H, W, R, cells, _ = CASES[i]
    d1, d2, ex, bands, ref_table, _ = _case(i, holes)
    # conditions of the test, on the CPU: no near-tie between the best two scores, no flat parabola
    _, _, ref_scores = RR.report_ref(ref_table, R)
    for sc in ref_scores:
        if (sc > -2).sum() > 1:
            gap, curv = RR.peak_margins(sc, R)
            assert gap > 1e-6 and (curv is None or curv >= 1e-3), (CASES[i], holes, gap, curv)
    d1_d, d2_d, ex_d = _device_case(i, holes)
    table_d = _corr(d1_d, d2_d, bands, R, cells, ex_d)
    report_d, field_d = _peak(table_d, R)
    table, report, field = table_d.cpu().numpy(), report_d.cpu().numpy(), field_d.cpu().numpy()
    want, want_field, _ = RR.report_ref(table, R)
    diff = float(np.abs(report - want).max())
    print(f'peak {CASES[i]} holes={holes}: largest |report - reference| = {diff:.3g}')
    assert np.array_equal(np.rint(report[:, :2]), np.rint(want[:, :2])) and np.array_equal(report[:, 3], want[:, 3])
    assert np.array_equal(_bits(report), _bits(want)), diff
    assert np.array_equal(_bits(field), _bits(want_field))
    if H > 4:
        assert report[-1, 3] == 1 and (round(report[-1, 0]), round(report[-1, 1])) == (-1, 1)
    if (H, W) == (1, 1):
        assert report.tolist() == [[0.0, 0.0, -2.0, 0.0]] * 2 and not field.any()


@guarded
def test_cells_below_min_ncc_and_cells_of_nodata_take_the_whole_scene_shift():
    r = np.random.default_rng(7)
    d1 = r.standard_normal((2, 64, 80)).astype(np.float32)
    d2 = (RR.shift_bilinear(d1, 2, -1) + np.float32(0.2) * r.standard_normal(d1.shape).astype(np.float32)).astype(np.float32)
    d2[:, :32, :40] = r.standard_normal((2, 32, 40)).astype(np.float32)       # cell (0, 0): unrelated
    d1[:, 32:, 40:] = np.nan                                                  # cell (1, 1): nodata
    d1_d, d2_d = dev(torch.from_numpy(d1)), dev(torch.from_numpy(d2))
    table_d = _corr(d1_d, d2_d, [0, 1], 3, (2, 2))
    table = table_d.cpu().numpy()
    assert not table[:, 1, 1].any()
    for min_ncc in (0.0, 0.5, 1.0):
        report_d, field_d = _peak(table_d, 3, min_ncc)
        report, field = report_d.cpu().numpy(), field_d.cpu().numpy()
        want, want_field, _ = RR.report_ref(table, 3, min_ncc)
        assert np.array_equal(_bits(report), _bits(want)) and np.array_equal(_bits(field), _bits(want_field)), min_ncc
        g = report[-1, :2].astype(np.float32)
        assert report[3].tolist() == [0.0, 0.0, -2.0, 0.0] and np.array_equal(field[1, 1], g)
        assert report[0, 2] < 0.5 < report[1, 2] and (round(report[-1, 0]), round(report[-1, 1])) == (-2, 1)
        assert np.array_equal(field[0, 0], g) == (min_ncc > 0) and np.array_equal(field[0, 1], g) == (min_ncc == 1.0)
    # nothing defined anywhere: every cell and the scene report ok = 0 and the field is zero
    nan_d = guard.full((2, 64, 80), float('nan'))
    report_d, field_d = _peak(_corr(nan_d, d2_d, [0, 1], 3, (2, 2)), 3, 0.5)
    assert report_d.cpu().tolist() == [[0.0, 0.0, -2.0, 0.0]] * 5 and not field_d.cpu().any()


# ---------------------------------------------------------------- the resampling
def _fields(h, w):
    r = np.random.default_rng(h * 1000 + w)
    out = {'zero': np.zeros((1, 1, 2), np.float32), 'integer': np.array([[[2, -3]]], np.float32), 'fraction': np.array([[[-1.25, 0.7]]], np.float32),
           'beyond': np.array([[[1000.5, -2000.25]]], np.float32), 'far beyond': np.array([[[3e9, -3e9]]], np.float32)}
    if h >= 3 and w >= 2:
        out['3x2'] = (r.uniform(-3, 3, (3, 2, 2))).astype(np.float32)
        out['3x2 integer'] = np.rint(out['3x2']).astype(np.float32)
    return out


@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (33, 65), (97, 131)])
@guarded
def test_apply_is_the_reference_bit_for_bit(shape):
    h, w = shape
    src = np.random.default_rng(h).standard_normal((3, h, w)).astype(np.float32)
    src_d = dev(torch.from_numpy(src))
    for name, f in _fields(h, w).items():
        out_d, oob_d = guard.empty(3, h, w), guard.empty(h, w, dtype=torch.uint8)
        f_d = dev(torch.from_numpy(f))
        _lib.call('bdn_shift_apply', src_d.data_ptr(), f_d.data_ptr(), f.shape[0], f.shape[1], out_d.data_ptr(), oob_d.data_ptr(), 3, h, w, st())
        want, want_oob = RR.apply_ref(src, f)
        out, oob = out_d.cpu().numpy(), oob_d.cpu().numpy()
        assert np.array_equal(_bits(out), _bits(want)), (shape, name, int((_bits(out) != _bits(want)).sum()))
        assert np.array_equal(oob, want_oob), (shape, name)
        if name == 'zero':
            assert np.array_equal(_bits(out), _bits(src)) and not oob.any()
        if name == 'integer':
            assert np.array_equal(_bits(out), _bits(src[:, np.clip(np.arange(h) + 2, 0, h - 1)][:, :, np.clip(np.arange(w) - 3, 0, w - 1)]))
        if name.endswith('beyond'):
            assert oob.all() and np.array_equal(_bits(out), _bits(np.broadcast_to(src[:, -1:, :1], src.shape)))
        out2_d = guard.empty(3, h, w)                        # oob = NULL: the same image
        _lib.call('bdn_shift_apply', src_d.data_ptr(), f_d.data_ptr(), f.shape[0], f.shape[1], out2_d.data_ptr(), None, 3, h, w, st())
        assert torch.equal(out_d.view(torch.int32), out2_d.view(torch.int32))


# ---------------------------------------------------------------- round trip with the warp kernel
@pytest.mark.parametrize('t', [(0, 0), (2, -3), (-4, 1)])
def test_estimate_recovers_the_translation_the_warp_kernel_applied(t):
    """One pair cut by bdn_sample_patches_warp from a city whose two dates are the same image, with override records that translate date 2
    by t: the estimate is -t (the peak exactly; the parabola through the noise beside a peak of exactly 1 moves it by thousandths)."""
    from fabric_amd.augment import PatchAugment, PatchWarp
    C, H, W, S = 2, 80, 90, 64
    img = np.random.default_rng(11).standard_normal((C, H, W)).astype(np.float32)
    with guard.checked(name='warp cut'):
        images = dev(torch.from_numpy(np.stack([img, img])))
        labels = guard.zeros(H, W, dtype=torch.uint8)
        city = guard.guard(torch.from_numpy(np.array([[images.data_ptr(), labels.data_ptr(), H | (W << 32)]], np.int64)))
        hw, desc = np.array([[H, W]], np.int32), np.array([[0, 8, 10, 0]], np.int32)
        rec = np.array([[[1, 0, 0, 0, 1, 0], [1, 0, t[0], 0, 1, t[1]]]], np.float32)
        desc_d, rec_d = guard.guard(torch.from_numpy(desc)), guard.guard(torch.from_numpy(rec))
        keys_d = guard.zeros(1, dtype=torch.int64)
        o1, o2, ol = guard.empty(1, C, S, S), guard.empty(1, C, S, S), guard.empty(1, S, S, dtype=torch.uint8)
        pol, warp = PatchAugment(seed=0, jitter=0, symmetry=False), PatchWarp()
        _lib.call('bdn_sample_patches_warp', city.data_ptr(), _lib.host_int32(hw), 1, C, _lib.host_int32(desc), desc_d.data_ptr(), 1, S,
                  o1.data_ptr(), o2.data_ptr(), ol.data_ptr(), keys_d.data_ptr(), *pol.abi_args(), None, None, *warp.abi_args(),
                  _lib.host_float32(rec), rec_d.data_ptr(), None, st())
        d1, d2 = o1[0].clone(), o2[0].clone()
    assert np.array_equal(d1.cpu().numpy(), img[:, 8:72, 10:74]) and np.array_equal(d2.cpu().numpy(), img[:, 8 + t[0]:72 + t[0], 10 + t[1]:74 + t[1]])
    est = RG.estimate_shift(d1.contiguous(), d2.contiguous(), max_shift=4).read()
    assert est['ok'] and est['ncc'] == 1.0 and est['cells_ok'] == 1
    assert (round(est['dy']), round(est['dx'])) == (-t[0], -t[1]) and abs(est['dy'] + t[0]) < 0.02 and abs(est['dx'] + t[1]) < 0.02
    if abs(t[0]) == 4:
        assert est['dy'] == -t[0]                            # on the window border: no parabola


# ---------------------------------------------------------------- end to end
def _cities(misreg):
    from fabric_amd.utils.dataloaders import synthetic_onera
    return synthetic_onera(n_cities=2, bands=4, size=(96, 110), seed=2, misreg=misreg)


def test_coregister_removes_an_integer_misregistration():
    data = _cities((2, -1))
    d1, d2 = (torch.from_numpy(data['city0']['images'][k]).cuda() for k in range(2))
    keep = d2.clone()
    oob = torch.empty(96, 110, dtype=torch.uint8, device='cuda')
    aligned, est = RG.coregister(d1, d2, max_shift=4, cells=(2, 2), oob=oob)
    rep = est.read()
    assert rep['ok'] and (round(rep['dy']), round(rep['dx'])) == (-2, 1) and rep['cells_ok'] == 4 and rep['ncc'] > 0.8
    assert torch.equal(d2, keep) and aligned.data_ptr() != d2.data_ptr()
    again = RG.estimate_shift(d1, aligned, max_shift=4).read()
    # the first estimate is -t plus a few thousandths of a pixel (the parabola through noise); so is what is left
    assert (round(again['dy']), round(again['dx'])) == (0, 0) and abs(again['dy']) < 0.02 and abs(again['dx']) < 0.02
    o = oob.cpu().numpy()
    assert o[:2].all() and o[:, -1:].all() and not o[3:, :-2].any()
    want, want_oob = RR.apply_ref(data['city0']['images'][1], rep['field'])
    assert np.array_equal(_bits(aligned.cpu().numpy()), _bits(want)) and np.array_equal(o, want_oob)


@pytest.mark.parametrize('on_device', [False, True])
def test_coregister_cities_aligns_date_2_in_place_and_nothing_else(on_device):
    data, clean = _cities((-1, 3)), _cities((0, 0))
    before = {c: {k: v.copy() for k, v in d.items()} for c, d in data.items()}
    if on_device:
        data = {c: {'images': torch.from_numpy(d['images']).cuda(), 'labels': torch.from_numpy(d['labels']).cuda()} for c, d in data.items()}
    reports = RG.coregister_cities(data, max_shift=4)
    assert list(reports) == list(data)
    for c, d in data.items():
        assert torch.is_tensor(d['images']) == on_device
        images, labels = (d[k].cpu().numpy() if on_device else d[k] for k in ('images', 'labels'))
        assert np.array_equal(_bits(images[0]), _bits(before[c]['images'][0])) and np.array_equal(labels, before[c]['labels'])
        assert (round(reports[c]['dy']), round(reports[c]['dx'])) == (1, -3)
        inner = (slice(None), slice(2, -2), slice(4, -4))
        assert np.abs(images[1][inner] - clean[c]['images'][1][inner]).max() < 0.1 < np.abs(before[c]['images'][1][inner] - clean[c]['images'][1][inner]).max()
    # with an ignore label: the label pixels whose date-2 taps left the scene take it, the others stay
    data = _cities((-1, 3))
    RG.coregister_cities(data, max_shift=4, ignore_label=255)
    for c, d in data.items():
        changed = d['labels'] != before[c]['labels']
        assert changed.any() and (d['labels'][changed] == 255).all() and not changed[2:-2, 4:-4].any()


def test_cli_aligns_logs_and_records_the_settings(tmp_path, capsys):
    from fabric_amd import train as T
    T.main(['--synthetic', '--synthetic_misreg', '2', '-1', '--coregister', '4', '--epochs', '1', '--batch_size', '8', '--patch_size', '64',
            '--stride', '128', '--num_workers', '0', '--log_dir', str(tmp_path)])
    lines = capsys.readouterr().out.strip().splitlines()
    coreg = [json.loads(ln[len('coreg '):]) for ln in lines if ln.startswith('coreg ')]
    assert [c['city'] for c in coreg] == [f'city{k}' for k in range(6)]
    for c in coreg:
        assert set(c) == {'city', 'dy', 'dx', 'ncc', 'cells_ok'} and (round(c['dy']), round(c['dx'])) == (-2, 1)
        assert abs(c['dy'] + 2) < 0.02 and abs(c['dx'] - 1) < 0.02 and c['cells_ok'] == 1 and c['ncc'] > 0.8
    assert json.loads(lines[-1])['epoch'] == 0
    meta = json.load(open(tmp_path / 'metadata_epoch_0.json'))
    assert meta['coregister'] == {'max_shift': 4, 'cells': [1, 1], 'bands': None, 'min_ncc': 0.0}


def test_cli_without_the_flags_does_what_it_did(tmp_path, capsys, monkeypatch):
    """At their defaults the flags add no call: no alignment, synthetic_onera called as before, no new metadata key."""
    from fabric_amd import train as T
    seen = []
    real = T.synthetic_onera
    monkeypatch.setattr(T, 'synthetic_onera', lambda **kw: seen.append(kw) or real(**kw))
    monkeypatch.setattr(T, 'coregister_loaded', lambda *a, **k: pytest.fail('alignment ran without --coregister'))
    T.main(['--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64', '--stride', '128', '--num_workers', '0',
            '--log_dir', str(tmp_path)])
    out = capsys.readouterr().out
    assert seen == [dict(n_cities=6, bands=13, size=(360, 360))] and 'coreg' not in out
    assert 'coregister' not in json.load(open(tmp_path / 'metadata_epoch_0.json'))
