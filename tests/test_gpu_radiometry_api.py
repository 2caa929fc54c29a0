"""-m gpu: fabric_amd.utils.radiometry and its wiring into fabric_amd.train against the numpy twin (tests/radiometry_ref.py), bit for bit:
match_histograms, match_range, normalize_cities on device stacks and on numpy (date 1 and the labels untouched, ignore_label pixels left
out of the fit), stretch_8bit, and one training epoch with --radiometric range on synthetic cities whose date 2 is 1.3 x + 0.2."""
import json

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import radiometry as RM
from fabric_amd.utils.dataloaders import synthetic_onera
from tests import radiometry_ref as RR

pytestmark = pytest.mark.gpu
NEW = ('bdn_band_quantiles', 'bdn_transfer_apply', 'bdn_stretch_u8')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _pair(seed=0, shape=(5, 97, 131)):
    r = np.random.default_rng(seed)
    d1 = r.gamma(2.0, 1.0, shape).astype(np.float32)
    d2 = (np.float32(1.3) * np.sqrt(d1) + np.float32(0.2) + np.float32(0.05) * r.standard_normal(shape).astype(np.float32)).astype(np.float32)
    d2[0, 0, :3] = [np.nan, np.inf, -np.inf]
    d1[1, 5, 5] = np.nan
    d1[4] = np.nan                                           # a band without a valid pixel in date 1: date 2's band passes through
    return d1, d2


def test_band_quantiles_and_read():
    d1, _ = _pair()
    probs = [0.0, 0.02, 0.5, 0.98, 1.0]
    q = RM.band_quantiles(torch.from_numpy(d1).cuda(), probs, bands=[3, 1, 4])
    got, want = q.read(), RR.quantiles_ref(d1, probs, [3, 1, 4])
    assert np.array_equal(_bits(got['value']), _bits(want[0])) and np.array_equal(_bits(got['order']), _bits(want[1]))
    assert np.array_equal(got['count'], want[2]) and got['count'].tolist() == [97 * 131, 97 * 131 - 1, 0] and got['bands'] == [3, 1, 4]
    on_device = RM.band_quantiles(torch.from_numpy(d1).cuda(), torch.tensor(probs, dtype=torch.float64).cuda(), bands=[3, 1, 4])
    assert torch.equal(on_device.value.view(torch.int64), q.value.view(torch.int64))


@pytest.mark.parametrize('method', ['histogram', 'range'])
def test_match_against_the_twin(method):
    d1, d2 = _pair()
    ex = (np.random.default_rng(1).random((97, 131)) < 0.1).astype(np.uint8) * 255
    a, b, e = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda(), torch.from_numpy(ex).cuda()
    keep1, keep2 = a.clone(), b.clone()
    if method == 'histogram':
        out, tr = RM.match_histograms(b, a, knots=64, bands=[0, 2, 4], exclude=e, exclude_value=255)
        want, s, t, n = RR.match_ref(d2, d1, 'histogram', knots=64, bands=[0, 2, 4], exclude=ex, exclude_value=255)
    else:
        out, tr = RM.match_range(b, a, 0.05, 0.9, bands=[0, 2, 4], exclude=e, exclude_value=255)
        want, s, t, n = RR.match_ref(d2, d1, 'range', lower=0.05, upper=0.9, bands=[0, 2, 4], exclude=ex, exclude_value=255)
    rep = tr.read()
    assert np.array_equal(_bits(rep['src']), _bits(s)) and np.array_equal(_bits(rep['dst']), _bits(t)) and np.array_equal(rep['count'], n)
    assert rep['extrapolate'] == ('offset' if method == 'histogram' else 'slope') and rep['bands'] == [0, 2, 4] and n[1, 2] == 0
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert torch.equal(a.view(torch.int32), keep1.view(torch.int32)) and torch.equal(b.view(torch.int32), keep2.view(torch.int32))
    assert np.array_equal(_bits(got[[1, 3, 4]]), _bits(d2[[1, 3, 4]])) and (got[2] != d2[2]).mean() > 0.9
    again = RM.apply_transfer(b, tr, out=b)                  # in place
    assert again is b and torch.equal(b.view(torch.int32), out.view(torch.int32))
    # date 2 now has date 1's median, to the twin's value (band 2: every pixel finite)
    m2 = RM.band_quantiles(out, [0.5], bands=[2], exclude=e, exclude_value=255).read()['value'][0, 0]
    assert m2 == RR.quantiles_ref(want, [0.5], [2], ex, 255)[0][0, 0]
    if method == 'histogram':                                # p = 0.5 lies between two of the 64 knots, whose images are date 1's quantiles
        lo, hi = RR.quantiles_ref(d1, [31 / 63, 32 / 63], [2], ex, 255)[0][0]
        slack = 4 * 2.0 ** -23 * max(abs(lo), abs(hi))       # the knots' rounding to float32 (half an ulp) and the segment's three roundings
        assert lo - slack <= m2 <= hi + slack


def _cities():
    return synthetic_onera(n_cities=2, bands=4, size=(96, 110), seed=2, radiometry=(1.3, 0.2), ignore_frac=0.1)


@pytest.mark.parametrize('on_device', [False, True])
@pytest.mark.parametrize('method', ['histogram', 'range'])
def test_normalize_cities_rewrites_date_2_in_place_and_nothing_else(method, on_device):
    data = _cities()
    before = {c: {k: v.copy() for k, v in d.items()} for c, d in data.items()}
    if on_device:
        data = {c: {'images': torch.from_numpy(d['images']).cuda(), 'labels': torch.from_numpy(d['labels']).cuda()} for c, d in data.items()}
    reports = RM.normalize_cities(data, method=method, knots=32, ignore_label=255)
    assert list(reports) == list(data)
    for c, d in data.items():
        assert torch.is_tensor(d['images']) == on_device
        images, labels = (d[k].cpu().numpy() if on_device else d[k] for k in ('images', 'labels'))
        im0, lab0 = before[c]['images'], before[c]['labels']
        assert np.array_equal(_bits(images[0]), _bits(im0[0])) and np.array_equal(labels, lab0) and (lab0 == 255).mean() > 0.05
        want, s, t, n = RR.match_ref(im0[1], im0[0], method, knots=32, exclude=lab0, exclude_value=255)
        assert np.array_equal(_bits(images[1]), _bits(want))
        rep = reports[c]
        assert rep['method'] == method and rep['bands'] == [0, 1, 2, 3] and rep['count'] == n.tolist() and n[0, 0] == int((lab0 != 255).sum())
        assert rep['p'] == [0.02, 0.5, 0.98]
        assert rep['src'] == RR.quantiles_ref(im0[1], rep['p'], None, lab0, 255)[0].tolist()
        assert rep['dst'] == RR.quantiles_ref(im0[0], rep['p'], None, lab0, 255)[0].tolist()
        unfitted = RR.match_ref(im0[1], im0[0], method, knots=32)[0]        # the ignored pixels did shape the other fit
        assert not np.array_equal(_bits(unfitted), _bits(want))
        line = RM.report_line(c, rep)
        assert json.loads(json.dumps(line)) == line and line['city'] == c


def test_stretch_8bit_on_a_device_band_a_stack_and_numpy():
    from fabric_amd.utils.dataloaders import stretch_8bit
    r = np.random.default_rng(3)
    x = (r.gamma(2.0, 500.0, (3, 97, 131)) * (r.random((3, 97, 131)) > 0.1)).astype(np.uint16)
    x[2] = 7
    want = RR.stretch_8bit_ref(x)
    got = stretch_8bit(torch.from_numpy(x[0].copy()).cuda())
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (97, 131) and np.array_equal(got.cpu().numpy(), want[0])
    assert want[0].max() == 255 and want[0].min() == 0 and len(np.unique(want[0])) > 200
    stack = stretch_8bit(torch.from_numpy(x).cuda())
    assert np.array_equal(stack.cpu().numpy(), want) and not want[2].any()
    host = stretch_8bit(x)
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and np.array_equal(host, want)
    f = x.astype(np.float32) * np.float32(0.37)
    assert np.array_equal(stretch_8bit(torch.from_numpy(f).cuda(), 5, 95).cpu().numpy(), RR.stretch_8bit_ref(f, 5, 95))


ARGS = ['--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64', '--stride', '128', '--num_workers', '0']


def _recorded(monkeypatch):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


def test_cli_matches_logs_and_records_the_settings(tmp_path, capsys, monkeypatch):
    from fabric_amd import train as T
    names = _recorded(monkeypatch)
    loaded = {}
    real = T.normalize_loaded
    monkeypatch.setattr(T, 'normalize_loaded', lambda full_load, *a, **k: (real(full_load, *a, **k), loaded.update(full_load))[0])
    T.main(ARGS + ['--synthetic_radiometry', '1.3', '0.2', '--radiometric', 'range', '--log_dir', str(tmp_path)])
    lines = capsys.readouterr().out.strip().splitlines()
    radiom = [json.loads(ln[len('radiom '):]) for ln in lines if ln.startswith('radiom ')]
    assert [c['city'] for c in radiom] == [f'city{k}' for k in range(6)] == list(loaded)
    cities = synthetic_onera(n_cities=6, bands=13, size=(360, 360), radiometry=(1.3, 0.2))
    for c in radiom:
        assert set(c) == {'city', 'method', 'bands', 'count', 'p', 'src', 'dst'} and c['method'] == 'range' and c['bands'] == list(range(13))
        im = cities[c['city']]['images']
        assert c['count'] == [[360 * 360] * 13] * 2
        assert c['src'] == RR.quantiles_ref(im[1], c['p'])[0].tolist() and c['dst'] == RR.quantiles_ref(im[0], c['p'])[0].tolist()
        # what the loop trained on: date 2 is the twin's raster, and its median per band -- measured on the device -- is the twin's value
        got = loaded[c['city']]['images']
        want = RR.match_ref(im[1], im[0], 'range')[0]
        assert np.array_equal(_bits(got[0]), _bits(im[0])) and np.array_equal(_bits(got[1]), _bits(want))
        p50 = RM.band_quantiles(torch.from_numpy(got[1]).cuda(), [0.5]).read()['value'][:, 0]
        assert np.array_equal(p50, RR.quantiles_ref(want, [0.5])[0][:, 0])
        # ... and lies between date 1's 2 % and 98 % quantiles, onto which the line carried date 2's
        dst = np.array(c['dst'])
        assert (dst[:, 0] < p50).all() and (p50 < dst[:, 2]).all()
    assert json.loads(lines[-1])['epoch'] == 0
    meta = json.load(open(tmp_path / 'metadata_epoch_0.json'))
    assert meta['radiometric'] == {'method': 'range', 'knots': 256, 'lower': 0.02, 'upper': 0.98, 'bands': None}
    assert names.count('bdn_band_quantiles') == 12 + 6 and names.count('bdn_transfer_apply') == 6      # two fits and one apply per city (+ the test's own)
    # --resume keeps the setting
    from fabric_amd.train import check_radiometric_flags, checkpoint_radiometric
    kept = checkpoint_radiometric(str(tmp_path / 'checkpoint_epoch_0.state_dict.pt'))
    assert kept == meta['radiometric'] and check_radiometric_flags(None, checkpoint=kept) == kept


def test_cli_without_the_flags_does_what_it_did(tmp_path, capsys, monkeypatch):
    """At their defaults the flags add no call: no matching, synthetic_onera called as before, no new metadata key, none of the new entry
    points among the library calls -- and the calls of a run with the matching on are these calls plus the new entries."""
    from fabric_amd import train as T
    names = _recorded(monkeypatch)
    T.main(ARGS + ['--radiometric', 'range', '--log_dir', str(tmp_path / 'on')])
    with_matching = list(names)
    del names[:]
    seen = []
    real = T.synthetic_onera
    monkeypatch.setattr(T, 'synthetic_onera', lambda **kw: seen.append(kw) or real(**kw))
    monkeypatch.setattr(T, 'normalize_loaded', lambda *a, **k: pytest.fail('matching ran without --radiometric'))
    T.main(ARGS + ['--log_dir', str(tmp_path / 'off')])
    out = capsys.readouterr().out
    assert seen == [dict(n_cities=6, bands=13, size=(360, 360))] and out.count('radiom ') == 6
    assert 'radiometric' not in json.load(open(tmp_path / 'off' / 'metadata_epoch_0.json'))
    assert names and not [n for n in names if n in NEW]
    assert [n for n in with_matching if n not in NEW] == names and len(with_matching) == len(names) + 18
