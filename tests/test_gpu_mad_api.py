"""-m gpu: fabric_amd.utils.mad (irmad, change_mask), normalize_cities(invariant='mad') and the CLI flags, on plain device tensors: the
public functions give the bits of the C ABI sequence done by hand, a ScoreCurve fed the device's probabilities scores what it scores when
fed the twin's, the raster that reaches the transfer fit is change_mask's, and a one-epoch run logs and records the settings."""
import json

import numpy as np
import pytest
import torch

from fabric_amd import _lib
from fabric_amd.utils import mad as MAD
from fabric_amd.utils import radiometry as RM
from fabric_amd.utils.dataloaders import synthetic_onera
from fabric_amd.utils.metrics import ScoreCurve
from tests import mad_ref as MR
from tests import radiometry_ref as RR

pytestmark = pytest.mark.gpu
NEW = ('bdn_mad_centre', 'bdn_mad_moments', 'bdn_mad_solve', 'bdn_mad_chi2', 'bdn_mad_mask')


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _by_hand(d1, d2, bands, ex, exv, iters, tol, min_var, thr, out_bad):
    c, h, w = d1.shape
    nb, dev, st = len(bands), d1.device, _lib.stream_ptr()
    band_t = torch.tensor(bands, dtype=torch.int32, device=dev)
    f64 = lambda n: torch.full((n,), float('nan'), dtype=torch.float64, device=dev)
    cen, mom, state, nv = f64(2 * nb), f64(MR.moment_doubles(nb)), f64(MR.state_doubles(nb)), torch.full((1,), -1, dtype=torch.int64, device=dev)
    chi2, proba, var = (torch.full(s, float('nan'), device=dev) for s in ((h, w), (2, h, w), (nb, h, w)))
    ws = torch.full((_lib.load().bdn_mad_workspace_bytes(nb, h, w),), 255, dtype=torch.uint8, device=dev)
    scene = (d1.data_ptr(), d2.data_ptr(), band_t.data_ptr(), nb, _lib.ptr(ex), exv)
    _lib.call('bdn_mad_centre', *scene, cen.data_ptr(), nv.data_ptr(), ws.data_ptr(), c, h, w, st)
    for it in range(iters):
        _lib.call('bdn_mad_moments', *scene, None if it == 0 else proba.data_ptr(), cen.data_ptr(), None if it == 0 else state.data_ptr(),
                  mom.data_ptr(), ws.data_ptr(), c, h, w, st)
        _lib.call('bdn_mad_solve', mom.data_ptr(), cen.data_ptr(), nv.data_ptr(), nb, int(it == 0), tol, min_var, state.data_ptr(), st)
        _lib.call('bdn_mad_chi2', *scene, state.data_ptr(), chi2.data_ptr(), proba.data_ptr(), var.data_ptr(), c, h, w, st)
    mask = torch.full((h, w), 77, dtype=torch.uint8, device=dev)
    _lib.call('bdn_mad_mask', proba.data_ptr(), *scene, thr, out_bad, mask.data_ptr(), c, h, w, st)
    return chi2, proba, var, state, mask


def test_irmad_and_change_mask_are_the_abi_sequence():
    d1, d2, _ = MR.scene(5, 5, 97, 131)
    d2 = d2.copy()
    d2[4, 3, :7] = np.nan
    ex = np.where(np.random.default_rng(1).random((97, 131)) < 0.05, 255, 0).astype(np.uint8)
    a, b, e = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda(), torch.from_numpy(ex).cuda()
    res = MAD.irmad(a, b, [4, 1, 2], e, 255, iters=12, tol=5e-3, min_var=1e-8, variates=True)
    mask = MAD.change_mask(res, 0.05, 3)
    want = _by_hand(a, b, [4, 1, 2], e, 255, 12, 5e-3, 1e-8, 0.05, 3)
    for got, w in zip((res.chi2, res.proba, res.variates, res.state, mask), want):
        assert torch.equal(_bits(got), _bits(w))
    rd = res.read()
    tw = MR.irmad_ref(d1, d2, [4, 1, 2], ex, 255, iters=12, tol=5e-3, min_var=1e-8)['state']
    assert rd['ok'] and rd['converged'] and rd['iters'] == tw['iter'] < 12 and rd['n_valid'] == tw['n_valid'] == int(((ex != 255).sum()) - (ex[3, :7] != 255).sum())
    # the weights of the later iterations are float32 rasters that may differ from the twin's in the last bit (2^-24 relative) at some
    # pixels: a weighted mean then moves by at most 2^-24 times the largest value
    assert np.abs(rd['rho'] - tw['rho']).max() <= 1e-10 and np.abs(rd['mean'] - tw['mean']).max() <= 2.0 ** -24 * float(np.abs(d1).max()) and rd['delta'] < 5e-3
    assert set(mask.unique().tolist()) == {0, 1, 3} and int((mask == 3).sum()) == 97 * 131 - rd['n_valid']
    plain = MAD.irmad(a, b, [4, 1, 2], e, 255, iters=12, tol=5e-3, min_var=1e-8)
    assert plain.variates is None and torch.equal(_bits(plain.chi2), _bits(res.chi2))
    out = torch.empty(97, 131, dtype=torch.uint8, device='cuda')
    assert MAD.change_mask(res, 0.05, 3, out=out) is out and torch.equal(out, mask)
    failed = MAD.irmad(a, a.clone(), [0], torch.full_like(e, 255), 255, iters=2)
    assert not failed.read()['ok'] and torch.isnan(failed.chi2).all() and (MAD.change_mask(failed, 0.5, 9) == 9).all()


@pytest.mark.parametrize('run', ['iters = 1', 'converged'])
def test_score_curve_on_the_device_proba_scores_what_the_twin_proba_scores(run):
    """The histogram of ScoreCurve is exact, so only the differences between the two proba rasters matter: the APs agree within 1e-3.  At
    iters = 1 the twin alone reaches AP >= 0.95 (tests/test_mad_cpu.py checks that on the CPU); the converged run is compared as well."""
    city = synthetic_onera(**MR.AP_CITY)['city0']
    kw = MR.AP_RUN if run == 'iters = 1' else dict(iters=30, tol=1e-3)
    tw = MR.irmad_ref(city['images'][0], city['images'][1], [0, 1, 2, 3], **kw)
    im, lab = torch.from_numpy(city['images']).cuda(), torch.from_numpy(city['labels']).cuda()
    res = MAD.irmad(im[0], im[1], **kw)
    aps = []
    for proba in (res.proba, torch.from_numpy(tw['proba']).cuda()):
        curve = ScoreCurve(1024)
        curve.update_proba(proba, lab)
        aps.append(curve.compute())
    print(f'{run}: AP device {aps[0]["ap"]:.6f}, twin {aps[1]["ap"]:.6f}')
    assert abs(aps[0]['ap'] - aps[1]['ap']) <= 1e-3 and aps[0]['n_pos'] == int((city['labels'] == 1).sum())
    assert res.read()['iters'] == tw['state']['iter']
    if run == 'iters = 1':
        assert aps[1]['ap'] >= 0.95


def test_normalize_cities_fits_on_the_invariant_pixels(monkeypatch):
    cities = synthetic_onera(n_cities=2, bands=3, size=(97, 131), seed=4, radiometry=(1.3, 0.2), ignore_frac=0.1)
    seen = []
    real = RM._fit
    monkeypatch.setattr(RM, '_fit', lambda d2, d1, probs, k, bands, exclude, exv, mode, extra=(): (
        seen.append((None if exclude is None else exclude.clone(), exv)), real(d2, d1, probs, k, bands, exclude, exv, mode, extra))[1])
    dev_in = {c: {'images': torch.from_numpy(d['images']).cuda(), 'labels': torch.from_numpy(d['labels']).cuda()} for c, d in cities.items()}
    reports = RM.normalize_cities(dev_in, 'range', ignore_label=255, invariant='mad', invariant_min=0.9, mad_iters=20, mad_tol=2e-3)
    monkeypatch.setattr(RM, '_fit', real)
    for i, (c, d) in enumerate(cities.items()):
        d1, d2 = (torch.from_numpy(d['images'][k]).cuda() for k in (0, 1))
        lab = torch.from_numpy(d['labels']).cuda()
        res = MAD.irmad(d1, d2, None, lab, 255, 20, 2e-3)
        inv = MAD.change_mask(res, 0.9, 1)
        assert seen[i][1] == 1 and torch.equal(seen[i][0], inv)                     # the raster that reached the fit, bit for bit
        tr = RM.fit_transfer(d2, d1, [0.02, 0.98], 2, None, inv, 1, 'slope')
        want = RM.apply_transfer(d2, tr)
        assert torch.equal(_bits(dev_in[c]['images'][1]), _bits(want)) and torch.equal(_bits(dev_in[c]['images'][0]), _bits(d1))
        m, rd = reports[c]['mad'], res.read()
        assert set(m) == {'ok', 'iters', 'converged', 'rho', 'invariant_frac', 'fallback'} and m['ok'] and not m['fallback']
        assert m['iters'] == rd['iters'] and m['rho'] == rd['rho'].tolist() and m['invariant_frac'] == float((inv == 0).sum()) / inv.numel()
        assert 0 < m['invariant_frac'] < 0.9 and (inv[lab == 255] == 1).all()
        assert reports[c]['count'][0] == [int((inv == 0).sum())] * 3
        line = RM.mad_line(c, reports[c])
        assert json.loads(json.dumps(line)) == line and line['city'] == c
    # invariant=None issues today's calls and gives today's bits; numpy in, numpy out
    names = []
    call = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), call(name, *a))[1])
    host = {c: {'images': d['images'].copy(), 'labels': d['labels']} for c, d in cities.items()}
    rep = RM.normalize_cities(host, 'range', ignore_label=255)
    assert not [n for n in names if n in NEW] and names.count('bdn_band_quantiles') == 4 and names.count('bdn_transfer_apply') == 2
    for c, d in cities.items():
        want = RR.match_ref(d['images'][1], d['images'][0], 'range', exclude=d['labels'], exclude_value=255)[0]
        assert isinstance(host[c]['images'], np.ndarray) and np.array_equal(host[c]['images'][1].view(np.uint32), want.view(np.uint32))
        assert 'mad' not in rep[c]
    del names[:]
    host = {c: {'images': d['images'].copy(), 'labels': d['labels']} for c, d in cities.items()}
    rep = RM.normalize_cities(host, 'range', ignore_label=255, invariant='mad', invariant_min=0.9, mad_iters=20, mad_tol=2e-3)
    assert names.count('bdn_mad_mask') == 2 and names.count('bdn_mad_centre') == 2 and names.count('bdn_mad_solve') == 40
    for c in cities:
        assert isinstance(host[c]['images'], np.ndarray) and np.array_equal(host[c]['images'][1].view(np.uint32), dev_in[c]['images'][1].cpu().numpy().view(np.uint32))
        assert rep[c]['mad'] == reports[c]['mad']


def test_a_failed_solve_falls_back_to_the_plain_exclude():
    cities = synthetic_onera(n_cities=1, bands=3, size=(40, 50), seed=5, ignore_frac=0.1)
    cities['city0']['images'][1][2] = 0.5                  # a constant band: date 2 is rank-deficient
    plain = {c: {'images': torch.from_numpy(d['images']).cuda(), 'labels': d['labels']} for c, d in cities.items()}
    mad = {c: {'images': torch.from_numpy(d['images']).cuda(), 'labels': d['labels']} for c, d in cities.items()}
    RM.normalize_cities(plain, 'histogram', knots=16, ignore_label=255)
    rep = RM.normalize_cities(mad, 'histogram', knots=16, ignore_label=255, invariant='mad')
    assert rep['city0']['mad']['ok'] is False and rep['city0']['mad']['fallback'] is True and rep['city0']['mad']['iters'] == 1
    assert torch.equal(_bits(plain['city0']['images']), _bits(mad['city0']['images']))


ARGS = ['--synthetic', '--epochs', '1', '--batch_size', '8', '--patch_size', '64', '--stride', '128', '--num_workers', '0']


def test_cli_logs_the_mad_lines_records_the_settings_and_resume_restores_them(tmp_path, capsys):
    from fabric_amd import train as T
    T.main(ARGS + ['--radiometric', 'range', '--radiometric_invariant', 'mad', '--mad_iters', '8', '--mad_invariant_min', '0.9',
                   '--log_dir', str(tmp_path)])
    lines = capsys.readouterr().out.strip().splitlines()
    mad = [json.loads(ln[len('mad '):]) for ln in lines if ln.startswith('mad ')]
    assert [m['city'] for m in mad] == [f'city{k}' for k in range(6)] and len([ln for ln in lines if ln.startswith('radiom ')]) == 6
    for m in mad:
        assert set(m) == {'city', 'ok', 'iters', 'converged', 'rho', 'invariant_frac', 'fallback'} and m['ok'] and 1 <= m['iters'] <= 8
        assert len(m['rho']) == 13 and 0 < m['invariant_frac'] < 1
    assert json.loads(lines[-1])['epoch'] == 0
    meta = json.load(open(tmp_path / 'metadata_epoch_0.json'))
    want = {'method': 'range', 'knots': 256, 'lower': 0.02, 'upper': 0.98, 'bands': None, 'invariant': 'mad', 'invariant_min': 0.9, 'mad_iters': 8,
            'mad_tol': 1e-3}
    assert meta['radiometric'] == want
    kept = T.checkpoint_radiometric(str(tmp_path / 'checkpoint_epoch_0.state_dict.pt'))
    radiom = T.check_radiometric_flags(None, checkpoint=kept)
    assert kept == want and dict(radiom, **T.check_mad_flags(radiom=radiom, checkpoint=kept)) == want
    # the twin keeps 1.5 % of these cities at 0.9 after the 6 iterations it takes: the uniform 10 % of a calibrated
    # probability, thinned by the reweighting
    assert all(0.005 < m['invariant_frac'] < 0.05 and m['iters'] == 6 and m['converged'] for m in mad), mad
    # a resumed run, given none of the flags, matches its pairs as the first run did: the same mad lines, the same metadata entry
    T.main(ARGS + ['--epochs', '2', '--log_dir', str(tmp_path), '--resume', str(tmp_path / 'checkpoint_epoch_0.state_dict.pt')])
    lines = capsys.readouterr().out.strip().splitlines()
    again = [json.loads(ln[len('mad '):]) for ln in lines if ln.startswith('mad ')]
    assert again == mad and len([ln for ln in lines if ln.startswith('radiom ')]) == 6
    assert json.loads([ln for ln in lines if ln.startswith('{"epoch"')][-1])['epoch'] == 1
    assert json.load(open(tmp_path / 'metadata_epoch_1.json'))['radiometric'] == want
    for flags in (['--radiometric_invariant', 'mad'], ['--mad_tol', '0.01']):
        with pytest.raises(SystemExit, match='add --radiometric'):
            T.main(ARGS + flags + ['--log_dir', str(tmp_path / 'refused')])
