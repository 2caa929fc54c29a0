"""Host-side parts of the blended full-scene scan (fabric_amd.utils.inference.predict_scene_blended): the tile plan, the
gaussian window, the symmetry codes and their inverses, and the argument checks -- none of them touches a device."""
import numpy as np
import pytest
import torch

from fabric_amd.utils import inference as inf
from fabric_amd.utils.dataloaders import _apply_symmetry


@pytest.mark.parametrize('h,w,p,s', [(100, 90, 32, 16), (100, 90, 32, 12), (64, 64, 32, 32), (96, 128, 32, 32), (40, 41, 40, 7),
                                     (37, 50, 16, 1), (150, 141, 40, 40)])
def test_tile_plan(h, w, p, s):
    o, ys, xs = inf.blend_tile_origins(h, w, p, s)
    assert o.dtype == np.int32 and o.shape == (len(ys) * len(xs), 2)
    for v, n in ((ys, h), (xs, w)):
        assert v[0] == 0 and v[-1] == n - p
        if len(v) > 1:
            assert all(b - a == s for a, b in zip(v[:-2], v[1:-1])) and 0 < v[-1] - v[-2] <= s
    # row-major, y outer: tile iy * len(xs) + ix sits at (ys[iy], xs[ix])
    assert np.array_equal(o, np.array([(y, x) for y in ys for x in xs], dtype=np.int32))
    assert (o >= 0).all() and (o[:, 0] + p <= h).all() and (o[:, 1] + p <= w).all()
    cover = np.zeros((h, w), dtype=np.int64)
    for y, x in o:
        cover[y:y + p, x:x + p] += 1
    assert (cover > 0).all()


def test_tile_plan_single_row_and_reference_set():
    o, ys, xs = inf.blend_tile_origins(32, 100, 32, 10)
    assert list(ys) == [0] and (o[:, 0] == 0).all()
    for h, w, p in ((64, 96, 32), (128, 128, 64), (40, 120, 40)):
        ref = {tuple(t) for t in inf.tile_origins(h, w, p)[0]}
        got = inf.blend_tile_origins(h, w, p, p)[0]
        assert {tuple(t) for t in got} == ref and len(got) == len(ref)


@pytest.mark.parametrize('p', [16, 32, 40, 128])
def test_gaussian_window(p):
    t = np.arange(p, dtype=np.float64)
    g = np.exp(-0.5 * ((t + 0.5 - p / 2) / (p / 8)) ** 2)
    ref = (g[:, None] * g[None, :]).astype(np.float32)
    got = inf.blend_window(p, 'gaussian')
    assert got.dtype == torch.float32 and got.shape == (p, p)
    assert np.array_equal(got.numpy(), ref) and (got > 0).all()
    assert torch.equal(inf.blend_window(p, 'flat'), torch.ones(p, p))


def test_symmetry_inverse_is_identity():
    x = np.arange(2 * 5 * 5).reshape(2, 5, 5)
    seen = set()
    for s in range(8):
        y = _apply_symmetry(x, inf.symmetry_bits(s))
        seen.add(y.tobytes())
        assert np.array_equal(_apply_symmetry(y, inf.symmetry_bits(inf.inverse_symmetry(s))), x), s
        assert inf.inverse_symmetry(inf.inverse_symmetry(s)) == s
    assert len(seen) == 8                                    # eight distinct elements of the group
    assert [inf.inverse_symmetry(s) for s in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    assert inf.TTA_SYMMETRIES == {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3), 8: tuple(range(8))}


def test_check_blend_args_accepts_and_normalises():
    assert inf.check_blend_args(100, 90, 32, None, 'gaussian', (0,), 2) == (16, (0,))
    assert inf.check_blend_args(100, 90, 32, 32, 'flat', 'all', 3) == (32, tuple(range(8)))
    assert inf.check_blend_args(32, 32, 32, 1, torch.full((32, 32), 0.5), [5, 0, 6], 2) == (1, (5, 0, 6))
    assert inf.check_blend_args(32, 32, 32, np.int64(8), 'flat', range(4), 2, batch_size=7) == (8, (0, 1, 2, 3))


@pytest.mark.parametrize('kw,match', [
    (dict(stride=0), 'stride'), (dict(stride=33), 'stride'), (dict(stride=2.0), 'stride'), (dict(stride=True), 'stride'),
    (dict(symmetries=(0, 8)), 'symmetries'), (dict(symmetries=(-1,)), 'symmetries'), (dict(symmetries=()), 'symmetries'),
    (dict(symmetries=(1, 2, 1)), 'distinct'), (dict(symmetries='some'), 'symmetries'),
    (dict(window='hann'), 'window'), (dict(window=torch.ones(31, 32)), 'window'), (dict(window=torch.ones(32, 32, dtype=torch.float64)), 'window'),
    (dict(window=torch.zeros(32, 32)), 'positive'), (dict(window=-torch.ones(32, 32)), 'positive'),
    (dict(window=torch.full((32, 32), float('nan'))), 'positive'),
    (dict(h=31), 'smaller'), (dict(w=20), 'smaller'),
    (dict(n_classes=1), 'softmax'), (dict(n_classes=0), 'n_classes'),
    (dict(batch_size=0), 'batch_size'),
])
def test_check_blend_args_errors(kw, match):
    args = dict(h=64, w=64, patch_size=32, stride=16, window='gaussian', symmetries=(0,), n_classes=2, batch_size=8)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        inf.check_blend_args(**args)
    assert not torch.cuda.is_initialized()


def test_tile_plan_errors():
    with pytest.raises(ValueError, match='stride'):
        inf.blend_tile_origins(64, 64, 32, 0)
    with pytest.raises(ValueError, match='smaller'):
        inf.blend_tile_origins(31, 64, 32, 8)
