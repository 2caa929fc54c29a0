"""The weight gradient's host decisions against tests/golden/wgrad_launches.json (host-side queries only, no GPU).

The golden was recorded at the commit BEFORE bdn_conv3x3_wgrad_kernels existed, from what stood in its place: the engine's
wgrad_gemm_name and launch_cases' wgrad_inst / wgrad_bnbwd_inst (Python restatements of the plan, the bf16x3 route and the reduction's
lane rule) and the library's size and variant queries.  Here the library must give the same sizes and variants, and the new queries --
the entry points' own code path with the launches replaced by their names -- the same kernels and lanes, for every phase selection.
The grid: all four dtypes; maps of 8 x 8 and below with even and odd imgs_per_group; ragged 9 x 17, 29 x 45, 61 x 125; C0 in 16 .. 512,
C1 in 0 / 64, Cout in 64 / 128 / 512; plain and BatchNorm+ReLU input; kernel override 0 / WG_SIMPLE / WG_ROLE x block targets
0 / 1 / 7 / 256 / 512; every layer of the batch-64 128 x 128 step in the four precisions.  Shapes whose split operands reach 2^30
elements are not in it (the old Python copy lacked the entry point's factor 2 there): one is pinned by hand below.
"""
import json
import os

import pytest

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X3, IN_BNRELU, IN_PLAIN, wg_flags
from tests import launch_cases as lc

with open(os.path.join(os.path.dirname(__file__), 'golden', 'wgrad_launches.json')) as f:
    G = json.load(f)
NAMES = G['names']


def _expected(gemm, lanes, phases):
    """The '+'-joined launch sequence of a phase selection from the recorded (GEMM names, lanes): GEMM, reduction, combine."""
    names = gemm.split('+')
    combine = names[1:]
    assert combine in ([], ['wgrad_x3_combine_kernel'])
    seq = (names[:1] if phases & 1 else []) + ([f'wgrad_reduce_kernel<{lanes}>'] + combine if phases & 2 else [])
    return '+'.join(seq)


def _check(lib, base, flags, ans):
    gemm, lanes, variant, nbytes = NAMES[ans[0]], ans[1], ans[2], ans[3]
    assert lib.bdn_conv3x3_wgrad_variant(*base, flags) == variant, (base, flags)
    assert lib.bdn_wgrad_workspace_bytes_ex(*base, flags) == nbytes, (base, flags)
    assert lc.wgrad_inst(*base, flags) == (gemm, lanes), (base, flags)
    for ph in (1, 2, 3):
        got = lib.bdn_conv3x3_wgrad_kernels(*base, (flags & ~3) | ph).decode()
        assert got == _expected(gemm, lanes, ph), (base, flags, ph)
    assert lib.bdn_conv3x3_wgrad_kernels(*base, flags & ~3).decode() == _expected(gemm, lanes, 3)        # phase bits 0 are read as 3


@pytest.mark.parametrize('dtype', sorted(lc.DTYPE.values()))
def test_grid_matches_the_recorded_decisions(dtype):
    lib = _lib.load()
    rows = [r for r in G['grid'] if r[0][0] == dtype]
    assert len(rows) >= 100
    for base, answers in rows:
        assert len(answers) == len(G['plans'])
        for (kernel, blocks), ans in zip(G['plans'], answers):
            _check(lib, base, wg_flags(3, kernel, blocks), ans)


def test_grid_holds_what_it_must():
    """The axes the golden was asked to span are in it."""
    col = lambda i: {r[0][i] for r in G['grid']}            # noqa: E731
    assert col(0) == set(lc.DTYPE.values())
    shapes = {tuple(r[0][1:4]) + (r[0][7],) for r in G['grid']}
    assert any(h <= 8 and w <= 8 and g % 2 == 0 for _, h, w, g in shapes) and any(h <= 8 and w <= 8 and g % 2 for _, h, w, g in shapes)
    assert {(9, 17), (29, 45), (61, 125)} <= {(h, w) for _, h, w, _ in shapes}
    assert col(5) == {16, 32, 64, 128, 192, 512} and col(6) == {0, 64} and col(4) == {64, 128, 512} and col(8) == {IN_PLAIN, IN_BNRELU}
    assert {tuple(p) for p in G['plans']} == {(k, b) for k in (0, _lib.WG_SIMPLE, _lib.WG_ROLE) for b in (0, 1, 7, 256, 512)}
    used = {NAMES[a[0]] for r in G['grid'] for a in r[1]} | {NAMES[r[1][0]] for s in G['step'].values() for r in s['wgrad']}
    assert {'wgrad7_kernel<true>', 'wgrad7_kernel<false>', 'wgrad7x_kernel<3>', 'wgrad7x_kernel<2>',
            'wgrad_kernel<bf16,8,8,2,false>+wgrad_x3_combine_kernel'} <= used
    assert {f'wgrad_kernel<{t},8,{g},{k}>' for t in ('bf16', 'f32') for g in ('8,2', '16,1') for k in ('true', 'false')} <= used
    assert {a[1] for r in G['grid'] for a in r[1]} == {1, 2, 4, 8, 16}


@pytest.mark.parametrize('precision', ['bf16', 'fp32', 'bf16x3', 'bf16x3-fast'])
def test_training_step_layers_match_the_recorded_decisions(precision):
    lib = _lib.load()
    rec = G['step'][precision]
    assert len(rec['wgrad']) + len(rec['first']) == 18
    for args, ans in rec['wgrad']:
        _check(lib, args[:9], args[9], ans)
    for args, (name, lanes) in rec['first']:
        assert lc.wgrad_bnbwd_inst(*args) == (NAMES[name], lanes)
        assert lib.bdn_conv3x3_wgrad_bnbwd_kernels(*args).decode() == f'{NAMES[name]}+wgrad_reduce_kernel<{lanes}>'


def test_first_layer_query_matches_the_recorded_decisions():
    lib = _lib.load()
    assert {ok for _, (ok, _, _) in G['bnbwd']} == {0, 1}
    for args, (ok, name, lanes) in G['bnbwd']:
        assert lib.bdn_conv3x3_wgrad_bnbwd_supported(*args) == ok, args
        got = lib.bdn_conv3x3_wgrad_bnbwd_kernels(*args).decode()
        assert got == (f'{NAMES[name]}+wgrad_reduce_kernel<{lanes}>' if ok else ''), args


def test_sizes_tiles_and_split_convolutions_match_the_recorded_answers():
    lib = _lib.load()
    for args, nbytes in G['generic']:
        assert lib.bdn_wgrad_workspace_bytes(*args) == nbytes, args
    for args, n in G['mtiles']:
        assert lib.bdn_conv3x3_num_mtiles_ex(*args) == n, args
    assert {NAMES[i] for _, i in G['conv']} > {''}
    for args, name in G['conv']:
        assert lib.bdn_conv3x3_variant(*args).decode() == NAMES[name], args


def test_split_operands_of_two_to_the_31_take_the_doubled_route():
    """BDN_BF16X3, 256 x 256 x 256 x 64: the split operands hold 2 * 2^24 * 64 = 2^31 elements, so bdn_conv3x3_wgrad_ex's guard
    (2 N H W max(Cout, C0) < 2^31) sends the call through the bf16 GEMM on the doubled operands [128] x [128]: 8 x 16 tiles,
    131072 chunks, 4 - 1 = 3 channel tiles (lo x lo left out); the doubled tensors reach 2^31 elements as well, so the one-chunk kernel
    with 2 x 128 blocks / 3 tiles -> 86 splits; the reduction of a 128 x 128 plane takes 2 lanes (16384 / 128 = 128 < 256, 16384 / 64
    = 256 is not); then the quadrant sum.  The Python copy this query replaced named wgrad7x_kernel<3> here."""
    lib = _lib.load()
    args = (BDN_BF16X3, 256, 256, 256, 64, 64, 0, 128, IN_PLAIN)
    want = 'wgrad_kernel<bf16,8,16,1,false>+wgrad_reduce_kernel<2>+wgrad_x3_combine_kernel'
    assert lib.bdn_conv3x3_wgrad_kernels(*args, wg_flags()).decode() == want
    assert lib.bdn_conv3x3_wgrad_kernels(*args, 0).decode() == want
    assert lc.wgrad_inst(*args) == ('wgrad_kernel<bf16,8,16,1,false>+wgrad_x3_combine_kernel', 2)
    # one image fewer per axis of the guard: half the elements, the fused kernel
    assert lib.bdn_conv3x3_wgrad_kernels(BDN_BF16X3, 128, 256, 256, 64, 64, 0, 128, IN_PLAIN, wg_flags()).decode() \
        == 'wgrad7x_kernel<3>+wgrad_reduce_kernel<8>'


@pytest.mark.parametrize('args', [
    (BDN_BF16, 4, 29, 45, 48, 64, 0, 2, IN_PLAIN),         # Cout = 48
    (BDN_BF16X3, 4, 29, 45, 48, 64, 0, 2, IN_PLAIN),
    (BDN_BF16, 4, 29, 45, 64, 8, 0, 2, IN_PLAIN),          # C0 = 8 in bf16
    (BDN_BF16, 4, 29, 45, 64, 64, 64, 2, IN_BNRELU),       # two sources with BatchNorm+ReLU
    (BDN_BF16, 5, 29, 45, 64, 64, 0, 2, IN_PLAIN),         # N not a multiple of imgs_per_group
    (7, 4, 29, 45, 64, 64, 0, 2, IN_PLAIN),                # no such dtype
], ids=['cout48', 'cout48-x3', 'c0-8', 'two-sources-bnrelu', 'ragged-groups', 'bad-dtype'])
def test_refused_arguments_have_no_kernels(args):
    lib = _lib.load()
    for ph in (0, 1, 2, 3):
        assert lib.bdn_conv3x3_wgrad_kernels(*args, ph) == b''
    assert lib.bdn_conv3x3_wgrad_bnbwd_kernels(BDN_BF16, 5, 29, 45, 64, 16, 2) == b''
    assert lib.bdn_conv3x3_wgrad_bnbwd_kernels(BDN_BF16, 4, 29, 45, 128, 16, 2) == b''
