"""The launch-shape table: one row per kernel instantiation that BiDateNet runs, at the smallest shape that selects it.

In this library the SHAPE of a launch picks the kernel instantiation (tile shape, wave layout, 64- or 128-wide column tiles,
single-chunk, eval epilogue, split-K plan).  Each row below names an entry point, its numerics, a shape and options, and the exact
instantiation that shape must select; tests/test_launch_cases_cpu.py checks that against the library's own dispatchers (host-side
queries, no GPU), tests/test_gpu_launch_shapes.py runs every row against a float64 reference.  The enumeration functions at the end
walk one training step / eval forward of BiDateNet layer by layer (fabric_amd/engine.py) and name what each launch runs, so the CPU
test can require that every instantiation of the real step has a row; the GPU test records the launches of real steps and checks that
they equal this enumeration.

ROWS is the table of the 13(16)-band model; WIDE_ROWS adds the first layer of models of 17 to 64 bands (padded to 32, 48 or 64 channels),
ALL_ROWS is both.  Shapes are ragged (H % 8 != 0, W % 16 != 0) wherever the plan allows it.  A plain module (like tests/gpu_util.py), not a conftest.
"""
from collections import namedtuple

from fabric_amd import _lib
from fabric_amd.engine import BiDateEngine
from fabric_amd._lib import (BDN_BF16, BDN_BF16X2, BDN_BF16X3, BDN_F32, EVAL_CLS, EVAL_PAIR, EVAL_STAGE, IN_BNRELU, IN_PLAIN,
                             wg_flags)

DTYPE = {'fp32': BDN_F32, 'bf16': BDN_BF16, 'bf16x3': BDN_BF16X3, 'bf16x2': BDN_BF16X2}

# op           entry point
#   fwd        bdn_conv3x3 forward, per-tile statistics when `stats` (then bdn_bn_finalize on them)
#   dgrad      bdn_conv3x3 on dz with the data-gradient filter image (C0 = the layer's Cout, Cout = its Cin)
#   dgrad_bs   bdn_conv3x3_dgrad_bs (masked gradient + BatchNorm-backward partial sums of the producing layer)
#   dgrad_bb   bdn_conv3x3_dgrad_bb (BatchNorm backward of the layer applied on load; C0 = 64)
#   x3         bdn_conv3x3 on the bdn_split_pack operand (prec bf16x3 / bf16x2; forward and data gradient run the same kernels)
#   x3src      bdn_conv3x3_x3src (float32 operand, BatchNorm+ReLU and the split on load when `bnrelu`)
#   eval / eval_pair / eval_cls   bdn_conv3x3_eval / _eval_pair (N = B pairs) / _eval_cls
#   wgrad      bdn_conv3x3_wgrad_ex at default flags (bf16x3 / bf16x2: split operands); `lanes` = split lanes of its reduction
#   wgrad_bnbwd  bdn_conv3x3_wgrad_bnbwd (first layer, C0 = 16, Cout = 64)
# creal (WIDE_ROWS): the layer's real input channels when the operand is padded to C0 -- the first layer of a model of creal bands.  The
#   filter then holds creal channels and goes through the packers with Cin = creal, Cin_pad = C0 and no data-gradient image, the operand's
#   padded channels are exact zeros, the float64 reference convolves the creal channels, and a wgrad row writes Cout * creal * 9 floats.
#   None = C0 (every row of ROWS)
Row = namedtuple('Row', 'op prec N H W C0 C1 Cout ipg bnrelu stats inst lanes creal', defaults=(None,))


def _r(op, prec, N, H, W, C0, C1, Cout, ipg, inst, bnrelu=False, stats=True, lanes=None, creal=None):
    return Row(op, prec, N, H, W, C0, C1, Cout, ipg, bnrelu, stats, inst, lanes, creal)


def _ck(t, cfg, to, bb=False, ev=False, x3=0, xf=False):
    return (f'conv3x3_kernel<{t},{cfg},{to},false,{"true" if bb else "false"},{"true" if ev else "false"},{x3},'
            f'{"true" if xf else "false"}>')


BF, F32 = 'bf16', 'float'
# tile configurations: CKB, TH, TW, TI, BN, WM, WN, ONE
K816_128 = '128,8,16,1,128,1,4,false'
K816_128_ONE = '128,8,16,1,128,1,4,true'
K816_64 = '128,8,16,1,64,2,2,false'
K1616_ONE = '128,16,16,1,64,2,2,true'
K1616 = '128,16,16,1,64,4,1,false'
K88_64 = '128,8,8,2,64,2,2,false'
K88_128 = '128,8,8,2,128,2,2,false'

ROWS = [
    # ---- forward + statistics, bf16 and fp32.  BN = 128 needs n_mtiles * Cout / 128 >= 512 (conv_plan): 4 x 61 x 125 on 8 x 16 tiles is
    # 4 * 8 * 8 = 256 tiles x 2 column tiles = 512 -- the smallest ragged shape at Cout = 256
    _r('fwd', 'bf16', 4, 61, 125, 64, 64, 256, 2, _ck(BF, K816_128, BF)),                       # two sources, two chunks
    _r('fwd', 'bf16', 4, 61, 125, 128, 0, 256, 2, _ck(BF, K816_128, BF), bnrelu=True),          # BatchNorm+ReLU on load
    _r('fwd', 'bf16', 4, 61, 125, 64, 0, 256, 2, _ck(BF, K816_128_ONE, BF)),                    # single chunk
    _r('fwd', 'bf16', 4, 61, 125, 64, 0, 256, 2, _ck(BF, K816_128_ONE, BF), bnrelu=True),
    _r('fwd', 'fp32', 4, 61, 125, 64, 64, 256, 2, _ck(F32, K816_128, F32)),
    _r('fwd', 'fp32', 4, 61, 125, 128, 0, 256, 2, _ck(F32, K816_128, F32), bnrelu=True),
    # the BN threshold itself: 3 x 37 x 270 = 3 * 5 * 17 = 255 tiles (510 blocks) stays at BN = 64, 4 x 37 x 270 = 340 tiles goes to 128
    _r('fwd', 'bf16', 3, 37, 270, 128, 0, 256, 1, _ck(BF, K816_64, BF), bnrelu=True),
    _r('fwd', 'bf16', 4, 37, 270, 128, 0, 256, 2, _ck(BF, K816_128, BF), bnrelu=True),
    # 64-wide outputs on 16 x 16 tiles; 8 x 8 maps with two images per tile (BN = 128 at 512 channels)
    _r('fwd', 'bf16', 4, 29, 45, 64, 0, 64, 2, _ck(BF, K1616_ONE, BF), bnrelu=True),
    _r('fwd', 'bf16', 4, 29, 45, 16, 0, 64, 2, _ck(BF, '32,16,16,1,64,2,2,true', BF)),          # the 13(16)-band first layer
    _r('fwd', 'bf16', 2, 29, 45, 128, 64, 64, 2, _ck(BF, K1616, BF)),
    _r('fwd', 'bf16', 4, 8, 8, 256, 256, 256, 2, _ck(BF, K88_64, BF)),
    _r('fwd', 'bf16', 4, 7, 5, 512, 0, 512, 2, _ck(BF, K88_64, BF), bnrelu=True),
    _r('fwd', 'fp32', 4, 29, 45, 64, 0, 64, 2, _ck(F32, '128,16,16,1,64,4,1,false', F32), bnrelu=True),
    _r('fwd', 'fp32', 4, 29, 45, 16, 0, 64, 2, _ck(F32, '64,16,16,1,64,2,2,true', F32)),
    _r('fwd', 'fp32', 3, 37, 270, 128, 0, 256, 1, _ck(F32, K816_64, F32), bnrelu=True),
    _r('fwd', 'fp32', 4, 7, 5, 512, 0, 512, 2, _ck(F32, K88_64, F32), bnrelu=True),
    # ---- plain data gradient (dz of Cout = C0 channels -> Cin = Cout channels)
    _r('dgrad', 'bf16', 4, 61, 125, 128, 0, 256, 2, _ck(BF, K816_128, BF)),
    _r('dgrad', 'fp32', 4, 61, 125, 128, 0, 256, 2, _ck(F32, K816_128, F32)),
    _r('dgrad', 'bf16', 2, 29, 45, 128, 0, 64, 2, _ck(BF, K1616, BF)),
    _r('dgrad', 'bf16', 4, 7, 5, 512, 0, 512, 2, _ck(BF, K88_64, BF)),
    # ---- masked data gradient with the producing layer's BatchNorm-backward partial sums
    _r('dgrad_bs', 'bf16', 4, 61, 125, 128, 0, 256, 2, _ck(BF, K816_128, BF)),
    _r('dgrad_bs', 'bf16', 4, 61, 125, 64, 0, 256, 2, _ck(BF, K816_128_ONE, BF)),
    _r('dgrad_bs', 'bf16', 4, 29, 45, 64, 0, 64, 2, _ck(BF, K1616_ONE, BF)),
    _r('dgrad_bs', 'bf16', 4, 29, 45, 128, 0, 64, 2, _ck(BF, K1616, BF)),
    _r('dgrad_bs', 'bf16', 4, 37, 53, 256, 0, 128, 2, _ck(BF, K816_64, BF)),
    _r('dgrad_bs', 'fp32', 4, 61, 125, 128, 0, 256, 2, _ck(F32, K816_128, F32)),
    _r('dgrad_bs', 'fp32', 4, 29, 45, 64, 0, 64, 2, _ck(F32, K1616, F32)),
    _r('dgrad_bs', 'fp32', 4, 7, 5, 512, 0, 512, 2, _ck(F32, K88_64, F32)),
    # ---- BatchNorm backward on load: all three instantiations
    _r('dgrad_bb', 'bf16', 4, 29, 45, 64, 0, 64, 2, _ck(BF, K1616_ONE, BF, bb=True)),
    _r('dgrad_bb', 'bf16', 4, 61, 125, 64, 0, 256, 2, _ck(BF, K816_128_ONE, BF, bb=True)),
    _r('dgrad_bb', 'bf16', 2, 37, 53, 64, 0, 128, 1, _ck(BF, K816_64, BF, bb=True)),
    # ---- bf16x3 / bf16x2 on the split operand (X3 = terms; 64-channel chunks, or 16 for the first layer)
    _r('x3', 'bf16x3', 4, 61, 125, 128, 0, 256, 2, _ck(BF, K816_128, F32, x3=3)),
    _r('x3', 'bf16x3', 4, 29, 45, 192, 0, 64, 2, _ck(BF, K816_64, F32, x3=3)),
    _r('x3', 'bf16x3', 4, 7, 5, 512, 0, 512, 2, _ck(BF, K88_64, F32, x3=3)),
    _r('x3', 'bf16x3', 4, 29, 45, 16, 0, 64, 2, _ck(BF, '32,8,16,1,64,2,2,false', F32, x3=3)),
    _r('x3', 'bf16x2', 4, 61, 125, 128, 0, 256, 2, _ck(BF, K816_128, F32, x3=2)),
    _r('x3', 'bf16x2', 4, 29, 45, 192, 0, 64, 2, _ck(BF, K816_64, F32, x3=2)),
    _r('x3', 'bf16x2', 4, 7, 5, 512, 0, 512, 2, _ck(BF, K88_64, F32, x3=2)),
    _r('x3src', 'bf16x3', 4, 61, 125, 128, 0, 256, 2, _ck(BF, K816_128, F32, x3=3, xf=True), bnrelu=True),
    _r('x3src', 'bf16x3', 4, 29, 45, 64, 0, 64, 2, _ck(BF, K816_64, F32, x3=3, xf=True), bnrelu=True),
    _r('x3src', 'bf16x3', 4, 7, 5, 512, 0, 512, 2, _ck(BF, K88_64, F32, x3=3, xf=True), bnrelu=True),
    _r('x3src', 'bf16x3', 4, 61, 125, 64, 0, 256, 2, _ck(BF, K816_128, F32, x3=3, xf=True), stats=False),       # plain operand (eval)
    _r('x3src', 'bf16x2', 4, 61, 125, 128, 0, 256, 2, _ck(BF, K816_128, F32, x3=2, xf=True), bnrelu=True),
    # ---- eval epilogue (EV): stage, date pair (N = B pairs), classifier
    _r('eval', 'bf16', 4, 61, 125, 64, 64, 256, 1, _ck(BF, K816_128, BF, ev=True)),
    _r('eval', 'bf16', 4, 61, 125, 64, 0, 256, 1, _ck(BF, K816_128_ONE, BF, ev=True)),
    _r('eval', 'bf16', 3, 37, 270, 128, 0, 256, 1, _ck(BF, K816_64, BF, ev=True)),
    _r('eval', 'bf16', 4, 29, 45, 64, 0, 64, 1, _ck(BF, K1616_ONE, BF, ev=True)),
    _r('eval', 'bf16', 4, 29, 45, 16, 0, 64, 1, _ck(BF, '32,16,16,1,64,2,2,true', BF, ev=True)),
    _r('eval', 'bf16', 2, 29, 45, 128, 64, 64, 1, _ck(BF, K1616, BF, ev=True)),
    _r('eval', 'bf16', 256, 7, 5, 64, 0, 512, 1, _ck(BF, K88_128, BF, ev=True)),              # 128 tiles of two images x 4: BN = 128
    _r('eval', 'bf16', 4, 7, 5, 512, 0, 512, 1, _ck(BF, K88_64, BF, ev=True)),
    _r('eval', 'fp32', 4, 61, 125, 64, 64, 256, 1, _ck(F32, K816_128, F32, ev=True)),
    _r('eval', 'fp32', 4, 29, 45, 16, 0, 64, 1, _ck(F32, '64,16,16,1,64,2,2,true', F32, ev=True)),
    _r('eval', 'fp32', 3, 37, 270, 128, 0, 256, 1, _ck(F32, K816_64, F32, ev=True)),
    _r('eval', 'fp32', 256, 7, 5, 64, 0, 512, 1, _ck(F32, K88_128, F32, ev=True)),
    _r('eval', 'fp32', 4, 7, 5, 512, 0, 512, 1, _ck(F32, K88_64, F32, ev=True)),
    _r('eval_pair', 'bf16', 4, 29, 45, 64, 0, 64, 1, _ck(BF, '128,8,16,2,64,2,2,true', BF, ev=True)),
    _r('eval_pair', 'bf16', 4, 29, 45, 128, 0, 64, 1, _ck(BF, '128,8,16,2,64,4,1,false', BF, ev=True)),
    _r('eval_pair', 'bf16', 8, 61, 61, 128, 0, 128, 1, _ck(BF, '128,8,8,2,128,1,4,false', BF, ev=True)),
    _r('eval_pair', 'bf16', 128, 8, 8, 512, 0, 512, 1, _ck(BF, K88_128, BF, ev=True)),
    _r('eval_pair', 'bf16', 4, 7, 5, 512, 0, 512, 1, _ck(BF, K88_64, BF, ev=True)),
    _r('eval_pair', 'fp32', 8, 61, 61, 128, 0, 128, 1, _ck(F32, '128,8,8,2,128,1,4,false', F32, ev=True)),
    _r('eval_pair', 'fp32', 4, 29, 45, 128, 0, 64, 1, _ck(F32, '128,8,16,2,64,4,1,false', F32, ev=True)),
    _r('eval_cls', 'bf16', 4, 29, 45, 64, 0, 64, 1, _ck(BF, K1616_ONE, BF, ev=True)),
    _r('eval_cls', 'fp32', 4, 29, 45, 64, 0, 64, 1, _ck(F32, K1616, F32, ev=True)),
    # ---- weight gradient at the production plan (default flags: 128 blocks, per_split >> 1 with a ragged last split).  lanes = split lanes
    # of the fixed-order reduction (launch_wgrad_reduce): 16 for a 64 x 16 filter, 8 for 64 x 64, 4 for 128 x 64, 2 for 128 x 128,
    # 1 from 256 x 128 on
    _r('wgrad', 'bf16', 4, 61, 125, 64, 0, 64, 2, 'wgrad7_kernel<true>', bnrelu=True, lanes=8),
    _r('wgrad', 'bf16', 4, 61, 125, 64, 0, 128, 2, 'wgrad7_kernel<false>', lanes=4),
    _r('wgrad', 'bf16', 4, 61, 125, 64, 64, 128, 2, 'wgrad7_kernel<false>', lanes=2),
    _r('wgrad', 'bf16', 4, 29, 45, 128, 128, 256, 2, 'wgrad7_kernel<false>', lanes=1),
    _r('wgrad', 'bf16', 4, 29, 45, 128, 0, 128, 2, 'wgrad7_kernel<true>', bnrelu=True, lanes=2),
    _r('wgrad', 'bf16', 8, 8, 8, 512, 0, 512, 4, 'wgrad_kernel<bf16,8,8,2,false>', bnrelu=True, lanes=1),
    _r('wgrad', 'bf16', 8, 8, 8, 512, 512, 512, 4, 'wgrad_kernel<bf16,8,8,2,false>', lanes=1),
    _r('wgrad', 'fp32', 4, 61, 125, 16, 0, 64, 2, 'wgrad_kernel<f32,8,16,1,true>', lanes=16),
    _r('wgrad', 'fp32', 4, 29, 45, 64, 0, 64, 2, 'wgrad_kernel<f32,8,16,1,false>', bnrelu=True, lanes=8),
    _r('wgrad', 'fp32', 8, 8, 8, 512, 0, 512, 4, 'wgrad_kernel<f32,8,8,2,false>', bnrelu=True, lanes=1),
    _r('wgrad', 'bf16x3', 4, 61, 125, 64, 0, 128, 2, 'wgrad7x_kernel<3>', lanes=4),
    _r('wgrad', 'bf16x3', 4, 29, 45, 128, 0, 128, 2, 'wgrad7x_kernel<3>', lanes=2),
    _r('wgrad', 'bf16x3', 8, 8, 8, 512, 0, 512, 4, 'wgrad_kernel<bf16,8,8,2,false>+wgrad_x3_combine_kernel', lanes=1),
    _r('wgrad', 'bf16x2', 4, 61, 125, 64, 0, 64, 2, 'wgrad7x_kernel<2>', lanes=8),
    _r('wgrad', 'bf16x2', 8, 8, 8, 512, 0, 512, 4, 'wgrad_kernel<bf16,8,8,2,false>+wgrad_x3_combine_kernel', lanes=1),
    # the first layer: 256-block grid, 16 split lanes
    _r('wgrad_bnbwd', 'bf16', 4, 61, 125, 16, 0, 64, 2, 'wgrad_first_kernel', lanes=16),
    _r('wgrad_bnbwd', 'bf16x3', 4, 61, 125, 16, 0, 64, 2, 'wgrad_first_x3_kernel<3>', lanes=16),
    _r('wgrad_bnbwd', 'bf16x2', 4, 61, 125, 16, 0, 64, 2, 'wgrad_first_x3_kernel<2>', lanes=16),
]


# ---- the first layer of models of 17 to 64 bands (cp = 32, 48, 64): 16-channel chunks with more than one chunk (bf16, the split operand),
# the single chunk of 32 float channels, three 16-channel float chunks, the split-K GEMMs at C0 = 32 / 48 and on the doubled operand, and at
# 64 padded channels the trunk's kernels on an operand whose real channels end inside the chunk.  Every row carries creal:
# (creal, C0) = (17, 32), (33, 48), (50, 64), and (64, 64) = a 64-band model, whose first layer has no data-gradient image either.
# The same smallest ragged shape as the 16-band rows.  A list of its own: the 2 to 4 GB twins of tests/bigtensor.py are made of ROWS.
WIDE_PAIRS = ((17, 32), (33, 48), (50, 64), (64, 64))
K1632 = '32,16,16,1,64,4,1,false'                         # bf16: 16-channel chunks, two or three of them
_WIDE_CONV = {                                            # C0 -> tile configuration of the 4 x 29 x 45 launch
    'bf16': {32: K1632, 48: K1632, 64: K1616_ONE},
    'fp32': {32: K1616_ONE, 48: '64,16,16,1,64,4,1,false', 64: K1616},
    'x3': {32: '32,8,16,1,64,2,2,false', 48: '32,8,16,1,64,2,2,false', 64: K816_64},
}
_WIDE_WGRAD = {                                           # C0 -> (GEMM, split lanes of its reduction)
    'bf16': {32: ('wgrad_kernel<bf16,8,16,1,true>', 16), 48: ('wgrad_kernel<bf16,8,16,1,false>', 16), 64: ('wgrad7_kernel<false>', 8)},
    'fp32': {32: ('wgrad_kernel<f32,8,16,1,true>', 16), 48: ('wgrad_kernel<f32,8,16,1,false>', 16), 64: ('wgrad_kernel<f32,8,16,1,false>', 8)},
    'bf16x3': {32: ('wgrad7_kernel<false>+wgrad_x3_combine_kernel', 4), 48: ('wgrad_kernel<bf16,8,16,1,false>+wgrad_x3_combine_kernel', 4),
               64: ('wgrad7x_kernel<3>', 8)},
    'bf16x2': {32: ('wgrad7_kernel<false>+wgrad_x3_combine_kernel', 4), 48: ('wgrad_kernel<bf16,8,16,1,false>+wgrad_x3_combine_kernel', 4),
               64: ('wgrad7x_kernel<2>', 8)},
}


def _wide_rows():
    out = []
    for creal, C0 in WIDE_PAIRS:
        for p, t in (('bf16', BF), ('fp32', F32)):
            out.append(_r('fwd', p, 4, 29, 45, C0, 0, 64, 2, _ck(t, _WIDE_CONV[p][C0], t), creal=creal))
            out.append(_r('eval', p, 4, 29, 45, C0, 0, 64, 1, _ck(t, _WIDE_CONV[p][C0], t, ev=True), creal=creal))
        for p, terms in (('bf16x3', 3), ('bf16x2', 2)):
            out.append(_r('x3', p, 4, 29, 45, C0, 0, 64, 2, _ck(BF, _WIDE_CONV['x3'][C0], F32, x3=terms), creal=creal))
        for p in ('bf16', 'fp32', 'bf16x3', 'bf16x2'):
            g, lanes = _WIDE_WGRAD[p][C0]
            out.append(_r('wgrad', p, 4, 29, 45, C0, 0, 64, 2, g, lanes=lanes, creal=creal))
    return out


WIDE_ROWS = _wide_rows()
ALL_ROWS = ROWS + WIDE_ROWS


def row_id(r):
    return (f'{r.op}-{r.prec}-{r.N}x{r.H}x{r.W}-{r.C0}' + (f'+{r.C1}' if r.C1 else '') + f'-{r.Cout}-g{r.ipg}'
            + ('-bnrelu' if r.bnrelu else '') + ('' if r.stats else '-nostats') + (f'-real{r.creal}' if r.creal else ''))


# ---- statistics reductions on synthetic partials: (rows per group, G).  bdn_bn_finalize / bdn_bn_bwd_finalize take the one-launch path up
# to 512 rows per group and the two-stage reduce_rows_kernel + finalize above it (513: ragged last block); 4096 and 8192 are the production
# counts of level 1 (batch 64 / 128 on 16 x 16 tiles: 4096 rows per date), where the row-split count is capped at 64
STATS_CASES = [(512, 1), (512, 2), (513, 1), (513, 2), (4096, 1), (4096, 2), (8192, 1), (8192, 2)]


# ------------------------------------------------------------------ instantiation of a launch, from the library's dispatchers
def _s(b):
    return b.decode()


def conv_inst(dtype, N, H, W, C0, C1, Cout, ipg):
    return _s(_lib.load().bdn_conv3x3_variant(dtype, N, H, W, C0, C1, Cout, ipg))


def x3src_inst(dtype, N, H, W, C0, Cout, ipg):
    return _s(_lib.load().bdn_conv3x3_x3src_variant(dtype, N, H, W, C0, Cout, ipg))


def bb_inst(N, H, W, Cout, ipg):
    return _s(_lib.load().bdn_conv3x3_dgrad_bb_variant(N, H, W, Cout, ipg))


def eval_inst(kind, dtype, N, H, W, C0, C1, Cout):
    return _s(_lib.load().bdn_conv3x3_eval_variant(kind, dtype, N, H, W, C0, C1, Cout))


def _gemm_and_lanes(kernels):
    """'+'-joined kernel names of a weight-gradient call -> (the names without the reduction, its split lanes)."""
    names = _s(kernels).split('+')
    red = [n for n in names if n.startswith('wgrad_reduce_kernel<')]
    assert len(red) == 1, names
    return '+'.join(n for n in names if n not in red), int(red[0][len('wgrad_reduce_kernel<'):-1])


def wgrad_inst(dtype, N, H, W, Cout, C0, C1, ipg, mode, flags=wg_flags()):
    """(GEMM instantiation(s), split lanes of the reduction) of bdn_conv3x3_wgrad_ex: the library's answer (bdn_conv3x3_wgrad_kernels)."""
    return _gemm_and_lanes(_lib.load().bdn_conv3x3_wgrad_kernels(dtype, N, H, W, Cout, C0, C1, ipg, mode, flags | 3))


def wgrad_bnbwd_inst(dtype, N, H, W, Cout, C0, ipg):
    """(instantiation, split lanes) of bdn_conv3x3_wgrad_bnbwd (bdn_conv3x3_wgrad_bnbwd_kernels)."""
    return _gemm_and_lanes(_lib.load().bdn_conv3x3_wgrad_bnbwd_kernels(dtype, N, H, W, Cout, C0, ipg))


def instantiation(r):
    """What the row's launch runs, asked from the library (for wgrad rows: the GEMM; `lanes` is checked apart)."""
    dt = DTYPE[r.prec]
    if r.op in ('fwd', 'dgrad', 'dgrad_bs', 'x3'):
        return conv_inst(dt, r.N, r.H, r.W, r.C0, r.C1, r.Cout, r.ipg)
    if r.op == 'dgrad_bb':
        return bb_inst(r.N, r.H, r.W, r.Cout, r.ipg)
    if r.op == 'x3src':
        return x3src_inst(dt, r.N, r.H, r.W, r.C0, r.Cout, r.ipg)
    if r.op in ('eval', 'eval_pair', 'eval_cls'):
        kind = {'eval': EVAL_STAGE, 'eval_pair': EVAL_PAIR, 'eval_cls': EVAL_CLS}[r.op]
        return eval_inst(kind, dt, r.N, r.H, r.W, r.C0, r.C1, r.Cout)
    if r.op == 'wgrad':
        return wgrad_inst(dt, r.N, r.H, r.W, r.Cout, r.C0, r.C1, r.ipg, IN_BNRELU if r.bnrelu else IN_PLAIN)[0]
    if r.op == 'wgrad_bnbwd':
        return wgrad_bnbwd_inst(dt, r.N, r.H, r.W, r.Cout, r.C0, r.ipg)[0]
    raise ValueError(r.op)


def reduce_lanes(r):
    dt = DTYPE[r.prec]
    if r.op == 'wgrad':
        return wgrad_inst(dt, r.N, r.H, r.W, r.Cout, r.C0, r.C1, r.ipg, IN_BNRELU if r.bnrelu else IN_PLAIN)[1]
    return wgrad_bnbwd_inst(dt, r.N, r.H, r.W, r.Cout, r.C0, r.ipg)[1]


def covered():
    """Every instantiation some row selects, with the wgrad rows' reductions."""
    out = {i for r in ALL_ROWS for i in r.inst.split('+')}
    out |= {f'wgrad_reduce_kernel<{r.lanes}>' for r in ALL_ROWS if r.lanes}
    return out


# ------------------------------------------------------------------ what BiDateNet launches (mirrors fabric_amd/engine.py)
def _layers(n_channels):
    from fabric_amd.engine import build_layers
    return {L.name: L for L in build_layers(n_channels)}


def call_instantiations(name, args):
    """Instantiations run by one recorded library call (name, args as passed to _lib.call); empty for entry points without MFMA GEMMs."""
    a = args
    if name == 'bdn_conv3x3':
        return [conv_inst(a[0], a[12], a[13], a[14], a[2], a[4], a[15], a[7])]
    if name == 'bdn_conv3x3_dgrad_bs':
        return [conv_inst(a[0], a[9], a[10], a[11], a[2], 0, a[12], a[7])]
    if name == 'bdn_conv3x3_dgrad_bb':
        return [bb_inst(a[13], a[14], a[15], a[16], a[6])]
    if name == 'bdn_conv3x3_x3src':
        return [x3src_inst(a[0], a[11], a[12], a[13], a[2], a[14], a[5])]
    if name == 'bdn_conv3x3_eval':
        return [eval_inst(EVAL_STAGE, a[0], a[11], a[12], a[13], a[2], a[4] if a[3] else 0, a[14])]
    if name == 'bdn_conv3x3_eval_pair':
        return [eval_inst(EVAL_PAIR, a[0], a[8], a[9], a[10], a[2], 0, a[11])]
    if name == 'bdn_conv3x3_eval_cls':
        return [eval_inst(EVAL_CLS, a[0], a[15], a[16], a[17], a[2], 0, a[18])]
    if name == 'bdn_conv3x3_wgrad_ex':
        g, sl = wgrad_inst(a[0], a[13], a[14], a[15], a[2], a[4], a[6] if a[5] else 0, a[9], a[7], a[16])
        return g.split('+') + [f'wgrad_reduce_kernel<{sl}>']
    if name == 'bdn_conv3x3_wgrad_bnbwd':
        g, sl = wgrad_bnbwd_inst(a[0], a[13], a[14], a[15], a[7], a[9], a[6])
        return [g, f'wgrad_reduce_kernel<{sl}>']
    return []


MFMA_ENTRY_POINTS = ('bdn_conv3x3', 'bdn_conv3x3_dgrad_bs', 'bdn_conv3x3_dgrad_bb', 'bdn_conv3x3_x3src', 'bdn_conv3x3_eval',
                     'bdn_conv3x3_eval_pair', 'bdn_conv3x3_eval_cls', 'bdn_conv3x3_wgrad_ex', 'bdn_conv3x3_wgrad_bnbwd')


def train_step_instantiations(precision, B=64, S=128, n_channels=13):
    """The instantiations of one training step (forward + backward) of BiDateNet(n_channels, 2) at batch B on S x S patches with the
    engine's default settings, layer by layer as fabric_amd/engine.py launches them; every backward decision is the engine's own."""
    from fabric_amd.engine import ENC_CH
    eng = BiDateEngine(n_channels, 2, precision)
    by = _layers(n_channels)
    dims = [(S >> k, S >> k) for k in range(5)]
    x3 = eng.x3
    mdt, dt = eng.mdt, eng.dt
    out = set()
    add = out.update

    def fwd(L, n, split_src):
        h, w = dims[L.level - 1]
        if x3 and not split_src:              # one float32 source of >= 64 channels: bdn_conv3x3_x3src
            add([x3src_inst(mdt, n, h, w, L.cin, L.cout, B)])
        elif x3:
            add([conv_inst(mdt, n, h, w, L.cin, 0, L.cout, B)])
        elif L.name.startswith('d') and L.name.endswith('a'):
            ck = ENC_CH[L.level - 1]
            add([conv_inst(dt, n, h, w, ck, L.cin - ck, L.cout, B)])
        else:
            add([conv_inst(dt, n, h, w, L.cin, 0, L.cout, B)])

    for k in range(1, 6):
        fwd(by[f'e{k}a'], 2 * B, True)
        fwd(by[f'e{k}b'], 2 * B, False)
    for j in range(1, 5):
        fwd(by[f'd{j}a'], B, True)
        fwd(by[f'd{j}b'], B, False)

    def layer(L, n, c0, c1, mode):            # the engine's per-layer backward: dz (maybe folded into the data gradient), wgrad, dgrad
        h, w = dims[L.level - 1]
        if L.name == 'e1a':
            fdt = eng.first_wgrad_dtype(n, h, w, B)
            if fdt is not None:
                g, sl = wgrad_bnbwd_inst(fdt, n, h, w, L.cout, L.cin, B)
                add([g, f'wgrad_reduce_kernel<{sl}>'])
                return
        wdt, wc0, wc1, wmode, flg = eng.wgrad_launch(L, c0, c1, mode)
        g, sl = wgrad_inst(wdt, n, h, w, L.cout, wc0, wc1, B, wmode, flg)
        add(g.split('+') + [f'wgrad_reduce_kernel<{sl}>'])
        if eng.folds_bn_bwd(L, h, w):
            add([bb_inst(n, h, w, L.cin, B)])
        elif L.name != 'e1a':                 # plain and with fused statistics: the same dispatcher
            add([conv_inst(eng.bwd_dtype, n, h, w, L.cout, 0, L.cin, B)])

    for j in range(4, 0, -1):
        La, Lb = by[f'd{j}a'], by[f'd{j}b']
        ck = ENC_CH[La.level - 1]
        layer(Lb, B, Lb.cin, 0, IN_BNRELU)
        layer(La, B, ck, La.cin - ck, IN_PLAIN)
    for k in range(5, 0, -1):
        layer(by[f'e{k}b'], 2 * B, by[f'e{k}b'].cin, 0, IN_BNRELU)
        layer(by[f'e{k}a'], 2 * B, by[f'e{k}a'].cin, 0, IN_PLAIN)
    return out


def eval_forward_instantiations(precision, B, S=128, n_channels=13):
    """The instantiations of one eval-mode forward (the eval-shaped schedule of bf16 / fp32, fabric_amd/engine.py _forward_eval)."""
    from fabric_amd.engine import ENC_CH
    eng = BiDateEngine(n_channels, 2, precision)
    assert eng._use_eval_schedule()
    by = _layers(n_channels)
    dt = eng.dt
    out = set()
    for k in range(1, 6):
        h = w = S >> (k - 1)
        La, Lb = by[f'e{k}a'], by[f'e{k}b']
        out.add(eval_inst(EVAL_STAGE, dt, 2 * B, h, w, La.cin, 0, La.cout))
        if k in eng.eval_pair:
            out.add(eval_inst(EVAL_PAIR, dt, B, h, w, Lb.cin, 0, Lb.cout))
        else:
            out.add(eval_inst(EVAL_STAGE, dt, B, h, w, Lb.cin, 0, Lb.cout))
    cprev = ENC_CH[4]
    for j in range(1, 5):
        k = 5 - j
        h = w = S >> (k - 1)
        La, Lb = by[f'd{j}a'], by[f'd{j}b']
        out.add(eval_inst(EVAL_STAGE, dt, B, h, w, ENC_CH[k - 1], cprev, La.cout))
        out.add(eval_inst(EVAL_CLS if j == 4 else EVAL_STAGE, dt, B, h, w, Lb.cin, 0, Lb.cout))
        cprev = Lb.cout
    return out
