"""CPU proof of tests/bigtensor.py: the shape chooser, the refusals at the 4 GB edge, the periodic comparator and the integer data.

Nothing here touches a device: the library is asked host-side questions only, and an entry point is called with fake pointers only after its
own instantiation query (which never launches) has confirmed that it refuses the shape.
"""
import pytest
import torch

from fabric_amd import _lib
from fabric_amd._lib import BDN_BF16, BDN_BF16X2, BDN_BF16X3, BDN_F32, IN_BNRELU, IN_PLAIN, WG_ROLE, WG_SIMPLE
from tests import bigtensor as bt
from tests import launch_cases as lc

TWO31, TWO32 = bt.TWO31, bt.TWO32
CASES = bt.twins()


# ------------------------------------------------------------------ the shape chooser
@pytest.mark.parametrize('t', CASES, ids=bt.twin_id)
def test_chooser(t):
    r, tw = t.row, t.twin
    assert tw.P % 2 == 0 and tw.N % (tw.G * tw.P) == 0 and tw.N > 0
    assert tw.G == (2 if r.op in bt.GROUPED else 1)
    widths, imgs = bt.bound_widths(r)
    assert tw.bound_bytes == tw.N * imgs * r.H * r.W * max(widths)
    if tw.size == 'cross':
        assert TWO31 + tw.period_bytes <= tw.bound_bytes < TWO32
        assert tw.bound_bytes - tw.step_bytes < TWO31 + tw.period_bytes, 'not the smallest such N'
    else:
        assert TWO32 - tw.step_bytes <= tw.bound_bytes < TWO32
        # tensors of half the widest width cross 2^31 here by more than a period
        assert tw.bound_bytes // 2 >= TWO31 - tw.step_bytes
    # a wrap by 2^31 or 2^32 bytes is not a whole number of periods, for every tensor of the launch
    for x in tw.tensors:
        pb = tw.P * x.pix * x.bpp
        assert TWO31 % pb and TWO32 % pb, (x, pb)
    assert bt.wrap_safe(r, tw.P)
    assert tw.mem_bytes == bt.memory_bytes(r, tw.N) <= bt.MEM_CAP
    # the widest tensor the test holds is the one the entry point bounds
    assert max(tw.N * x.imgs * x.pix * x.bpp for x in tw.tensors) == tw.bound_bytes
    # raising N keeps the instantiation the twin names
    assert lc.instantiation(bt.twin_row(r, tw.N)) == t.inst != ''
    s = bt.small_row(r, tw.P)
    assert s.N == tw.G * tw.P and s.ipg == tw.P


def test_power_of_two_maps_take_a_period_with_an_odd_factor():
    r = next(r for r in lc.ROWS if r.op == 'eval_pair' and (r.H, r.W) == (8, 8))
    assert not bt.wrap_safe(r, 2) and not bt.wrap_safe(r, 4) and bt.period(r) == 6
    r = next(r for r in lc.ROWS if r.op == 'fwd' and (r.H, r.W) == (61, 125))
    assert bt.period(r) == 2


def test_every_row_has_a_twin_or_a_reason():
    """Rows of the twinned ops without a twin of their own: duplicates of a twin's (op, precision, instantiation, modes)."""
    keys = {(t.row.op, t.row.prec, t.inst, t.row.bnrelu, bool(t.row.C1), t.row.stats) for t in CASES}
    own = {t.row for t in CASES}
    assert {lc.row_id(r) for r in lc.ROWS if r.op in bt.TWIN_OPS and r not in own} == {
        'fwd-bf16-4x37x270-128-256-g2-bnrelu', 'fwd-bf16-3x37x270-128-256-g1-bnrelu', 'fwd-fp32-3x37x270-128-256-g1-bnrelu',
        'dgrad_bs-bf16-4x37x53-256-128-g2', 'dgrad_bb-bf16-2x37x53-64-128-g1', 'eval-bf16-4x7x5-512-512-g1', 'eval-fp32-4x7x5-512-512-g1',
        'eval_pair-bf16-4x7x5-512-512-g1'}                 # the list in the docstring of tests/test_gpu_bigtensor.py
    assert {r.op for r in lc.ROWS} == set(bt.TWIN_OPS) | {'wgrad', 'wgrad_bnbwd'}
    for r in lc.ROWS:
        if r.op not in bt.TWIN_OPS or r in own:
            continue
        inst = lc.instantiation(bt.twin_row(r, bt.choose(r, 'top').N))
        assert (r.op, r.prec, inst, r.bnrelu, bool(r.C1), r.stats) in keys, lc.row_id(r)
    # instantiations the raised N moves across the BN = 64 / 128 threshold keep a twin under their big name
    moved = {t.inst for t in CASES if t.inst != t.row.inst}
    assert 'conv3x3_kernel<bf16,128,8,8,2,128,2,2,false,bf16,false,false,false,0,false>' in moved


# ------------------------------------------------------------------ refusals
def _refused(name, args, match='4 GB'):
    with pytest.raises(RuntimeError, match=match) as e:
        _lib.call(name, *args)
    assert 'rc=-2' in str(e.value), e.value                # BDN_E_SHAPE


@pytest.mark.parametrize('t', [t for t in CASES if t.twin.size == 'top'], ids=bt.twin_id)
def test_the_next_n_is_refused(t):
    r, tw = t.row, t.twin
    N = bt.next_refused(tw)
    widths, imgs = bt.bound_widths(r)
    assert N * imgs * r.H * r.W * max(widths) >= TWO32
    assert lc.instantiation(bt.twin_row(r, N)) == '', 'the query (which launches nothing) must refuse first'
    _refused(*bt.entry_call(r, N))


def test_dgrad_bb_refuses_at_4gb():
    r = next(r for r in lc.ROWS if r.op == 'dgrad_bb' and r.Cout == 256)
    per = r.H * r.W * 256 * 2
    N = -(-TWO32 // per)
    N += N % 2
    assert lc.bb_inst(N - 2, r.H, r.W, r.Cout, (N - 2) // 2) == r.inst and lc.bb_inst(N, r.H, r.W, r.Cout, N // 2) == ''
    _refused(*bt.entry_call(r, N))


def test_pack_input_refuses_at_its_bound():
    """head.hip: 2 B H W Cpad / 4 units must stay below 2^31 (the unit index is divided in 32 bits)."""
    B = TWO31 // (2 * 128 * 128 * 4)                       # Cpad = 16
    assert 2 * B * 128 * 128 * 4 == TWO31
    _refused('bdn_pack_input', (BDN_BF16, 16, 16, 16, B, 13, 128, 128, 16, None), match='reaches 2\\^31')


def test_weight_gradient_plans_switch_at_two_to_the_31_elements():
    lib = _lib.load()
    H, W = 61, 125
    for C in (64, 128):
        n_hi = -(-TWO31 // (H * W * C))                    # the first N with N H W C >= 2^31
        n_hi += n_hi % 2
        n_lo = n_hi - 2
        assert n_lo * H * W * C < TWO31 <= n_hi * H * W * C
        for mode in (IN_PLAIN, IN_BNRELU):
            assert lib.bdn_conv3x3_wgrad_variant(BDN_BF16, n_lo, H, W, C, C, 0, n_lo // 2, mode, 0) == WG_ROLE
            assert lib.bdn_conv3x3_wgrad_variant(BDN_BF16, n_hi, H, W, C, C, 0, n_hi // 2, mode, 0) == WG_SIMPLE
        assert lc.wgrad_inst(BDN_BF16, n_lo, H, W, C, C, 0, n_lo // 2, IN_PLAIN)[0] == 'wgrad7_kernel<false>'
        assert lc.wgrad_inst(BDN_BF16, n_hi, H, W, C, C, 0, n_hi // 2, IN_PLAIN)[0] == 'wgrad_kernel<bf16,8,16,1,false>'
        assert lc.wgrad_inst(BDN_BF16, n_lo, H, W, C, C, 0, n_lo // 2, IN_BNRELU)[0] == 'wgrad7_kernel<true>'
        # the split operands are twice as wide: the fused kernel leaves at half the N
        m_hi = -(-TWO31 // (H * W * 2 * C))
        m_hi += m_hi % 2
        m_lo = m_hi - 2
        for dt, k in ((BDN_BF16X3, 3), (BDN_BF16X2, 2)):
            assert lc.wgrad_inst(dt, m_lo, H, W, C, C, 0, m_lo // 2, IN_PLAIN)[0] == f'wgrad7x_kernel<{k}>'
            assert lc.wgrad_inst(dt, m_hi, H, W, C, C, 0, m_hi // 2, IN_PLAIN)[0] == 'wgrad_kernel<bf16,8,16,1,false>+wgrad_x3_combine_kernel'
    # the first layer's fused kernel: N H W 64 < 2^31
    n_hi = -(-TWO31 // (H * W * 64))
    n_hi += n_hi % 2
    n_lo = n_hi - 2
    for dt in (BDN_BF16, BDN_BF16X3, BDN_BF16X2):
        assert lib.bdn_conv3x3_wgrad_bnbwd_supported(dt, n_lo, H, W, 64, 16, n_lo // 2) == 1
        assert lib.bdn_conv3x3_wgrad_bnbwd_supported(dt, n_hi, H, W, 64, 16, n_hi // 2) == 0
        assert lc.wgrad_bnbwd_inst(dt, n_lo, H, W, 64, 16, n_lo // 2)[0] != ''
        assert _lib.load().bdn_conv3x3_wgrad_bnbwd_kernels(dt, n_hi, H, W, 64, 16, n_hi // 2) == b''
    assert lib.bdn_conv3x3_wgrad_variant(BDN_F32, 4, H, W, 64, 64, 0, 2, IN_PLAIN, 0) == WG_SIMPLE


def test_scene_batch_bound_is_the_documented_one():
    """utils/inference._check_widest: 1023 (bf16), 511 (fp32) and 511 (bf16x3) tiles of 128 x 128 pass, one more is refused."""
    from fabric_amd.engine import BiDateEngine
    from fabric_amd.utils.inference import _check_widest
    for prec, top in (('bf16', 1023), ('fp32', 511), ('bf16x3', 511)):
        eng = BiDateEngine(13, 2, prec)
        _check_widest(eng, top, 128)
        _check_widest(eng, top - 1, 128)
        with pytest.raises(ValueError, match='4 GB'):
            _check_widest(eng, top + 1, 128)


# ------------------------------------------------------------------ the comparator
def _periodic(nblocks, reps, rows, cols, dtype):
    g = torch.Generator().manual_seed(3)
    per = torch.randn(nblocks, 1, rows, cols, generator=g).to(dtype)
    return per.expand(nblocks, reps, rows, cols).reshape(nblocks * reps * rows, cols).contiguous()


def _flip_bit(t, row, col, bit=0):
    v = t.view(bt._VIEW[t.element_size()])
    v[row, col] ^= (1 << bit)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('slab', [bt.SLAB_BYTES, 64], ids=['one-slab', 'many-slabs'])
def test_comparator(dtype, slab):
    nblocks, reps, rows, cols = 2, 5, 3, 4
    es = torch.empty((), dtype=dtype).element_size()
    clean = _periodic(nblocks, reps, rows, cols, dtype)
    f = bt.period_findings(clean, nblocks, reps, slab)
    assert f == {'differ': 0, 'first_differ': None, 'unwritten': 0, 'first_unwritten': None}
    bt.assert_periodic('clean', clean, nblocks, reps)
    assert torch.equal(bt.period0(clean, nblocks, reps).view(nblocks, rows, cols), clean.view(nblocks, reps, rows, cols)[:, 0])
    # one bit in a far period: block 1, period 3, row 2, column 1
    far = clean.clone()
    _flip_bit(far, (1 * reps + 3) * rows + 2, 1)
    f = bt.period_findings(far, nblocks, reps, slab)
    assert f['differ'] == 1 and f['first_differ'] == (1, 3, (2 * cols + 1) * es) and f['unwritten'] == 0
    with pytest.raises(AssertionError, match=r'differ from period 0.*\(1, 3, '):
        bt.assert_periodic('far', far, nblocks, reps)
    # one bit in period 0 of block 0: every other period of the block now differs from it
    p0 = clean.clone()
    _flip_bit(p0, 1, 2, bit=3)
    f = bt.period_findings(p0, nblocks, reps, slab)
    assert f['differ'] == reps - 1 and f['first_differ'] == (0, 1, (1 * cols + 2) * es)
    # an element nobody wrote
    born = clean.clone()
    born.view(torch.uint8).view(-1, cols * es)[(0 * reps + 4) * rows + 0, 3 * es:4 * es] = 0xFF
    f = bt.period_findings(born, nblocks, reps, slab)
    assert f['unwritten'] == 1 and f['first_unwritten'] == (0, 4, 3 * es) and f['differ'] == 1
    with pytest.raises(AssertionError, match='still hold the 0xFF'):
        bt.assert_periodic('born', born, nblocks, reps)
    # ... in period 0 of every period alike (a kernel that skips the same element everywhere): still reported
    allp = clean.clone().view(nblocks, reps, rows, cols)
    allp.view(torch.uint8).view(nblocks, reps, rows, cols * es)[:, :, 1, 0:es] = 0xFF
    f = bt.period_findings(allp.view(-1, cols), nblocks, reps, slab)
    assert f['differ'] == 0 and f['unwritten'] == nblocks * reps and f['first_unwritten'] == (0, 0, 1 * cols * es)


def test_comparator_on_bytes():
    m = torch.tensor([0, 1, 1, 0] * 6, dtype=torch.uint8).view(12, 2)       # 3 periods of 2 rows x 2 blocks ... as [12, 2]
    assert bt.period_findings(m, 2, 3)['differ'] == 0
    m[7, 1] = 255
    f = bt.period_findings(m, 2, 3)
    assert f['unwritten'] == 1 and f['first_unwritten'] == (1, 0, 3) and f['differ'] == 2


def test_tile_builds_blocks_of_periods():
    small = torch.arange(4 * 3, dtype=torch.float32).view(4, 3)              # 2 blocks x P = 2
    big = bt.tile(small, 2, 12, lambda shape, dtype: torch.empty(shape, dtype=dtype))
    assert big.shape == (12, 3)
    assert torch.equal(big[:6], small[:2].repeat(3, 1)) and torch.equal(big[6:], small[2:].repeat(3, 1))
    assert bt.period_findings(big, 2, 3)['differ'] == 0
    assert torch.equal(bt.period0(big, 2, 3), small)


# ------------------------------------------------------------------ integer-valued data
def test_integer_data_sums_exactly_in_any_order():
    x = bt.int_values((64, 9, 50), 5)
    y = bt.int_values((64, 9, 50), 6, values=(-3, -1, 1, 2), density=0.5, scale=2.0 ** -3)
    assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.equal(y.to(torch.bfloat16).float(), y)
    assert 0.3 < (y != 0).float().mean() < 0.7
    terms = (x * y).reshape(-1)
    unit = 2.0 ** -3
    reps = 100
    assert bt.exact_in_f32(terms.abs().sum().item(), reps, unit)
    assert not bt.exact_in_f32(terms.abs().sum().item(), 10 ** 6, unit)
    exact = int((terms.double() / unit).round().to(torch.int64).sum().item())
    big = terms.repeat(reps)
    fwd = torch.zeros((), dtype=torch.float32)
    for chunk in big.split(997):                          # sequential float32 accumulation of chunk sums
        fwd = fwd + chunk.sum(dtype=torch.float32)
    perm = big[torch.randperm(big.numel(), generator=torch.Generator().manual_seed(1))]
    other = perm.view(-1, 100).sum(0, dtype=torch.float32).flip(0).cumsum(0, dtype=torch.float32)[-1]
    want = torch.tensor(exact * reps * unit, dtype=torch.float32)
    assert exact * reps * unit == float(want)              # representable
    assert fwd.view(torch.int32) == want.view(torch.int32) and other.view(torch.int32) == want.view(torch.int32)


# ------------------------------------------------------------------ weight-gradient twins
WG = bt.wg_twins()


@pytest.mark.parametrize('tw', WG, ids=bt.wg_twin_id)
def test_weight_gradient_chooser(tw):
    r = tw.row
    assert tw.G == 2 and tw.P % 2 == 0 and tw.N % (tw.G * tw.P) == 0
    ts = bt.wg_tensors(r)
    assert tw.widest_bytes == max(tw.N * x.pix * x.bpp for x in ts)
    for x in ts:
        assert TWO31 % (tw.P * x.pix * x.bpp) and TWO32 % (tw.P * x.pix * x.bpp)
    if tw.size == 'cross':
        assert TWO31 + tw.period_bytes <= tw.widest_bytes < TWO31 + tw.period_bytes + tw.step_bytes
    elif tw.size == 'top':
        assert TWO32 - tw.step_bytes <= tw.widest_bytes < TWO32
    else:
        assert TWO32 <= tw.widest_bytes < TWO32 + tw.step_bytes
    assert tw.mem_bytes <= bt.MEM_CAP
    # the library's plan: the row's kernel up to 'top', wgrad_kernel on the far side of 2^31 elements
    assert lc.instantiation(bt.twin_row(r, tw.N)) == tw.inst
    if r.inst.startswith('wgrad7'):
        x3 = r.inst.startswith('wgrad7x')
        elems = tw.N * r.H * r.W * (2 if x3 else 1) * max(r.Cout, r.C0, r.C1)
        assert (elems < TWO31) == (tw.size != 'far') and (tw.inst == r.inst) == (tw.size != 'far')
    else:
        assert tw.inst == r.inst


@pytest.mark.parametrize('r', [r for r in lc.ROWS if r.op == 'wgrad'], ids=lc.row_id)
def test_weight_gradient_integer_data(r):
    """The period's data at the density of the largest twin: integers (split operands: multiples of LO with non-zero lo halves) whose sum of
    |terms| over the whole tensor stays below 2^24 units (wg_case asserts it from the data), exact in bf16, and not degenerate."""
    far = bt.wg_choose(r, 'far')
    rs = r._replace(N=far.G * far.P, ipg=far.P)
    c = bt.wg_case(rs, far.N)
    reps = far.N // rs.N
    assert bt.exact_in_f32(c['abs_sum'], reps, c['unit']) and 0 < c['density'] <= 1
    x3 = r.prec in ('bf16x3', 'bf16x2')
    for k in ('x0', 'x1', 'dz'):
        t = c[k]
        if t is None:
            continue
        hi = t.to(torch.bfloat16).float()
        lo = (t - hi).to(torch.bfloat16).float()
        assert torch.equal(hi + lo, t), 'not exact as hi + lo'
        if x3:
            assert (lo != 0).any() and torch.equal(hi, hi.round()), 'the lo half must be non-zero and the hi half the integer part'
        else:
            assert torch.equal(hi, t)
    # every group's period carries gradient
    P = far.P
    assert all((c['dz'][g * P:(g + 1) * P] != 0).any() for g in range(far.G))
    assert (c['ref'] * reps / c['unit']).abs().max() < 2 ** 24


# ------------------------------------------------------------------ stage-boundary twins
@pytest.mark.parametrize('s', bt.stage_twins() + bt.stage_backward_twins() + bt.outc_twins(), ids=bt.stage_id)
def test_stage_chooser(s):
    edge = {'cross': TWO31, 'far': TWO32}[s.size]
    assert s.P % 2 == 0 and s.N % (2 * s.P) == 0
    assert s.widest_bytes == max(int(s.N * x.imgs) * x.pix * x.bpp for x in s.tensors)
    assert edge + s.period_bytes <= s.widest_bytes < edge + s.period_bytes + s.step_bytes
    for x in s.tensors:
        assert TWO31 % (s.P * x.pix * x.bpp) and TWO32 % (s.P * x.pix * x.bpp)
    assert s.mem_bytes <= bt.MEM_CAP
    assert s.N // 2 * s.H * s.W < TWO31                    # the kernels' int pixel indices (per group / per date) are far from their range
    assert (s.H, s.W, s.C) in bt.STAGE_SHAPES


# ------------------------------------------------------------------ the first layer's fused weight gradient
@pytest.mark.parametrize('tw', bt.wb_twins(), ids=bt.wb_twin_id)
def test_first_layer_weight_gradient_chooser_and_data(tw):
    r = tw.row
    lib = _lib.load()
    assert tw.G == 2 and tw.P % 2 == 0 and tw.N % (tw.G * tw.P) == 0 and tw.mem_bytes <= bt.MEM_CAP
    for x in bt.wb_tensors(r):
        assert TWO31 % (tw.P * x.pix * x.bpp) and TWO32 % (tw.P * x.pix * x.bpp)
    dt = lc.DTYPE[r.prec]
    assert lib.bdn_conv3x3_wgrad_bnbwd_supported(dt, tw.N, r.H, r.W, 64, 16, tw.N // 2) == 1
    assert lc.instantiation(bt.twin_row(r, tw.N)) == r.inst
    if tw.size == 'cross':
        assert TWO31 + tw.period_bytes <= tw.widest_bytes < TWO31 + tw.period_bytes + tw.step_bytes
    else:
        n = tw.N + tw.G * tw.P                             # the next N is outside the supported class: refused before anything is launched
        assert n * r.H * r.W * 64 >= TWO31 and lib.bdn_conv3x3_wgrad_bnbwd_supported(dt, n, r.H, r.W, 64, 16, n // 2) == 0
        with pytest.raises(RuntimeError, match='wgrad_bnbwd: only') as e:
            _lib.call('bdn_conv3x3_wgrad_bnbwd', dt, 16, bt.WB_LDA, 16, 16, 16, n // 2, 64, 16, 16, 16, 16, 13, n, r.H, r.W, None)
        assert 'rc=-2' in str(e.value)
        assert tw.widest_bytes >= TWO32                    # the wider dA passes 4 GB inside the supported range
        rs = r._replace(N=tw.G * tw.P, ipg=tw.P)
        c = bt.wb_case(rs, tw.N)                           # asserts the 2^24 bound from the data
        assert bt.exact_in_f32(c['abs_sum'], tw.N // rs.N, c['unit'])
        if r.prec != 'bf16':
            hi = c['x'].to(torch.bfloat16).float()
            assert ((c['x'] - hi) != 0).any() and torch.equal(hi, hi.round())


@pytest.mark.parametrize('s', bt.bn_bwd_twins(), ids=bt.stage_id)
def test_bn_bwd_chooser_and_data(s):
    test_stage_chooser(s)
    if s.size == 'far':
        c = bt.bn_bwd_case(s.C, s.H, s.W, s.P, s.N)        # asserts the 2^24 bound from the data
        want = c['sums'] * (s.N // (2 * s.P))
        assert torch.equal(want.float().double(), want) and want.abs().max() < 2 ** 24
        assert torch.equal(c['dA'].to(torch.bfloat16).float(), c['dA']) and torch.equal(c['z'].to(torch.bfloat16).float(), c['z'])


# ------------------------------------------------------------------ integer cases of the reductions over N x tiles rows
def test_integer_cases_of_the_big_reductions():
    """The builders assert integrality, bf16 range and the 2^24 bound themselves; here: their totals are float32 numbers at the largest N."""
    rows = {lc.row_id(t.row): t for t in CASES if t.twin.size == 'top'}
    for rid, maker, field in (('fwd-bf16-4x29x45-64-64-g2-bnrelu', bt.int_forward_case, 'totals'),
                              ('dgrad_bs-fp32-4x29x45-64-64-g2', bt.int_dgrad_bs_case, 'sums')):
        t = rows[rid]
        rs = bt.small_row(t.row, t.twin.P)
        c = maker(rs)
        tot = getattr(c, field) * (t.twin.N // rs.N)
        assert torch.equal(tot, tot.round()) and (tot != 0).float().mean() > 0.9 and tot.abs().max() < 2 ** 53
        if field == 'sums':
            assert torch.equal(tot.float().double(), tot)
        for x in (c.ref, c.w):
            assert torch.equal(x.to(torch.bfloat16).double(), x.double())
    far = bt.stage_choose('enc_skip_bwd', 'bf16', 64, 64, 64, 'far')
    c = bt.int_enc_skip_case(64, 64, 64, far.P)
    tot = c['sums'] * (far.N // (2 * far.P))
    assert torch.equal(tot.float().double(), tot) and torch.equal(c['g'].to(torch.bfloat16).double(), c['g'])
    far = bt.stage_choose('outc', 'bf16', 64, 64, 64, 'far')
    c = bt.int_outc_case(64, 64, 64, far.P, far.N)
    reps = far.N // (2 * far.P)
    for k in ('dw', 'db', 'sums'):
        assert torch.equal((c[k] * reps).float().double(), c[k] * reps)
    t = bt.tile(torch.arange(8.).view(4, 2), 2, 8, lambda shape, dtype: torch.empty(shape, dtype=dtype))
    assert bt.n_reaching(10, 3, 4) == 4 and bt.n_below(10, 3, 4) == 0 and bt.n_below(25, 3, 4) == 8 and t.shape == (8, 2)
