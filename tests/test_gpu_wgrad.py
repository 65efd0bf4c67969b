"""GPU tests of the weight-gradient kernels (csrc/wgrad.hip: msdf_wgrad_k, msdf_wgrad_b16_k, msdf_reduce_k), item by
item and exactly.

The operands are small integers stored as fp32 (uniform in -3 ... 3), so every product, partial sum, split partial and
reduced sum is an integer below 2^24: fp32 accumulation is exact in any order and the expected gradient is the float64
product of tests/wgrad_numpy.py cast to fp32, compared with == on every element.  Small integers are exact in bf16 too
(lo plane 0), so the same data pins the bf16x3 kernel's hi path and addressing; its lo planes get a data set of their
own (x = a + b 2^-10).  Each test asserts that precondition on the data it generated.

Partial buffer and destination are pre-filled with NaN (the library allocates them uninitialised when the plan claims
full coverage), so an element nobody wrote shows, and both are followed by a guard band that must stay untouched."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import wgrad_numpy as wn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monosdf_amd import _lib, plan as planlib  # noqa: E402

F32, BF16X3 = 0, 1
PREC_MODE = {F32: 'fp32', BF16X3: 'bf16x3'}
GUARD = 256
EXACT = float(2 ** 24)


def _sentinel(n, dev):
    return -(torch.arange(n, device=dev, dtype=torch.float32) + 7001.0)


def _dev_tables(prog, maps_np, dev):
    return dict(items=torch.from_numpy(prog.items_bytes()).to(dev), wg_map=torch.from_numpy(prog.wg_map()).to(dev),
                rules=torch.from_numpy(prog.rules_bytes()).to(dev),
                maps=torch.from_numpy(np.ascontiguousarray(maps_np, np.int32)).to(dev))


def _check_part_layout(prog):
    """Every partial block an item writes and every block range a rule reads lies inside [0, part_f)."""
    for it in prog.items:
        S = it['n_splits']
        assert S >= 1 and it['wx'] % 16 == 0 and it['wy'] % 16 == 0
        for off, n in ((it['part_off'], it['wx'] * it['wy']), (it['colsum_off'], it['wx']), (it['vrow_off'], it['wy'])):
            if n > 0 and off >= 0:
                assert off + S * n <= prog.part_f
    for r in prog.rules:
        assert 0 <= r.part_off and r.part_off + r.n_blocks * r.wx * r.wy <= prog.part_f


def run_program(prog, maps_np, bufs_dev, P_pad, n_total, precision):
    """The two launches of ops.FusedMlp.run_wgrad over NaN-filled, guarded buffers -> flat gradient [n_total] (numpy)."""
    dev = bufs_dev['ws'].device
    _check_part_layout(prog)
    t = _dev_tables(prog, maps_np, dev)
    part = torch.full((prog.part_f + 64 + GUARD,), float('nan'), device=dev)
    grad = torch.full((n_total + GUARD,), float('nan'), device=dev)
    part[prog.part_f + 64:] = _sentinel(GUARD, dev)
    grad[n_total:] = _sentinel(GUARD, dev)
    st = _lib.stream_ptr()
    _lib.call('msdf_wgrad', _lib.ptr(t['items']), _lib.ptr(t['wg_map']), t['wg_map'].numel() // 2, _lib.ptr(part), P_pad,
              precision, _lib.ptr(bufs_dev['ws']), _lib.ptr(bufs_dev.get('feat')), st)
    _lib.call('msdf_reduce', _lib.ptr(t['rules']), len(prog.rules), _lib.ptr(t['maps']), _lib.ptr(part), _lib.ptr(grad),
              st)
    torch.cuda.synchronize()
    assert torch.equal(part[prog.part_f + 64:], _sentinel(GUARD, dev)), 'store behind the partial buffer'
    assert torch.equal(grad[n_total:], _sentinel(GUARD, dev)), 'store behind the gradient'
    assert torch.isnan(part[prog.part_f:prog.part_f + 64]).all(), 'store into the slack of the partial buffer'
    return grad[:n_total].cpu().numpy()


def assert_exact_precondition(prog, bufs, P_pad, unit=1.0):
    """n_terms * K * max|x| * max|y| < 2^24 in units of `unit` (also covers v * y and the column sums)."""
    m = max(float(np.abs(b).max()) for b in bufs.values())
    bound = wn.terms_per_rule(prog) * P_pad * max(m * m, m) / unit
    assert bound < EXACT, bound
    return bound


# ---------------------------------------------------------------------------
# 3a. synthetic single-rule programs
# ---------------------------------------------------------------------------
class Synth:
    """One reduce rule fed by one or two items of the same shape (+ the column-sum and v-row rules of the first)."""

    def __init__(self, wx, wy, n_stages=3, splits=(2,), colsum=True, vrow=False, x_pad=0, y_pad=0, y_c0=0,
                 xbuf='ws', ybuf='ws', vbuf='ws', y_is_x=False, holes=True, scale=1.0, dst_pad=0):
        self.__dict__.update(locals())
        del self.__dict__['self']
        self.P_pad = P_pad = 32 * n_stages
        assert y_c0 % 16 == 0 and x_pad % 16 == 0 and y_pad % 16 == 0 and (wy > 0 or not vrow)
        sizes = {'ws': 64, 'feat': 64}
        self.regions = []                 # (buffer, offset, row pitch, width, kind)

        def region(buf, ld, w, kind, c0=0):
            off = sizes[buf]
            sizes[buf] += (P_pad * ld + 63) & ~63
            self.regions.append((buf, off + c0, ld, w, kind))
            return (buf, off + c0)

        prog = planlib.WgradProgram(lambda w: splits[0], P_pad)
        n = wx * wy
        x_ld = wx + x_pad
        y_ld = x_ld if y_is_x else y_c0 + wy + y_pad
        assert not y_is_x or y_c0 + wy <= x_ld
        part = prog.alloc(sum(splits) * n)
        cs = vr = -1
        off = part
        for t, S in enumerate(splits):
            x = region(xbuf, x_ld, wx, 'x')
            y = None
            if wy > 0:
                y = (x[0], x[1] + y_c0) if y_is_x else region(ybuf, y_ld, wy, 'y', y_c0)
            v = None
            if t == 0 and colsum:
                cs = prog.alloc(S * wx)
            if t == 0 and vrow:
                v = region(vbuf, 1, 1, 'v')
                vr = prog.alloc(S * wy)
            prog.add_item(x, x_ld, wx, y, y_ld if wy > 0 else 0, wy, off, S, colsum_off=(cs if t == 0 else -1), v=v,
                          vrow_off=(vr if t == 0 else -1))
            off += S * n
        self.sizes = sizes

        rng = np.random.default_rng(1000 * wx + wy)

        def slot_map(w, shift):
            m = np.full(w, -1, np.int32)
            valid = np.array([i for i in range(w) if not (holes and (i == 5 or i >= w - 3))])
            m[valid] = shift + rng.permutation(len(valid)) if holes else shift + np.arange(len(valid))
            return m, len(valid)

        rowmap, n_rows = slot_map(wx, 1 if vrow else 0)
        colmap, n_cols = slot_map(wy, 0) if wy > 0 else (np.zeros(0, np.int32), 0)
        n_rows += 1 if vrow else 0
        self.maps = np.concatenate([np.full(3, -1, np.int32), rowmap, colmap])
        rm, cm = 3, 3 + wx
        dst_ld = n_cols + dst_pad
        n_w = n_rows * dst_ld
        if wy > 0:
            prog.add_rule(part, sum(splits), wx, wy, rm, cm, 0, dst_ld, scale)
        if vrow:
            prog.add_rule(vr, splits[0], 1, wy, -1, cm, 0, dst_ld, scale, fixed_row=0)
        if colsum:
            prog.add_rule(cs, splits[0], wx, 1, rm, -1, n_w, 1, 1.0)
        self.prog, self.n_total = prog, n_w + n_rows

    def data(self, kind, seed):
        """'rand': every float of both buffers (the padding columns too) an integer in -3 ... 3;
        'first' / 'last': zero but for one point of every operand; 'lo': a + b 2^-10, v integer."""
        rng = np.random.default_rng(seed)
        if kind == 'rand':
            return {k: rng.integers(-3, 4, n).astype(np.float32) for k, n in self.sizes.items()}
        if kind == 'lo':
            bufs = {}
            for k, n in self.sizes.items():
                # b takes a's sign (and is 0 where a is): |x| = |a| + |b| 2^-10 rounds to hi = a, lo = b 2^-10.  With
                # opposite signs 1 - 3 2^-10 lies below 1, where bf16 is finer, and hi would not be an integer
                a = rng.integers(-3, 4, n)
                b = rng.integers(0, 4, n) * np.sign(a)
                bufs[k] = (a + b * 2.0 ** -10).astype(np.float32)
            for buf, off, ld, w, what in self.regions:
                if what == 'v':
                    bufs[buf][off:off + self.P_pad] = rng.integers(-3, 4, self.P_pad)
            return bufs
        p = {'first': 0, 'last': self.P_pad - 1}[kind]
        bufs = {k: np.zeros(n, np.float32) for k, n in self.sizes.items()}
        for buf, off, ld, w, what in self.regions:
            bufs[buf][off + p * ld:off + p * ld + w] = rng.integers(1, 4, w) * rng.choice([-1, 1], w)
        return bufs


def run_synth(c, precision, kind='rand', seed=0):
    bufs = c.data(kind, seed)
    if kind == 'lo':
        # hi integer, lo a multiple of 2^-10, lo * lo dropped: every partial sum is a multiple of 2^-10
        for b in bufs.values():
            hi, lo = wn.bf16_split(b)
            assert (hi == np.round(hi)).all() and (lo * 1024 == np.round(lo * 1024)).all() and np.abs(lo).max() > 0
            np.testing.assert_array_equal(hi + lo, b)
        assert c.P_pad <= 1024
        assert_exact_precondition(c.prog, bufs, c.P_pad, unit=2.0 ** -10)
    else:
        assert_exact_precondition(c.prog, bufs, c.P_pad)
    want = wn.reference_grad(c.prog, c.maps, bufs, c.P_pad, c.n_total, init=np.nan, mode=PREC_MODE[precision])
    bufs_dev = {k: torch.from_numpy(v).cuda() for k, v in bufs.items()}
    got = run_program(c.prog, c.maps, bufs_dev, c.P_pad, c.n_total, precision)
    np.testing.assert_array_equal(got, want)      # NaN == NaN here: elements no rule stores to must stay NaN
    assert np.isfinite(want).any()
    return got, want


# fp32 grids (msdf_wgrad_k): thin = wx <= 32 and wy > 32 (1 x 8 waves of 32 x 32); otherwise by columns: NBN 2 (<= 64),
# 3 (<= 96), 4 (<= 128): 8 x 1 waves of 32 rows; wide (> 128): 2 x 4 waves of 128 x 64.
# bf16x3 grids (msdf_wgrad_b16_k): narrow (wy <= 64): 8 x 1 waves of 32 x 64; wide: 2 x 4 waves of 128 x 64.
SHAPES = [
    (16, 0),      # column sums only, one 16-row piece pair: every wave re-copies the clamped last piece
    (256, 0),     # column sums only, full width
    (16, 16),     # NBN 2: wave 0 alone, half a row tile and half a column tile; waves 1-7 inactive
    (32, 32),     # NBN 2 (wx <= 32 but wy <= 32 is not thin): wave 0's first tile exactly, second column tile off
    (256, 16),    # NBN 2: all 8 wave rows, column tail of 16
    (256, 48),    # NBN 2: second column tile half used (the PE block of the headline networks)
    (256, 64),    # NBN 2: both column tiles full; bf16x3 narrow grid full
    (48, 64),     # NBN 2: wave 1 half a row tile, waves 2-7 inactive
    (240, 48),    # NBN 2: last wave row half used
    (112, 32),    # NBN 2: wave 3 half used, waves 4-7 inactive
    (16, 48),     # thin: waves 0-1 (wave 1 a 16-column tail), waves 2-7 inactive; 16 of 32 rows
    (32, 64),     # thin: two full waves
    (16, 144),    # thin: five waves, 16-column tail
    (32, 256),    # thin: all 8 waves full (first and last column tile)
    (256, 80),    # NBN 3: third column tile half used (PE + hash features of the headline grid network)
    (256, 96),    # NBN 3 full
    (144, 80),    # NBN 3: wave 4 half a row tile, waves 5-7 inactive
    (48, 96),     # NBN 3: waves 2-7 inactive
    (256, 112),   # NBN 4: fourth column tile half used
    (256, 128),   # NBN 4 full
    (128, 128),   # NBN 4: waves 4-7 inactive; bf16x3 wide: wave row 1 and wave columns 2-3 inactive
    (224, 112),   # NBN 4: wave 7 inactive, tails in both directions
    (256, 144),   # wide: wave column 2 has 16 columns, wave column 3 inactive
    (256, 208),   # wide: wave column 3 has 16 columns
    (144, 256),   # wide: wave row 1 has 16 rows (one of its four row tiles, half used)
    (128, 256),   # wide: wave row 1 inactive
    (112, 144),   # wide: inactive wave row and wave column, tails in both
    (48, 256),    # wide (48 rows is not thin): two of wave row 0's four row tiles
    (240, 208),   # wide: last row tile and last column tile half used
    (224, 256),   # wide: the feature rows of the 217-wide skip layer
    (256, 256),   # wide, full: first and last tile of every wave
]
PRECISIONS = [pytest.param(F32, id='fp32'), pytest.param(BF16X3, id='bf16x3')]
GRID_SHAPES = [(32, 80), (256, 48), (256, 80), (256, 128), (256, 256)]      # thin, NBN 2 / 3 / 4, wide
_shape_id = lambda s: '%dx%d' % s


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('shape', SHAPES, ids=_shape_id)
def test_item_shapes(shape, precision):
    """Every wave grid with its first / last tiles, tails and inactive waves: 3 stages in 2 splits (2 + 1), holed maps,
    column sums on."""
    run_synth(Synth(*shape), precision)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('kw', [
    dict(wx=256, wy=256, colsum=False), dict(wx=256, wy=256, colsum=False, vrow=True),
    dict(wx=256, wy=256, colsum=True, vrow=True), dict(wx=16, wy=256, colsum=True, vrow=True),
    dict(wx=256, wy=48, colsum=True, vrow=True), dict(wx=256, wy=80, colsum=False, vrow=True),
    dict(wx=256, wy=128, colsum=True, vrow=True), dict(wx=256, wy=48, colsum=False),
], ids=lambda kw: '%dx%d_cs%d_v%d' % (kw['wx'], kw['wy'], kw['colsum'], kw.get('vrow', False)))
def test_side_products(kw, precision):
    """Column sums and the v-weighted row on and off (wy = 256: the last of the 256 v-row threads)."""
    run_synth(Synth(n_stages=9, splits=(4,), **kw), precision)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('kw', [
    dict(wx=224, wy=256, x_pad=32),                                   # x_ld > wx (feature rows of the last layer's a-bar)
    dict(wx=256, wy=48, y_pad=16, y_c0=256),                          # the skip layer's QB + c0 block
    dict(wx=256, wy=256, y_pad=48, y_c0=0),                           # ... and its first 256 columns
    dict(wx=256, wy=256, xbuf='ws', ybuf='feat'),                     # the colour network's first unit
    dict(wx=16, wy=80, xbuf='feat', ybuf='ws', vbuf='feat', vrow=True, x_pad=16, y_c0=32),
    dict(wx=256, wy=256, y_is_x=True),                                # Y = X region
    dict(wx=256, wy=80, y_is_x=True, y_c0=16, vrow=True),             # ... a column window of it
], ids=lambda kw: '_'.join('%s%s' % (k, v) for k, v in kw.items()))
def test_operand_placement(kw, precision):
    run_synth(Synth(**kw), precision)


RANGES = [(1, 1), (1, 4), (2, 1), (2, 2), (3, 2), (3, 5), (9, 3), (9, 4), (9, 6), (67, 1), (67, 8), (67, 67)]


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('shape', [(256, 256), (256, 48), (32, 80)], ids=_shape_id)
@pytest.mark.parametrize('rng_', RANGES, ids=lambda r: '%dst_%dsp' % r)
def test_point_ranges(rng_, shape, precision):
    """Exact division (9 / 3), short last split (3 / 2, 67 / 8), empty last split (9 / 6: per = 2, split 5 starts behind
    the end; 9 / 4), more splits than stages (1 / 4, 3 / 5), one stage per split (67 / 67), a single workgroup."""
    n_stages, n_splits = rng_
    assert [e - b for b, e in wn.split_ranges(9, 6)] == [2, 2, 2, 2, 1, 0]
    run_synth(Synth(*shape, n_stages=n_stages, splits=(n_splits,), vrow=True), precision)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('kind', ['first', 'last'])
@pytest.mark.parametrize('shape', GRID_SHAPES, ids=_shape_id)
def test_single_point(shape, kind, precision):
    """Only the first point of the first stage / the last point of the last non-empty split is non-zero (9 stages in 6
    splits: the last point sits in the short split 4): a dropped edge point cannot hide in a sum."""
    c = Synth(*shape, n_stages=9, splits=(6,), vrow=True)
    got, _ = run_synth(c, precision, kind=kind, seed=3)
    assert np.nanmax(np.abs(got)) >= 1


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('kw', [
    dict(splits=(1,)), dict(splits=(3, 4)), dict(splits=(8,)), dict(splits=(4, 5)), dict(splits=(8, 9)),   # 1 7 8 9 17
    dict(splits=(7,), holes=False), dict(splits=(9,), scale=math.sqrt(0.5), dst_pad=5),
    dict(splits=(3, 4), scale=math.sqrt(0.5), dst_pad=1, vrow=True),
    dict(splits=(17,), scale=math.sqrt(0.5), holes=False, dst_pad=16),
], ids=lambda kw: '_'.join('%s%s' % (k, v) for k, v in kw.items()).replace(' ', ''))
@pytest.mark.parametrize('shape', [(256, 256), (48, 16)], ids=_shape_id)
def test_reduce_rules(shape, kw, precision):
    """Block counts around the 8-way unroll, -1 slots, fixed_row, scale 1 and float32(sqrt(1/2)), dst_ld > wy."""
    kw = dict(kw)
    if 'scale' in kw:
        kw['scale'] = float(np.float32(kw['scale']))
    run_synth(Synth(*shape, n_stages=9, **kw), precision)


@pytest.mark.parametrize('kw', [dict(colsum=False), dict(colsum=True, vrow=True)], ids=['mm', 'all'])
@pytest.mark.parametrize('shape', [(256, 64), (256, 256), (112, 144), (48, 32)], ids=_shape_id)
def test_bf16x3_lo_planes(shape, kw):
    """x = a + b 2^-10: hi = a, lo = b 2^-10, result hi^T hi + hi^T lo + lo^T hi exactly (K = 1024, both grids)."""
    run_synth(Synth(*shape, n_stages=32, splits=(5,), **kw), BF16X3, kind='lo', seed=11)


# ---------------------------------------------------------------------------
# 3b. the real programs
# ---------------------------------------------------------------------------
REAL = [('mlp', 32), ('mlp', 64), ('mlp', 4096), ('mlp', 104448), ('grid', 32), ('grid', 64), ('grid', 4096),
        ('grid', 104448), ('color', 100352), ('sdf64', 100352)]


@pytest.mark.parametrize('name,P_pad', REAL, ids=['%s_%d' % r for r in REAL])
def test_real_programs(name, P_pad):
    """The library's own programs (fp32: balanced_program; bf16x3: uniform_program) over
    a synthetic integer workspace, flat gradient [n_w + n_b] compared element by element."""
    from monosdf_amd import ops
    mp, build, wsfn, P_head = wn.headline_plans()[name]
    assert P_pad <= P_head
    _, total = wsfn(mp, P_pad)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(17 + P_pad)
    bufs_dev = {'ws': torch.empty(total, device='cuda').random_(-3, 4, generator=gen)}
    if mp.kind == 'color':
        bufs_dev['feat'] = torch.empty(P_pad * 256, device='cuda').random_(-3, 4, generator=gen)
    bufs = {k: v.cpu().numpy() for k, v in bufs_dev.items()}
    assert all(np.abs(b).max() == 3 and (b == np.round(b)).all() for b in bufs.values())
    n_total = mp.n_w + mp.n_b
    cache = {}
    for precision, pname in ((F32, 'fp32'), (BF16X3, 'bf16x3')):
        prog = ops.FusedMlp(mp, torch.device('cuda'), precision=pname).wgrad_program(P_pad)['prog']
        if pname == 'bf16x3':
            assert {it['n_splits'] for it in prog.items} == {max(1, -(-P_pad // (planlib.UNIFORM_STAGES_PER_SPLIT * planlib.STAGE_POINTS)))}
        assert_exact_precondition(prog, bufs, P_pad)
        # integer data: lo = 0, both kernels compute the plain product (the item sums are shared through `cache`)
        want = wn.reference_grad(prog, mp.maps_np, bufs, P_pad, n_total, init=np.nan, mode='fp32', cache=cache)
        assert not np.isnan(want).any()
        got = run_program(prog, mp.maps_np, bufs_dev, P_pad, n_total, precision)
        np.testing.assert_array_equal(got, want, err_msg='%s %s P_pad=%d' % (name, pname, P_pad))
    del bufs_dev, bufs, cache
    torch.cuda.empty_cache()


def test_float64_cross_check_of_the_bf16_mode_on_integers():
    """The real-program test hands integer data to the 'fp32' mode of the restatement for both kernels; at small size,
    the three-product definition gives the same."""
    mp, build, wsfn, _ = wn.headline_plans()['grid']
    _, total = wsfn(mp, 64)
    bufs = {'ws': np.random.default_rng(5).integers(-3, 4, total).astype(np.float32)}
    prog = planlib.balanced_program(build, mp, 64)
    a = wn.reference_grad(prog, mp.maps_np, bufs, 64, mp.n_w + mp.n_b, mode='fp32')
    b = wn.reference_grad(prog, mp.maps_np, bufs, 64, mp.n_w + mp.n_b, mode='bf16x3')
    np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# 3c. full-mantissa data, fp32 kernel: a derived bound, and run-to-run equality
# ---------------------------------------------------------------------------
def test_normal_data_within_the_summation_bound_and_reproducible():
    """Standard-normal operands at K = 104448 with the headline split counts, one item per family (wide 256 x 256,
    narrow 256 x 48, thin 16 x 256), element-wise against float64:  |d - d64| <= gamma (|X|^T |Y|) with
    gamma = K u / (1 - K u), u = 2^-23 -- the bound for any summation order when every operation has relative error
    <= u (2^-23, not 2^-24, so that it also holds should the matrix unit truncate).  Loose by design; the exact tests
    carry the weight.  The wide item is run 12 times over the same operands (816 workgroups: several rounds of the
    256 CUs); all copies and a second run of the whole program must be bit-equal (fixed order, no float atomics)."""
    K = 104448
    mlp, col = wn.headline_plans()['mlp'], wn.headline_plans()['color']
    S = {it['cls']: it['n_splits'] for it in planlib.balanced_program(mlp[1], mlp[0], K).items}
    S.update({it['cls']: it['n_splits'] for it in planlib.balanced_program(col[1], col[0], K).items
              if it['cls'] == planlib.THIN})
    shapes = [(256, 256, S[planlib.WIDE], 12), (256, 48, S[planlib.COLS64], 1), (16, 256, S[planlib.THIN], 1)]
    prog = planlib.WgradProgram(lambda w: 1, K)
    n_total, outs = 0, []
    xo = 0
    yo = K * 256
    for wx, wy, s, copies in shapes:
        for c in range(copies):
            part, cs = prog.alloc(s * wx * wy), prog.alloc(s * wx)
            prog.add_item(('ws', xo), 256, wx, ('ws', yo), 256, wy, part, s, colsum_off=cs)
            prog.add_rule(part, s, wx, wy, 0, 0, n_total, wy, 1.0)
            prog.add_rule(cs, s, wx, 1, 0, -1, n_total + wx * wy, 1, 1.0)
            outs.append((wx, wy, n_total))
            n_total += wx * wy + wx
    maps = np.arange(256, dtype=np.int32)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(31)
    ws = torch.randn(2 * K * 256, device='cuda', generator=gen)
    bufs_dev = {'ws': ws}
    got = run_program(prog, maps, bufs_dev, K, n_total, F32)
    again = run_program(prog, maps, bufs_dev, K, n_total, F32)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    host = ws.cpu().numpy().reshape(2, K, 256).astype(np.float64)
    X, Y = host[0], host[1]
    u = 2.0 ** -23
    gamma = K * u / (1 - K * u)
    worst = 0.0
    first = {}
    for wx, wy, o in outs:
        d = got[o:o + wx * wy].reshape(wx, wy)
        cs = got[o + wx * wy:o + wx * wy + wx]
        if (wx, wy) in first:
            assert np.array_equal(d, first[(wx, wy)])
            continue
        first[(wx, wy)] = d
        d64 = X[:, :wx].T @ Y[:, :wy]
        bound = gamma * (np.abs(X[:, :wx]).T @ np.abs(Y[:, :wy]))
        ratio = np.abs(d - d64) / bound
        cs_ratio = np.abs(cs - X[:, :wx].sum(0)) / (gamma * np.abs(X[:, :wx]).sum(0))
        print('wgrad %dx%d K=%d: max |d - d64| / bound = %.3e, column sums %.3e' % (wx, wy, K, ratio.max(),
                                                                                     cs_ratio.max()))
        worst = max(worst, ratio.max(), cs_ratio.max())
        assert (np.abs(d - d64) <= bound).all() and (cs_ratio <= 1).all()
    assert 0 < worst <= 1


# ---------------------------------------------------------------------------
# 3d. argument checks
# ---------------------------------------------------------------------------
def test_argument_checks():
    c = Synth(32, 32, n_stages=2, splits=(2,))
    bufs_dev = {k: torch.from_numpy(v).cuda() for k, v in c.data('rand', 1).items()}
    dev = bufs_dev['ws'].device
    t = _dev_tables(c.prog, c.maps, dev)
    part = torch.full((c.prog.part_f + 64,), float('nan'), device=dev)
    grad = torch.full((c.n_total,), float('nan'), device=dev)
    st = _lib.stream_ptr()
    n_wgs = t['wg_map'].numel() // 2

    def wgrad(n_wgs=n_wgs, P_pad=c.P_pad, precision=F32, base0=bufs_dev['ws']):
        _lib.call('msdf_wgrad', _lib.ptr(t['items']), _lib.ptr(t['wg_map']), n_wgs, _lib.ptr(part), P_pad, precision,
                  _lib.ptr(base0), _lib.ptr(bufs_dev['feat']), st)

    def reduce(n_rules):
        _lib.call('msdf_reduce', _lib.ptr(t['rules']), n_rules, _lib.ptr(t['maps']), _lib.ptr(part), _lib.ptr(grad), st)

    for bad in (dict(P_pad=48), dict(P_pad=33), dict(P_pad=-32), dict(n_wgs=-1), dict(base0=None), dict(precision=3),
                dict(precision=-1)):
        with pytest.raises(RuntimeError, match='invalid argument'):
            wgrad(**bad)
    with pytest.raises(RuntimeError, match='invalid argument'):
        reduce(-1)
    # nothing to do: success, nothing launched
    wgrad(n_wgs=0)
    wgrad(P_pad=0)
    wgrad(n_wgs=0, base0=None)
    reduce(0)
    torch.cuda.synchronize()
    assert torch.isnan(part).all() and torch.isnan(grad).all()
    # and the same tables do run
    wgrad()
    reduce(len(c.prog.rules))
    torch.cuda.synchronize()
    assert not torch.isnan(part[:c.prog.part_f]).any()
    want = wn.reference_grad(c.prog, c.maps, {k: v.cpu().numpy() for k, v in bufs_dev.items()}, c.P_pad, c.n_total)
    np.testing.assert_array_equal(grad.cpu().numpy(), want)
