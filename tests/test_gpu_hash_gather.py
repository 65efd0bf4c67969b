"""The hash grid's read side (csrc/hashgrid.hip outside hash_scatter.h) through raw ctypes: forward and node forward in
every index form and layout, the four small kernels, the transposes and the return codes.

The exact tests feed inputs on which every fp32 product and sum of these kernels is exact (tests/gather_cases.py: points
on quarter cells, integer tables and gradients): every result must be BIT-EQUAL to the float64 oracle, so a corner with
the weight of another, a wrong index form, a misplaced row or a Jacobian that is off in the last digit of a coarse level
all fail.  Each test asserts the exactness certificate of its inputs before it looks at a GPU result.  Every output
buffer is pre-filled with NaN and followed by guard floats that must come back untouched.  The last test runs realistic
geometry against the float64 oracle, level by level."""
import pytest
import torch

import gather_cases as gc
import scatter_cases as sc

pytestmark = pytest.mark.gpu

GUARD, GUARD_VALUE = 96, 1234.5
OK, ARG, UNSUPPORTED = 0, 1, 3


def _lib():
    from monosdf_amd import _lib
    return _lib


class Buf:
    """n floats filled with `fill` (NaN), then GUARD floats of GUARD_VALUE."""

    def __init__(self, n, fill=float('nan')):
        self.n = n
        self.all = torch.full((n + GUARD,), float(fill), device='cuda')
        self.all[n:] = GUARD_VALUE
        self.t = self.all[:n]

    def view(self, *shape):
        return self.t.view(*shape)

    def guard_ok(self):
        return bool((self.all[self.n:] == GUARD_VALUE).all())


def _P(t):
    if isinstance(t, Buf):
        t = t.all
    return _lib().ptr(t)


def _call(name, *args):
    _lib().call(name, *args, _lib().stream_ptr())


def _exact(got, want, what, levels=1):
    want = want.float().cuda() if want.dtype != torch.float32 or not want.is_cuda else want
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        pytest.fail('%s: %s' % (what, gc.first_difference(got, want, levels)))


def _guards(what, *bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b.guard_ok(), '%s: the floats after output %d were written' % (what, i)


def _assert_certificate(case):
    cert = case.certificate()
    assert cert['ok'], cert


_DEV = {}


def _dev(case):
    """The case's operands on the device, once per case."""
    d = _DEV.get(id(case))
    if d is None or d['case'] is not case:
        d = _DEV[id(case)] = dict(
            case=case, x01=case.x01.cuda(), emb=case.emb.cuda(), grad=case.grad.cuda(), gg=case.gg.cuda(),
            offs=torch.tensor(case.geo['offsets'], dtype=torch.int32).cuda(),
            dy=case.dy_dx.float().cuda(), dy_lm=case.dy_lm.float().cuda(), oob=(~case.in_range).cuda())
    return d


def _dims(case):
    return case.B, case.C, case.L, case.geo['S'], case.geo['H']


# ---- the kernels, each against the oracle ----
def check_forward(case):
    """msdf_hash_encode_forward with calc_grad_inputs 0 (dy_dx stays NaN), 1 and 2."""
    d = _dev(case)
    B, C, L, S, H = _dims(case)
    for calc in (0, 1, 2):
        what = 'forward, calc_grad_inputs = %d' % calc
        out, dy = Buf(L * B * C), Buf(B * L * 3 * C)
        _call('msdf_hash_encode_forward', _P(d['x01']), _P(d['emb']), _P(d['offs']), _P(out), B, 3, C, L, S, H, calc, _P(dy))
        _guards(what, out, dy)
        _exact(out.view(L, B, C), case.outputs, what + ': outputs', L)
        assert not bool(out.view(L, B, C)[:, d['oob']].any()), what
        if calc == 0:
            assert bool(dy.t.isnan().all()), what + ': dy_dx was written'
        elif calc == 1:
            _exact(dy.view(B, L * 3 * C), d['dy'], what + ': dy_dx [B, L 3 C]')
            assert not bool(dy.view(B, L * 3 * C)[d['oob']].any()), what
        else:
            _exact(dy.view(L, B, 3 * C), d['dy_lm'], what + ': dy_dx [L, B, 3 C]', L)
            assert not bool(dy.view(L, B, 3 * C)[:, d['oob']].any()), what


def _features(case, feat, pitch, want, what):
    B, C, L = case.B, case.C, case.L
    if pitch == 0:
        _exact(feat.view(L, B, C), want, what, L)
    else:
        rows = feat.view(B, pitch)
        _exact(rows, case.rows(want, pitch, 0.0), what)
        assert not bool(rows[:, L * C:].any()), what + ': padding columns'


def check_node_forward(case):
    """msdf_hash_node_forward on world coordinates: divide_factor 1 and 2, pitch 0, L C and padded; x01_out NULL;
    dy_dx NULL."""
    d = _dev(case)
    B, C, L, S, H = _dims(case)
    pitches = (0, L * C, case.padded_pitch())
    runs = [(df, p, True, True) for df in (1.0, 2.0) for p in pitches]
    runs += [(1.0, pitches[2], False, True), (2.0, 0, True, False), (1.0, pitches[1], False, False)]
    for df, pitch, want_x01, want_dy in runs:
        what = 'node forward, divide_factor %g, pitch %d%s%s' % (df, pitch, '' if want_x01 else ', x01_out NULL',
                                                                 '' if want_dy else ', dy_dx NULL')
        xw = case.world(df).cuda()
        x01, feat, dy = Buf(3 * B), Buf(B * max(pitch, L * C)), Buf(L * B * 3 * C)
        _call('msdf_hash_node_forward', _P(xw), df, _P(x01) if want_x01 else None, _P(d['emb']), _P(d['offs']), _P(feat),
              pitch, B, C, L, S, H, _P(dy) if want_dy else None)
        _guards(what, x01, feat, dy)
        _features(case, feat, pitch, case.outputs, what + ': features')
        if want_x01:
            _exact(x01.view(B, 3), d['x01'], what + ': x01')
        else:
            assert bool(x01.t.isnan().all()), what
        if want_dy:
            _exact(dy.view(L, B, 3 * C), d['dy_lm'], what + ': dy_dx', L)
        else:
            assert bool(dy.t.isnan().all()), what


def check_small_kernels(case):
    """The input backward and the second-order gradient in their reference-order and node forms, fed the oracle's exact
    dy_dx."""
    d = _dev(case)
    B, C, L, S, H = _dims(case)
    lc, padded = L * C, case.padded_pitch()
    for calc, dy in ((1, d['dy']), (2, d['dy_lm'])):
        what = 'input backward, calc_grad_inputs = %d' % calc
        gi = Buf(3 * B)
        _call('msdf_hash_encode_backward', _P(d['grad']), _P(d['x01']), None, _P(d['offs']), None, B, 3, C, L, S, H, calc,
              _P(dy), _P(gi))
        _guards(what, gi)
        _exact(gi.view(B, 3), case.grad_inputs, what)
        if C == 1:
            continue                        # no C = 1 second backward (as the reference): test_return_codes
        what = 'second backward, calc_grad_inputs = %d' % calc
        gg = Buf(L * B * C)
        _call('msdf_hash_encode_second_backward', _P(d['grad']), _P(d['x01']), None, _P(d['offs']), B, 3, C, L, S, H, calc,
              _P(dy), _P(d['gg']), _P(gg), None)
        _guards(what, gg)
        _exact(gg.view(L, B, C), case.grad_grad, what, L)
    for pitch in (0, padded):
        g = d['grad'] if pitch == 0 else case.rows(case.grad, pitch, float('nan')).cuda()
        for scale in (0.5, 0.25):
            what = 'node input gradient, pitch %d, scale %g' % (pitch, scale)
            inout = Buf(3 * B)
            inout.t.copy_(case.inout.flatten())
            _call('msdf_hash_node_input_gradient', _P(g), pitch, _P(d['dy_lm']), B, C, L, scale, _P(inout))
            _guards(what, inout)
            _exact(inout.view(B, 3), case.node_input_gradient(scale), what)
        splits = sorted({0, min(1, B), B - 1, B})
        runs = [(n, True, True) for n in splits] + [(n, a, b) for n in sorted({min(1, B), B - 1})
                                                    for a, b in ((False, True), (True, False))]
        for n_split, have_a, have_b in runs:
            what = 'node second grad, pitch %d, n_split %d%s%s' % (pitch, n_split, '' if have_a else ', g_a NULL',
                                                                   '' if have_b else ', g_b NULL')
            g_a = d['gg'][:n_split].contiguous() if have_a and n_split > 0 else None
            g_b = d['gg'][n_split:].contiguous() if have_b and n_split < B else None
            gg_out, out = Buf(3 * B), Buf(B * max(pitch, lc))
            _call('msdf_hash_node_second_grad', _P(g_a), _P(g_b), n_split, 0.5, _P(gg_out), _P(d['dy_lm']), _P(out), pitch,
                  B, C, L)
            _guards(what, gg_out, out)
            want_gg, want = case.node_second_grad(0.5, n_split, have_a, have_b)
            _exact(gg_out.view(B, 3), want_gg, what + ': gg_out')
            _features(case, out, pitch, want, what + ': grad_grad')


# ---- A1, A3: every index form, C in {1, 2, 4, 8} ----
@pytest.mark.parametrize('C', gc.CHANNELS)
def test_forward_every_index_form(C):
    """One call holding a dense level, a dense level with slack after the last stride, a power-of-two hashed level, a
    hashed level of another size (the modulo) and a tiny level, B = 1,025: msdf_hash_encode_forward in its three modes
    and msdf_hash_node_forward in its layouts, bit-equal to the oracle; exact zeros for out-of-range points; points on
    0 and on 1 (upper corners outside the dense grid: the modulo keeps them inside the level)."""
    case = gc.case_every_form(C)
    _assert_certificate(case)
    s = case.structure()
    assert s['kinds'] == gc.KINDS_EVERY_FORM and all(v >= 32 for v in s['generic'].values()) and s['skew'] >= 32
    assert s['weights_distinct'] and s['n_oob'] >= 2 and s['n_on0'] >= 2 and s['n_on1'] >= 2 and s['corner_beyond_dense']
    assert case.B == 1025
    check_forward(case)
    check_node_forward(case)


@pytest.mark.parametrize('C', gc.CHANNELS)
def test_small_kernels_exact(C):
    """hg_backward_input_kernel, hg_second_backward_grad_kernel (both dy_dx layouts), hg_node_input_gradient_kernel
    (both pitches, NaN in the padding of g, inout pre-filled) and hg_node_second_grad_kernel (n_split 0, 1, B - 1, B; a
    NULL part) on the oracle's exact dy_dx: bit-equal to encode_backward_input / second_backward_grad in float64."""
    case = gc.case_every_form(C)
    _assert_certificate(case)
    check_small_kernels(case)


# ---- A2: batch edges ----
@pytest.mark.parametrize('B', gc.BATCH_EDGES)
def test_batch_edges(B):
    """One point; a wave and a block of the forward kernels more or less (one lane per point and level, 256-lane blocks);
    B = 257: the last block of hg_node_input_gradient_kernel (one lane per point and axis) holds exactly one point;
    B = 513."""
    case = gc.case_batch_edge(B)
    _assert_certificate(case)
    s = case.structure()
    assert s['kinds'] == ['dense', 'mask', 'modulo'] and s['first_generic'] and s['last_generic']
    assert case.C == 2 and case.B == B
    if B == 257:
        assert 3 * B - (3 * B // 256) * 256 == 3
    check_forward(case)
    check_node_forward(case)
    check_small_kernels(case)


# ---- A4: the transposes ----
@pytest.mark.parametrize('L,C', gc.TRANSPOSE_LC)
def test_transposes(L, C):
    """msdf_hash_transpose is a pure copy: L C odd, small, 32 and 248 (the largest multiple of 8 whose tile fits the
    LDS limit); B around the 64-point tile; pitch L C, padded and padded + 16; both directions; one and two tensors."""
    lc = L * C
    assert gc.transpose_lds_bytes(L, C) <= gc.HT_LDS_MAX
    g = torch.Generator().manual_seed(1000 * L + C)
    for B in gc.TRANSPOSE_B:
        for pitch in gc.transpose_pitches(L, C):
            for two in (False, True):
                what = 'L %d C %d B %d pitch %d, %d tensor(s)' % (L, C, B, pitch, 2 if two else 1)
                lm = [torch.rand(L, B, C, generator=g).cuda() for _ in range(2)]
                dst = [Buf(B * pitch) for _ in range(2)]
                _call('msdf_hash_transpose', _P(lm[0]), _P(dst[0]), _P(lm[1]) if two else None,
                      _P(dst[1]) if two else None, L, B, C, pitch, 1)
                _guards(what, *dst)
                for i in range(2 if two else 1):
                    want = torch.nn.functional.pad(lm[i].permute(1, 0, 2).reshape(B, lc), (0, pitch - lc))
                    _exact(dst[i].view(B, pitch), want, what + ' to rows, tensor %d' % i)
                if not two:
                    assert bool(dst[1].t.isnan().all()), what
                rows = [torch.rand(B, pitch, generator=g).cuda() for _ in range(2)]
                for r in rows:
                    r[:, lc:] = float('nan')
                dst = [Buf(L * B * C) for _ in range(2)]
                _call('msdf_hash_transpose', _P(rows[0]), _P(dst[0]), _P(rows[1]) if two else None,
                      _P(dst[1]) if two else None, L, B, C, pitch, 0)
                _guards(what, *dst)
                for i in range(2 if two else 1):
                    want = rows[i][:, :lc].reshape(B, L, C).permute(1, 0, 2).contiguous()
                    _exact(dst[i].view(L, B, C), want, what + ' to level-major, tensor %d' % i, L)
                if not two:
                    assert bool(dst[1].t.isnan().all()), what


def test_transpose_refuses_a_tile_over_the_lds_limit():
    L, C, B = 32, 8, 65
    assert gc.transpose_lds_bytes(L, C) == 64 * 257 * 4 > gc.HT_LDS_MAX
    lib, st = _lib().load(), _lib().stream_ptr()
    src = torch.rand(L, B, C).cuda()
    for to_pm in (1, 0):
        dst = Buf(L * B * C)
        assert lib.msdf_hash_transpose(_P(src), _P(dst), None, None, L, B, C, L * C, to_pm, st) == UNSUPPORTED
        torch.cuda.synchronize()
        assert bool(dst.t.isnan().all()) and dst.guard_ok()


# ---- A5: return codes ----
def test_return_codes():
    """The second return-code table of include/monosdf_hip.h (hash-grid block), row by row: every refusal gives its
    code, in the documented order where two overlap, and launches nothing (the outputs stay NaN).  Host-side returns
    only; every buffer is nevertheless a valid operand of its call."""
    case = gc.case_batch_edge(65)
    d = _dev(case)
    B, C, L, S, H = _dims(case)
    lc = L * C
    lib, st = _lib().load(), _lib().stream_ptr()
    out = dict(outputs=Buf(L * B * C), dy=Buf(B * L * 3 * C), x01=Buf(3 * B), feat=Buf(B * 16), gi=Buf(3 * B),
               ggrad=Buf(L * B * C), gg_out=Buf(3 * B), dst=Buf(B * 16), dst2=Buf(B * 16))
    xw = case.world(1.0).cuda()
    base = dict(out, x=d['x01'], xw=xw, emb=d['emb'], offs=d['offs'], grad=d['grad'], gg=d['gg'], dy_in=d['dy_lm'],
                g_a=d['gg'][:7].contiguous(), g_b=d['gg'][7:].contiguous(), inout=Buf(3 * B),
                src=d['grad'], src2=d['grad'], B=B, D=3, C=C, L=L, pitch=0, n_split=7, calc=2)

    def status(name, **kw):
        a = dict(base, **kw)
        p = lambda k: _P(a[k])                                  # None -> NULL
        if name == 'forward':
            return lib.msdf_hash_encode_forward(p('x'), p('emb'), p('offs'), p('outputs'), a['B'], a['D'], a['C'], a['L'],
                                                S, H, a['calc'], p('dy'), st)
        if name == 'backward':
            return lib.msdf_hash_encode_backward(p('grad'), p('x'), None, p('offs'), None, a['B'], a['D'], a['C'], a['L'],
                                                 S, H, a['calc'], p('dy_in'), p('gi'), st)
        if name == 'second':
            return lib.msdf_hash_encode_second_backward(p('grad'), p('x'), None, p('offs'), a['B'], a['D'], a['C'],
                                                        a['L'], S, H, a['calc'], p('dy_in'), p('gg'), p('ggrad'), None, st)
        if name == 'node_forward':
            return lib.msdf_hash_node_forward(p('xw'), 1.0, p('x01'), p('emb'), p('offs'), p('feat'), a['pitch'], a['B'],
                                              a['C'], a['L'], S, H, p('dy'), st)
        if name == 'node_input':
            return lib.msdf_hash_node_input_gradient(p('grad'), a['pitch'], p('dy_in'), a['B'], a['C'], a['L'], 0.5,
                                                     p('inout'), st)
        if name == 'node_second':
            return lib.msdf_hash_node_second_grad(p('g_a'), p('g_b'), a['n_split'], 0.5, p('gg_out'), p('dy_in'),
                                                  p('ggrad'), a['pitch'], a['B'], a['C'], a['L'], st)
        assert name == 'transpose', name
        return lib.msdf_hash_transpose(p('src'), p('dst'), p('src2'), p('dst2'), a['L'], a['B'], a['C'],
                                       a['pitch'] or lc, 1, st)

    def refused(names, code, **kw):
        for name in names:
            assert status(name, **kw) == code, (name, sorted(kw), code)

    REF = ('forward', 'backward', 'second')
    NODE = ('node_forward', 'node_input', 'node_second')
    CHANNELS = REF + NODE
    ALL = CHANNELS + ('transpose',)
    none = dict(x=None, xw=None, emb=None, offs=None, grad=None, gg=None, dy_in=None, g_a=None, g_b=None, inout=None,
                src=None, src2=None, **{k: None for k in out})
    # 1: D, and for the two backward entries C, before B == 0 and before any pointer is looked at
    refused(REF, UNSUPPORTED, D=2, B=0, **none)
    refused(REF, UNSUPPORTED, D=2)
    refused(('backward', 'second'), UNSUPPORTED, C=3, B=0, **none)
    refused(('second',), UNSUPPORTED, C=1, B=0)
    # 2: no points -- every pointer NULL; B == 0 wins over what rows 3 to 5 would refuse
    refused(ALL, OK, B=0, **none)
    refused(('forward',) + NODE, OK, B=0, C=3)
    refused(NODE + ('transpose',), OK, B=0, pitch=lc - 1)
    refused(('node_second',), OK, B=0, n_split=1)
    refused(('transpose',), OK, B=0, L=0)
    refused(('transpose',), OK, B=0, L=32, C=8)
    # 3: a NULL required operand
    for name, keys in (('forward', ('x', 'emb', 'offs', 'outputs', 'dy')), ('backward', ('grad', 'dy_in', 'gi')),
                       ('second', ('gg', 'dy_in')), ('node_forward', ('xw', 'emb', 'offs', 'feat')),
                       ('node_input', ('grad', 'dy_in', 'inout')), ('node_second', ('gg_out', 'dy_in', 'ggrad')),
                       ('transpose', ('src', 'dst'))):
        for k in keys:
            refused((name,), ARG, **{k: None})
    # ... the pitch, the split, the transpose's shapes and its pair of second tensors
    refused(NODE, ARG, pitch=lc - 1)
    refused(NODE, ARG, pitch=1)
    refused(('transpose',), ARG, pitch=lc - 1)
    refused(('node_second',), ARG, n_split=B + 1)
    refused(('transpose',), ARG, L=0)
    refused(('transpose',), ARG, C=0)
    refused(('transpose',), ARG, src2=None)
    refused(('transpose',), ARG, dst2=None)
    # ... and they win over rows 4 and 5
    refused(('forward',) + NODE, ARG, C=3, **{'x': None, 'xw': None, 'grad': None, 'gg_out': None})
    refused(NODE, ARG, C=3, pitch=lc - 1)
    refused(('node_second',), ARG, C=3, n_split=B + 1)
    refused(('transpose',), ARG, L=32, C=8, pitch=16)
    refused(('node_input',), ARG, B=2 ** 31, inout=None)
    # 4: 3 B does not fit 32 bits (before C); the transpose's LDS tile
    refused(('node_input',), UNSUPPORTED, B=2 ** 31)
    refused(('node_input',), UNSUPPORTED, B=2 ** 31, C=3)
    refused(('transpose',), UNSUPPORTED, L=32, C=8, pitch=256)
    # 5: the channels
    for bad in (0, 3, 5, 16):
        refused(('forward',) + NODE, UNSUPPORTED, C=bad)
    refused(('backward',), UNSUPPORTED, C=3)
    torch.cuda.synchronize()
    for k, b in list(out.items()) + [('inout', base['inout'])]:
        assert bool(b.t.isnan().all()), k + ' was written by a refused call'
    # not refused: what the table leaves optional (these run; the exact tests check their results)
    refused(('forward',), OK, calc=0, dy=None)
    refused(('node_forward',), OK, x01=None, dy=None)
    refused(('node_second',), OK, g_a=None)
    refused(('node_second',), OK, g_b=None)
    torch.cuda.synchronize()
    for k in ('x01', 'dy', 'gi', 'dst', 'dst2'):
        assert bool(out[k].t.isnan().all()), k
    for k, b in list(out.items()) + [('inout', base['inout'])]:
        assert b.guard_ok(), k


# ---- A6: realistic geometry against the float64 oracle, per level ----
@pytest.mark.parametrize('index', range(len(sc.REAL_CONFIGS)))
def test_realistic_geometry_against_float64_oracle_per_level(index, errlog):
    """The four configurations of scatter_cases.REAL_CONFIGS with the points of RealCase (ray-ordered runs, cell borders,
    out-of-range points) and a random float table: outputs and dy_dx of msdf_hash_encode_forward and
    msdf_hash_node_forward against the float64 oracle, max |a - b| / max |b| over each level.  Admitted per level and
    tensor: 4 x what the float32 oracle loses against the float64 oracle there (the same arithmetic; the factor allows
    for another order of the 8-term and 4-term sums), at least 4 x 2^-23; both numbers go to the error log.
    Measured on an MI355X: on all 58 (level, tensor) pairs the kernels' error EQUALS the float32 oracle's deviation
    (same products, same order), a quarter of the bar -- 1.2e-6 on the coarsest level (scale 15) to 2.0e-4 on the
    finest (scale 2047) of the 16-level configuration.  The deviation grows with the scale because x * scale is rounded
    to float32 before the cell is taken off it, in the kernels as in the float32 oracle."""
    case = gc.real_case(index)
    geo = case.geo
    B, C, L, S, H = case.B, geo['C'], geo['L'], geo['S'], geo['H']
    x, emb = case.x.cuda().contiguous(), case.emb.cuda()
    offs = torch.tensor(geo['offsets'], dtype=torch.int32).cuda()
    out, dy = Buf(L * B * C), Buf(L * B * 3 * C)
    _call('msdf_hash_encode_forward', _P(x), _P(emb), _P(offs), _P(out), B, 3, C, L, S, H, 2, _P(dy))
    xw = (x * 2 - 1).contiguous()
    n_out, n_dy, x01 = Buf(L * B * C), Buf(L * B * 3 * C), Buf(3 * B)
    _call('msdf_hash_node_forward', _P(xw), 1.0, _P(x01), _P(emb), _P(offs), _P(n_out), 0, B, C, L, S, H, _P(n_dy))
    _guards('cfg%d' % index, out, dy, n_out, n_dy, x01)
    got = dict(outputs=out.view(L, B, C).cpu(), dy_dx=dy.view(L, B, 3 * C).cpu())
    # the node form on the points where x -> 2 x - 1 -> x01 is the identity in float32: the same bits
    same = (x01.view(B, 3) == x).all(1)
    assert int(same.sum()) > B // 2
    assert torch.equal(n_out.view(L, B, C)[:, same], out.view(L, B, C)[:, same])
    assert torch.equal(n_dy.view(L, B, 3 * C)[:, same], dy.view(L, B, 3 * C)[:, same])
    name = 'cfg%d' % index
    failures = []
    for key in ('outputs', 'dy_dx'):
        assert bool(torch.isfinite(got[key]).all()), key
        for l in range(L):
            dev, bar = case.oracle_dev[key][l], case.bar(key, l)
            errlog('hash_gather.oracle_f32', name, 'L%02d.%s' % (l, key), dev, bar)
            err = errlog('hash_gather', name, 'L%02d.%s' % (l, key), gc.rel_level(got[key], case.ref[key], l), bar)
            print('hash_gather %s L%02d.%s err %.3e oracle_f32 %.3e bar %.3e' % (name, l, key, err, dev, bar))
            if not err <= bar:
                failures.append((key, l, err, bar))
    assert not failures, failures
