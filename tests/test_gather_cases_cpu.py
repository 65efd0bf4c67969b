"""tests/gather_cases.py on the CPU: every exact case holds its certificate and reaches the index forms, corner weights
and edge points it is named for; the certificate rejects hand-made violations; and the cases have teeth -- the
mistakes the GPU tests are there to catch change a reference value."""
import numpy as np
import pytest
import torch

import gather_cases as gc
import scatter_cases as sc
from oracle import hashgrid_oracle as hg

EXACT = [('form', C) for C in gc.CHANNELS] + [('edge', B) for B in gc.BATCH_EDGES] + \
        [('other', i) for i in range(len(gc.OTHER_GEOMETRIES))]


def _case(kind, arg):
    return {'form': gc.case_every_form, 'edge': gc.case_batch_edge, 'other': gc.case_other}[kind](arg)


@pytest.mark.parametrize('kind,arg', EXACT)
def test_certificate_holds(kind, arg):
    case = _case(kind, arg)
    cert = case.certificate()
    assert cert['ok'], cert
    # far from the bound: the input gradient of 16 levels x 2 channels is the largest sum
    assert max(cert['max_granules'].values()) < 2.0 ** 22, cert
    for t in (case.outputs, case.dy_dx, case.grad_inputs, case.grad_grad, case.node_input_gradient(0.5),
              case.node_input_gradient(0.25)):
        assert torch.equal(t.float().double(), t)
    for divide in (1.0, 2.0):
        x = case.world(divide)
        assert torch.equal((x.double() / divide + 1) / 2, case.x01.double())


@pytest.mark.parametrize('kind,arg', EXACT)
def test_structure(kind, arg):
    case = _case(kind, arg)
    s = case.structure()
    if kind == 'form':
        assert s['kinds'] == gc.KINDS_EVERY_FORM
        hsize = [case.geo['offsets'][l + 1] - case.geo['offsets'][l] for l in range(case.L)]
        assert hsize[1] > (2 ** case.n + 1) ** 3 and hsize[3] & (hsize[3] - 1) and hsize[4] * case.C < 256
    elif kind == 'edge':
        assert s['kinds'] == ['dense', 'mask', 'modulo']
    else:
        assert set(s['kinds']) >= {'mask', 'modulo'}
    assert s['weights_distinct'] and s['first_generic'] and s['last_generic']
    assert all(v >= min(32, (case.B + 1) // 2) for v in s['generic'].values()), s
    assert s['skew'] >= (case.B + 3) // 4
    if case.B >= 63:
        assert all(v >= 32 for v in s['generic'].values()) and s['skew'] >= 16, s
    if case.B >= 8:
        assert s['n_oob'] >= 2 and s['below'] >= 1 and s['above'] >= 1 and s['n_on0'] >= 2 and s['n_on1'] >= 2, s
        if 'dense' in s['kinds']:
            assert s['corner_beyond_dense']
    # out-of-range points: exact zeros in every reference
    oob = ~case.in_range
    assert not case.outputs[:, oob].any() and not case.dy_dx[oob].any()
    # the references are not trivially zero on any level, and the Jacobian has all three axes
    for l in range(case.L):
        assert case.outputs[l].any() and case.dy_lm[l].reshape(case.B, 3, case.C).abs().sum((0, 2)).all()


def test_quarter_cells_tell_the_corners_apart():
    """What half cells cannot: with the weights of two axes exchanged inside the trilinear weight (corner k weighted as
    corner k') the outputs change -- on quarter cells, and not on the scatter's half cells."""
    case = gc.case_every_form(2)
    geo, x, emb = case.geo, case.x01.double(), case.emb.double()
    swapped = x[:, [1, 0, 2]]                       # the cell of x with the fractional positions of x and y exchanged
    cell = torch.floor(x * 2 ** case.n)
    mixed = (cell + (swapped * 2 ** case.n - torch.floor(swapped * 2 ** case.n))) / 2 ** case.n
    out = hg.encode_forward(mixed, emb, geo, False)[0]
    assert not torch.equal(out, case.outputs)
    half = (torch.floor(x * 2 ** (case.n + 1)) / 2 ** (case.n + 1))
    inside = ((half * 2 ** case.n) % 1 != 0).all(1)
    cell = torch.floor(half * 2 ** case.n)
    sw = half[:, [1, 0, 2]]
    mixed = (cell + (sw * 2 ** case.n - torch.floor(sw * 2 ** case.n))) / 2 ** case.n
    a = hg.encode_forward(half[inside], emb, geo, False)[0]
    b = hg.encode_forward(mixed[inside], emb, geo, False)[0]
    assert inside.sum() > 32 and torch.equal(a, b)


def test_a_dropped_modulo_or_slack_changes_the_outputs():
    """The index forms matter to the references: the modulo level read as if its size were a power of two, or the
    level with slack read as a hashed level, gives other outputs on that level alone."""
    case = gc.case_every_form(2)
    geo = dict(case.geo)
    x, emb = case.x01.double(), case.emb.double()
    off = list(geo['offsets'])
    # level 3 (3001 entries, modulo) squeezed to 2048 entries: mask
    geo2 = dict(geo, offsets=off[:4] + [off[3] + 2048, off[3] + 2048 + 25])
    assert sc.level_kind(geo2, 3) == 'mask'
    emb2 = torch.cat([emb[:off[3] + 2048], emb[off[4]:]])
    out = hg.encode_forward(x, emb2, geo2, False)[0]
    assert torch.equal(out[:3], case.outputs[:3]) and torch.equal(out[4], case.outputs[4])
    assert not torch.equal(out[3], case.outputs[3])


def test_certificate_rejects_violations():
    base = gc.case_batch_edge(65)
    assert base.certificate()['ok']
    # a table value that is no integer: the outputs leave their granule
    bad = gc.GatherCase(865, gc.N_EXP, 2, gc.SIZES_BATCH_EDGES, 65)
    bad.emb[::2, 0] += 2.0 ** -12               # every other entry: the weights of a point's changed corners do not sum to 1
    bad.outputs, bad.dy_dx = hg.encode_forward(bad.x01.double(), bad.emb.double(), bad.geo, True)
    cert = bad.certificate()
    assert not cert['granular'] and not cert['ok']
    # gradients so large that the input gradient's sum leaves 24 bits
    big = gc.GatherCase(865, gc.N_EXP, 2, gc.SIZES_BATCH_EDGES, 65)
    big.grad *= 2.0 ** 12
    big.grad[0, 0, 0] += 1
    big.grad_inputs = hg.encode_backward_input(big.grad.double(), big.dy_dx, big.geo)
    cert = big.certificate()
    assert not cert['bounded'] and not cert['ok']


def test_first_difference_names_level_and_point():
    want = torch.zeros(3, 10, 2)
    assert gc.first_difference(want.clone(), want, 3) is None
    got = want.clone()
    got[1, 7, 1] = 2.0
    msg = gc.first_difference(got, want, 3)
    assert msg.startswith('level 1 (10 entries), entry 7 ') and 'channel 1' in msg
    assert 'entry 4 ' in gc.first_difference(torch.arange(6.0).reshape(6, 1), torch.tensor([0, 1, 2, 3, 9, 5.0]).reshape(6, 1))


@pytest.mark.parametrize('L,C', gc.TRANSPOSE_LC)
def test_transpose_shapes(L, C):
    assert gc.transpose_lds_bytes(L, C) <= gc.HT_LDS_MAX
    p = gc.transpose_pitches(L, C)
    assert p[0] == L * C and all(q % 16 == 0 for q in p[1:]) and p[-1] - L * C >= 16 and len(set(p)) == len(p)


def test_transpose_limits():
    assert gc.transpose_lds_bytes(32, 8) == 64 * 257 * 4 > gc.HT_LDS_MAX
    assert gc.transpose_lds_bytes(31, 8) <= gc.HT_LDS_MAX            # the largest multiple of 8 under the limit
    lcs = [L * C for L, C in gc.TRANSPOSE_LC]
    assert any(v % 2 for v in lcs) and 32 in lcs and 248 in lcs and min(lcs) < 8


@pytest.mark.parametrize('index', range(len(sc.REAL_CONFIGS)))
def test_real_case_bars(index):
    """The per-level deviation of the float32 oracle is finite and small on every level (it grows with the level's
    scale: the float32 product x * scale is rounded before the cell is taken off it); the bar is 4 x it, at least
    4 x 2^-23."""
    case = gc.real_case(index)
    L = case.geo['L']
    for key in ('outputs', 'dy_dx'):
        for l in range(L):
            dev = case.oracle_dev[key][l]
            assert np.isfinite(dev) and dev < 2.0 ** -22 * hg.level_scale(case.geo, l)[0] + 2.0 ** -20, (key, l, dev)
            assert case.bar(key, l) == 4 * max(dev, 2.0 ** -23)
