"""The hash grid's table-gradient scatter (csrc/hash_scatter.h) through raw ctypes, branch by branch.

The exact tests feed inputs for which every fp32 sum is exact in any order (tests/scatter_cases.py): the result of every
entry point must be BIT-EQUAL to the float64 oracle, so one lost, doubled or misplaced record fails whatever else lands in
its entry.  Each test first asserts the exactness certificate of its inputs and, on scatter_cases.structure(), that they
reach the branch the test is named for (a retuning of the kernels' constants then fails here instead of silently
uncovering the branch).  The last test runs realistic geometry against the float64 oracle, level by level."""
import os
import subprocess
import sys

import pytest
import torch

import scatter_cases as sc
from helpers import check, hash_table_gradients

pytestmark = pytest.mark.gpu

FIRST_FORM = os.environ.get('MSDF_HASH_BINNED_FORM') == '1'      # what the library read (once per process)
ADDING = ('atomic', 'atomic_second', 'ws', 'ws_second', 'fused')  # the "+=" forms; 'fused_out' and 'node' are "="


def _want(case, form):
    if form in ('atomic', 'ws'):
        return case.first
    return case.second if form.endswith('_second') else case.both


def _forms(case, forms):
    """C = 1 has the first-order forms only (as the reference)."""
    return tuple(f for f in forms if case.second_order or f in ('atomic', 'ws'))


def _run(case, forms, **kw):
    geo = case.geo
    dev = lambda t: t.cuda().contiguous()
    offs = torch.tensor(geo['offsets'], dtype=torch.int32).cuda()
    emb = torch.zeros(geo['n_entries'], geo['C'], device='cuda')
    ops = [dev(t) for t in (case.x, case.grad, case.grad2, case.gg)]
    r = hash_table_gradients(emb, offs, geo['S'], geo['H'], *ops, forms, **kw)
    torch.cuda.synchronize()
    return r


def _assert_exact(case, got, want, what):
    want = want.float().cuda()
    if not torch.equal(got, want):
        pytest.fail('%s: %s' % (what, sc.first_difference(got, want, case.geo)))


def _assert_certificate(case):
    cert = case.certificate()
    assert cert['ok'], cert


def _padded_pitch(case):
    """L C rounded up to 16, with at least one padding column."""
    lc = case.geo['L'] * case.C
    return (lc // 16 + 1) * 16


# ---- a: every entry point, exact, with several place workgroups ----
@pytest.mark.parametrize('C', [1, 2, 4, 8])
def test_every_entry_point_exact_with_several_place_workgroups(C):
    """B = 3,109 (four place workgroups, the last partial), one call holding a dense level of many slices with a partial
    last slice, a power-of-two level of one slice (shared slice: atomic flush, one group per place workgroup), a hashed
    level of three slices (groups of three place workgroups, the last group partial) and a tiny level.  Every form into
    zeros / NaN, the "+=" forms also into a prefilled table, msdf_hash_node_scatter level-major and point-major with NaN
    in the padding columns."""
    case = sc.case_every_entry_point(C)
    _assert_certificate(case)
    s = sc.structure(case.geo, case.B, C)
    lv = s['levels']
    assert s['second_form'] and s['n_wg'] == 4 and s['last_wg_partial'] and case.B % 16 != 0
    assert lv[0]['kind'] == 'dense' and lv[0]['ns'] >= s['n_wg'] and lv[0]['partial_last_slice'] and not lv[0]['shared_slice']
    assert lv[1]['kind'] == 'mask' and lv[1]['ns'] == 1 and lv[1]['shared_slice'] and lv[1]['groups'] == s['n_wg']
    assert lv[2]['kind'] == 'modulo' and 1 < lv[2]['ns'] < s['n_wg'] and lv[2]['partial_group'] and lv[2]['shared_slice']
    assert lv[3]['hsize'] * C < 256 and lv[3]['zero_share']
    assert all(v['zero_share'] for v in lv[1:]) and not lv[0]['zero_share']
    n = case.geo['n_entries']
    forms = _forms(case, ADDING)
    r = _run(case, forms, guard=3)
    for f in forms:
        _assert_exact(case, r[f], _want(case, f), f)
        assert bool((r[f + '_guard'] == 1234.5).all()), f
    # "+=": into a table that holds small integers
    g = torch.Generator().manual_seed(5 + C)
    prefill = torch.randint(-3, 4, (n, C), generator=g).float()
    adding = _forms(case, ADDING)
    r = _run(case, adding, prefill=prefill.cuda(), guard=3)
    for f in adding:
        _assert_exact(case, r[f], prefill.double() + _want(case, f), f + ' into a prefilled table')
        assert bool((r[f + '_guard'] == 1234.5).all()), f
    if not case.second_order:
        return
    # "=": into NaN -- finite everywhere, zero outside the reference's support; the node form in its three layouts
    lc = case.geo['L'] * C
    outs = [('fused_out', _run(case, ('fused_out',), guard=3))]
    for pitch, pad in ((0, 0.0), (lc, 0.0), (_padded_pitch(case), float('nan'))):
        outs.append(('node pitch %d' % pitch, _run(case, ('node',), pitch=pitch, pad=pad, guard=3)))
    support = (case.both != 0).cuda()
    for what, r in outs:
        f = what.split()[0]
        assert bool(torch.isfinite(r[f]).all()), what
        assert not bool(r[f][~support].any()), what
        _assert_exact(case, r[f], case.both, what)
        assert bool((r[f + '_guard'] == 1234.5).all()), what


# ---- b: batch edges ----
@pytest.mark.parametrize('B', sc.BATCH_EDGES)
def test_batch_edges_exact(B):
    """One point, one row of 16 lanes more or less, one place workgroup more or less (C = 2; dense, mask, modulo)."""
    case = sc.case_batch_edge(B)
    _assert_certificate(case)
    s = sc.structure(case.geo, B, 2)
    assert s['second_form'] and s['n_wg'] == (B + 1023) // 1024
    assert [v['kind'] for v in s['levels']] == ['dense', 'mask', 'modulo']
    assert all(v['shared_slice'] == (s['n_wg'] > 1) for v in s['levels'][1:])
    r = _run(case, ('ws', 'fused_out'), guard=1)
    r.update(_run(case, ('node',), pitch=_padded_pitch(case), pad=float('nan'), guard=1))
    for f in ('ws', 'fused_out', 'node'):
        _assert_exact(case, r[f], _want(case, f), '%s at B = %d' % (f, B))
        assert bool((r[f + '_guard'] == 1234.5).all()), f


# ---- c: the second pass of the HB2_TILE loop ----
def test_second_pass_over_the_place_workgroups_of_a_group():
    """More than HB2_TILE place workgroups feed one slice group: B = 263,205 (258 place workgroups), one C = 8 level of
    257 slices -- the first group holds 257 place workgroups, so its accumulate workgroups take a second pass."""
    case = sc.case_second_pass()
    _assert_certificate(case)
    s = sc.structure(case.geo, case.B, case.C)
    lv = s['levels'][0]
    assert s['second_form'] and s['n_wg'] > sc.K['HB2_TILE'] and lv['ns'] > sc.K['HB2_TILE']
    assert lv['G'] > sc.K['HB2_TILE'] and lv['passes'] == 2 and lv['shared_slice'] and lv['partial_group']
    r = _run(case, ('fused_out',), guard=1)
    _assert_exact(case, r['fused_out'], case.both, 'fused_out')
    assert bool((r['fused_out_guard'] == 1234.5).all())


# ---- d: the first form (count / scan / place / accumulate), small and exact ----
@pytest.mark.parametrize('C,which', sc.FIRST_FORM_CASES)
def test_first_form_case(C, which):
    """Exact on the geometries that reach the first form's branches.  MSDF_HASH_BINNED_FORM=1 (read once per process)
    selects that form: test_first_form_small_and_exact runs these cases in a child process with it set.  Run as they
    are they take the second form, on the same inputs."""
    case = sc.case_first_form(C, which)
    _assert_certificate(case)
    s = sc.structure(case.geo, case.B, C)
    lv = s['levels']
    chunks = sc.first_form_chunks(case.geo, case.x.double(), C)
    assert s['n_wg'] == 4
    if which == 'large':
        assert lv[0]['kind'] == 'modulo' and lv[0]['count_local'] and not lv[0]['place_local']
        assert lv[1]['ns'] == 1 and lv[1]['hashed'] and int(chunks[1][0]) > 1          # shared flag, atomic flush
        assert all(int(c.max()) == 1 for c in chunks[:1] + chunks[2:])                 # ... the others own their slice
        if C == 8:
            assert not lv[2]['count_local'] and not lv[2]['place_local']
    else:
        assert lv[0]['kind'] == 'dense' and not lv[0]['hashed'] and lv[1]['hashed'] and lv[0]['partial_last_slice']
    if FIRST_FORM:
        # the first form reads level-major operands only: its refusal shows that the variable took effect
        with pytest.raises(RuntimeError, match='unsupported'):
            _run(case, ('node',), pitch=_padded_pitch(case))
    forms = _forms(case, ('ws', 'ws_second', 'fused', 'fused_out', 'node'))       # 'node' at pitch 0: "=" of the first form
    r = _run(case, forms, guard=1)
    for f in forms:
        _assert_exact(case, r[f], _want(case, f), f)
        assert bool((r[f + '_guard'] == 1234.5).all()), f


def test_first_form_small_and_exact():
    """The cases above in one fresh child process with MSDF_HASH_BINNED_FORM=1."""
    env = dict(os.environ, MSDF_HASH_BINNED_FORM='1')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', os.path.abspath(__file__), '-k',
                        'test_first_form_case'], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '%d passed' % len(sc.FIRST_FORM_CASES) in r.stdout, r.stdout[-500:]


# ---- f: the atomic form's LDS kernel ----
@pytest.mark.parametrize('C', sc.LDS_ATOMIC_CHANNELS)
def test_atomic_lds_kernel_exact(C):
    """H = 17: every level's dense table fits the LDS budget, so the atomic entry points send all three to
    hg_scatter_lds_kernel -- a dense level that fills the LDS table, a level larger than it (direct atomics from inside
    the kernel) and a tiny modulo-hashed one; the last three of the 128 workgroups of a level have no points.  Into zeros
    and into a prefilled table."""
    case = sc.case_lds_atomic(C)
    _assert_certificate(case)
    a = sc.atomic_structure(case.geo, case.B, C)
    assert a['n_small'] == 3 and a['fits'] == [True, False, True] and a['kinds'] == ['dense', 'dense', 'modulo']
    assert a['empty_wgs'] == 3
    forms = _forms(case, ('atomic', 'atomic_second'))
    g = torch.Generator().manual_seed(17 + C)
    prefill = torch.randint(-3, 4, (case.geo['n_entries'], C), generator=g).float()
    for start, what in ((None, ''), (prefill, ' into a prefilled table')):
        r = _run(case, forms, guard=3, **({} if start is None else {'prefill': start.cuda()}))
        for f in forms:
            want = _want(case, f) if start is None else start.double() + _want(case, f)
            _assert_exact(case, r[f], want, f + what)
            assert bool((r[f + '_guard'] == 1234.5).all()), f


# ---- e: realistic geometry against the float64 oracle, per level ----
@pytest.mark.parametrize('index', range(len(sc.REAL_CONFIGS)))
def test_realistic_geometry_against_float64_oracle_per_level(index, errlog):
    """The configurations of test_hash_encoder_kernels at B = 3,109 (four place workgroups), ray-ordered samples with
    runs of every length among the points, random float operands: every binned form and msdf_hash_node_scatter against
    the float64 oracle, max |a - b| / max |b| over each level's rows.  Admitted per level: 4 x what the float32 oracle
    deviates from the float64 oracle on the same inputs (the same products, summed in another order); both numbers go
    to the error log."""
    case = sc.real_case(index)
    geo = case.geo
    L, C = geo['L'], geo['C']
    assert sc.structure(geo, case.B, C)['n_wg'] == 4
    offs = torch.tensor(geo['offsets'], dtype=torch.int32).cuda()
    emb = torch.zeros(geo['n_entries'], C, device='cuda')
    ops = [t.cuda().contiguous() for t in (case.x, case.grad, case.grad2, case.gg)]
    r = hash_table_gradients(emb, offs, geo['S'], geo['H'], *ops, ('ws', 'ws_second', 'fused', 'fused_out'))
    pitch = (L * C // 16 + 1) * 16
    r.update(hash_table_gradients(emb, offs, geo['S'], geo['H'], *ops, ('node',), pitch=pitch, pad=float('nan')))
    torch.cuda.synchronize()
    name = 'cfg%d' % index
    for f, term in (('ws', 'first'), ('ws_second', 'second'), ('fused', 'both'), ('fused_out', 'both'), ('node', 'both')):
        got = r[f].cpu()
        assert bool(torch.isfinite(got).all()), f
        for l in range(L):
            dev = case.oracle_dev[term][l]
            errlog('hash_scatter.oracle_f32', name, 'L%02d.%s' % (l, term), dev, 4 * dev)
            check(errlog, 'hash_scatter', name, 'L%02d.%s' % (l, f), sc.rel_level(got, case.ref[term], geo, l),
                  default=4 * dev)
