"""tests/scatter_cases.py on the CPU: the inputs of tests/test_gpu_hash_scatter.py are what they claim to be -- exact in
every fp32 summation order (the certificate), and shaped so that the scatter takes the branch each GPU test is named
for (structure(), restated from the constants of csrc/hash_scatter.h)."""
import os
import re

import numpy as np
import pytest
import torch

import scatter_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXACT_CASES = [('entry-C%d' % C, lambda C=C: sc.case_every_entry_point(C)) for C in (1, 2, 4, 8)] + \
              [('edge-B%d' % B, lambda B=B: sc.case_batch_edge(B)) for B in sc.BATCH_EDGES] + \
              [('second-pass', sc.case_second_pass)] + \
              [('first-C%d-%s' % (C, w), lambda C=C, w=w: sc.case_first_form(C, w)) for C, w in sc.FIRST_FORM_CASES] + \
              [('lds-atomic-C%d' % C, lambda C=C: sc.case_lds_atomic(C)) for C in sc.LDS_ATOMIC_CHANNELS]


@pytest.fixture(params=EXACT_CASES, ids=[n for n, _ in EXACT_CASES])
def case(request):
    return request.param[1]()


def test_constants_are_those_of_hash_scatter_h():
    text = open(os.path.join(ROOT, 'monosdf_amd', 'csrc', 'hash_scatter.h')).read()
    for name in ('HB_SLICE_FLOATS', 'HB_CHUNK', 'HB_THREADS', 'HB_PTS', 'HB_MAX_SLICES', 'HB_RANK_SHIFT', 'HB2_NS_MAX',
                 'HB2_TILE', 'HG_LDS_WGS', 'HG_LDS_THREADS'):
        m = re.search(r'#define %s (\d+)\b' % name, text)
        assert m and int(m.group(1)) == sc.K[name], name
    m = re.search(r'#define HG_LDS_MAX_BYTES \((\d+) \* (\d+)\)', text)
    assert m and int(m.group(1)) * int(m.group(2)) == sc.K['HG_LDS_MAX_BYTES']


def test_exactness_certificate_holds(case):
    cert = case.certificate()
    assert cert['granular'] and cert['majorant_covers'], cert
    assert cert['max_sum_abs'] < sc.SUM_BOUND / 2, cert            # below 2^21 with a margin of two at least
    # the operands are what the construction says
    top = 2 ** (case.n + 1)
    assert torch.equal(case.x.double() * top, torch.from_numpy(case.m).double())
    for t, hi in ((case.grad, 4), (case.grad2, 4), (case.gg, 2)):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= hi
    assert case.geo['S'] == 0.0 and case.geo['H'] == 2 ** case.n + 1
    # every reference holds something on every level
    for t in case.references():
        for l in range(case.geo['L']):
            assert bool(t[case.level_rows(l)].any()), l


def test_float32_oracle_equals_float64_oracle_bit_for_bit(case):
    for a, b in zip(case.oracle_float32(), (case.first, case.second, case.both)):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == torch.float32 and torch.equal(a.double(), b)


def test_work_items_per_level_and_their_bound(case):
    s = sc.structure(case.geo, case.B, case.C)
    n_wg = -(-case.B // 1024)
    assert s['n_wg'] == n_wg
    for v in s['levels']:
        assert v['items'] == v['ns'] * -(-n_wg // min(v['ns'], n_wg))
        assert v['items'] <= v['ns'] + n_wg
    # hb2_layout's work_max: slices of the whole table + L + L * n_wg
    L, C, n = case.geo['L'], case.C, case.geo['n_entries']
    assert s['work_max'] == (n * C + 8191) // 8192 + L + L * n_wg
    assert s['items'] <= s['work_max']


def test_point_patterns_sit_where_the_kernel_merges_runs():
    """Runs are merged inside 16-lane rows of the place kernel; point b is lane b % 16 of row b // 16, thread b % 256,
    p = (b // 256) % 4 of workgroup b // 1024."""
    B = sc.B_MULTI
    runs = sc.run_table(B)
    lengths = {length for _, length, kind in runs if kind == 'same'}
    assert {1, 2, 3, 15, 16, 17, 64, 130} <= lengths
    assert any(s % 16 == 15 and n > 1 for s, n, _ in runs) and any(s % 16 == 15 and n == 1 for s, n, _ in runs)
    crosses = lambda s, n, k: s // k != (s + n - 1) // k
    for k in (16, 64, 256, 1024):
        assert any(crosses(s, n, k) and (k == 1024 or not crosses(s, n, 4 * k)) for s, n, _ in runs), k
    assert {kind for _, _, kind in runs} == {'same', 'mixed', 'cut'}
    s, n, _ = runs[-1]
    assert s + n == B and B % 16 != 0 and n > B % 16                 # ends at B - 1, longer than the last row's live lanes
    spans = sorted((s, s + n) for s, n, _ in runs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))       # no run overwrites another
    # ... and the points are what the table says
    case = sc.case_every_entry_point(2)
    cell = case.m // 2
    inside = ((case.m >= 0) & (case.m <= 2 ** (case.n + 1))).all(1)
    for s, n, kind in runs:
        assert (cell[s:s + n][inside[s:s + n]] == cell[s]).all(), (s, n, kind)
        if kind == 'same':
            assert (case.m[s:s + n] == case.m[s]).all() and inside[s:s + n].all()
        elif kind == 'mixed':
            assert len(np.unique(case.m[s:s + n], axis=0)) > 1 and inside[s:s + n].all()
        else:
            assert (~inside[s:s + n]).sum() == 1 and inside[s] and inside[s + n - 1]
    assert 20 <= (~inside).sum() <= 21


@pytest.mark.parametrize('C', [1, 2, 4, 8])
def test_every_entry_point_case_reaches_its_branches(C):
    case = sc.case_every_entry_point(C)
    s = sc.structure(case.geo, case.B, C)
    lv = s['levels']
    assert s['second_form'] and s['n_wg'] == 4 and s['last_wg_partial']
    assert (lv[0]['kind'], lv[1]['kind'], lv[2]['kind']) == ('dense', 'mask', 'modulo')
    assert lv[0]['ns'] >= 4 and lv[0]['partial_last_slice'] and not lv[0]['shared_slice'] and not lv[0]['zero_share']
    assert lv[1]['ns'] == 1 and lv[1]['shared_slice'] and lv[1]['groups'] == 4 and lv[1]['zero_share']
    assert lv[2]['ns'] == 3 and lv[2]['G'] == 3 and lv[2]['groups'] == 2 and lv[2]['partial_group'] and lv[2]['shared_slice']
    assert lv[3]['hsize'] * C < 256


@pytest.mark.parametrize('B', sc.BATCH_EDGES)
def test_batch_edge_case_reaches_its_branches(B):
    s = sc.structure(sc.case_batch_edge(B).geo, B, 2)
    assert s['second_form'] and s['n_wg'] == {1: 1, 15: 1, 16: 1, 17: 1, 1023: 1, 1024: 1, 1025: 2, 2049: 3}[B]
    assert [v['kind'] for v in s['levels']] == ['dense', 'mask', 'modulo']


def test_second_pass_case_reaches_its_branch():
    case = sc.case_second_pass()
    s = sc.structure(case.geo, case.B, case.C)
    lv = s['levels'][0]
    assert case.C == 8 and s['second_form'] and s['n_wg'] == 258 and lv['ns'] == 257 and lv['G'] == 257
    assert lv['passes'] == 2 and lv['groups'] == 2 and lv['shared_slice']


@pytest.mark.parametrize('C,which', sc.FIRST_FORM_CASES)
def test_first_form_case_reaches_its_branches(C, which):
    case = sc.case_first_form(C, which)
    lv = sc.structure(case.geo, case.B, C)['levels']
    chunks = sc.first_form_chunks(case.geo, case.x.double(), C)
    assert [c.size for c in chunks] == [v['ns'] for v in lv]
    n_records = 8 * int(sc.hg._in_range(case.x).sum())
    assert all(int(c.sum()) >= -(-n_records // sc.K['HB_CHUNK']) for c in chunks)
    if which == 'large':
        assert lv[0]['hsize'] == 2 ** 19 + 8 and lv[0]['kind'] == 'modulo' and not lv[0]['place_local']
        assert lv[1]['ns'] == 1 and lv[1]['hashed'] and n_records > sc.K['HB_CHUNK'] and int(chunks[1][0]) > 1
        assert (len(lv) == 3) == (C == 8)
        if C == 8:
            assert lv[2]['ns'] > sc.K['HB_MAX_SLICES'] and not lv[2]['count_local']
    else:
        assert lv[0]['kind'] == 'dense' and lv[1]['kind'] == 'modulo'


@pytest.mark.parametrize('C', sc.LDS_ATOMIC_CHANNELS)
def test_lds_atomic_case_reaches_its_branches(C):
    """All three levels go to hg_scatter_lds_kernel: the dense one fills the LDS table, the second is larger than it (the
    kernel's fallback to direct atomics), the third is modulo-hashed inside LDS; the last workgroups have no points."""
    case = sc.case_lds_atomic(C)
    a = sc.atomic_structure(case.geo, case.B, C)
    assert a['n_small'] == 3 == case.geo['L'] and a['fits'] == [True, False, True]
    assert a['kinds'] == ['dense', 'dense', 'modulo']
    assert 17 ** 3 * C <= a['lds_floats'] < 17 ** 3 * C + 64 and a['lds_floats'] * 4 <= sc.K['HG_LDS_MAX_BYTES']
    assert a['per'] == 25 and a['empty_wgs'] == 3
    # C = 8 would not reach the kernel at all
    assert sc.atomic_structure(sc.make_geo(sc.N_EXP_LDS, 8, sc.SIZES_LDS_ATOMIC), case.B, 8)['n_small'] == 0
    # ... and the cases of the other tests never do (H = 65: a dense table of 1.1 MB)
    assert sc.atomic_structure(sc.case_every_entry_point(C).geo, sc.B_MULTI, C)['n_small'] == 0


def test_realistic_cases_have_runs_and_a_measured_tolerance():
    for i in range(len(sc.REAL_CONFIGS)):
        case = sc.real_case(i)
        assert case.B == sc.B_MULTI and case.x.shape == (case.B, 3)
        for term, devs in case.oracle_dev.items():
            assert len(devs) == case.geo['L'] and all(0 < d < 1e-3 for d in devs), (i, term, devs)
