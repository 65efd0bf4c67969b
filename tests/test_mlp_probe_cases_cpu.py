"""tests/mlp_probe_cases.py does what it claims, shown on the CPU: the routing of every probe is exact (or carries the one
rounding its bound names), the fp32 restatement of every kernel formula stays within its derived bound (within half of it on nine
elements in ten: _within() says why not on all), the cases
reach every switch, slot and column they are there for, and every mutant of a restatement leaves a bound somewhere."""
import numpy as np
import pytest

import mlp_probe_cases as mp

f32, f64 = np.float32, np.float64


def _within(got, ref, bound):
    """The restatement within its bound on every element, and within half of it on nine elements in ten.  Not within half
    on all: a bound that counts half an ulp per operation is attained, nearly, by a correct result wherever ONE rounding
    is all there is -- h just above a power of two (the fma's own rounding), the log branch near e = 1e-4 (the rounding of
    1 + e), a0 = slot + 1.25 -- so 'half of the bound everywhere' would need every such term doubled, and the GPU held to
    a wider bar.  The float64 reference itself consumes nothing (its error is 2^-29 of these bounds)."""
    got = np.asarray(got, dtype=f64)
    err = np.abs(got - ref)
    bound = np.broadcast_to(bound, err.shape)
    ok = (err <= bound).all() and (err <= 0.5 * bound).mean() >= 0.9
    return bool(ok), float((err / np.maximum(bound, 1e-300)).max())


def _escapes(got, ref, bound):
    with np.errstate(invalid='ignore'):
        return bool((~(np.abs(np.asarray(got, dtype=f64) - ref) <= bound)).any())


def test_routing_is_certified():
    """Every routed pre-activation is exact in fp32 and is the float64 value (the encodings': off by the one rounding of
    slot + bias at most): what the GPU tests assert before they look at a GPU result."""
    assert mp.certificate('softplus') == []
    for m in mp.PE_MULTIRES:
        assert mp.certificate('pe', m) == [], m
    for mode, m in mp.VIEW_CASES.values():
        assert mp.certificate('view', mode, m) == [], (mode, m)
    assert mp.certificate('sigmoid') == []
    # and the certificate can fail: a point off the grid, a bias that lets a slot's unit out of the pass-through range
    x = mp.SP_X.copy()
    try:
        mp.SP_X[0, 0] += 2.0 ** -30
        assert mp.sp_certificate()
    finally:
        mp.SP_X[:] = x
    assert mp.sp_certificate() == []


def _sp():
    a0, a1 = mp.sp_preactivations(mp.SP_X)
    return a0, a1, a1.astype(f32)


def test_restatements_stay_within_their_bounds():
    a0, a1, a32 = _sp()
    assert np.array_equal(a32.astype(f64), a1)
    for lean in (False, True):
        h = mp.softplus_lean_restated(a32) if lean else mp.softplus_restated(a32)[0]
        ok, worst = _within(h, mp.softplus64(a1), mp.bound_h(a1, lean))
        assert ok, ('h', lean, worst)
        u, s = mp.sigmoid_restated(h)
        ok, worst = _within(s, mp.sigmoid64(100 * a1), mp.bound_s(a1, lean))
        assert ok, ('s', lean, worst)
        t = mp.second_order_restated(h, mp.UNIT_SCALE.astype(f32))
        ref = 100 * mp.sigmoid64(100 * a1) * mp.sigmoid64(-100 * a1) * mp.UNIT_SCALE
        ok, worst = _within(t, ref, mp.bound_t(a1, mp.UNIT_SCALE, lean))
        assert ok, ('t', lean, worst)
        assert np.isfinite(t.astype(f64)).all()
    # the bounds are not vacuous: relative for h where a <= 0 takes the series, a few 2^-24 absolute for s
    T, e, de = mp._err_e(a1)
    series = (a1 <= 0) & (e * (1 + de) < 1e-4) & (mp.softplus64(a1) > 1e-30)
    assert series.any() and (mp.bound_h(a1)[series] / mp.softplus64(a1)[series]).max() < 420 * mp.U      # (2 x 200 + 8.2) U
    dense = np.linspace(-2, 2, 400001)
    for lean in (False, True):
        top = mp.bound_s(dense, lean).max() / mp.U
        assert top <= mp.S_MULTIPLE[lean] and top > mp.S_MULTIPLE[lean] - 0.05, (lean, top)
    feat, o, g = mp.sigmoid_inputs()
    y, gy = mp.color_sigmoid_restated(o, g)
    dy, dg = mp.bound_color_sigmoid(o, g)
    assert np.isfinite(y).all() and y[o == -89].max() == 0 and y[o == -110].max() == 0 and y[o == 89].min() == 1
    assert _within(y, mp.sigmoid64(o), dy)[0]
    assert _within(gy, g * mp.sigmoid64(o) * mp.sigmoid64(-o), dg)[0]
    for m in mp.PE_MULTIRES:
        for j in range(mp.pe_slots(m)):
            s, c = mp.pe_reference(m, j)
            assert c == s.c
            assert _within(s.a0_32, s.a0, mp.pe_da0(s, 'fp32'))[0], (m, j)
            assert _within(s.dval32, s.dval, mp.bound_pe(s.dval) if j >= 3 else 0.0)[0], (m, j)


def test_softplus_cases_reach_every_switch_from_both_sides():
    """Adjacent grid values on either side of e = 1e-4, of 1 + e == 1 and (a < 0) of s == 0, both signs, and of 100 a = 20:
    the restated decision differs between the two, and both are among the probed values."""
    vals = set(mp.SP_VALUES.tolist())

    def decisions(a):
        a = np.asarray(a, dtype=f32)
        h, series = mp.softplus_restated(a)
        _, e = mp._exp_part(a, None)
        _, s = mp.sigmoid_restated(h)
        return {'series': series, 'one_plus_e': (f32(1) + e) == 1, 'sg': s > 0, 'threshold': a * f32(100) > f32(20)}

    for name, T in mp.SWITCHES.items():
        for sgn in (1, -1):
            if (name == 'threshold' and sgn < 0) or (name == 'sg' and sgn > 0):
                continue
            lo, hi = mp._around(sgn * T)
            assert lo in vals and hi in vals and hi - lo <= 2 * mp.GRID
            k = [k for k in range(7, -1, -1) if abs(T / 100 * 2.0 ** k) <= 2 - mp.GRID][0]
            d = decisions(np.array([lo, hi]) * 2.0 ** -k)[name]
            assert d[0] != d[1], (name, sgn, lo, hi, k)
    a0, a1, a32 = _sp()
    T = np.abs(100 * a1)
    assert (a1 == 0).any() and (T == 200).any() and 0 < T[T > 0].min() <= 100 * 2.0 ** -19
    for t in mp.SUBNORMAL_T:
        assert ((T > t - 0.01) & (T < t + 0.01)).any(), t
    _, e = mp._exp_part(a32, None)
    assert ((e > 0) & (e < 2.0 ** -126)).any() and ((e == 0) & (T < 110)).any()        # subnormal e, underflow
    assert len(np.unique(np.round(T[T < 30], 1))) > 200                                  # the sweep
    # the hot points of the double backward take SweepDownHooks::tile's s > 0 switch both ways (and s = 2^-24)
    hot = a32[mp.SP_HOT]
    _, s = mp.sigmoid_restated(mp.softplus_restated(hot)[0])
    assert (s == 0).any() and (s == f32(2.0 ** -24)).any() and (s == 1).any() and ((s > 0.2) & (s < 0.8)).any()
    assert 24 <= len(mp.SP_HOT) <= 64
    assert set(mp.UNIT_K.tolist()) == set(range(8)) and all(set(mp.UNIT_K[mp.UNIT_CHANNEL == c]) == set(range(8)) for c in range(3))


def test_every_slot_and_every_lead_column_is_probed():
    for m in mp.PE_MULTIRES:
        n = mp.pe_slots(m)
        assert n <= mp.PE_WIDTH and n == {6: 39, 7: 45, 1: 9}[m]
        st = mp.pe_state(m, np.ones(mp.PE_WIDTH), False)
        assert st['lin0.weight'].shape == (mp.PE_WIDTH, n)
        assert (st['lin0.weight'] != 0).sum(0).tolist() == [1] * n                      # every slot read by one unit
        x = mp.PE_X[m]
        assert x.shape == (96, 3) and (x == 0).all(1).any() and ((x != 0).sum(1) == 1).sum() >= 3
        top = 2.0 ** (m - 1) * x
        if m > 1:         # (multires 1: |x| <= 1.5 stays below pi / 2)
            assert (np.abs(top / (np.pi / 2) - np.round(top / (np.pi / 2)))[np.abs(top) > 1] < 2e-3 * 2.0 ** (m - 1)).any()
    for mode, m in mp.VIEW_CASES.values():
        lead = mp.view_lead(mode, m)
        picked = []
        for st in range(mp.view_states(mode, m)):
            W1 = mp.view_state(mode, m, st)['lin1.weight']
            picked += [int(W1[r].argmax()) for r in range(3) if W1[r].any()]
        assert picked == list(range(lead)), (mode, m)
        assert mp.view_columns(mode, m)[0].shape == (mp.COLOR_P, lead)
    assert mp.COLOR_P == 217 and mp.COLOR_P % mp.COLOR_SPR == 0
    # the normal's slots at multires_view = 4 cross a quarter boundary (slots 28 .. 31 | 32 .. 35)
    assert 6 + 6 * 4 == 30 and 30 // 4 != 32 // 4
    o = mp.sigmoid_inputs()[1]
    for v in mp.SIG_SPECIAL:
        assert all((o[:, r] == v).any() for r in range(3)), v


def _mutant_escapes(name):
    """Does mutant `name` of a restatement leave a bound (the widest one: bf16x3's) on at least one case?"""
    a0, a1, a32 = _sp()
    h = mp.softplus_restated(a32)[0]
    if name in ('select_inverted', 'const_100', 'threshold_dropped'):
        out = _escapes(mp.softplus_restated(a32, name)[0], mp.softplus64(a1), mp.bound_h(a1, True) + mp.PLANE2 * mp.softplus64(a1))
        if name == 'const_100':
            s = mp.sigmoid_restated(h, name)[1]
            out = out and _escapes(s, mp.sigmoid64(100 * a1), mp.bound_s(a1, True) + mp.PLANE2)
        return out
    if name == 's_wrong_side':
        return _escapes(mp.sigmoid_restated(h, name)[1], mp.sigmoid64(100 * a1), mp.bound_s(a1, True) + mp.PLANE2)
    if name in ('u_dropped', 's_for_u', 'no_division'):
        ref = 100 * mp.sigmoid64(100 * a1) * mp.sigmoid64(-100 * a1) * mp.UNIT_SCALE
        return _escapes(mp.second_order_restated(h, mp.UNIT_SCALE.astype(f32), name), ref, mp.bound_t(a1, mp.UNIT_SCALE, True))
    if name in ('sincos_swapped', 'octave_off', 'dval_sign', 'channel_rotated'):
        out = True
        for m in mp.PE_MULTIRES:
            hit = False
            for j in range(3, mp.pe_slots(m)):
                s, c = mp.pe_reference(m, j, name)
                if name == 'channel_rotated':
                    # the derivative lands in a channel where exactly 0 is expected
                    hit = hit or (c != s.c and bool((s.dval32 != 0).any()))
                elif name == 'dval_sign':
                    hit = hit or _escapes(s.dval32, s.dval, mp.bound_pe(s.dval))
                else:
                    hit = hit or _escapes(s.a0_32, s.a0, mp.pe_da0(s, 'bf16x3') + mp.PLANE2 * s.a0)
            out = out and hit
        if name in ('sincos_swapped', 'octave_off'):
            for mode, m in mp.VIEW_CASES.values():
                val, val32, pre, pre32, bnd, n0 = mp.view_columns(mode, m, name)
                out = out and _escapes(pre32, pre, mp.view_bound(val, pre, bnd, 'bf16x3'))
        return out
    if name == 'normal_shifted':
        return all(any(not np.array_equal(mp.view_g_nrm('idr', m, st), mp.view_g_nrm('idr', m, st, name))
                       for st in range(mp.view_states('idr', m))) for m in (4, 2))
    if name == 'sigmoid_backward_gy':
        feat, o, g = mp.sigmoid_inputs()
        ref = g * mp.sigmoid64(o) * mp.sigmoid64(-o)
        return _escapes(mp.color_sigmoid_restated(o, g, name)[1], ref, mp.bound_color_sigmoid(o, g)[1] + mp.PLANE2 * np.abs(ref))
    raise AssertionError(name)


@pytest.mark.parametrize('name', mp.MUTANTS)
def test_bounds_separate_the_formula_from_its_mutants(name):
    assert _mutant_escapes(name), name


def test_the_threshold_select_is_the_one_thing_unseen():
    """Dropping `100 a > 20 ? a : ...` changes h by less than 2.1e-11 at a >= 0.2, where half an ulp is 7.5e-9: it stays
    within the tightest bound (fp32's), so no probe of h can see it.  Named, not hidden."""
    assert mp.UNSEEN == ('threshold_dropped',)
    a0, a1, a32 = _sp()
    h, hv = mp.softplus_restated(a32)[0], mp.softplus_restated(a32, 'threshold_dropped')[0]
    assert (np.abs(h.astype(f64) - hv)[a1 > 0.2]).max() < 2.1e-11 + 2 * mp.U * 2
    assert not _escapes(hv, mp.softplus64(a1), mp.bound_h(a1))
