"""tests/mlp_exact_cases.py on the CPU: the cases keep their conditions, the certificate accepts them and rejects
hand-made violations, an emulation of the three matrix cores reproduces the float64 reference bit for bit on every
certified product, and the probe cases have teeth -- each kept plane product, k tile, out tile and point, removed,
changes a result."""
import pytest
import torch

import mlp_exact_cases as mx

NAMES = list(mx.ALL_CASES)
# what the two-plane core is certified on: everything whose products need no more than (1,1), (1,2), (2,1)
X3_NOT_CERTIFIED = {'color.w64_h2_idr_big_p65', 'probe.w3f1g1', 'probe.w1f3g1', 'probe.w1f1g3', 'probe.w2f2g1',
                    'probe.w2f1g2', 'probe.h2_w1f3g1', 'probe.h2_w1f1g3'}
P_EDGES = {1, 15, 16, 17, 63, 64, 65, 213}


# ---- the cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_products_amount_to_the_reference(name):
    """The pass written product by product (what the certificate looks at) gives exactly what float64 autograd gives."""
    case = mx.ALL_CASES[name]
    _, out, _ = mx.products(case)
    ref = mx.reference(case)
    assert set(out) == set(ref)
    for k in ref:
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), (name, k)
        assert torch.equal(ref[k].float().double(), ref[k]), (name, k, 'not an fp32 value')


def test_cases_cover_the_sizes_and_options():
    for cases in (mx.COLOR_CASES, mx.SDF_CASES):
        assert P_EDGES <= {c.args['P'] for c in cases.values()}
    col = [c.args for c in mx.COLOR_CASES.values()]
    assert {a['width'] for a in col} >= {64, 48, 100, 176, 256} and {a['hidden'] for a in col} == {1, 2, 3}
    assert {a['mode'] for a in col} == {'idr', 'nerf'} and {a['code'] for a in col} == {True, False}
    assert 256 in {a['F'] for a in col} and any(a['F'] % 16 for a in col)
    assert any(a['spr'] == 7 and a['P'] % 64 and a['P'] > 128 for a in col)
    sdf = [c.args for c in mx.SDF_CASES.values()]
    assert {a['width'] for a in sdf} >= {64, 48, 100, 256} and {a['hidden'] for a in sdf} == {2, 3}


@pytest.mark.parametrize('name', ['sdf.' + n for n in mx.SDF_CASES] + ['grid.' + n for n in mx.GRID_CASES])
def test_sdf_inputs_keep_softplus_at_relu(name):
    case = mx.ALL_CASES[name]
    hid = case.args['hidden']
    for l in range(hid):
        W, b = case.state['lin%d.weight' % l], case.state['lin%d.bias' % l]
        assert torch.equal(W % 4, torch.zeros_like(W)) and torch.equal(b % 4, torch.full_like(b, 2))
    x = case.inputs['x']
    if case.kind == 'grid':
        # points on multiples of 1/8 inside [-1, 1], both kinds of position (on a node, half-way) and both ends; integer
        # tables; first-layer weights multiples of 32; levels of scale 8, dense or (logmap 9) hashed with 512 entries
        W0, emb = case.state['lin0.weight'], case.state['encoding.embeddings']
        assert torch.equal(W0 % 32, torch.zeros_like(W0)) and torch.equal(emb, emb.round())
        assert x.abs().max() <= 1 and ((8 * x) % 2 == 0).any() and ((8 * x) % 2 == 1).any()
        x = 8 * x
        conf = mx.grid_conf(case)
        geo = mx.hg.level_geometry(conf)
        assert (conf['base_size'], conf['end_size'], conf['divide_factor']) == (9, 9, 1.0)
        assert (geo['L'], geo['C']) == (case.args['num_levels'], case.args['level_dim'])
        assert geo['S'] == 0.0 and all(mx.hg.level_scale(geo, l) == (8.0, 9) for l in range(geo['L']))
        size = 729 if case.args['logmap'] == 19 else 2 ** case.args['logmap']
        assert size <= 729 and [geo['offsets'][l + 1] - geo['offsets'][l] for l in range(geo['L'])] == [size] * geo['L']
        assert emb.shape == (geo['n_entries'], geo['C']) and W0.shape[1] == 3 + geo['L'] * geo['C']
    assert torch.equal(x, x.round())
    pre = mx.products(case)[2]
    assert len(pre) == hid and not mx.check_preactivations(pre)
    for a in pre:                                       # both sides of the switch in every layer
        assert (a >= 2).any() and (a <= -2).any()


@pytest.mark.parametrize('name', ['w64_h1_idr_p213', 'w48_h2_idr_p65', 'w64_h2_idr_code_spr7_p217', 'w64_h3_nerf_p15'])
def test_color_cases_hold_relu_ties(name):
    """Hidden and output pre-activations of exactly zero (mask h > 0 / y > 0: zero on both sides), next to both signs."""
    pre = mx.products(mx.COLOR_CASES[name])[2]
    for a in pre:
        assert (a == 0).any() and (a > 0).any() and (a < 0).any()


# ---- hash-grid cases: geometry, layouts and paths ---------------------------------------------------------------------
def test_first_grid_cases_keep_their_geometry():
    """The three cases from before the geometry moved into case.args: four dense levels of two features."""
    for n in ('w64_h2_p213', 'w48_h3_p65', 'w64_h2_p17'):
        a = mx.GRID_CASES[n].args
        assert (a['num_levels'], a['level_dim'], a['logmap'], a['second_order']) == (4, 2, 19, True)
        assert mx.GRID_CASES[n].state['encoding.embeddings'].shape == (4 * 729, 2)


def test_grid_layout_cases_cover_the_table():
    layouts = {(c.args['level_dim'], c.args['num_levels'], c.args['logmap']) for c in mx.GRID_CASES.values()}
    assert layouts == set(mx.GRID_REACHES) and set(mx.GRID_LAYOUTS) | {(2, 4, 19)} == layouts
    for c, l, m in mx.GRID_LAYOUTS:
        ps = {P for P in (17, 65, 213) if mx.grid_layout_name(c, l, m, P) in mx.GRID_CASES}
        assert ps == ({17, 65, 213} if (c, l) == (2, 16) else {17, 65}), (c, l, m)
    # level_dim 1 alone has no second-order term
    assert {n for n, c in mx.GRID_CASES.items() if not c.args['second_order']} == {'l5c1_p17', 'l5c1_p65'}
    for n in ('l5c1_p17', 'l5c1_p65'):
        assert not mx.GRID_CASES[n].up['C'].any() and mx.GRID_CASES[n].up['a'].any()


@pytest.mark.parametrize('name', ['grid.' + n for n in mx.GRID_CASES])
def test_grid_cases_reach_their_layout_and_paths(name):
    case = mx.ALL_CASES[name]
    paths = {run: mx.assert_grid_reaches(name, run) for run in mx.GRID_RUNS}
    assert set(paths.values()) <= set(mx.PATH_CALLS)
    gs = mx.grid_structure(case)
    assert gs['full'] + gs['half'] + gs['empty'] == 4 * gs['aux_tiles'] and gs['aux_tiles'] == -(-gs['LC'] // 16)
    assert (gs['half'] == 1) == (gs['level_major'] and case.args['num_levels'] % 2 == 1) or not gs['level_major']
    if gs['hashed']:
        # corners of different grid points share table entries: the table gradient sums colliding records
        geo = mx.hg.level_geometry(mx.grid_conf(case))
        p = torch.stack(torch.meshgrid(*[torch.arange(10)] * 3, indexing='ij'), -1).reshape(-1, 3)
        idx = mx.hg.grid_index(p, geo['offsets'][1] - geo['offsets'][0], 9)
        assert idx.unique().numel() < p.shape[0] and mx.hg.grid_index(p[:1], 729, 9).item() == 0


def test_grid_cases_take_every_piece_and_every_path():
    """Between them the level-major cases take a full, a half and an empty piece in tile 0 and in tile 1, the half-piece
    at every quarter; and the runs of GRID_RUNS take all five paths."""
    seen, halves, paths = set(), set(), set()
    for name, case in mx.GRID_CASES.items():
        gs = mx.grid_structure(case)
        if gs['level_major']:
            seen |= {(t, k) for t, _, k in gs['pieces']}
            halves |= {q for _, q, k in gs['pieces'] if k == 'half'}
        for run, (core, fuse, scatter) in mx.GRID_RUNS.items():
            paths.add(mx.grid_path(case, core, fuse, scatter))
    assert seen == {(t, k) for t in (0, 1) for k in ('full', 'half', 'empty')}
    assert halves == {0, 1, 2, 3}
    assert paths == set(mx.PATH_CALLS)


def test_grid_path_follows_the_flags():
    c2, c4, c1 = mx.GRID_CASES['l16c2_p17'], mx.GRID_CASES['l8c4_p17'], mx.GRID_CASES['l5c1_p17']
    assert mx.grid_path(c2, 'fp32') == 'fused_jacobian' and mx.grid_path(c2, 'fp32', fuse_jacobian=False) == 'level_major'
    assert mx.grid_path(c2, 'bf16x6', fuse_jacobian=False) == 'rows_b16' and mx.grid_path(c4, 'fp32') == 'rows_fp32'
    assert mx.grid_path(c4, 'bf16x3') == 'rows_b16' and mx.grid_path(c4, 'fp32', hash_scatter='atomic') == 'separate'
    assert mx.grid_path(c1, 'fp32') == 'separate' and mx.grid_path(c1, 'bf16x6') == 'separate'
    for must, must_not in mx.PATH_CALLS.values():
        assert not set(must) & set(must_not)


# ---- the certificate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_certificate_accepts_the_cases(name):
    case = mx.ALL_CASES[name]
    for core in ('fp32', 'bf16x6'):
        cert = mx.certificate(case, core)
        assert cert.ok, (core, cert.failures[:3])
    assert mx.certificate(case, 'bf16x3').ok == (name not in X3_NOT_CERTIFIED)


def test_every_core_has_a_full_case_of_every_kind():
    ok3 = [n for n in NAMES if mx.certificate(mx.ALL_CASES[n], 'bf16x3').ok]
    for kind in ('color.', 'sdf.', 'probe.', 'grid.', 'skip.', 'clamp.', 'group.'):
        assert any(n.startswith(kind) for n in ok3)
    # a full case: forward, transposed and weight-gradient products, all of them certified
    for n in ('color.w100_h2_idr_code_f40_p63', 'sdf.w48_h3_f24_p65'):
        assert n in ok3 and {p.role for p in mx.products(mx.ALL_CASES[n])[0]} == {'forward', 'transposed', 'wgrad', 'dot'}


def _product(A, B, unit='core', adds=()):
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    return mx.Product('hand', 'forward', unit, t(A), t(B), tuple(t(a) for a in adds), None)


def test_certificate_rejects_a_sum_over_the_bound():
    fits = _product([[2.0 ** 23, 2.0 ** 23 - 1]], [[1.0], [1.0]])
    over = _product([[2.0 ** 23 + 1, 2.0 ** 23 - 1]], [[1.0], [1.0]])
    for core in mx.CORES:
        assert not mx.check_product(fits, 'fp32')
        assert any('2^24' in w for w in mx.check_product(over, core)), core
    # the granule counts: the same magnitudes in steps of 1/8 are eight times too many
    assert mx.check_product(_product([[2.0 ** 21, 2.0 ** 21 + 0.125]], [[1.0], [4.0]]), 'fp32')
    assert not mx.check_product(_product([[2.0 ** 19, 2.0 ** 18 + 0.125]], [[1.0], [4.0]]), 'fp32')
    # ... and the summand a product starts from or ends with
    assert mx.check_product(_product([[2.0 ** 23 + 1]], [[1.0]], adds=[[[2.0 ** 23 - 1]]]), 'fp32')
    assert not mx.check_product(_product([[2.0 ** 23 + 1]], [[1.0]], adds=[[[2.0 ** 23 - 2]]]), 'fp32')
    # a whole case: three-plane weights against three-plane features
    case = mx.color_case('over', wp=3, fp=3, P=17, in_max=1, seed=7)
    for core in mx.CORES:
        assert not mx.certificate(case, core).ok


def test_certificate_rejects_plane_products_a_core_does_not_form():
    two_by_two = _product([[257.0]], [[257.0]])
    assert not mx.check_product(two_by_two, 'fp32') and not mx.check_product(two_by_two, 'bf16x6')
    assert any('(2, 2)' in w for w in mx.check_product(two_by_two, 'bf16x3'))
    # the weight-gradient kernel of bf16x6 is the fp32 one, that of bf16x3 forms the same three products
    assert not mx.check_product(two_by_two._replace(unit='wgrad'), 'bf16x6')
    assert mx.check_product(two_by_two._replace(unit='wgrad'), 'bf16x3')
    assert not mx.check_product(two_by_two._replace(unit='dot'), 'bf16x3')
    two_by_three = _product([[257.0]], [[131329.0]])
    assert any('(2, 3)' in w for w in mx.check_product(two_by_three, 'bf16x6'))
    assert not mx.check_product(_product([[1.0]], [[131329.0]]), 'bf16x6')
    assert not mx.check_product(_product([[131329.0]], [[3.0]]), 'bf16x6')
    cert = mx.certificate(mx.PROBE_CASES['w2f2g1'], 'bf16x3')
    assert not cert.ok and any(w.startswith('u0.fwd') and '(2, 2)' in w for w in cert.failures)
    # not an fp32 value at all
    assert mx.check_product(_product([[2.0 ** 24 + 1]], [[1.0]]), 'fp32')


@pytest.mark.parametrize('bias', [0.0, 1.0, -1.0, 0.5])
def test_certificate_rejects_a_preactivation_near_the_switch(bias):
    base = mx.SDF_CASES['w64_h2_p15']
    state = dict(base.state)
    state['lin0.bias'] = torch.full_like(state['lin0.bias'], bias)      # a = 4 k + bias
    case = base._replace(state=state)
    for core in mx.CORES:
        cert = mx.certificate(case, core)
        assert not cert.ok and any(w.startswith('layer 0') for w in cert.failures)


def test_plane_units_have_the_planes_they_are_named_for():
    for n, unit in mx.PLANE_UNIT.items():
        for k in (1, 2, 3, -1, -3):
            planes = mx.split_planes(torch.tensor([k * unit]))
            assert [bool(p.any()) for p in planes] == [i < n for i in range(3)], (n, k)
            assert sum(p.double() for p in planes).item() == k * unit


# ---- emulation of the cores ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_emulated_cores_equal_the_reference_on_certified_products(name):
    case = mx.ALL_CASES[name]
    for core in mx.CORES:
        for pr in mx.products(case)[0]:
            if mx.check_product(pr, core):
                continue
            exact = mx.want(pr)
            for seed in (1, 2):
                got = mx.emulate(pr, core, seed=seed)
                assert torch.equal(got.double(), exact), (name, core, pr.name, mx.first_difference(got, exact))


def test_an_uncertified_product_is_not_exact():
    """The plane condition is needed: where the certificate names a missing plane product, the emulation is off."""
    for name, product, core in (('w2f2g1', 'u0.fwd', 'bf16x3'), ('w3f1g1', 'u0.bwd', 'bf16x3'),
                                ('w1f3g1', 'u0.fwd', 'bf16x3')):
        pr = [p for p in mx.products(mx.PROBE_CASES[name])[0] if p.name == product][0]
        assert mx.check_product(pr, core)
        assert not torch.equal(mx.emulate(pr, core).double(), mx.want(pr))
        assert torch.equal(mx.emulate(pr, 'bf16x6').double(), mx.want(pr))


# ---- teeth --------------------------------------------------------------------------------------------------------
def _changed_by(drop, core, role, cases):
    """The (case, product) pairs, certified on this core, whose emulated result changes when `drop` is lost."""
    hit = []
    for name, case in cases.items():
        if not mx.certificate(case, core).ok:
            continue
        for pr in mx.products(case)[0]:
            if pr.role == role and mx.arithmetic(pr.unit, core) and \
                    not torch.equal(mx.emulate(pr, core, drop=drop).double(), mx.want(pr)):
                hit.append((name, pr.name))
    return hit


@pytest.mark.parametrize('core,role', [('bf16x3', 'forward'), ('bf16x3', 'transposed'), ('bf16x3', 'wgrad'),
                                       ('bf16x6', 'forward'), ('bf16x6', 'transposed')])
def test_every_kept_plane_product_carries_a_result_bit(core, role):
    """b16_step without one of its lines (three for bf16x3, six for bf16x6): a probe case certified on that core changes,
    in the forward product, in a transposed one and (bf16x3: its own weight-gradient kernel) in a weight gradient."""
    for pair in mx.KEPT[mx.PLANES[core]]:
        assert _changed_by(('pair', pair), core, role, mx.PROBE_CASES), (core, role, pair)


def test_probes_reach_the_first_layers_feature_product():
    """... and it is the product the probes are built around that notices: weights x features, weights^T x a-bar."""
    want = {('bf16x6', 'forward', (1, 3)): ('w1f3g1', 'u0.fwd'), ('bf16x6', 'forward', (3, 1)): ('w3f1g1', 'u0.fwd'),
            ('bf16x6', 'forward', (2, 2)): ('w2f2g1', 'u0.fwd'), ('bf16x6', 'transposed', (3, 1)): ('w3f1g1', 'u0.bwd'),
            ('bf16x6', 'transposed', (1, 3)): ('w1f1g3', 'u0.bwd'), ('bf16x6', 'transposed', (2, 2)): ('w2f1g2', 'u0.bwd'),
            ('bf16x3', 'forward', (1, 2)): ('w1f2g1', 'u0.fwd'), ('bf16x3', 'forward', (2, 1)): ('w2f1g1', 'u0.fwd'),
            ('bf16x3', 'transposed', (1, 2)): ('w1f1g2', 'u0.bwd'), ('bf16x3', 'transposed', (2, 1)): ('w2f1g1', 'u0.bwd'),
            ('bf16x3', 'wgrad', (1, 2)): ('w1f2g1', 'u0.wgrad'), ('bf16x3', 'wgrad', (2, 1)): ('w1f1g2', 'u0.wgrad')}
    for (core, role, pair), hit in want.items():
        assert hit in _changed_by(('pair', pair), core, role, mx.PROBE_CASES), (core, role, pair)
    # the hidden product behind a first layer that hands it two- and three-plane activations, and its transpose
    for core, role, pair, hit in (('bf16x6', 'forward', (1, 3), ('h2_w1f3g1', 'u2.fwd')),
                                  ('bf16x6', 'forward', (1, 2), ('h2_w1f3g1', 'u2.fwd')),
                                  ('bf16x6', 'transposed', (1, 3), ('h2_w1f1g3', 'u2.bwd')),
                                  ('bf16x3', 'forward', (1, 2), ('h2_w1f2g1', 'u2.fwd')),
                                  ('bf16x3', 'transposed', (1, 2), ('h2_w1f1g2', 'u2.bwd'))):
        assert hit in _changed_by(('pair', pair), core, role, mx.PROBE_CASES), (core, role, pair)


@pytest.mark.parametrize('name', ['color.w100_h2_idr_code_f40_p63', 'sdf.w48_h3_f24_p65', 'probe.w2f1g1'])
@pytest.mark.parametrize('core', mx.CORES)
def test_a_lost_tile_or_point_changes_the_result(name, core):
    """One k tile, one out tile or one point dropped from a product of a matrix core: the result differs wherever the
    dropped part contributes at all, and every out tile and every point does."""
    case = mx.ALL_CASES[name]
    for pr in mx.products(case)[0]:
        if pr.unit != 'core':
            continue
        exact = mx.want(pr)
        contributes = lambda A, B: bool((A @ B).any())
        m, k = pr.A.shape
        n = pr.B.shape[1]
        live = 0
        for t in range(-(-k // 16)):
            s = slice(16 * t, 16 * t + 16)
            changed = not torch.equal(mx.emulate(pr, core, drop=('ktile', t)).double(), exact)
            assert changed == contributes(pr.A[:, s], pr.B[s]), (pr.name, 'k tile', t)
            live += changed
        assert live >= 1, pr.name
        for t in range(-(-m // 16)):
            s = slice(16 * t, 16 * t + 16)
            changed = not torch.equal(mx.emulate(pr, core, drop=('otile', t)).double(), exact)
            assert changed == contributes(pr.A[s], pr.B), (pr.name, 'out tile', t)
            if pr.role == 'forward' and pr.name != 'out.fwd':
                assert changed, (pr.name, 'out tile', t)
        for p in sorted({0, n // 2, n - 1}):
            changed = not torch.equal(mx.emulate(pr, core, drop=('point', p)).double(), exact)
            assert changed == contributes(pr.A, pr.B[:, p:p + 1]), (pr.name, 'point', p)
            if pr.role == 'forward' and pr.name.endswith('.fwd'):
                assert changed, (pr.name, 'point', p)


# ---- structure ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('core', mx.CORES)
def test_cases_reach_the_branches_they_are_named_for(core):
    for name in mx.REACHES:
        mx.assert_reaches(name, core)
    kernels, flags = set(), set()
    for name, case in mx.ALL_CASES.items():
        for d in mx.structure(case, core).values():
            if 'kernel' not in d:               # the two-part weight-gradient item of a skip layer: no matrix-core product
                continue
            kernels.add(d['kernel'])
            flags |= {k for k in ('odd_last_tile', 'dead_pair', 'partial_last_chunk') if d[k]}
            if core == 'fp32' and d['pairs_per_chunk'] > 1:
                flags.add('chunks=%d' % d['chunks'] if d['chunks'] > 1 else 'one chunk')
    if core == 'fp32':
        assert kernels == {'gemm_tiles<3,4>', 'gemm_tiles<5,3>', 'gemm_tiles<16,1>', 'gemm_tiles<17,1>', 'gemm_tiles<0,1>'}
        assert {'chunks=2', 'one chunk'} <= flags
    else:
        ns = mx.PLANES[core]
        assert kernels == {'gemm_b16<%d,%d>' % (ns, k) for k in (0, 2, 3, 8, 9)}
    assert {'odd_last_tile', 'dead_pair'} <= flags and (('partial_last_chunk' in flags) == (core != 'bf16x6'))


def test_structure_follows_the_plans():
    """structure() reads the tile counts from the plans of monosdf_amd/plan.py, not from the case names."""
    case = mx.SDF_CASES['w256_h2_f256_p17']
    mp = mx.build_plan(case)
    assert [(mp.plan.layer[l].kt, mp.plan.layer[l].ot, mp.plan.layer[l].ktp, mp.plan.layer[l].otp) for l in range(3)] == \
        [(3, 16, 3, 16), (16, 16, 16, 16), (16, 17, 16, 17)]
    p16 = mp.build_b16(3)
    assert [(p16.layer[l].ktp, p16.layer[l].otp) for l in range(3)] == [(2, 8), (8, 8), (8, 9)]
    st = mx.structure(case, 'fp32')
    assert st['out.fwd']['chunks'] == 9 and st['out.fwd']['pairs'] == 9 and st['l0.fwd']['pairs_per_chunk'] == 4


def test_first_difference_names_the_slot():
    want = torch.zeros(130, 48)
    assert mx.first_difference(want.clone(), want) is None
    got = want.clone()
    got[77, 39] = 1.0
    got[100, 2] = 1.0
    d = mx.first_difference(got, want)
    assert (d['row'], d['column'], d['workgroup'], d['wave'], d['tile'], d['quarter'], d['component']) == (77, 39, 1, 0, 2, 1, 3)
    assert d['n_different'] == 2 and d['got'] == 1.0 and d['want'] == 0.0
    assert mx.first_difference(torch.zeros(3), torch.zeros(4)) == dict(shape=((3,), (4,)))
    assert mx.first_difference(torch.tensor([0.0, 2.0]), torch.tensor([0.0, 1.0]))['row'] == 1


# ---- the skip layer, the sphere clamp and the point groups ----------------------------------------------------------
NEW_SDF = ['skip.' + n for n in mx.SDF_SKIP_CASES] + ['clamp.' + n for n in mx.SDF_CLAMP_CASES] + \
    ['group.' + n for n in mx.SDF_GROUP_CASES]


def test_new_sdf_cases_are_certified_on_all_three_cores():
    """Skip, clamp and group cases hold their certificates on fp32, bf16x6 and -- every one of them -- on bf16x3: the
    effective skip weights +-4, +-8 have one bf16 plane, and so has everything the two-plane weight-gradient unit reads."""
    for name in NEW_SDF:
        for core in mx.CORES:
            cert = mx.certificate(mx.ALL_CASES[name], core)
            assert cert.ok, (name, core, cert.failures[:3])
    assert not set(NEW_SDF) & X3_NOT_CERTIFIED


def test_skip_magnitudes_are_found_not_written_down():
    case = mx.SDF_SKIP_CASES['w64_h3_s2_p213']
    shapes = [tuple(case.state['lin%d.weight' % l].shape) for l in range(4)]
    assert shapes == [(64, 3), (61, 64), (64, 64), (17, 64)]
    s32 = mx.skip_scale(shapes, (2,), 16)
    # the rule's scale is a C float: it reads back as the Python float of float32(1 / sqrt(2))
    assert isinstance(s32, float) and s32 == torch.tensor(0.5).sqrt().item()
    v4, v8 = mx.skip_magnitudes(s32)
    s = torch.tensor(s32, dtype=torch.float32)
    for v, k in ((v4, 4.0), (v8, 8.0)):
        t = torch.tensor(v, dtype=torch.float32)
        assert t.item() == v and (s * t).item() == k and (s * -t).item() == -k
        assert abs(v - k * 2 ** 0.5) <= 4 * 2.0 ** -21            # within 4 ulp (ulp of [4, 16): 2^-21, 2^-20)
    assert v8 == 2 * v4
    # no such weight exists for 3 or 12: the skip layer uses +-4 and +-8 only
    for k in (3.0, 12.0):
        t = torch.tensor(k * 2 ** 0.5, dtype=torch.float32)
        lo = hi = t
        for _ in range(64):
            assert (s * lo).item() != k and (s * hi).item() != k
            lo, hi = torch.nextafter(lo, torch.tensor(0.0)), torch.nextafter(hi, torch.tensor(100.0))


@pytest.mark.parametrize('name', [n for n in NEW_SDF if mx.ALL_CASES[n].args['skip_in']])
def test_skip_cases_keep_softplus_at_relu_and_are_the_reference_module(name):
    case = mx.ALL_CASES[name]
    a = case.args
    hid, (l,) = a['hidden'], a['skip_in']
    assert case.state['lin%d.weight' % (l - 1)].shape[0] == a['width'] - 3
    assert case.state['lin%d.weight' % l].shape == (a['width'], a['width'])
    We = mx.effective_weight(case, l)
    assert set(We.abs().unique().tolist()) == {0.0, 4.0, 8.0}
    assert ((We[:, :-3] != 0).sum(1) == 2).all() and ((We[:, -3:] != 0).sum(1) == 1).all()
    for i in range(hid):
        W, b = mx.effective_weight(case, i), case.state['lin%d.bias' % i]
        assert torch.equal(W % 4, torch.zeros_like(W)) and torch.equal(b % 4, torch.full_like(b, 2))
    pre = mx.products(case)[2]
    assert len(pre) == hid and not mx.check_preactivations(pre)
    for p in pre:
        assert (p >= 2).any() and (p <= -2).any()
    # the module the reference defines -- cat([h, x]) / sqrt(2) @ W^T in float64 with the STORED weights -- against the
    # effective-weight network.  Only the skip layer differs, each weight by a factor 1 + d with |d| <= 2^-23 (two fp32
    # roundings: of 1 / sqrt(2) and of the product), so every output differs by at most 2^-23 of the sum of its terms'
    # magnitudes M (the same network on |W|, |b|, |x|; ReLU is monotone and 1-Lipschitz, no switch flips at |a| >= 2):
    # 1.2e-7 M, inside 1e-6 relative.  (Relative to an output itself, where terms cancel, up to 1.1e-6 was measured.)
    x = case.inputs['x'].double()
    h, m = x, x.abs()
    for i in range(hid + 1):
        W, b = case.state['lin%d.weight' % i].double(), case.state['lin%d.bias' % i].double()
        if i == l:
            h, m = torch.cat([h, x], 1) / 2 ** 0.5, torch.cat([m, x.abs()], 1) / 2 ** 0.5
        h, m = h @ W.t() + b, m @ W.abs().t() + b.abs()
        if i < hid:
            assert (h.abs() > 1.9).all()
            h = torch.relu(h)
    ref = mx.reference(case)
    exact = torch.cat([ref.get('sdf_raw', ref['sdf']), ref['feat']], 1)
    assert ((h - exact).abs() <= 2.0 ** -23 * m).all() and ((h - exact).abs() <= 1e-6 * m).all()
    assert (h - exact).abs().max() > 0


def test_skip_gradient_is_scaled_once_and_stays_fp32():
    """The expected gradient of the stored skip weights is float32(s32) * float32(G), G the exact integer gradient of the
    effective weights with |G| < 2^24 (certified: the 'scaled_gradient' sum): one rounding, an fp32 value; the bias
    gradient is unscaled (an integer)."""
    for name in NEW_SDF:
        case = mx.ALL_CASES[name]
        for l in case.args['skip_in']:
            ref = mx.reference(case)
            sums = dict((n, mag) for n, mag, _ in mx.other_sums(case))
            G = sums['l%d.scaled_gradient' % l]
            assert torch.equal(G, G.round()) and G.max() < 2.0 ** 24 and G.max() > 0
            got = ref['lin%d.weight' % l]
            assert torch.equal(got.abs(), mx.scaled_gradient(case, G)) and torch.equal(got.float().double(), got)
            assert not torch.equal(got, got.round())
            bg = ref['lin%d.bias' % l]
            assert torch.equal(bg, bg.round()) and bg.any()


def test_skip_cases_cover_the_widths_and_sizes():
    args = [c.args for c in mx.SDF_SKIP_CASES.values()]
    assert {(a['width'], a['hidden'], a['skip_in']) for a in args} == \
        {(64, 3, (2,)), (48, 2, (1,)), (100, 3, (2,)), (176, 4, (2,)), (227, 3, (2,))}
    assert {a['P'] for a in args} == {1, 17, 63, 65, 213}
    kts = {mx.build_plan(c).plan.layer[c.args['skip_in'][0]].kt for c in mx.SDF_SKIP_CASES.values()}
    assert kts == {7, 6, 10, 14, mx.MT}
    for c in mx.SDF_SKIP_CASES.values():
        st = mx.structure(c, 'fp32')
        l, = c.args['skip_in']
        w = st['l%d.wgrad' % l]
        assert w['two_part'] and w['parts'][1] == (16 * w['skip_tile'], 48) and w['kt'] == w['skip_tile'] + 3
        assert st['l%d.fwd' % l]['k'] in (w['kt'], 16) and st['l%d.sweep' % l]['out_tiles'] == w['kt']
        assert st['l%d.down' % l]['out_tiles'] == w['kt'] and st['l%d.up' % l]['k'] == st['l%d.fwd' % l]['k']
    clamp = [c.args for c in mx.SDF_CLAMP_CASES.values()]
    assert {a['width'] for a in clamp} == {64, 100} and {a['P'] for a in clamp} == {65, 213}
    assert any(a['skip_in'] for a in clamp) and {(a['radius'], a['sphere_scale']) for a in clamp} == {(2.5, 1.0), (3.0, 0.5)}


def test_a_skip_layer_at_width_256_does_not_fit():
    """253 outputs are 16 tiles; with the input block behind them the skip layer has 19 > MT in-tiles: the plan refuses."""
    from monosdf_amd import plan as planlib
    with pytest.raises(RuntimeError, match='tile'):
        planlib.build_sdf_plan([(256, 3), (253, 256), (256, 256), (17, 256)], (2,), 0, 0, False, 16)
    planlib.build_sdf_plan([(227, 3), (224, 227), (227, 227), (17, 227)], (2,), 0, 0, False, 16)


@pytest.mark.parametrize('name', [n for n in NEW_SDF if mx.ALL_CASES[n].args['radius'] > 0])
def test_clamp_cases_hold_every_kind_of_point(name):
    case = mx.ALL_CASES[name]
    a = case.args
    assert not mx.clamp_conditions(case)
    n_clamp, n_feat, split = mx.groups(case)
    c = mx.clamp_restatement(case)
    x = case.inputs['x']
    assert torch.equal(x, x.round()) and torch.equal(x[:len(mx.SPECIAL_POINTS)], torch.tensor(mx.SPECIAL_POINTS).float())
    assert not x[0].any() and not x[-1].any()
    # integer and power-of-two norms come out exactly, whatever the sqrt
    assert c.nx[:12].tolist() == [0, 1, 2, 4, 3, 3, 3, 7, 7, 5, 5, 5]
    ref = mx.reference(case)
    raw = ref['sdf_raw'][:, 0]
    assert ((raw - c.sph).abs() >= mx.CLAMP_MARGIN).all()
    clamped = (torch.arange(a['P']) < n_clamp) & (c.sph < raw)
    assert torch.equal(ref['sdf'][:, 0], torch.where(clamped, c.sph, raw))
    assert torch.equal(ref['grad'][clamped], c.normals[clamped]) and torch.equal(ref['grad'][~clamped], ref['grad_raw'][~clamped])
    if n_clamp > 0:
        # the origin: clamped, sdf = scale * r, normals 0 (torch's minimum gives the point a zero gradient)
        assert clamped[0] and ref['sdf'][0, 0] == a['sphere_scale'] * a['radius'] and (ref['grad'][0] == 0).all()
    # float64 autograd agrees with the fp32 restatement to fp32 rounding on the clamped rows
    x64 = x.double().requires_grad_()
    sph64 = a['sphere_scale'] * (a['radius'] - x64.norm(dim=1))
    n64, = torch.autograd.grad(sph64.sum(), x64)
    assert (c.sph - sph64.detach()).abs().max() <= 2.0 ** -22 and (c.normals - n64).abs().max() <= 2.0 ** -22


def test_group_cases_cover_every_value():
    args = [c.args for c in mx.SDF_GROUP_CASES.values()]
    assert all((a['width'], a['hidden'], a['P']) == (64, 2, 150) and a['radius'] > 0 for a in args)
    assert {a['n_feat'] for a in args} == {0, 1, 16, 63, 64, 65, 150}
    assert {a['n_clamp'] for a in args} == {0, 17, 64, 150}
    assert {a['split'] for a in args} == {0, 15, 64, 129, 150}
    assert any(len({a['n_clamp'], a['n_feat'], a['split']}) == 3 and
               all(v % 16 for v in (a['n_clamp'], a['n_feat'], a['split'])) for a in args)
    for c in mx.SDF_GROUP_CASES.values():
        s, P = c.args['split'], c.args['P']
        assert c.up['a'][0].shape == (s, 1) and c.up['a'][1] is None
        assert c.up['C'][0].shape == (s, 3) and c.up['C'][1].shape == (P - s, 3) and c.up['B'].shape == (P, 16)
        ref = mx.reference(c)
        assert ref['feat'].shape == (c.args['n_feat'], 16) and ref['sdf'].shape == (P, 1)


SKIP = {'skip.' + n: c for n, c in mx.SDF_SKIP_CASES.items()}
CLAMP = {'clamp.' + n: c for n, c in mx.SDF_CLAMP_CASES.items()}
GROUP = {'group.' + n: c for n, c in mx.SDF_GROUP_CASES.items()}


def _noticed(mutation, cases):
    """{case: the outputs that differ} over the cases, certified on all three cores, on which the mistake shows."""
    hit = {}
    for name, case in cases.items():
        assert all(mx.certificate(case, core).ok for core in mx.CORES)
        ref, got = mx.reference(case), mx.mutated_outputs(case, mutation)
        assert set(got) == set(ref)
        diff = sorted(k for k in ref if got[k].shape != ref[k].shape or not torch.equal(got[k], ref[k]))
        if diff:
            hit[name] = diff
    return hit


def test_every_mutation_is_listed():
    assert set(mx.MUTATIONS) == {m for m, _, _ in MUTATION_TEETH}
    for case in list(SKIP.values())[:1] + list(GROUP.values())[:1]:
        ref, same = mx.reference(case), mx._sdf_products(case)[1]
        assert all(torch.equal(same[k], ref[k]) for k in ref)


# mutation, the cases it must show on, outputs that must be among the differing ones
MUTATION_TEETH = [
    ('one_input_arrival', SKIP, {'grad'}),
    ('no_input_columns', SKIP, set()),
    ('scale_twice', SKIP, set()),
    ('no_scale', SKIP, set()),
    ('clamp_all', GROUP, {'sdf', 'grad'}),
    ('clamped_live', dict(CLAMP, **GROUP), {'lin0.weight', 'lin0.bias'}),
    ('no_feat_grad_when_clamped', dict(CLAMP, **GROUP), {'lin0.weight'}),
    ('feat_row_n_feat', GROUP, {'lin2.weight', 'lin2.bias'}),
    ('second_tensor_at_pt', GROUP, {'lin0.weight'}),
]


@pytest.mark.parametrize('mutation,cases,keys', MUTATION_TEETH, ids=[m for m, _, _ in MUTATION_TEETH])
def test_each_mistake_changes_a_certified_expected_value(mutation, cases, keys):
    """The pass restated with one mistake in it (mlp_exact_cases.MUTATIONS): an expected value of a case certified on
    all three cores changes, so the bit-exact comparison on the GPU sees that mistake."""
    hit = _noticed(mutation, cases)
    assert hit, mutation
    assert any(keys <= set(d) for d in hit.values()), (mutation, hit)
    if cases is SKIP:
        # every skip case notices, in the skip layer's own weight gradient (or in d sdf / d x)
        assert set(hit) == set(SKIP), (mutation, sorted(set(SKIP) - set(hit)))
        if mutation != 'one_input_arrival':
            for name, d in hit.items():
                assert d == ['lin%d.weight' % SKIP[name].args['skip_in'][0]], (name, d)
    if mutation == 'clamp_all':
        # shows exactly where n_clamp < P
        assert set(hit) == {n for n, c in GROUP.items() if c.args['n_clamp'] < c.args['P']}
    if mutation == 'feat_row_n_feat':
        assert set(hit) == {n for n, c in GROUP.items() if c.args['n_feat'] < c.args['P']}
    if mutation == 'second_tensor_at_pt':
        # every row from `split` on reads another row of the second tensor, or past its end
        assert set(hit) == {n for n, c in GROUP.items() if 0 < c.args['split'] < c.args['P']}
    if mutation == 'clamped_live':
        assert set(hit) >= set(CLAMP)


def test_point_groups_do_not_change_what_a_point_gets():
    """Both forms of the output layer and both gradient tensors carry the same exact integers: a row's sdf, features and
    gradient depend on the groups only through the clamp (cases of one seed share network and points)."""
    by_seed = {}
    for n, c in mx.SDF_GROUP_CASES.items():
        by_seed.setdefault(tuple(c.inputs['x'].flatten().tolist()), []).append(c)
    assert max(len(v) for v in by_seed.values()) >= 2
    for cs in by_seed.values():
        for c in cs[1:]:
            r0, r1 = mx.reference(cs[0]), mx.reference(c)
            assert torch.equal(r0['sdf_raw'], r1['sdf_raw']) and torch.equal(r0['grad_raw'], r1['grad_raw'])
            k = min(cs[0].args['n_feat'], c.args['n_feat'])
            assert torch.equal(r0['feat'][:k], r1['feat'][:k])
