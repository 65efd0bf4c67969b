"""The sampler's edge cases (tests/sampler_cases.py) are fair: conditions on the INPUTS that the GPU test
(tests/test_gpu_sampler_edges.py) relies on, checked on the CPU.  If one fails, the case (its seed) changes, not the bar.

  conditioning   the fp32 reference stays within half of each bar of tests/test_gpu_sampler.py against the float64 one
                 (d*, the bound at beta0, beta, the cdf); where a cdf misses that, the GPU test's bar for that case is
                 four times the fp32 reference's own deviation (sampler_cases.cdf_bar) and stays below 1e-4;
  coverage       every 64-interval chunk holds 5% of some ray's pdf mass, in both pdf forms, and the argmax of some
                 ray's bound at beta0; rays on both sides of eps; every d* branch on both sides of a chunk edge;
  knife edges    rays whose err0 test or a bisection step decides within 1e-4 eps in float64 are left out of the beta,
                 cdf and sample comparisons: at most one ray in 16, none of the rays that cross at a chunk edge;
  restatement    sampler_cases.finish_restatement against torch.sort and tests/reuse_numpy.py.
"""
import numpy as np
import pytest
import torch

import reuse_numpy as rn
import sampler_cases as sc
from oracle import monosdf_oracle as mo
from test_gpu_sampler import TOL_BETA, TOL_CDF, TOL_DSTAR, TOL_ERR0

HALF = {'dstar': TOL_DSTAR / 2, 'err0': TOL_ERR0 / 2, 'beta': TOL_BETA / 2, 'cdf': TOL_CDF / 2}


@pytest.fixture(scope='module')
def refs():
    memo = {}

    def get(c, mode):
        if (c, mode) not in memo:
            case = sc.edge_case(*c)
            memo[(c, mode)] = (case, sc.reference(case, mode, torch.float32), sc.reference(case, mode, torch.float64))
        return memo[(c, mode)]
    return get


@pytest.mark.parametrize('mode', sc.MODES)
@pytest.mark.parametrize('c', sc.CASES, ids=sc.case_id)
def test_fp32_reference_within_half_of_the_bars(c, mode, refs):
    case, r32, r64 = refs(c, mode)
    dev = sc.deviation(r32, r64)
    print('deviation', sc.case_id(c), mode, dev, 'knife-edge rays', int(sc.knife_edge_rays(r64).sum()))
    for k in ('dstar', 'err0', 'beta'):
        assert dev[k] <= HALF[k], (c, mode, k, dev[k])
    # the fp32 and the float64 reference take the same decisions on the rays that are compared
    keep = ~sc.knife_edge_rays(r64)
    assert torch.equal(r32['err0'][keep] <= sc.EPS, r64['err0'][keep] <= sc.EPS)
    if dev['cdf'] > HALF['cdf']:
        assert mode != 'more', (c, mode, dev['cdf'])         # the error-proportional pdf has no such excuse
    bar = sc.cdf_bar(case, mode, TOL_CDF, r64)
    assert bar <= 1e-4 and bar >= TOL_CDF and (bar == TOL_CDF or bar == 4.0 * dev['cdf']), (c, mode, bar)


@pytest.mark.parametrize('c', sc.CASES, ids=sc.case_id)
def test_every_chunk_is_covered(c, refs):
    case, _, more64 = refs(c, 'more')
    _, _, final64 = refs(c, 'final_eval')
    M = case['M']
    for lo in range(0, M - 1, 64):
        for form, r in (('error', more64), ('final', final64)):
            mass = r['pdf'][:, lo:lo + 64].sum(1).max().item()
            assert mass >= 0.05, (c, lo, form, mass)
        arg = more64['bound0'].argmax(1)
        here = (arg >= lo) & (arg < lo + 64) & (more64['err0'] > 0)
        assert bool(here.any()), (c, lo, arg.tolist())
    assert bool((more64['err0'] <= sc.EPS).any()) and bool((more64['err0'] > sc.EPS).any())
    # the first ray alone decides `more` for the one-ray run
    assert bool(more64['err0'][0] > sc.EPS) and bool(more64['beta'][0] > sc.BETA0)
    # d* branches on both sides of every chunk edge (interval 64 c - 1 | interval 64 c)
    z, d = case['z'].double(), case['sdf'].double()
    a = z[:, 1:] - z[:, :-1]
    b, cc = d[:, :-1].abs(), d[:, 1:].abs()
    first, second = a ** 2 + b ** 2 <= cc ** 2, a ** 2 + cc ** 2 <= b ** 2
    same = d[:, 1:].sign() * d[:, :-1].sign() == 1
    tri = ~first & ~second & (b + cc - a > 0) & same
    for edge in range(64, M - 1, 64):
        for i in (edge - 1, edge):
            assert bool(((first | second) & same)[:, i].any()) and bool(tri[:, i].any()), (c, i)
    if M - 1 > 64:
        assert bool((first & same).any()) and bool((second & same).any())


@pytest.mark.parametrize('c', sc.CASES, ids=sc.case_id)
def test_inputs_are_what_the_docstring_says(c, refs):
    case = refs(c, 'more')[0]
    M, z, sdf = case['M'], case['z'], case['sdf']
    assert z.shape == sdf.shape == (len(case['kinds']), M) and M == case['n_eval'] * (case['r'] + 1)
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and float(z.min()) >= 0 and float(z.max()) < sc.FAR
    assert 1 <= case['n_final'] <= case['n_eval']
    ks = [k[1] for k in case['kinds'] if k[0] == 'cross']
    want = {k for lo in range(0, M, 64) for k in (lo, lo + 1, lo + 62, lo + 63) if k < M - 1} | {M - 2}
    assert set(ks) == want
    for ray, kind in enumerate(case['kinds']):
        if kind[0] == 'cross':
            assert bool((sdf[ray, :kind[1]] > 0).all()) and bool((sdf[ray, kind[1]:] < 0).all()), (c, kind)
        if kind[0] in ('free', 'saturated'):
            assert bool((sdf[ray] > 0).all())
        if kind[0] == 'zero':
            assert float(sdf[ray, kind[1]]) == 0.0 and int((sdf[ray] == 0).sum()) == 1
        if kind[0] == 'repeat':
            assert all(float(z[ray, i]) == float(z[ray, kind[1]]) for i in kind[2:])
        else:
            assert bool((z[ray, 1:] > z[ray, :-1]).all())
    # slopes well below 1, the free space within 10 beta0 of the surface or far past saturation
    cross = [i for i, k in enumerate(case['kinds']) if k[0] in ('cross', 'free')]
    s = sdf[cross]
    assert float(s.max()) <= 10 * sc.BETA0 + 1e-7
    assert float(sdf[[i for i, k in enumerate(case['kinds']) if k[0] == 'saturated']].min()) >= 60 * sc.BETA0
    if M >= 65:
        assert {k[0] for k in case['kinds']} >= {'zero', 'repeat'}
    assert case['u_final_eval'][0, 0] == 0 and (case['n_final'] == 1 or case['u_final_eval'][0, -1] == 1)
    assert float(case['u_final_train'].min()) >= 0 and float(case['u_final_train'].max()) < 1


@pytest.mark.parametrize('mode', sc.MODES)
@pytest.mark.parametrize('c', sc.CASES, ids=sc.case_id)
def test_knife_edge_rays_are_few(c, mode, refs):
    case, _, r64 = refs(c, mode)
    knife = sc.knife_edge_rays(r64)
    N = knife.numel()
    assert int(knife.sum()) <= N // 16, (c, mode, knife.nonzero().flatten().tolist())
    for ray, kind in enumerate(case['kinds']):
        if kind[0] == 'cross' and kind[1] % 64 in (0, 1, 62, 63):
            assert not bool(knife[ray]), (c, mode, kind)


def test_sizes_modes_and_ray_counts():
    assert [n * (r + 1) for n, K, r in sc.CASES] == [2, 4, 10, 65, 64, 128, 33, 66, 99, 129, 65, 130, 195, 63]
    assert set(sc.N_FINAL) == {(n, r) for n, K, r in sc.CASES} and all(sc.N_FINAL[(n, r)] <= n for n, K, r in sc.CASES)
    assert {1, 65} <= set(sc.N_FINAL.values()) and any(sc.N_FINAL[(n, r)] == n for n, K, r in sc.CASES)
    for n, K, r in sc.CASES:
        assert r + 1 < sc.max_rounds_for(K, r, True) and r + 1 == sc.max_rounds_for(K, r, False)
        assert sc.m_max_for(n, K, r) >= n * (r + 3)
    assert sc.RAY_COUNT_CASE in sc.CASES and all(s in sc.CASES for s in sc.SCATTERED)
    case = sc.edge_case(*sc.RAY_COUNT_CASE)
    assert len(case['kinds']) >= max(sc.RAY_COUNTS)
    for n in sc.RAY_COUNTS:
        cut = sc.take(case, n)
        assert cut['z'].shape[0] == n and cut['u_eval'].shape[0] == n and len(cut['kinds']) == n
        assert cut['beta0'].shape == (1,)
        r64 = sc.reference(cut, 'more', torch.float64)
        assert torch.equal(r64['beta'], sc.reference(case, 'more', torch.float64)['beta'][:n])
    for n, K, r in sc.SCATTERED:
        M = n * (r + 1)
        cols = sc.scatter_columns(n, M, 1)
        assert cols.numel() == n and bool((cols[1:] > cols[:-1]).all()) and int(cols[-1]) == M - 1
        assert M <= 64 or 64 in cols.tolist()
        assert not torch.equal(cols, torch.arange(n))
    assert {66, 130} <= {n * (r + 1) for n, K, r in sc.SCATTERED}


def test_one_round_is_the_oracles_loop_body():
    """sampler_cases.one_round against mo.error_bound_sampler's own trace of its first round, with the case's sdf
    handed over as the sdf function."""
    case = sc.edge_case(33, 3, 0)
    conf = {'ray_sampler': {'eps': sc.EPS, 'N_samples_eval': 33, 'N_samples': 1, 'N_samples_extra': 0,
                            'beta_iters': sc.BETA_ITERS, 'max_total_iters': 3, 'near': 0.0, 'add_tiny': sc.ADD_TINY},
            'scene_bounding_sphere': 1.0}
    # the oracle builds its own uniform z: give it the sdf of its points through a table over the SAME z instead
    z = mo.uniform_z(conf, case['ray_d'].double(), case['ray_o'].double(), 33)[0]
    table = case['sdf'].double()
    trace = {}
    real = mo.get_beta
    mo.get_beta = lambda state, conf: torch.tensor(sc.BETA0, dtype=torch.float64)
    try:
        mo.error_bound_sampler(None, conf, case['ray_d'].double(), case['ray_o'].double(), trace=trace,
                               sdf_fn=lambda p: table.reshape(-1, 1) if p.shape[0] == table.numel() else
                               torch.ones(p.shape[0], 1, dtype=torch.float64))
    finally:
        mo.get_beta = real
    t = trace['per_round'][0]
    mine = sc.one_round(z, table, sc.lemma2_beta(z), torch.tensor([sc.BETA0], dtype=torch.float64), True, 33,
                        case['u_eval'])
    for k in ('dstar', 'beta', 'cdf', 'samples'):
        assert torch.equal(mine[k], t[k]), k


# ---- the finish kernel's contract ----------------------------------------------------------------------------------
def test_finish_restatement_against_sort_on_tie_free_inputs():
    g = torch.Generator().manual_seed(3)
    N, n_eval, K, n_final, n_extra = 5, 16, 3, 7, 6
    final_z = torch.rand(N, n_final, generator=g) + 0.1
    z_dense = torch.sort(torch.rand(N, n_eval * K, generator=g) + 0.1, -1)[0]
    extra = torch.stack([torch.randperm(n_eval * (k + 1), generator=g)[:n_extra] for k in range(K)])
    for ran in (1, 2, 3):
        flags = np.zeros(2 * K, dtype=np.int32)
        flags[1:2 * (ran - 1):2] = 1
        rounds, v, pos, z_out, rmap = sc.finish_restatement(final_z, 0.0, 3.5, z_dense, extra, flags, n_eval, K, n_eik=4 * N)
        assert rounds == ran
        want = torch.cat([final_z, torch.zeros(N, 1), torch.full((N, 1), 3.5), z_dense[:, extra[ran - 1]]], 1)
        assert np.array_equal(v, want.numpy())
        assert np.array_equal(z_out, torch.sort(want, -1)[0].numpy())
        assert np.array_equal(pos, rn.merged_positions(v))
        assert np.array_equal(rmap, rn.row_map(rn.merged_positions(v), n_extra, 4 * N))
        assert sorted(rmap.tolist()) == list(range(N * (n_final + n_extra + 2) + 4 * N))


def test_finish_restatement_ties_nan_and_clamp():
    n_eval, K = 4, 2
    z_dense = np.array([[0.0, 1.0, 2.0, 3.5, 9.0, 9.0, 9.0, 9.0]], dtype=np.float32)
    final_z = np.array([[0.0, np.nan, 2.0]], dtype=np.float32)
    extra = np.array([[1, 1, 7], [0, 0, 0]])                  # one round ran: row 0; column 7 clamps to 3 (= far)
    rounds, v, pos, z_out, rmap = sc.finish_restatement(final_z, 0.0, 3.5, z_dense, extra, np.zeros(4), n_eval, K)
    assert rounds == 1
    assert np.array_equal(v, np.array([[0.0, np.inf, 2.0, 0.0, 3.5, 1.0, 1.0, 3.5]], dtype=np.float32))
    assert pos.tolist() == [[0, 7, 4, 1, 5, 2, 3, 6]]
    assert z_out.tolist() == [[0.0, 0.0, 1.0, 1.0, 2.0, 3.5, 3.5, float('inf')]]
    assert sorted(rmap.tolist()) == list(range(8))
    assert np.array_equal(pos, rn.merged_positions(v))          # a stable sort, ties included
