"""The sampler kernels (csrc/sampler.hip) at sizes off the 64-lane grid, each kernel on its own through raw ctypes, against
the float64 references of tests/sampler_cases.py (why the cases are constructed, and why they are fair: that module and
tests/test_sampler_cases_cpu.py).

  round kernels   msdf_sampler_beta + msdf_sampler_resample on ONE constructed round per case: M = 2 ... 195 (partial
                  chunks, a carry out of a partial chunk, less than a wave), a crossing on every chunk edge, the "new" sdf
                  values scattered into the row, `more` and the final round in eval and in training mode;
  ties            a u that equals a cdf entry exactly, next to a bin too flat to interpolate (searchsorted right=True);
  error bound     msdf_sampler_error_bound alone, one beta and one beta per ray;
  init            msdf_sampler_init alone: samples, jitter, the cube test, Lemma-2 beta;
  finish          msdf_sampler_finish alone against the numpy restatement of its contract: ties, NaN, the extra_idx row,
                  the index clamp, the eikonal block;
  LDS limit       a size beyond 160 KiB is refused and nothing is launched.

Every measured maximum goes to the parity table as 'sampler_edges'.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_cases as sc
from test_gpu_sampler import TOL_BETA, TOL_CDF, TOL_DSTAR, TOL_ERR0, TOL_SAMPLES, _cdf_residual

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
F64 = torch.float64


@pytest.fixture(scope='module')
def cases():
    memo = {}

    def get(c):
        if c not in memo:
            memo[c] = sc.edge_case(*c)
        return memo[c]
    return get


def _round_args(case, mode, columns):
    """SamplerArgs of one round and the tensors behind it.  The row of sdf holds SENTINEL at the "new" columns: their
    values arrive through new_sdf / new_pos, as from the SDF kernel."""
    from monosdf_amd import _lib
    more, n_new, u, training = sc.mode_inputs(case, mode)
    n_eval, K, r, M, n_final = case['n_eval'], case['K'], case['r'], case['M'], case['n_final']
    N = case['z'].shape[0]
    max_rounds, m_max = sc.max_rounds_for(K, r, more), sc.m_max_for(n_eval, K, r)
    dev = 'cuda'
    t = {k: torch.full(shape, SENTINEL, device=dev) for k, shape in dict(
        z=(N, m_max), sdf=(N, m_max), new_z=(N, n_eval), pts=(N * n_eval, 3), final_z=(N, n_final),
        dbg_dstar=(N, m_max), dbg_cdf=(N, m_max), dbg_err0=(N,)).items()}
    t['z'][:, :M], t['sdf'][:, :M] = case['z'].cuda(), case['sdf'].cuda()
    t['sdf'][:, columns.cuda()] = SENTINEL
    t['new_sdf'] = case['sdf'][:, columns].cuda().contiguous()
    t['new_pos'] = columns.to(torch.int32).repeat(N, 1).cuda().contiguous()
    t['beta'] = case['beta_in'].clone().cuda()
    t['beta0'] = case['beta0'].cuda()
    t['flags'] = torch.zeros(2 * max_rounds, device=dev, dtype=torch.int32)
    if r > 0:
        t['flags'][2 * (r - 1) + 1] = 1
    t['ray_o'], t['ray_d'] = case['ray_o'].cuda().contiguous(), case['ray_d'].cuda().contiguous()
    t['u_final'] = case['u_final_train'].cuda().contiguous() if training else None
    a = _lib.SamplerArgs()
    a.ray_o, a.ray_d, a.N, a.M, a.m_max = t['ray_o'].data_ptr(), t['ray_d'].data_ptr(), N, M, m_max
    a.n_eval, a.n_final, a.n_extra = n_eval, n_final, 0
    a.round_idx, a.max_rounds, a.training, a.beta_iters = r, max_rounds, int(training), sc.BETA_ITERS
    a.near, a.far, a.bound, a.eps, a.add_tiny = 0.0, sc.FAR, 1.0, sc.EPS, sc.ADD_TINY
    a.lemma = float(1.0 / (4.0 * torch.log(torch.tensor(sc.EPS + 1.0))))
    for k in ('beta0', 'z', 'sdf', 'new_z', 'new_sdf', 'new_pos', 'pts', 'beta', 'flags', 'final_z', 'dbg_dstar',
              'dbg_err0', 'dbg_cdf'):
        setattr(a, k, t[k].data_ptr())
    a.u_final = t['u_final'].data_ptr() if training else None
    return a, t


def _check_round(errlog, name, case, mode, columns):
    from monosdf_amd import _lib
    more, n_new, u, training = sc.mode_inputs(case, mode)
    n_eval, r, M, N = case['n_eval'], case['r'], case['M'], case['z'].shape[0]
    ref = sc.reference(case, mode, F64)
    keep = ~sc.knife_edge_rays(ref)
    bar_cdf = sc.cdf_bar(case, mode, TOL_CDF, ref)
    a, t = _round_args(case, mode, columns)
    st = _lib.stream_ptr()
    _lib.call('msdf_sampler_beta', C.byref(a), st)
    _lib.call('msdf_sampler_resample', C.byref(a), st)
    torch.cuda.synchronize()
    g = {k: v.cpu() for k, v in t.items() if v is not None}
    log = lambda key, err, tol: errlog('sampler_edges', name, mode + '.' + key, err, tol)

    # the scatter put every new sdf value into its column, and wrote the row back
    sdf_row = g['sdf'][:, :M + n_eval] if more else g['sdf'][:, :M]
    e = log('dstar', (g['dbg_dstar'][:, :M - 1].double() - ref['dstar']).abs().max(), TOL_DSTAR)
    assert e <= TOL_DSTAR, (name, mode, 'dstar', e)
    e = log('err0', ((g['dbg_err0'].double() - ref['err0']).abs() / ref['err0'].abs().clamp(min=1e-3)).max(), TOL_ERR0)
    assert e <= TOL_ERR0, (name, mode, 'err0', e)
    e = log('beta', ((g['beta'].double() - ref['beta']).abs() / ref['beta'])[keep].max(), TOL_BETA)
    assert e <= TOL_BETA, (name, mode, 'beta', e)
    # the batch-global decision
    assert np.float32(g['flags'][2 * r].numpy().view(np.float32)) == np.float32(g['beta'].max().item())
    assert int(g['flags'][2 * r + 1]) == int(more), (name, mode)
    assert int(g['flags'].ne(0).sum()) == 1 + int(more) + int(r > 0)
    e = log('cdf', (g['dbg_cdf'][:, :M].double() - ref['cdf']).abs()[keep].max(), bar_cdf)
    assert e <= bar_cdf, (name, mode, 'cdf', e)
    assert bool((g['dbg_cdf'][:, 0] == 0).all())
    got = g['new_z'] if more else g['final_z']
    assert got.shape == ref['samples'].shape
    assert bool((got >= case['z'][:, :1]).all()) and bool((got <= case['z'][:, -1:]).all())
    in_z = (got.double() - ref['samples']).abs()
    in_cdf = _cdf_residual(ref['cdf'], case['z'].double(), got.double(), ref['u'])
    e = log('samples (z or cdf space)', torch.minimum(in_z, in_cdf)[keep].max(), TOL_SAMPLES)
    assert e <= TOL_SAMPLES, (name, mode, 'samples', e)
    log('samples (z space, not asserted)', in_z[keep].max(), float('inf'))
    # columns nobody may touch
    for k in ('z', 'sdf', 'dbg_cdf'):
        assert bool((g[k][:, M + (n_eval if more and k != 'dbg_cdf' else 0):] == SENTINEL).all()), (name, mode, k)
    assert bool((g['dbg_dstar'][:, M - 1:] == SENTINEL).all())
    if not more:
        assert torch.equal(g['z'][:, :M], case['z']) and torch.equal(g['sdf'][:, :M], case['sdf'])
        assert bool((g['new_z'] == SENTINEL).all()) and bool((g['pts'] == SENTINEL).all())
        assert torch.equal(g['new_pos'], columns.to(torch.int32).repeat(N, 1))
        return
    assert bool((g['final_z'] == SENTINEL).all())
    # the merged row is exactly the sorted union, every new sample where new_pos says, its point on the ray
    both, _ = torch.sort(torch.cat([case['z'], got], 1), 1)
    assert torch.equal(g['z'][:, :M + n_eval], both), (name, mode)
    pos = g['new_pos'].long()
    assert torch.equal(torch.gather(g['z'], 1, pos), got)
    assert bool((pos[:, 1:] != pos[:, :-1]).all()) if n_eval > 1 else True
    want = case['ray_o'].unsqueeze(1) + got.unsqueeze(2) * case['ray_d'].unsqueeze(1)
    assert torch.allclose(g['pts'].reshape(N, n_eval, 3), want, rtol=0, atol=1e-6)
    # sdf moved with z: old sample i now stands `number of new samples before it` further right
    shift = (got.unsqueeze(1) < case['z'].unsqueeze(2)).sum(-1)
    old_pos = torch.arange(M).unsqueeze(0) + shift
    assert torch.equal(torch.gather(sdf_row, 1, old_pos), case['sdf']), (name, mode)
    assert torch.equal(torch.gather(g['z'], 1, old_pos), case['z'])
    taken = torch.zeros(N, M + n_eval, dtype=torch.int32)
    taken.scatter_add_(1, old_pos, torch.ones_like(old_pos, dtype=torch.int32))
    taken.scatter_add_(1, pos, torch.ones_like(pos, dtype=torch.int32))
    assert bool((taken == 1).all()), (name, mode)


def _columns(c):
    n_eval, K, r = c
    M = n_eval * (r + 1)
    return sc.scatter_columns(n_eval, M, 5) if c in sc.SCATTERED else torch.arange(n_eval)


@pytest.mark.parametrize('mode', sc.MODES)
@pytest.mark.parametrize('c', sc.CASES, ids=sc.case_id)
def test_one_round_at_every_size(c, mode, cases, errlog):
    _check_round(errlog, sc.case_id(c), cases(c), mode, _columns(c))


@pytest.mark.parametrize('mode', ['more', 'final_train'])
@pytest.mark.parametrize('n', sc.RAY_COUNTS)
def test_ray_counts_around_the_four_wave_workgroup(n, mode, cases, errlog):
    case = sc.take(cases(sc.RAY_COUNT_CASE), n)
    assert case['z'].shape == (n, 65)
    _check_round(errlog, '%s_rays%d' % (sc.case_id(sc.RAY_COUNT_CASE), n), case, mode, torch.arange(case['n_eval']))


def test_a_u_on_a_cdf_entry_falls_into_the_bin_that_starts_there(cases):
    """searchsorted(right=True), ray_sampler.py:216: with u equal to cdf[i] the sample is z[i] itself, also where the bin
    before it grew by less than 1e-5 and is therefore not interpolated (there a search that stops one bin early returns
    z[i - 1]; everywhere else the interpolation is continuous and hides it).  The ties are made with the kernel's own
    fp32 cdf: the final round runs twice on the same inputs, the second time with u read from the first one's cdf."""
    from monosdf_amd import _lib
    from oracle import monosdf_oracle as mo
    case = dict(cases((65, 3, 1)))
    M, n_final = case['M'], case['n_final']
    a, t = _round_args(case, 'final_train', torch.arange(case['n_eval']))
    st = _lib.stream_ptr()
    _lib.call('msdf_sampler_beta', C.byref(a), st)
    _lib.call('msdf_sampler_resample', C.byref(a), st)
    torch.cuda.synchronize()
    cdf = t['dbg_cdf'][:, :M].cpu()
    idx = torch.arange(n_final) * 2 + 1                   # 63 and 65 among them; then the ends and 64
    idx[0], idx[-1], idx[33] = 0, M - 1, 64
    case['u_final_train'] = cdf[:, idx].contiguous()
    small = (cdf[:, idx[1:]] - cdf[:, idx[1:] - 1]) < 1e-5
    assert int(small.sum()) >= 8                           # bins that are not interpolated, before a tie
    a, t = _round_args(case, 'final_train', torch.arange(case['n_eval']))
    _lib.call('msdf_sampler_beta', C.byref(a), st)
    _lib.call('msdf_sampler_resample', C.byref(a), st)
    torch.cuda.synchronize()
    assert torch.equal(t['dbg_cdf'][:, :M].cpu(), cdf)
    want = mo._inverse_cdf(cdf, case['z'], case['u_final_train'])
    assert torch.equal(want, case['z'][:, idx])
    assert torch.equal(t['final_z'].cpu(), want)


# ---- msdf_sampler_error_bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', sc.ERROR_BOUND_M)
def test_error_bound_operator(M, errlog):
    from monosdf_amd import _lib
    from oracle import monosdf_oracle as mo
    case = sc.error_bound_case(M)
    N = case['z'].shape[0]
    z, sdf, dstar = case['z'].cuda().contiguous(), case['sdf'].cuda().contiguous(), case['dstar'].cuda().contiguous()
    dists64 = (case['z'][:, 1:] - case['z'][:, :-1]).double()
    per_ray = sc.reference(case, 'more', F64)['beta'].float()           # where the bisection ended: the bound is about eps
    # at beta0 most bounds sit on the 1e6 clamp of exp(E); at 5 beta0 none does, and the sums decide
    for label, beta, stride in (('scalar', case['beta0'], 0), ('scalar_5beta0', 5.0 * case['beta0'], 0),
                                ('per_ray', per_ray, 1)):
        out = torch.full((N + 1,), SENTINEL, device='cuda')
        b = beta.cuda().contiguous()
        _lib.call('msdf_sampler_error_bound', _lib.ptr(z), _lib.ptr(sdf), _lib.ptr(dstar), _lib.ptr(b), stride, N, M,
                  _lib.ptr(out), _lib.stream_ptr())
        torch.cuda.synchronize()
        b64 = beta.double().reshape(-1, 1) if stride else beta.double().reshape(())
        ref = mo.error_bound(b64, case['sdf'].double(), dists64, case['dstar'].double())
        e = errlog('sampler_edges', 'error_bound_M%d' % M, label,
                   ((out[:N].cpu().double() - ref).abs() / ref.abs().clamp(min=1e-3)).max(), TOL_ERR0)
        assert e <= TOL_ERR0, (M, label, e)
        assert float(out[N]) == SENTINEL
        if stride:
            assert bool(((ref - sc.EPS).abs() < 0.05)[ref > 1e-3].any())


# ---- msdf_sampler_init ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bound', [sc.INIT_BOUND, 0.0, -1.0])
@pytest.mark.parametrize('jitter', [False, True])
@pytest.mark.parametrize('n_eval', sc.INIT_N_EVAL)
def test_init_alone(n_eval, jitter, bound, errlog):
    from monosdf_amd import _lib
    o, d, kind = sc.init_rays()
    N = o.shape[0]
    near = sc.INIT_NEAR
    far_clip = 3.5 * bound if bound > 0 else 1.9
    K, m_max = 3, n_eval + 3
    jit = torch.rand(N, n_eval, generator=torch.Generator().manual_seed(n_eval)) if jitter else None
    dev = 'cuda'
    z = torch.full((N, m_max), SENTINEL, device=dev)
    new_z = torch.full((N, n_eval), SENTINEL, device=dev)
    new_pos = torch.full((N, n_eval), -7, device=dev, dtype=torch.int32)
    pts = torch.full((N * n_eval, 3), SENTINEL, device=dev)
    beta, far_out = torch.full((N,), SENTINEL, device=dev), torch.full((N,), SENTINEL, device=dev)
    flags = torch.full((2 * K + 1,), 77, device=dev, dtype=torch.int32)
    h_saved = torch.full((2,), 77, device=dev, dtype=torch.int32)
    o_d, d_d = o.cuda(), d.cuda()
    jit_d = jit.cuda().contiguous() if jitter else None
    lemma = float(1.0 / (4.0 * torch.log(torch.tensor(sc.EPS + 1.0))))
    a = _lib.SamplerArgs()
    a.ray_o, a.ray_d, a.N, a.M, a.m_max = o_d.data_ptr(), d_d.data_ptr(), N, n_eval, m_max
    a.n_eval, a.n_final, a.n_extra, a.max_rounds = n_eval, 1, 0, K
    a.near, a.far, a.bound, a.eps, a.add_tiny, a.lemma = near, far_clip, bound, sc.EPS, sc.ADD_TINY, lemma
    a.z, a.new_z, a.new_pos, a.pts, a.beta = [x.data_ptr() for x in (z, new_z, new_pos, pts, beta)]
    a.flags, a.h_saved, a.far_out = flags.data_ptr(), h_saved.data_ptr(), far_out.data_ptr()
    a.jitter = jit_d.data_ptr() if jitter else None
    _lib.call('msdf_sampler_init', C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    z_ref, far_ref = sc.uniform_reference(o, d, n_eval, bound, near, far_clip, jit)
    # the rays that end at the far clip (those that miss the cube; all of them without a cube) are held to 1e-6 far
    clipped = far_ref[:, 0] == far_clip
    assert bound > 0 or bool(clipped.all())
    if bound > 0:
        assert [k == 'miss' for k in kind] == clipped.tolist()
    bar = torch.where(clipped, 1e-6 * far_clip, 1e-6).double()
    name = 'init_n%d_%s_bound%g' % (n_eval, 'jitter' if jitter else 'even', bound)
    zc = z.cpu()
    rel = lambda err: (err / bar.reshape([-1] + [1] * (err.dim() - 1))).max()
    e = errlog('sampler_edges', name, 'z / bar', rel((zc[:, :n_eval].double() - z_ref).abs()), 1.0)
    assert e <= 1.0, (name, 'z', e)
    assert torch.equal(new_z.cpu(), zc[:, :n_eval]) and bool((zc[:, n_eval:] == SENTINEL).all())
    e = errlog('sampler_edges', name, 'far / bar', rel((far_out.cpu().double() - far_ref[:, 0]).abs()), 1.0)
    assert e <= 1.0, (name, 'far', e)
    want = o.double().unsqueeze(1) + z_ref.unsqueeze(2) * d.double().unsqueeze(1)
    e = errlog('sampler_edges', name, 'pts / bar', rel((pts.cpu().reshape(N, n_eval, 3).double() - want).abs()), 1.0)
    assert e <= 1.0, (name, 'pts', e)
    # Lemma 2 of the samples the kernel wrote
    dz = zc[:, 1:n_eval].double() - zc[:, :n_eval - 1].double()
    beta_ref = torch.sqrt(float(np.float32(lemma)) * (dz ** 2).sum(-1))
    e = errlog('sampler_edges', name, 'beta', ((beta.cpu().double() - beta_ref).abs() / beta_ref).max(), TOL_BETA)
    assert e <= TOL_BETA, (name, 'beta', e)
    assert torch.equal(new_pos.cpu(), torch.arange(n_eval, dtype=torch.int32).repeat(N, 1))
    assert flags.cpu().tolist() == [0] * (2 * K) + [77] and h_saved.cpu().tolist() == [0, 77]


# ---- msdf_sampler_finish ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nan', [False, True])
@pytest.mark.parametrize('fc', sc.FINISH_CASES, ids=lambda fc: 'S%d_N%d_ran%d' % (fc[0] + fc[1] + 2, fc[4], fc[5]))
def test_finish_alone(fc, nan, errlog):
    from monosdf_amd import _lib
    c = sc.finish_case(*fc, nan=nan)
    N, S, K, n_extra, bound = c['N'], c['S'], c['K'], c['n_extra'], 1.1
    rounds, v, pos, z_ref, rmap_ref = sc.finish_restatement(c['final_z'], sc.FINISH_NEAR, sc.FINISH_FAR, c['z_dense'],
                                                            c['extra_idx'], c['flags'], c['n_eval'], K, n_eik=4 * N)
    assert rounds == c['ran'] and sorted(rmap_ref.tolist()) == list(range(N * S + 4 * N))
    assert bool(np.isinf(z_ref).any()) == nan
    dev = 'cuda'
    inp = {k: c[k].cuda().contiguous() for k in ('z_dense', 'final_z', 'extra_idx', 'flags', 'ray_o', 'ray_d', 'eik_idx',
                                                  'eik_u', 'eik_uniform', 'nei_rand')}
    o64, d64 = c['ray_o'].double(), c['ray_d'].double()
    for eik_unit in (0, 1):
        z_out = torch.full((N, S + 1), SENTINEL, device=dev).reshape(-1)[:N * S + 1]
        z_eik = torch.full((N + 1,), SENTINEL, device=dev)
        pts_out = torch.full((N * S + 4 * N + 1, 3), SENTINEL, device=dev)
        row_map = torch.full((N * S + 4 * N + 1,), -1, device=dev, dtype=torch.int32)
        rounds_out = torch.full((2,), -1, device=dev, dtype=torch.int32)
        a = _lib.SamplerArgs()
        a.ray_o, a.ray_d, a.N, a.M, a.m_max = inp['ray_o'].data_ptr(), inp['ray_d'].data_ptr(), N, c['n_eval'], c['m_max']
        a.n_eval, a.n_final, a.n_extra, a.max_rounds = c['n_eval'], c['n_final'], n_extra, K
        a.near, a.far, a.bound = sc.FINISH_NEAR, sc.FINISH_FAR, bound
        a.z, a.flags, a.final_z = inp['z_dense'].data_ptr(), inp['flags'].data_ptr(), inp['final_z'].data_ptr()
        a.extra_idx = inp['extra_idx'].data_ptr() if n_extra else None
        a.z_out, a.z_eik, a.pts_out, a.row_map = z_out.data_ptr(), z_eik.data_ptr(), pts_out.data_ptr(), row_map.data_ptr()
        a.rounds_out, a.eik_uniform, a.nei_rand = rounds_out.data_ptr(), inp['eik_uniform'].data_ptr(), inp['nei_rand'].data_ptr()
        a.eik_unit = eik_unit
        if eik_unit:
            a.eik_idx, a.eik_u = None, inp['eik_u'].data_ptr()
            idx = torch.clamp((c['eik_u'] * np.float32(S)).long(), max=S - 1)
            assert int(idx[0]) == 0 and (N < 2 or int(idx[1]) == S - 1)
        else:
            a.eik_idx, a.eik_u = inp['eik_idx'].data_ptr(), None
            idx = c['eik_idx']
        _lib.call('msdf_sampler_finish', C.byref(a), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rounds_out.cpu().tolist() == [rounds, -1]
        got = z_out.cpu()
        assert np.array_equal(got[:N * S].reshape(N, S).numpy(), z_ref) and float(got[N * S]) == SENTINEL
        assert np.array_equal(row_map.cpu().numpy(), np.concatenate([rmap_ref, [-1]]))
        ze_ref = torch.from_numpy(z_ref)[torch.arange(N), idx]
        assert torch.equal(z_eik.cpu(), torch.cat([ze_ref, torch.tensor([SENTINEL])]))
        p = pts_out.cpu().double()
        assert bool((p[-1] == SENTINEL).all())
        zr = torch.from_numpy(z_ref).double()
        want = o64.unsqueeze(1) + zr.unsqueeze(2) * d64.unsqueeze(1)
        fin = torch.isfinite(zr)
        e = (p[:N * S].reshape(N, S, 3) - want)[fin].abs().max()
        u = c['eik_uniform'].double()
        if eik_unit:
            u = (2.0 * u - 1.0) * float(np.float32(bound))
        od = o64 + ze_ref.double().unsqueeze(1) * d64
        nei = c['nei_rand'].double()
        block = torch.cat([u, od, u + (nei[:N] - 0.5) * float(np.float32(0.01)),
                           od + (nei[N:] - 0.5) * float(np.float32(0.01))])
        ok = torch.isfinite(block)
        e = max(e, (p[N * S:N * S + 4 * N] - block)[ok].abs().max())
        e = errlog('sampler_edges', 'finish_S%d_N%d_ran%d%s' % (S, N, rounds, '_nan' if nan else ''),
                   'pts_out eik_unit=%d' % eik_unit, e, 1e-6)
        assert e <= 1e-6, (fc, nan, eik_unit, e)
        assert bool(ok.all()) or nan


# ---- the LDS limit ----------------------------------------------------------------------------------------------------
def test_rows_beyond_the_lds_limit_are_refused_and_nothing_is_launched():
    """n_eval = 420 with 5 rounds: four waves of 5 (2100 + 1) + 420 floats are 174 800 bytes, more than the 160 KiB of a
    workgroup.  Valid buffers all the same."""
    from monosdf_amd import _lib
    n_eval, K, N = 420, 5, 2
    assert 4 * (5 * (n_eval * K + 1) + n_eval) * 4 == 174800 > 160 * 1024
    g = torch.Generator().manual_seed(1)
    case = {'n_eval': n_eval, 'K': K, 'r': 0, 'M': n_eval, 'n_final': 64,
            'z': torch.sort(torch.rand(N, n_eval, generator=g) * sc.FAR, -1)[0], 'sdf': torch.rand(N, n_eval, generator=g),
            'beta0': torch.tensor([sc.BETA0]), 'u_eval': torch.linspace(0., 1., n_eval).repeat(N, 1), 'u_final_train': torch.rand(N, 64, generator=g),
            'ray_o': torch.zeros(N, 3), 'ray_d': torch.ones(N, 3)}
    case['beta_in'] = sc.lemma2_beta(case['z'])
    a, t = _round_args(case, 'more', torch.arange(n_eval))
    a.m_max = n_eval * K
    for k in ('z', 'sdf', 'dbg_dstar', 'dbg_cdf'):                 # the pitch the refused size asks for
        t[k] = torch.full((N, a.m_max), SENTINEL, device='cuda')
        setattr(a, k, t[k].data_ptr())
    t['flags'].zero_()
    before = {k: v.clone() for k, v in t.items() if v is not None}
    for fn in ('msdf_sampler_beta', 'msdf_sampler_resample'):
        with pytest.raises(RuntimeError, match='unsupported configuration'):
            _lib.call(fn, C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(t[k], v), k
