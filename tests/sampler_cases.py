"""Inputs and references for the sampler's edge tests, in plain CPU torch (tests/test_sampler_cases_cpu.py proves the
cases fair, tests/test_gpu_sampler_edges.py runs them through the kernels of csrc/sampler.hip).

Why constructed cases: the kernels walk a ray's M samples in 64-lane chunks and carry every cumulative sum from lane 63
into the next chunk.  With a free random sdf the mass of either pdf and the argmax of the error bound sit in the first
chunk, and a wrong carry disappears under a maximum.  Here every ray is ONE round with constructed inputs (no earlier
round hides or amplifies anything): sorted random z in [0, 3.5), and one ray per crossing index k -- the first and last
lane of every 64-interval chunk and their neighbours -- whose sdf is positive before sample k and negative from k on,
with a slope of 0.15 ... 0.3, so that d* is loose, the bound at beta0 exceeds eps and the bisection really runs.  The free
space is capped at 0.06 ... 0.1 = at most 10 beta0: 0.5 + 0.5 expm1(-s/beta) loses its digits for s/beta of 15 to 50
(tests/composite_cases.py) and the transmittance sums that loss, which this cap keeps out of the final-round cdf.  One
ray never crosses, one is far past saturation everywhere (sdf about 1 = 100 beta0: inside the bound at beta0, the
iters = 0 branch).  Cases with M >= 66 add four variant rays: sdf == 0.0 exactly at sample 63 and at sample 64 (a chunk's
last and first lane), z repeated inside a chunk (30 = 31) and across the chunk edge (63 = 64 = 65); M = 65 has 63 = 64.

Sizes: M = n_eval * (round + 1) for the (n_eval, K, rounds) of SIZES.  `more` is selected the way the kernel selects it:
round_idx + 1 < max_rounds and a batch maximum of beta above beta0 (max_rounds_for).

One more ray kind, 'late', exists for the chunks that are one or two intervals long (M = 66, 130, 195): LATE_FREE below.

Measured on the CPU (tests/test_sampler_cases_cpu.py prints them with -s): fp32 reference against float64 reference,
maxima over all 14 cases x 3 modes, next to half of the bar of tests/test_gpu_sampler.py each is held to:
    d*                          1.4e-7   (1e-6 absolute)
    bound at beta0              4.0e-6   (1e-5 relative)
    beta                        1.7e-7   (5e-7 relative)
    cdf, error-proportional     4.1e-7   (1e-6 absolute)
    cdf, final round            3.3e-7   (1e-6 absolute)
Rays left out as knife edges: none in any case.  The final-round cdf needs the run-time bar of cdf_bar in no case: the
capped free space keeps s/beta below 2 at the betas the bisection ends at (0.05 ... 3).
"""
import numpy as np
import torch

from oracle import monosdf_oracle as mo

BETA0, EPS, BETA_ITERS, ADD_TINY = 0.01, 0.1, 10, 1e-6
FAR = 3.5
SATURATED = 1.0              # sdf of the free space far past saturation: 100 beta0 and rising with z at slope 0.5
# The 'late' ray (crossing at M - 2) is free of density and of error until LATE_WINDOW samples before its crossing, so that
# the last interval holds mass even where it is a chunk of its own (M = 66, 130).  Its beta ends at 0.15 ... 0.3: at
# sdf = 1 the bound's exp(E) - 1 would be 1e-4 per interval there, formed in fp32 from exp(E) = 1.0001 with 6e-4 of it
# lost, and the sum of a hundred of them under a pdf mass of 0.3 moves the fp32 REFERENCE's cdf by 6e-6.  At 8 it is 0.
LATE_FREE, LATE_WINDOW = 8.0, 1
# (n_eval, K, rounds tested): M = n_eval (round + 1)
SIZES = ((2, 5, (0, 1, 4)), (13, 5, (4,)), (32, 4, (1, 3)), (33, 3, (0, 1, 2)), (43, 3, (2,)), (65, 3, (0, 1, 2)),
         (63, 2, (0,)))
CASES = tuple((n, K, r) for n, K, rs in SIZES for r in rs)
# samples of the final round per case: 1, n_eval and 65 among them
N_FINAL = {(2, 0): 1, (2, 1): 2, (2, 4): 2, (13, 4): 7, (32, 1): 32, (32, 3): 16, (33, 0): 1, (33, 1): 33, (33, 2): 17,
           (43, 2): 21, (65, 0): 65, (65, 1): 64, (65, 2): 33, (63, 0): 63}
MODES = ('more', 'final_eval', 'final_train')
# the case the ray counts around the four-ray workgroup are cut from, and the counts
RAY_COUNT_CASE, RAY_COUNTS = (13, 5, 4), (1, 3, 4, 5)
# cases whose "new" columns are scattered over the row instead of standing first (M = 66 and M = 130 among them)
SCATTERED = ((33, 3, 1), (65, 3, 1), (43, 3, 2))
KNIFE = 1e-4                 # |err - eps| <= KNIFE eps in float64: the decision may flip inside the err0 bar


def case_id(c):
    return 'n%d_K%d_r%d' % c


# seed offsets of the cases whose first seed left a ray on a knife edge (test_knife_edge_rays_are_few)
RESEED = {(33, 1): 1}


def case_seed(n_eval, K, r):
    return 7000 + 100 * n_eval + r + 10000 * RESEED.get((n_eval, r), 0)


def max_rounds_for(K, r, more):
    """The max_rounds that makes round r decide `more`: the last round never asks for another one, an earlier one does
    as soon as one ray's beta stays above beta0.  (The configurations' K where it already says so.)"""
    return max(K, r + 2) if more else r + 1


def m_max_for(n_eval, K, r):
    """Row pitch of z / sdf: one n_eval more than the merged row needs, so that there are columns nobody may touch."""
    return n_eval * (max(K, r + 2) + 1)


def crossing_indices(M):
    """First and last lane of every 64-interval chunk and their neighbours, below M - 1; and M - 2."""
    ks = []
    for lo in range(0, M, 64):
        ks += [lo, lo + 1, lo + 62, lo + 63]
    return sorted({k for k in ks if k < M - 1} | {M - 2})


def lemma2_beta(z, eps=EPS):
    """The Lemma-2 bound the first round starts from (ray_sampler.py:118-120), in z's dtype."""
    d = z[:, 1:] - z[:, :-1]
    lemma = 1.0 / (4.0 * torch.log(torch.tensor(eps + 1.0, dtype=z.dtype)))
    return torch.sqrt(lemma * (d ** 2.).sum(-1))


def edge_case(n_eval, K, r, seed=None):
    """fp32 inputs of one round: rays = one per crossing index, the never-crossing ray, the saturated ray, then the
    late ray (M >= 8), then the variant rays.  'kinds' names each ray: ('cross', k), ('free',), ('saturated',),
    ('late', k), ('zero', i), ('repeat', i, ...)."""
    M = n_eval * (r + 1)
    g = torch.Generator().manual_seed(case_seed(n_eval, K, r) if seed is None else seed)
    ks = crossing_indices(M)
    kinds = [('cross', k) for k in ks] + [('free',), ('saturated',)]
    if M >= 8:
        kinds.append(('late', M - 2))
    variants = []
    if M >= 66:
        variants = [('zero', 63), ('zero', 64), ('repeat', 30, 31), ('repeat', 63, 64, 65)]
    elif M == 65:
        variants = [('zero', 63), ('zero', 64), ('repeat', 30, 31), ('repeat', 63, 64)]
    N = len(kinds) + len(variants)
    z = torch.sort(torch.rand(N, M, generator=g) * FAR, -1)[0]
    slope = 0.15 + 0.15 * torch.rand(N, 1, generator=g)
    frac = 0.1 + 0.3 * torch.rand(N, generator=g)
    cap = 0.08 * (1.0 + 0.25 * (2.0 * torch.rand(N, M, generator=g) - 1.0))
    # the variant rays are crossing rays too: the crossing next to the edited samples
    for v in variants:
        if v[0] == 'repeat':
            for i in v[2:]:
                z[len(kinds), i] = z[len(kinds), v[1]]
        kinds.append(v)
    sdf = torch.empty(N, M)
    for ray, kind in enumerate(kinds):
        if kind[0] == 'free':
            sdf[ray] = cap[ray]
            continue
        if kind[0] == 'saturated':
            sdf[ray] = SATURATED + 0.5 * z[ray]
            continue
        k = {'cross': kind[1], 'late': kind[1], 'zero': 64 if M > 65 else 63, 'repeat': min(kind[-1] + 1, M - 2)}[kind[0]]
        zc = z[ray, k] - frac[ray] * (z[ray, k] - z[ray, k - 1]) if k > 0 else z[ray, 0] - 0.01
        lin = slope[ray] * (zc - z[ray])
        sdf[ray] = torch.where(lin > 0, torch.minimum(lin, cap[ray]), torch.maximum(lin, -cap[ray]))
        sdf[ray, :k] = sdf[ray, :k].abs().clamp(min=1e-4)
        sdf[ray, k:] = -sdf[ray, k:].abs().clamp(min=1e-4)
        if kind[0] == 'zero':
            sdf[ray, kind[1]] = 0.0
        if kind[0] == 'late':
            sdf[ray, :k - LATE_WINDOW] = LATE_FREE + 0.5 * z[ray, :k - LATE_WINDOW]
    n_final = N_FINAL.get((n_eval, r), n_eval)
    return {'n_eval': n_eval, 'K': K, 'r': r, 'M': M, 'n_final': n_final, 'kinds': kinds, 'z': z, 'sdf': sdf,
            'beta_in': lemma2_beta(z), 'beta0': torch.tensor([BETA0], dtype=torch.float32),
            'u_eval': torch.linspace(0., 1., n_eval).repeat(N, 1),
            'u_final_eval': torch.linspace(0., 1., n_final).repeat(N, 1),
            'u_final_train': torch.rand(N, n_final, generator=g),
            'ray_o': torch.randn(N, 3, generator=g) * 0.3,
            'ray_d': torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)}


def take(case, n):
    """The first n rays of a case."""
    out = {k: (v[:n] if torch.is_tensor(v) and v.dim() >= 1 and k != 'beta0' else v) for k, v in case.items()}
    out['kinds'] = case['kinds'][:n]
    return out


def mode_inputs(case, mode):
    """(more, n_new, u, training) of a run."""
    if mode == 'more':
        return True, case['n_eval'], case['u_eval'], False
    if mode == 'final_eval':
        return False, case['n_final'], case['u_final_eval'], False
    return False, case['n_final'], case['u_final_train'], True


def one_round(z, sdf, beta_in, beta0, more, n_new, u, eps=EPS, beta_iters=BETA_ITERS, add_tiny=ADD_TINY):
    """One round of mo.error_bound_sampler (its loop body, from the oracle's own pieces) in the dtype of z: d*, the
    bound at beta0, the bisection, the pdf of either form, the cdf and the inverse-CDF samples.  'errs' [iters, N] is
    the bound at every bisection step, 'bound0' [N, M - 1] the bound at beta0 before its maximum."""
    dt = z.dtype
    n_rays = z.shape[0]
    assert u.shape == (n_rays, n_new)
    sdf, beta_in, beta0, u = sdf.to(dt), beta_in.to(dt), beta0.to(dt).reshape(()), u.to(dt)
    d_star, dists = mo._d_star(z, sdf)
    err0 = mo.error_bound(beta0, sdf, dists, d_star)
    beta = torch.where(err0 <= eps, beta0.expand_as(beta_in), beta_in)
    lo, hi = beta0.expand(n_rays).clone(), beta.clone()
    errs = []
    for _ in range(beta_iters):
        mid = (lo + hi) / 2.
        err = mo.error_bound(mid.unsqueeze(-1), sdf, dists, d_star)
        errs.append(err)
        hi = torch.where(err <= eps, mid, hi)
        lo = torch.where(err > eps, mid, lo)
    beta = hi
    dens = mo.laplace_density(sdf, beta.unsqueeze(-1))
    weights, trans, _ = mo.transmittance_weights(z, dens)
    if more:
        b = beta.unsqueeze(-1)
        per_section = torch.exp(-d_star / b) * (dists ** 2.) / (4 * b ** 2)
        pdf = (torch.clamp(torch.exp(torch.cumsum(per_section, dim=-1)), max=1.e6) - 1.0) * trans[:, :-1] + add_tiny
    else:
        pdf = weights[..., :-1] + 1e-5
    pdf = pdf / torch.sum(pdf, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    samples = mo._inverse_cdf(cdf, z, u)
    return {'dstar': d_star, 'err0': err0, 'beta': beta, 'pdf': pdf, 'cdf': cdf, 'samples': samples, 'u': u,
            'errs': torch.stack(errs) if errs else torch.zeros(0, n_rays, dtype=dt), 'bound0': bound_curve(
                beta0, sdf, dists, d_star)}


def bound_curve(beta, sdf, dists, d_star):
    """mo.error_bound before its maximum: the bound after every interval, [N, M - 1]."""
    dens = mo.laplace_density(sdf, beta)
    shifted = torch.cat([torch.zeros_like(dists[:, :1]), dists * dens[:, :-1]], dim=-1)
    integral = torch.cumsum(shifted, dim=-1)
    err_int = torch.cumsum(torch.exp(-d_star / beta) * (dists ** 2.) / (4 * beta ** 2), dim=-1)
    return (torch.clamp(torch.exp(err_int), max=1.e6) - 1.0) * torch.exp(-integral[:, :-1])


def reference(case, mode, dtype):
    more, n_new, u, _ = mode_inputs(case, mode)
    return one_round(case['z'].to(dtype), case['sdf'], case['beta_in'], case['beta0'], more, n_new, u)


def knife_edge_rays(ref64, eps=EPS, margin=KNIFE):
    """[N] bool: in float64 the err0 test or some bisection step the ray really takes decides within margin * eps."""
    near = (ref64['err0'] - eps).abs() <= margin * eps
    bisected = ref64['err0'] > eps
    if ref64['errs'].numel():
        near = near | (bisected & ((ref64['errs'] - eps).abs() <= margin * eps).any(0))
    return near


def deviation(r32, r64):
    """fp32 reference against float64 reference in the measures of tests/test_gpu_sampler.py; beta, cdf on the rays
    that are no knife edge."""
    keep = ~knife_edge_rays(r64)
    d = {'dstar': (r32['dstar'].double() - r64['dstar']).abs().max().item(),
         'err0': ((r32['err0'].double() - r64['err0']).abs() / r64['err0'].abs().clamp(min=1e-3)).max().item(),
         'beta': 0.0, 'cdf': 0.0}
    if bool(keep.any()):
        d['beta'] = ((r32['beta'].double() - r64['beta']).abs() / r64['beta'])[keep].max().item()
        d['cdf'] = (r32['cdf'].double() - r64['cdf']).abs()[keep].max().item()
    return d


def cdf_bar(case, mode, tol_cdf, r64=None):
    """The bar of the cdf comparison: the project's constant, or -- where the reference's own fp32 arithmetic is
    further than a quarter of it from float64 -- four times that deviation (the kernel sums as long a chain in another
    order).  tests/test_sampler_cases_cpu.py holds it below 1e-4: a wrong carry moves the cdf by a chunk's mass, 0.05."""
    r64 = reference(case, mode, torch.float64) if r64 is None else r64
    return max(tol_cdf, 4.0 * deviation(reference(case, mode, torch.float32), r64)['cdf'])


def scatter_columns(n_eval, M, seed):
    """Sorted positions of the n_eval "new" columns of a round's row: scattered, with the last column and the first
    column of the second chunk (when there is one) among them."""
    if M == n_eval:
        return torch.arange(n_eval)
    must = {M - 1} | ({64} if M > 64 else set())
    g = torch.Generator().manual_seed(seed)
    rest = [int(i) for i in torch.randperm(M, generator=g) if int(i) not in must][:n_eval - len(must)]
    return torch.tensor(sorted(must | set(rest)))


# ---- msdf_sampler_error_bound and msdf_sampler_init alone -------------------------------------------------------------
ERROR_BOUND_M = (2, 3, 64, 65, 66, 129)
INIT_N_EVAL = (2, 3, 63, 64, 65, 130)
INIT_BOUND, INIT_NEAR = 1.0, 0.05


def error_bound_case(M):
    """The rays of edge_case at M samples in one round, with d* in fp32 as the operator's third input."""
    case = edge_case(M, 1, 0, seed=8000 + M)
    case['dstar'] = mo._d_star(case['z'].double(), case['sdf'].double())[0].float()
    return case


def init_rays():
    """(origins, directions, kind) for the cube [-1, 1]^3: rays along every axis from inside and from outside, general
    rays from inside, rays that graze the cube (a chord of about 0.01 across an edge or a corner, the decision 1e-3
    clear of the edge) and rays that miss it by as little.  Hits end before z = 2.3."""
    o, d, kind = [], [], []
    for ax in range(3):
        for sgn in (1.0, -1.0):
            e = [0.0, 0.0, 0.0]
            e[ax] = sgn
            o.append([0.3, -0.2, 0.1]); d.append(e); kind.append('axis')
            far_side = [0.25, -0.4, 0.35]
            far_side[ax] = -1.2 * sgn
            o.append(far_side); d.append(e); kind.append('axis')
    g = torch.Generator().manual_seed(11)
    for _ in range(4):
        o.append((torch.rand(3, generator=g) - 0.5).tolist()); d.append(torch.randn(3, generator=g).tolist())
        kind.append('hit')
    # across the edge x = -1, y = 1: through (-1 + t, 1 - t) with direction (1, 1, 0) / sqrt(2)
    for t, k in ((5e-3, 'graze'), (-5e-3, 'miss')):
        o.append([-1.5 + t, 0.5 - t, 0.2]); d.append([1.0, 1.0, 0.0]); kind.append(k)
    # across the corner (1, 1, 1)
    for t, k in ((5e-3, 'graze'), (-5e-3, 'miss')):
        o.append([1.0 - t + 0.5, 1.0 - t + 0.5, 1.0 - t - 1.0]); d.append([-1.0, -1.0, 2.0]); kind.append(k)
    o.append([1.6, 1.7, -1.3]); d.append([0.2, 1.0, 0.1]); kind.append('miss')
    o, d = torch.tensor(o), torch.nn.functional.normalize(torch.tensor(d), dim=-1)
    return o.float().contiguous(), d.float().contiguous(), kind


def uniform_reference(o, d, n, bound, near, far_clip, jitter=None):
    """float64 mo.uniform_z for bound > 0 (far_clip = mo.sampler_far); for bound <= 0 the same samples between near
    and the constant far_clip.  Returns z [N, n], far [N, 1]."""
    o, d = o.double(), d.double()
    jit = None if jitter is None else jitter.double()
    if bound > 0:
        conf = {'ray_sampler': {'near': near}, 'scene_bounding_sphere': bound}
        assert mo.sampler_far(conf) == far_clip
        z, _, far = mo.uniform_z(conf, d, o, n, jit)
        return z, far
    far = torch.full((o.shape[0], 1), far_clip, dtype=torch.float64)
    t = torch.linspace(0., 1., steps=n, dtype=torch.float64)
    z = near * (1. - t) + far * t
    if jit is not None:
        mids = .5 * (z[..., 1:] + z[..., :-1])
        upper, lower = torch.cat([mids, z[..., -1:]], -1), torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * jit
    return z, far


# ---- msdf_sampler_finish -----------------------------------------------------------------------------------------
def finish_restatement(final_z, near, far, z_dense, extra_idx, flags, n_eval, max_rounds, n_eik=0):
    """The finish kernel's contract in numpy.  final_z [N, n_final], z_dense [N, m_max], extra_idx [K, n_extra] int64,
    flags [2 K] (odd entries: the round asked for another one).  Candidates of a ray: its final samples, near, far, then
    the dense-set columns of row rounds - 1 of extra_idx, clamped to rounds * n_eval - 1; NaN counts as +inf; the rank
    of a candidate is the number of candidates before it by (value, candidate index).
    Returns rounds, v (candidates), pos (ranks), z_out, row_map."""
    from reuse_numpy import row_map
    final_z, z_dense = np.asarray(final_z, dtype=np.float32), np.asarray(z_dense, dtype=np.float32)
    extra_idx, flags = np.asarray(extra_idx, dtype=np.int64).reshape(max_rounds, -1), np.asarray(flags)
    N = final_z.shape[0]
    rounds = 1
    while rounds < max_rounds and flags[2 * (rounds - 1) + 1] != 0:
        rounds += 1
    cols = np.minimum(extra_idx[rounds - 1], rounds * n_eval - 1)
    v = np.concatenate([final_z, np.full((N, 1), near, np.float32), np.full((N, 1), far, np.float32),
                        z_dense[:, cols]], 1)
    v = np.where(np.isnan(v), np.float32(np.inf), v)
    S = v.shape[1]
    idx = np.arange(S)
    before = (v[:, None, :] < v[:, :, None]) | ((v[:, None, :] == v[:, :, None]) & (idx[None, None, :] < idx[None, :, None]))
    pos = before.sum(-1)                                  # pos[ray, j] = candidates k that stand before candidate j
    z_out = np.empty_like(v)
    np.put_along_axis(z_out, pos, v, axis=1)
    return rounds, v, pos, z_out, row_map(pos, extra_idx.shape[1], n_eik)


# (n_final, n_extra, n_eval, K, rays, rounds that ran): S = n_final + n_extra + 2 = 3, 64, 65, 98, 129
FINISH_CASES = ((1, 0, 2, 2, 1, 1), (30, 32, 16, 3, 3, 2), (31, 32, 16, 3, 4, 3), (64, 32, 40, 2, 5, 1),
                (65, 62, 70, 2, 5, 2), (30, 32, 16, 3, 5, 1))
FINISH_NEAR, FINISH_FAR = 0.05, 3.5


def finish_case(n_final, n_extra, n_eval, K, N, ran, nan=False, seed=0):
    """Inputs of msdf_sampler_finish alone.  Ties: final sample 0 of ray 0 equals near; extra columns 0 and 1 name the
    same dense column; the dense column extra column 2 names holds far on every ray; and (ran < K) the last extra column
    names column m_max - 1, beyond the rounds * n_eval columns that exist: it clamps.  Every row of extra_idx differs.
    nan: final sample 2 of the last ray is NaN."""
    g = torch.Generator().manual_seed(100 * (n_final + n_extra + 2) + seed)
    m_max = n_eval * K
    z_dense = torch.sort(torch.rand(N, m_max, generator=g) * (FINISH_FAR - FINISH_NEAR) + FINISH_NEAR, -1)[0]
    final_z = torch.sort(torch.rand(N, n_final, generator=g) * (FINISH_FAR - FINISH_NEAR) + FINISH_NEAR, -1)[0]
    final_z[0, 0] = FINISH_NEAR
    extra = torch.stack([torch.randint(n_eval * (k + 1), (n_extra,), generator=g).sort()[0] for k in range(K)]) \
        if n_extra else torch.zeros(K, 0, dtype=torch.int64)
    if n_extra >= 4:
        extra[:, 1] = extra[:, 0]
        for k in range(K):
            z_dense[:, extra[k, 2]] = FINISH_FAR
        if ran < K:
            extra[ran - 1, -1] = m_max - 1
    if nan:
        final_z[-1, min(2, n_final - 1)] = float('nan')
    flags = torch.zeros(2 * K, dtype=torch.int32)
    flags[0::2] = 0x3c23d70a                                  # the bits of a beta, as the round kernels leave them
    for k in range(ran - 1):
        flags[2 * k + 1] = 1
    S = n_final + n_extra + 2
    return {'n_final': n_final, 'n_extra': n_extra, 'n_eval': n_eval, 'K': K, 'N': N, 'ran': ran, 'S': S, 'm_max': m_max,
            'z_dense': z_dense, 'final_z': final_z, 'extra_idx': extra.contiguous(), 'flags': flags,
            'ray_o': torch.randn(N, 3, generator=g) * 0.3,
            'ray_d': torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1),
            'eik_idx': torch.randint(S, (N,), generator=g), 'eik_u': torch.cat([torch.tensor([0.0, 0.9999999])[:N],
                                                                                 torch.rand(max(N - 2, 0), generator=g)]),
            'eik_uniform': torch.rand(N, 3, generator=g), 'nei_rand': torch.rand(2 * N, 3, generator=g)}
