"""Inputs and references for the compositor's edge tests, in plain CPU torch (tests/test_composite_cases_cpu.py proves
the cases fair, tests/test_gpu_composite_edges.py runs them through the kernels).

Why constructed cases: with free random sdf the weight mass sits in the first 64 samples, and an error of the carry into
a later register chunk disappears under a maximum taken over the whole tensor.  And at a small beta the reference's
formula 0.5 + 0.5 expm1(-s/beta) loses its digits for s > 0, which the 1e10 length of the last interval multiplies
whenever the last sample has s/beta between about 15 and 50: fp32 and float64 then disagree by O(1) about the reference
itself.  The cases here keep beta at 0.07 ... 0.1, every free-space sample within 3 beta of the surface, and put one
surface crossing at every edge of the kernels' 64-sample chunks, so that each chunk carries weight and the fp32 oracle
stays within 1e-5 of the float64 one.
"""
import torch

from oracle import monosdf_oracle as mo

# samples per ray the GPU test runs: the chunk (wave) boundaries of the kernels and one to either side, the headline 98,
# and the three shortest rays
SAMPLES = (1, 2, 3, 63, 64, 65, 98, 128, 129, 192, 193, 255, 256)
BETAS = (0.1, 0.07)
# where a ray's surface crossing is put: first / last lane of every 64-sample chunk and the lanes next to them
CROSSINGS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, 254, 255)
# last sample of the two rays that escape, in units of beta.  Beyond 60 sigma is exactly 0 in fp32 and in float64 (expm1
# has saturated to -1).  Autograd then derives expm1(t) as expm1(t) + 1 = 0, where the derivative is e^t: on a ray that
# escapes with ONE sample, e^-80 meets the 1e10 interval and the 1e8 of depth = wz / (wsum + 1e-8), the true d/d sdf is
# 1e-15, the reference's whole tensor is 0, and rel_err's 1e-12 floor turns a correct kernel's 1e-15 into 1e-3 (measured
# on the GPU at 80: 1.2e-3 and 8.2e-3; the CPU condition below gives the same figures).  At 100 both are below 1e-21
# (tests/test_composite_cases_cpu.py: test_autograd_of_the_oracle_is_the_derivative).
ESCAPE = 100.0
BG = (0.9, 0.8, 0.7)
OUTPUTS = ('rgb_values', 'depth', 'normal_map', 'weights')


# the beta_raw run: 130 rays (msdf_beta_grad then sums more than 64 partials) of 3 samples, beta = |-0.06| + 0.01
BETA_RAW, BETA_MIN = -0.06, 0.01
BETA_RAW_CASE = (3, 0.07, 4242, 130)          # edge_case(S, beta, seed, rays)
# ray counts cut from the S = 65 case: the kernels put four rays into a workgroup
RAY_COUNTS = (1, 3, 4, 5)


def case_seed(S, beta):
    return 1000 * BETAS.index(beta) + S


def chunk_rel_err(a, b, width=64):
    """helpers.rel_err over each block of `width` sample columns (dim 1) on its own, every block normalised by ITS
    reference maximum; the worst block."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and a.dim() >= 2
    worst = 0.0
    for lo in range(0, b.shape[1], width):
        x, y = a[:, lo:lo + width], b[:, lo:lo + width]
        if y.numel():
            worst = max(worst, ((x - y).abs().max() / (y.abs().max() + 1e-12)).item())
    return worst


def crossing_indices(S):
    """One crossing ray per entry: the listed indices below S, then S-2 and S-1."""
    return [k for k in CROSSINGS if k < S] + [k for k in (S - 2, S - 1) if k >= 0]


def edge_case(S, beta, seed, rays=0):
    """fp32 inputs: one ray per crossing index (crossing_indices) and two rays that never cross and escape (last sample
    at +ESCAPE beta: sigma is exactly 0 there, wsum < 1); `rays` > 0 pads with further crossing rays to that many.  No sdf
    sample is exactly 0: with_zero_crossings, and why, below."""
    g = torch.Generator().manual_seed(seed)
    ks = crossing_indices(S)
    base = len(ks)
    while len(ks) + 2 < rays:
        ks.append(ks[len(ks) % base])
    N = len(ks) + 2
    z = torch.sort(torch.rand(N, S, generator=g) * 3.5, -1)[0]
    sdf = beta * (0.5 + 2.5 * torch.rand(N, S, generator=g))              # free space: beta U(0.5, 3)
    inside = -0.3 * beta * (0.2 + torch.rand(N, S, generator=g))          # shallow inside: -0.3 beta U(0.2, 1.2)
    for r, k in enumerate(ks):
        sdf[r, k:] = inside[r, k:]
    sdf[N - 2:, S - 1] = ESCAPE * beta
    rgb = torch.rand(N, S, 3, generator=g)
    nrm = torch.randn(N, S, 3, generator=g)
    # n / (|n| + 1e-6) = 0 with gradient 1e6 w g: at the end of the ray that crosses first, where w is small, so that
    # this one entry does not become the maximum its chunk's other gradients are measured against
    nrm[0, S - 1] = 0.0
    case = {'S': S, 'crossings': ks, 'z': z, 'sdf': sdf, 'rgb': rgb, 'nrm': nrm,
            'beta': torch.tensor(beta, dtype=torch.float32), 'scale': torch.rand(N, 1, generator=g) + 0.5,
            'c_rgb_values': torch.randn(N, 3, generator=g), 'c_depth': torch.randn(N, 1, generator=g),
            'c_normal_map': torch.randn(N, 3, generator=g), 'c_weights': torch.randn(N, S, generator=g) * 0.1}
    # d/d beta is ONE number, the sum over rays and outputs of terms of either sign: with free random cotangents one case
    # in ten cancels to a few percent of its terms, and the fp32 oracle then misses the float64 one by more than 1e-5 for
    # no fault of anyone's.  Each ray's cotangent of each output gets the sign that makes its term non-negative.
    for k in OUTPUTS:
        sign = torch.where(beta_partials(case, use=(k,)) < 0, -1.0, 1.0).float()
        case['c_' + k] = case['c_' + k] * sign[:, None]
    return case


def low_beta_case(S, beta, seed):
    """Free sdf spanning +-0.5 at a small beta: no float64 parity exists there (module docstring); finiteness only."""
    g = torch.Generator().manual_seed(seed)
    c = edge_case(S, beta, seed)
    N = c['z'].shape[0]
    c['sdf'] = torch.rand(N, S, generator=g) - 0.5
    c['sdf'][0, 0] = 0.0
    c['crossings'] = None
    return c


def take(case, n):
    """The first n rays of a case."""
    return {k: (v[:n] if torch.is_tensor(v) and v.dim() >= 2 else v) for k, v in case.items()}


def random_poses(n, seed):
    """[n, 4, 4] fp32 poses with random rotations and translations."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))
    pose = torch.eye(4).repeat(n, 1, 1)
    pose[:, :3, :3], pose[:, :3, 3] = q, torch.randn(n, 3, generator=g)
    return pose


def density_smooth(sdf, beta):
    """The Laplace density written without sign() and expm1(): 0.5 e^{-s/beta} / beta outside, (1 - 0.5 e^{s/beta}) / beta
    inside and AT the surface.  The same sigma as mo.laplace_density to 1e-16 of 1/beta in float64, but autograd's
    derivative of it is the derivative: -0.5 e^{-|s|/beta} / beta^2, continuous through s = 0, never saturated.
    A yardstick for the reference's autograd, not a reference."""
    outside = 0.5 * torch.exp(-sdf.clamp(min=0.0) / beta)
    inside = 1.0 - 0.5 * torch.exp(sdf.clamp(max=0.0) / beta)          # clamp passes the gradient at its bound
    return torch.where(sdf > 0, outside, inside) / beta


def with_zero_crossings(case, value=0.0):
    """The case with the crossing sample of every second crossing ray set to `value`.

    At sdf == 0.0 exactly the reference's formula has sign(s) = 0: sigma = 0.5 / beta is the right value, but autograd
    returns d sigma / d s = 0 where the derivative is -0.5 / beta^2, the limit from either side (density_smooth).  The
    compositor kernel returns the derivative, which is also what the reference computes an ulp away, where its own
    sample falls when the kernel's happens to be 0.  So a gradient reference for s == 0 is the oracle at +-tiny, and
    the parity cases hold no exact zero (tests/test_composite_cases_cpu.py shows the artefact: 6e-2 of the chunk's maximum)."""
    c = dict(case)
    c['sdf'] = case['sdf'].clone()
    for r, k in enumerate(case['crossings']):
        if r % 2 == 0:
            c['sdf'][r, k] = value
    return c


def _compose(case, dtype, sdf, rgb, nrm, beta, pose=None, white=False, density=mo.laplace_density):
    """The oracle's compositor: mo.laplace_density -> mo.transmittance_weights -> the composites of mo.render."""
    z, ds = case['z'].to(dtype), case['scale'].to(dtype)
    w = mo.transmittance_weights(z, density(sdf, beta))[0]
    wsum = w.sum(1, keepdim=True)
    rgbv = (w.unsqueeze(-1) * rgb).sum(1)
    if white:
        rgbv = rgbv + (1. - wsum) * torch.tensor(BG, dtype=torch.float32).to(dtype)
    dep = ds * ((w * z).sum(1, keepdim=True) / (wsum + 1e-8))
    nm = (w.unsqueeze(-1) * (nrm / (nrm.norm(2, -1, keepdim=True) + 1e-6))).sum(1)
    if pose is not None:
        rot = pose.to(dtype).reshape(-1, 4, 4)[:, :3, :3].transpose(1, 2)
        nm = (rot @ nm.unsqueeze(-1)).squeeze(-1)
    return {'weights': w, 'rgb_values': rgbv, 'depth': dep, 'normal_map': nm, 'depth_vals': z * ds}


def beta_partials(case, use=OUTPUTS, pose=None, white=False):
    """float64 d loss / d beta ray by ray, [N]: the terms whose sum is d/d beta."""
    d = torch.float64
    beta = case['beta'].to(d).expand(case['z'].shape[0], 1).clone().requires_grad_(True)
    out = _compose(case, d, case['sdf'].to(d), case['rgb'].to(d), case['nrm'].to(d), beta, pose, white)
    loss = sum((case['c_' + k].to(d) * out[k]).sum() for k in use)
    return torch.autograd.grad(loss, beta)[0].reshape(-1)


# the option runs of the GPU test, at OPTION_SAMPLES: name -> (white background, poses: 0 none / 1 one / 2 one per ray,
# outputs that enter the loss).  A loss of one output alone hands the kernel null pointers for the other cotangents.
OPTION_SAMPLES = (65, 193)
OPTIONS = {
    'white': (True, 0, OUTPUTS),
    'pose_one': (False, 1, OUTPUTS),
    'pose_per_ray': (False, 2, OUTPUTS),
    'pose_per_ray_white': (True, 2, OUTPUTS),
    'rgb_values_alone': (False, 0, ('rgb_values',)),
    'rgb_values_alone_white': (True, 0, ('rgb_values',)),
    'depth_alone': (False, 0, ('depth',)),
    'weights_alone': (False, 0, ('weights',)),
    'normal_map_alone_pose': (False, 2, ('normal_map',)),
}


def option_pose(case, n_poses, seed=77):
    return None if n_poses == 0 else random_poses(1 if n_poses == 1 else case['z'].shape[0], seed)


def reference(case, dtype, pose=None, white=False, use=OUTPUTS, beta_raw=None, beta_min=0.0,
              density=mo.laplace_density):
    """The oracle's compositor on the case's fp32 inputs cast to `dtype` (_compose), R^T m for `pose` ([1,4,4] or
    [N,4,4]), depth_vals = z * scale.  `use`: the outputs that enter the loss (each times its cotangent).  beta_raw:
    beta = |beta_raw| + beta_min and the gradient is taken to beta_raw.  Returns (outputs, gradients); the gradient of
    an input the loss does not reach is zeros."""
    sdf, rgb, nrm = [case[k].to(dtype).requires_grad_(True) for k in ('sdf', 'rgb', 'nrm')]
    if beta_raw is None:
        bleaf = beta = case['beta'].to(dtype).requires_grad_(True)
    else:
        bleaf = torch.tensor(beta_raw, dtype=torch.float32).to(dtype).requires_grad_(True)
        beta = bleaf.abs() + torch.tensor(beta_min, dtype=torch.float32).to(dtype)
    out = _compose(case, dtype, sdf, rgb, nrm, beta, pose, white, density)
    loss = sum((case['c_' + k].to(dtype) * out[k]).sum() for k in use)
    leaves = [sdf, rgb, nrm, bleaf]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for t, gr in zip(leaves, grads)]
    return ({k: v.detach() for k, v in out.items()},
            dict(zip(('d/d sdf', 'd/d rgb', 'd/d normals', 'd/d beta'), grads)))
