"""The loss kernels (csrc/loss.hip) and the Laplace density operator (csrc/sampler.hip) past the sizes at which their loops
take a second trip, against the float64 oracles.

msdf_monosdf_loss and msdf_probe_loss are ONE workgroup of 1,024 threads: a thread takes rows tid, tid + 1024, ..., and in
the mask pass a wave takes rays wave, wave + 16, ... with its lanes over samples lane, lane + 64, ...  The shapes here sit
on and around 1,024 rays / points, 16 rays and 64 samples, and at the workload's 1,024 x 98 with 2,048 eikonal points.
msdf_laplace_density[_backward] launch at most 2,048 x 256 threads and stride over the rest.

Scalars are held to the criterion of test_monosdf_loss_against_reference_fixtures, 1e-5 max(1, |ref|); gradients to
helpers.TOL of the reference's maximum.  Every figure goes to the parity table ('monosdf_loss_edges', 'probe_loss_edges',
'laplace_density_edges').
"""
import pytest
import torch

from helpers import check, rel_err

pytestmark = pytest.mark.gpu

SCALARS = ['loss', 'rgb_loss', 'eikonal_loss', 'smooth_loss', 'depth_loss', 'normal_l1', 'normal_cos']
GRAD_KEYS = ['rgb_values', 'depth_values', 'normal_map', 'grad_theta', 'grad_theta_nei']
WEIGHTS = dict(eikonal=0.1, smooth=0.005, depth=0.1, normal_l1=0.05, normal_cos=0.05)
# (rays, samples per ray, eikonal points)
SHAPES = [(1, 1, 1), (15, 65, 17), (16, 64, 1024), (17, 63, 1025), (1023, 12, 2047), (1024, 98, 2048),
          (1025, 129, 2049), (2050, 3, 4100)]
# one shape of each group -- less than one trip of every loop, one full trip, more than one -- also without grad_theta
NO_EIKONAL = [(15, 65, 17), (1024, 98, 2048), (1025, 129, 2049)]
SCALAR_TOL = 1e-5


def _loss_inputs(N, S, E, seed, all_masked=False):
    """Model outputs and ground truth (fp32, CPU): every third ray is background (all sdf positive), some samples are
    exactly 0 (neither sign; ray 1 holds only positive values and zeros and is background too), ~20 % of the ground-truth
    mask is off."""
    g = torch.Generator().manual_seed(seed)
    sdf = torch.randn(N, S, generator=g) * 0.2
    sdf[::3] = sdf[::3].abs() + 0.01
    if N > 1:
        sdf[1] = sdf[1].abs()
        sdf[1, ::2] = 0.0
    sdf.view(-1)[torch.randint(0, N * S, (max(1, N * S // 50),), generator=g)] = 0.0
    out = {'rgb_values': torch.rand(N, 3, generator=g), 'depth_values': torch.rand(N, 1, generator=g) + 0.5,
           'normal_map': torch.randn(N, 3, generator=g) * 0.5, 'sdf': sdf,
           'grad_theta': torch.randn(E, 3, generator=g), 'grad_theta_nei': torch.randn(E, 3, generator=g)}
    mask = (torch.rand(1, N, 1, generator=g) > 0.2).float()
    # the depth cue follows the prediction, as a monocular cue does (target = 50 cue + 0.5 = 1.4 p + 0.3 + noise): see
    # _scale_cancellation
    cue = (1.4 * out['depth_values'] - 0.2 + 0.15 * torch.randn(N, 1, generator=g)) / 50.0
    gt = {'rgb': torch.rand(1, N, 3, generator=g), 'depth': cue[None],
          'normal': torch.randn(1, N, 3, generator=g), 'mask': torch.zeros_like(mask) if all_masked else mask}
    return out, gt


def _scale_cancellation(out, gt):
    """How much the numerator of the least-squares scale, M sum(p t) - sum(p) sum(t) over the masked rays, cancels
    (float64).  The fp32 sums carry a rounding error of a few 2^-24 each, the solved scale -- and with it every depth
    gradient, which is proportional to it -- that times this factor: with a cue that is independent of the prediction
    the scale is ~0, the factor reaches 1e4 and NO fp32 evaluation of the reference's formula is within 1e-4 of
    float64.  Below 100, the error of the scale stays below ~2e-5, a fifth of the bar."""
    sdf = out['sdf']
    m = ((gt['mask'].reshape(-1) > 0.5) & (sdf > 0).any(-1) & (sdf < 0).any(-1)).double()
    p, t = out['depth_values'].reshape(-1).double(), gt['depth'].reshape(-1).double() * 50 + 0.5
    if m.sum() < 2:
        return 0.0
    a, b = m.sum() * (m * p * t).sum(), (m * p).sum() * (m * t).sum()
    return (a.abs() / (a - b).abs()).item()


def _reference(out, gt, gamma, scale_invariant, weights=WEIGHTS):
    from oracle import loss_oracle as lo
    leaves = {k: (v.double().requires_grad_(True) if k in GRAD_KEYS else v.double()) for k, v in out.items()}
    res = lo.monosdf_loss(leaves, {k: v.double() for k, v in gt.items()}, weights, if_gamma_loss=gamma,
                          scale_invariant=scale_invariant)
    grads = torch.autograd.grad(res['loss'], [leaves[k] for k in GRAD_KEYS], allow_unused=True)
    grads = {k: (torch.zeros_like(leaves[k]) if gr is None else gr) for k, gr in zip(GRAD_KEYS, grads)}
    return {k: res[k].item() for k in SCALARS}, grads


def _check_scalars(errlog, test, name, got, ref):
    for k in SCALARS:
        check(errlog, test, name, k, abs(got[k] - ref[k]) / max(1.0, abs(ref[k])), default=SCALAR_TOL)


def _module(gamma, scale_invariant):
    from monosdf_amd.model.loss import MonoSDFLoss
    return MonoSDFLoss(rgb_loss='torch.nn.L1Loss', eikonal_weight=WEIGHTS['eikonal'], smooth_weight=WEIGHTS['smooth'],
                       depth_weight=WEIGHTS['depth'], normal_l1_weight=WEIGHTS['normal_l1'],
                       normal_cos_weight=WEIGHTS['normal_cos'], if_gamma_loss=gamma,
                       if_scale_invariant_depth=scale_invariant)


def _run_module(out, gt, gamma, scale_invariant):
    leaves = {k: (v.cuda().requires_grad_(True) if k in GRAD_KEYS else v.cuda()) for k, v in out.items()}
    res = _module(gamma, scale_invariant)(leaves, gt, if_pixel_input=True)       # ground truth on the host, as loaded
    res['loss'].backward()
    return {k: res[k].item() for k in SCALARS}, {k: leaves[k].grad for k in GRAD_KEYS}


@pytest.mark.parametrize('scale_invariant', [True, False])
@pytest.mark.parametrize('gamma', [False, True])
@pytest.mark.parametrize('N,S,E', SHAPES)
def test_monosdf_loss_across_the_workgroup_strides(N, S, E, gamma, scale_invariant, errlog):
    out, gt = _loss_inputs(N, S, E, seed=100 + N)
    assert _scale_cancellation(out, gt) < 100            # a condition on the inputs: change them, not the bound
    ref, g_ref = _reference(out, gt, gamma, scale_invariant)
    got, g_got = _run_module(out, gt, gamma, scale_invariant)
    name = 'N%d_S%d_E%d_gamma%d_si%d' % (N, S, E, gamma, scale_invariant)
    _check_scalars(errlog, 'monosdf_loss_edges', name, got, ref)
    for k in GRAD_KEYS:
        assert g_got[k].shape == out[k].shape
        check(errlog, 'monosdf_loss_edges', name, 'd/d ' + k, rel_err(g_got[k], g_ref[k]))
    if N >= 15:
        assert ref['depth_loss'] > 0 and ref['normal_cos'] > 0          # some rays are in the mask


@pytest.mark.parametrize('N,S,E', NO_EIKONAL)
def test_monosdf_loss_without_grad_theta(N, S, E, errlog):
    """The kernel's path without the eikonal block (null grad_theta / grad_nei): the same loss as the oracle's with zero
    eikonal and smoothness weights, and exact zeros for the two terms it skips."""
    from monosdf_amd import ops
    out, gt = _loss_inputs(N, S, E, seed=300 + N)
    assert _scale_cancellation(out, gt) < 100
    ref, g_ref = _reference(out, gt, True, True, dict(WEIGHTS, eikonal=0.0, smooth=0.0))
    leaves = {k: out[k].cuda().requires_grad_(True) for k in GRAD_KEYS[:3]}
    w = (WEIGHTS['eikonal'], WEIGHTS['smooth'], WEIGHTS['depth'], WEIGHTS['normal_l1'], WEIGHTS['normal_cos'])
    res = ops.MonoSdfLossFunction.apply(leaves['rgb_values'], leaves['depth_values'], leaves['normal_map'], None, None,
                                        out['sdf'].cuda(), gt['rgb'], gt['depth'], gt['normal'], gt['mask'], w, True, True)
    res[0].backward()
    got = dict(zip(SCALARS, res.detach().cpu().tolist()))
    assert got['eikonal_loss'] == 0.0 and got['smooth_loss'] == 0.0
    ref['eikonal_loss'] = ref['smooth_loss'] = 0.0
    name = 'N%d_S%d_no_grad_theta' % (N, S)
    _check_scalars(errlog, 'monosdf_loss_edges', name, got, ref)
    for k in GRAD_KEYS[:3]:
        check(errlog, 'monosdf_loss_edges', name, 'd/d ' + k, rel_err(leaves[k].grad, g_ref[k]))


def test_monosdf_loss_with_every_ray_masked_out(errlog):
    """No ray in the mask: the depth term and its gradient are exactly 0 (M = 0, singular scale / shift system), the
    masked normals are zero vectors."""
    N, S, E = 17, 63, 1025
    out, gt = _loss_inputs(N, S, E, seed=7, all_masked=True)
    ref, g_ref = _reference(out, gt, False, True)
    got, g_got = _run_module(out, gt, False, True)
    assert ref['depth_loss'] == 0.0 and got['depth_loss'] == 0.0
    _check_scalars(errlog, 'monosdf_loss_edges', 'N17_all_masked', got, ref)
    for k in GRAD_KEYS:
        check(errlog, 'monosdf_loss_edges', 'N17_all_masked', 'd/d ' + k, rel_err(g_got[k], g_ref[k]))
    assert not g_got['depth_values'].any() and not g_got['normal_map'].any()


@pytest.mark.parametrize('N,M', [(1, 1), (1023, 2047), (1025, 2049), (5, 1030), (1030, 5)])
def test_probe_loss_across_the_workgroup_stride(N, M, errlog):
    from oracle import monosdf_oracle as mo
    from monosdf_amd import ops
    g = torch.Generator().manual_seed(21 + N)
    vals = {'rgb_values': torch.rand(N, 3, generator=g) - 0.3, 'normal_map': torch.randn(N, 3, generator=g),
            'depth_values': torch.rand(N, 1, generator=g) + 0.5, 'grad_theta': torch.randn(M, 3, generator=g),
            'grad_theta_nei': torch.randn(M, 3, generator=g)}
    ref_in = {k: v.double().requires_grad_(True) for k, v in vals.items()}
    l_ref = mo.probe_loss(ref_in)
    g_ref = torch.autograd.grad(l_ref, list(ref_in.values()))
    gpu_in = {k: v.cuda().requires_grad_(True) for k, v in vals.items()}
    l = ops.probe_loss(gpu_in)
    name = 'N%d_M%d' % (N, M)
    check(errlog, 'probe_loss_edges', name, 'loss', abs(l.item() - l_ref.item()) / max(1.0, abs(l_ref.item())),
          default=SCALAR_TOL)
    l.backward()
    for (k, t), gr in zip(gpu_in.items(), g_ref):
        assert t.grad.shape == vals[k].shape
        check(errlog, 'probe_loss_edges', name, 'd/d ' + k, rel_err(t.grad, gr))


def _density_case(sdf, beta, name, errlog):
    """LaplaceDensityFunction forward and both gradients against the float64 oracle."""
    from oracle import monosdf_oracle as mo
    from monosdf_amd import ops
    g = torch.Generator().manual_seed(3)
    cot = torch.randn(sdf.shape, generator=g)
    s_o, b_o = sdf.double().requires_grad_(True), beta.double().requires_grad_(True)
    dens_o = mo.laplace_density(s_o, b_o)
    gs_o, gb_o = torch.autograd.grad((cot.double() * dens_o).sum(), [s_o, b_o])
    s, b = sdf.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    dens = ops.LaplaceDensityFunction.apply(s, b)
    (cot.cuda() * dens).sum().backward()
    assert dens.shape == sdf.shape and b.grad.shape == beta.shape
    check(errlog, 'laplace_density_edges', name, 'sigma', rel_err(dens, dens_o))
    check(errlog, 'laplace_density_edges', name, 'd/d sdf', rel_err(s.grad, gs_o))
    check(errlog, 'laplace_density_edges', name, 'd/d beta', rel_err(b.grad, gb_o))
    # the last elements are those of the grid-stride loop's second trip
    tail = slice(-513, None)
    check(errlog, 'laplace_density_edges', name, 'sigma (past the grid)',
          rel_err(dens.reshape(-1)[tail], dens_o.reshape(-1)[tail]))
    check(errlog, 'laplace_density_edges', name, 'd/d sdf (past the grid)',
          rel_err(s.grad.reshape(-1)[tail], gs_o.reshape(-1)[tail]))


def test_laplace_density_past_the_grid_scalar_beta(errlog):
    """2,048 x 256 + 513 elements: the last 513 are the second trip of the grid-stride loop; sdf/beta within +-12, some
    samples exactly 0 (sign 0: sigma = 0.5 / beta, d/d sdf = 0)."""
    n = 2048 * 256 + 513
    g = torch.Generator().manual_seed(1)
    beta = torch.tensor([0.07])
    sdf = (torch.rand(n, generator=g) * 2 - 1) * (12 * 0.07 * 0.999)
    sdf[::1001] = 0.0
    sdf[-1] = 0.0
    assert (sdf.abs() / beta).max() <= 12
    _density_case(sdf, beta, 'n%d_scalar_beta' % n, errlog)


def test_laplace_density_past_the_grid_beta_per_row(errlog):
    """74,973 rows of 7 (524,811 elements, past the grid too) with one beta per row: the row of an element is i / 7."""
    rows, cols = 74973, 7
    assert rows * cols > 2048 * 256
    g = torch.Generator().manual_seed(2)
    beta = torch.rand(rows, 1, generator=g) * 0.09 + 0.01
    sdf = (torch.rand(rows, cols, generator=g) * 2 - 1) * (12 * 0.999) * beta
    sdf[::997, 3] = 0.0
    assert (sdf.abs() / beta).max() <= 12
    _density_case(sdf, beta, 'rows%d_cols%d_beta_per_row' % (rows, cols), errlog)
