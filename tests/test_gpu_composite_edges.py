"""The compositor kernels (csrc/composite.hip) at the edges of their 64-sample register chunks, of the wave and of the
four-ray workgroup, against the float64 oracle on the constructed cases of tests/composite_cases.py (why constructed, and
why they are fair: that module and tests/test_composite_cases_cpu.py).

Per-sample tensors (weights, d/d sdf, d/d rgb, d/d normals) are compared chunk by chunk, every 64-sample chunk normalised
by its own reference maximum (composite_cases.chunk_rel_err), so that a wrong carry into a later chunk is measured
against that chunk and not against the first one; per-ray outputs and d/d beta with helpers.rel_err.  Every comparison is
held to helpers.TOL and recorded in the parity table as 'compositor_edges'.
"""
import ctypes as C

import pytest
import torch

import composite_cases as cc
from helpers import check, rel_err

pytestmark = pytest.mark.gpu

PER_SAMPLE = ('weights', 'd/d sdf', 'd/d rgb', 'd/d normals')


def _run(case, white=False, pose=None, use=cc.OUTPUTS, scale=None, beta_raw=None, beta_min=0.0, depth_vals=False):
    """ops.CompositeFunction forward + backward of the loss over `use`; (outputs, gradients) named like the
    reference's.  scale: the depth-scale tensor to hand over instead of the case's contiguous [N, 1]."""
    from monosdf_amd import ops
    leaf = lambda t: t.detach().cuda().requires_grad_(True)
    sdf, rgb, nrm = leaf(case['sdf']), leaf(case['rgb']), leaf(case['nrm'])
    if beta_raw is None:
        bleaf = beta = leaf(case['beta'])
        raw = None
    else:
        bleaf = raw = leaf(torch.tensor(beta_raw, dtype=torch.float32))
        beta = ops.effective_beta(raw, beta_min)
    res = ops.CompositeFunction.apply(case['z'].cuda(), sdf, rgb, nrm, beta,
                                      case['scale'].cuda() if scale is None else scale, white, list(cc.BG),
                                      None if pose is None else pose.cuda(), raw, depth_vals)
    out = dict(zip(('weights', 'rgb_values', 'depth', 'normal_map', 'depth_vals'), res))
    loss = sum((case['c_' + k].cuda() * out[k]).sum() for k in use)
    loss.backward()
    grads = {k: (torch.zeros_like(t) if t.grad is None else t.grad)
             for k, t in zip(('d/d sdf', 'd/d rgb', 'd/d normals', 'd/d beta'), (sdf, rgb, nrm, bleaf))}
    return {k: v.detach() for k, v in out.items()}, grads


def _compare(errlog, name, got, want):
    (out, grads), (out_o, grads_o) = got, want
    for k in ('weights', 'rgb_values', 'depth', 'normal_map'):
        err = cc.chunk_rel_err(out[k], out_o[k]) if k in PER_SAMPLE else rel_err(out[k], out_o[k])
        check(errlog, 'compositor_edges', name, k, err)
    for k in ('d/d sdf', 'd/d rgb', 'd/d normals', 'd/d beta'):
        assert grads[k].shape == grads_o[k].shape, (name, k)
        err = cc.chunk_rel_err(grads[k], grads_o[k]) if k in PER_SAMPLE else rel_err(grads[k], grads_o[k])
        check(errlog, 'compositor_edges', name, k, err)


@pytest.fixture(scope='module')
def cases():
    memo = {}

    def get(S, beta=0.07):
        if (S, beta) not in memo:
            memo[(S, beta)] = cc.edge_case(S, beta, cc.case_seed(S, beta))
        return memo[(S, beta)]
    return get


@pytest.mark.parametrize('beta', cc.BETAS)
@pytest.mark.parametrize('S', cc.SAMPLES)
def test_parity_at_chunk_and_wave_edges(S, beta, cases, errlog):
    """One crossing at the first / last lane of every chunk and next to it, S on and around every chunk boundary, the
    fourth chunk (S > 192), S = 1, 2, 3 (S = 1 against the oracle that follows the reference's one-sample construction),
    one zero normal, two escaping rays."""
    c = cases(S, beta)
    _compare(errlog, 'S%d_beta%g' % (S, beta), _run(c), cc.reference(c, torch.float64))


@pytest.mark.parametrize('S', cc.OPTION_SAMPLES)
def test_sdf_exactly_zero(S, cases, errlog):
    """Crossing samples at sdf == 0.0 exactly (the first lane of a chunk among them).  sigma = 0.5 / beta there, so
    every OUTPUT is compared with the float64 oracle on the same inputs.  The GRADIENTS are compared with the oracle at
    +1e-30 and at -1e-30: at 0.0 itself the reference's autograd returns d sigma / d s = 0 (sign(0) = 0) where the
    derivative is -0.5 / beta^2 from either side, and the kernel returns the derivative (composite_cases.
    with_zero_crossings; the artefact is 6e-2 of the chunk's maximum here, tests/test_composite_cases_cpu.py)."""
    c = cc.with_zero_crossings(cases(S))
    assert (c['sdf'] == 0).sum() >= 4
    out, grads = _run(c, white=True)
    out_o = cc.reference(c, torch.float64, white=True)[0]
    for tiny in (1e-30, -1e-30):
        near = cc.with_zero_crossings(cases(S), tiny)
        assert (near['sdf'] == tiny).sum() >= 4                        # representable in fp32
        _compare(errlog, 'S%d_sdf_zero_vs_%+g' % (S, tiny), (out, grads),
                 (out_o, cc.reference(near, torch.float64, white=True)[1]))


def _composite_args(N, S, n_alloc):
    """CompositeArgs / CompositeBwdArgs over buffers of n_alloc samples per ray, outputs filled with 1234.5."""
    from monosdf_amd import _lib
    g = torch.Generator().manual_seed(5)
    t = {k: torch.rand(N, n_alloc, generator=g).cuda() for k in ('z', 'sdf')}
    t.update({k: torch.rand(N, n_alloc, 3, generator=g).cuda() for k in ('rgb', 'nrm')})
    t['beta'], t['depth_scale'] = torch.tensor([0.1]).cuda(), torch.ones(N).cuda()
    outs = {k: torch.full(shape, 1234.5).cuda() for k, shape in (
        ('weights', (N, n_alloc)), ('rgb_values', (N, 3)), ('depth_values', (N,)), ('normal_map', (N, 3)),
        ('wsum', (N,)), ('depth_vals', (N, n_alloc)))}
    gin = {k: torch.ones(shape).cuda() for k, shape in (
        ('g_rgb_values', (N, 3)), ('g_depth', (N,)), ('g_normal', (N, 3)), ('g_weights', (N, n_alloc)))}
    gout = {k: torch.full(shape, 1234.5).cuda() for k, shape in (
        ('g_sdf', (N, n_alloc)), ('g_rgb', (N, n_alloc, 3)), ('g_nrm', (N, n_alloc, 3)), ('g_beta_part', (N,)))}
    a, b = _lib.CompositeArgs(), _lib.CompositeBwdArgs()
    for k, v in list(t.items()) + list(outs.items()):
        setattr(a, k, v.data_ptr())
    for k, v in list(t.items()) + list(gin.items()) + list(gout.items()):
        setattr(b, k, v.data_ptr())
    b.weights, b.wsum, b.depth_values = [outs[k].data_ptr() for k in ('weights', 'wsum', 'depth_values')]
    for s in (a, b):
        s.N, s.S, s.white_bkgd, s.bg0, s.bg1, s.bg2 = N, S, 0, 1.0, 1.0, 1.0
        s.pose, s.pose_stride, s.depth_scale_stride = None, 0, 1
    return a, b, outs, gout, (t, gin)                    # the inputs stay alive with the caller


@pytest.mark.parametrize('S', [0, 257, -1])
def test_unsupported_sample_counts_are_refused_and_nothing_is_written(S):
    """More than 64 * 4 samples do not fit the backward's registers, fewer than one is no ray: an error, no launch."""
    from monosdf_amd import _lib
    a, b, outs, gout, keep = _composite_args(5, S, 257)
    with pytest.raises(RuntimeError, match='invalid argument'):
        _lib.call('msdf_composite_forward', C.byref(a), _lib.stream_ptr())
    with pytest.raises(RuntimeError, match='invalid argument'):
        _lib.call('msdf_composite_backward', C.byref(b), _lib.stream_ptr())
    torch.cuda.synchronize()
    for k, v in list(outs.items()) + list(gout.items()):
        assert bool((v == 1234.5).all()), k


@pytest.mark.parametrize('name', sorted(cc.OPTIONS))
@pytest.mark.parametrize('S', cc.OPTION_SAMPLES)
def test_options_against_the_oracle(S, name, cases, errlog):
    """White background, one pose and one per ray (R^T m forward, R g backward), losses of ONE output (the other
    cotangents then reach the kernel as null pointers, and the gradients they alone would feed are exact zeros)."""
    white, n_poses, use = cc.OPTIONS[name]
    c = cases(S)
    pose = cc.option_pose(c, n_poses)
    _compare(errlog, 'S%d_%s' % (S, name), _run(c, white=white, pose=pose, use=use),
             cc.reference(c, torch.float64, white=white, pose=pose, use=use))


@pytest.mark.parametrize('S', cc.OPTION_SAMPLES)
def test_strided_depth_scale_and_depth_vals(S, cases, errlog):
    """The depth scale read in place as a column of an [N, 3] table (pitch 3 floats), and depth_vals = z * scale, which
    is one fp32 product per sample: bit-equal."""
    c = cases(S)
    N = c['z'].shape[0]
    table = torch.full((N, 3), float('nan')).cuda()
    table[:, 1:2] = c['scale'].cuda()
    column = table[:, 1:2]
    assert column.stride() == (3, 1) and not column.is_contiguous()
    want = cc.reference(c, torch.float64, white=True)
    for label, scale in (('strided', column), ('dense', c['scale'].cuda())):
        got = _run(c, white=True, scale=scale, depth_vals=True)
        _compare(errlog, 'S%d_scale_%s' % (S, label), got, want)
        assert torch.equal(got[0]['depth_vals'].cpu(), c['z'] * c['scale']), label
    assert torch.equal(table[:, 1:2].cpu(), c['scale']) and bool(torch.isnan(table[:, 0]).all())


def test_beta_raw_gradient_sums_more_than_a_wave_of_partials(errlog):
    """beta = |beta_raw| + beta_min with a negative raw value at N = 130: msdf_beta_grad's 64 lanes take three trips over
    the per-ray partials, and the sign is -1.  At beta_raw = 0 the reference's abs has gradient 0."""
    c = cc.edge_case(*cc.BETA_RAW_CASE)
    assert c['z'].shape[0] == 130
    got = _run(c, beta_raw=cc.BETA_RAW, beta_min=cc.BETA_MIN)
    want = cc.reference(c, torch.float64, beta_raw=cc.BETA_RAW, beta_min=cc.BETA_MIN)
    _compare(errlog, 'N130_S3_beta_raw', got, want)
    assert want[1]['d/d beta'].item() != 0
    # the same value through the plain beta argument has the opposite sign
    plain = _run(c)[1]['d/d beta']
    assert rel_err(-plain, want[1]['d/d beta']) <= 1e-4
    got0 = _run(c, beta_raw=0.0, beta_min=0.07)
    want0 = cc.reference(c, torch.float64, beta_raw=0.0, beta_min=0.07)
    assert want0[1]['d/d beta'].item() == 0 and got0[1]['d/d beta'].item() == 0
    for k in ('weights', 'd/d sdf'):
        check(errlog, 'compositor_edges', 'N130_S3_beta_raw0', k,
              cc.chunk_rel_err({**got0[0], **got0[1]}[k], {**want0[0], **want0[1]}[k]))


@pytest.mark.parametrize('N', cc.RAY_COUNTS + (0,))
def test_ray_counts_around_the_four_ray_workgroup(N, cases, errlog):
    c = cc.take(cases(65), N)
    assert c['z'].shape == (N, 65)
    got, want = _run(c, white=True), cc.reference(c, torch.float64, white=True)
    if N == 0:
        for k in ('weights', 'rgb_values', 'depth', 'normal_map'):
            assert got[0][k].shape == want[0][k].shape and got[0][k].numel() == 0
        for k in ('d/d sdf', 'd/d rgb', 'd/d normals'):
            assert got[1][k].shape == want[1][k].shape
        assert got[1]['d/d beta'].item() == 0
        return
    _compare(errlog, 'N%d_S65' % N, got, want)


@pytest.mark.parametrize('beta', [0.005, 0.001])
@pytest.mark.parametrize('S', [65, 193])
def test_low_beta_stays_finite(S, beta):
    """NO parity is asserted here: at beta = 0.005 ... 0.001 the reference's own fp32 arithmetic deviates from float64
    by O(1) in the sdf, rgb and normal gradients (0.5 + 0.5 expm1(-s/beta) has no digits left for s > 0, and the 1e10 last
    interval multiplies what is left), so a float64 reference would fail a correct kernel.  What must hold: every output
    and gradient is finite wherever the fp32 CPU oracle's is, weights are non-negative and sum to at most 1."""
    c = cc.low_beta_case(S, beta, 9000 + S)
    assert c['sdf'].min() < -0.45 and c['sdf'].max() > 0.45
    (out, grads), (out_o, grads_o) = _run(c, white=True), cc.reference(c, torch.float32, white=True)
    for k in ('weights', 'rgb_values', 'depth', 'normal_map'):
        ok = torch.isfinite(out_o[k])
        assert bool(torch.isfinite(out[k].cpu())[ok].all()), k
    for k in grads:
        ok = torch.isfinite(grads_o[k])
        assert bool(torch.isfinite(grads[k].cpu())[ok].all()), k
    w = out['weights'].cpu()
    assert bool((w >= 0).all()) and bool((w.sum(1) <= 1 + 1e-6).all())
