"""The fused MLP kernels against the exact answer, bit for bit, on all three matrix cores.

tests/mlp_exact_cases.py builds integer ReLU networks on which every sum the kernels form is exact in fp32 -- in any order,
on the fp32 matrix instructions and as bf16 plane products -- and certifies that on the float64 operands of every product.
Here the real modules (RenderingNetwork, ImplicitNetwork, set_precision) run those cases and every output, input gradient
and weight gradient is compared with torch.equal: a lost plane product, a wrong tile, a padded slot that leaks or a
gradient column far below the tensor's maximum all show, which the 1e-4 max-norm bar of the parity tests does not see.

A case runs on a core only where its certificate holds (the bf16x3 core forms three of the nine plane products); the fp32
and bf16x6 cores run every case, and test_every_core_runs_every_kind asserts what is left for bf16x3.  The hash-grid
cases run on every path a grid model can take (mlp_exact_cases.GRID_RUNS), bf16x3 among them: it is certified on all."""
import pytest
import torch

import mlp_exact_cases as mx

pytestmark = pytest.mark.gpu


def _certified(name, core):
    case = mx.ALL_CASES[name]
    cert = mx.certificate(case, core)
    if core != 'bf16x3':
        assert cert.ok, (name, core, cert.failures[:3])
    mx.assert_reaches(name, core)
    return case, cert.ok


def _same(name, core, key, got, want):
    want32 = want.float()
    assert torch.equal(want32.double(), want), (name, key, 'the reference is no fp32 value')
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == want32.shape, (name, core, key, got.dtype, got.shape, want32.shape)
    if not torch.equal(got, want32):
        raise AssertionError('%s on %s: %s differs from the exact result, first at %r'
                             % (name, core, key, mx.first_difference(got, want32)))


def _color_net(case, core):
    from monosdf_amd.model.network import RenderingNetwork
    a = case.args
    net = RenderingNetwork(a['F'], a['mode'], 9 if a['mode'] == 'idr' else 3, 3, [a['width']] * a['hidden'],
                           weight_norm=False, multires_view=0, per_image_code=a['code'], if_hdr=True)
    net.load_state_dict({k: v.clone() for k, v in case.state.items()}, strict=True)
    net = net.cuda()
    net.set_precision(core)
    return net


def _run_color(name, core):
    case, ok = _certified(name, core)
    if not ok:
        return False
    a, i = case.args, case.inputs
    net = _color_net(case, core)
    feat = i['feat'].cuda().requires_grad_()
    nrm = i['normals'].cuda().requires_grad_()
    rgb = net(i['points'].cuda(), nrm, i['dirs'].cuda(), feat, i['indices'].cuda(), if_pixel_input=True,
              samples_per_ray=a['spr'] if a['spr'] > 1 else None)['rgb']
    (rgb * case.up['g_rgb'].cuda()).sum().backward()
    ref = mx.reference(case)
    got = {'rgb': rgb, 'g_feat': feat.grad}
    if a['mode'] == 'idr':
        got['g_nrm'] = nrm.grad
    else:
        assert nrm.grad is None
    for k, p in net.named_parameters():
        got['g_code' if k == 'embeddings' else k] = p.grad
    assert set(got) == set(ref)
    for k in ref:
        _same(name, core, k, got[k], ref[k])
    return True


@pytest.mark.parametrize('core', mx.CORES)
@pytest.mark.parametrize('name', list(mx.COLOR_CASES))
def test_color_network_exact(name, core):
    """Forward, the gradients of features, normals and per-image code, and every weight and bias gradient: widths 64, 48
    (odd last tile), 100 (padded slots), 176 (several pairs per chunk), 256 (K = 16); one to three hidden layers; idr and
    nerf; with and without the code; 256 and 40 features; 7 samples per ray; P of every wave and workgroup edge; ReLU
    inputs of exactly zero in hidden and output layers."""
    _run_color('color.' + name, core)


@pytest.mark.parametrize('core', mx.CORES)
@pytest.mark.parametrize('name', list(mx.PROBE_CASES))
def test_plane_probes(name, core):
    """One- to three-plane weights, features and upstream gradients: between them every kept plane product of b16_step
    carries a result bit in the forward and in the transposed product (test_mlp_exact_cases_cpu.py shows that each one,
    removed, changes a result)."""
    _run_color('probe.' + name, core)


def _sdf_net(case, core):
    from monosdf_amd.model.network import ImplicitNetwork
    a = case.args
    net = ImplicitNetwork(a['F'], a.get('radius', 0.0), 3, 1, [a['width']] * a['hidden'], geometric_init=False,
                          skip_in=a.get('skip_in', ()), weight_norm=False, multires=0,
                          sphere_scale=a.get('sphere_scale', 1.0))
    net.load_state_dict({k: v.clone() for k, v in case.state.items()}, strict=True)
    net = net.cuda()
    net.set_precision(core)
    return net


def _run_sdf(name, core):
    case, ok = _certified(name, core)
    if not ok:
        return False
    net = _sdf_net(case, core)
    ref = mx.reference(case)
    x = case.inputs['x'].cuda()
    # forward(): the output layer as a matrix product; gradient_sdf(): the sdf row as a dot product, no features;
    # get_sdf_vals() without autograd: the forward-only kernel.  The first two never clamp (sdf_raw, grad_raw of a clamp
    # case); get_sdf_vals() clamps every point, through the forward + gradient kernel under autograd and through the
    # forward-only kernel (fminf) without
    out = net(x)
    _same(name, core, 'forward().sdf', out[:, :1], ref.get('sdf_raw', ref['sdf']))
    _same(name, core, 'forward().feat', out[:, 1:], ref['feat'])
    _same(name, core, 'gradient_sdf()', net.gradient_sdf(x), ref.get('grad_raw', ref['grad']))
    if 'sdf_raw' in ref:
        _same(name, core, 'get_sdf_vals() under autograd', net.get_sdf_vals(x), ref['sdf'])
    with torch.no_grad():
        _same(name, core, 'get_sdf_vals()', net.get_sdf_vals(x), ref['sdf'])
    # all three outputs of one evaluation and the double backward to every parameter
    sdf, feat, grad = net.get_outputs(x)
    for k, t in (('sdf', sdf), ('feat', feat), ('grad', grad)):
        _same(name, core, k, t, ref[k])
    up = {k: v.cuda() for k, v in case.up.items()}
    ((up['a'] * sdf).sum() + (up['B'] * feat).sum() + (up['C'] * grad).sum()).backward()
    params = dict(net.named_parameters())
    assert set(params) == set(case.state)
    for k, p in params.items():
        _same(name, core, k, p.grad, ref[k])
    return True


@pytest.mark.parametrize('core', mx.CORES)
@pytest.mark.parametrize('name', list(mx.SDF_SKIP_CASES))
def test_sdf_skip_exact(name, core):
    """The skip layer: the input block behind 3, 4, 7, 11 and 14 hidden tiles (kt = 17, the register layout's maximum) in
    all four kernel bodies, d sdf / d input arriving twice, the second load of C in the double backward, the two-part
    weight-gradient item, and 1 / sqrt(2) folded into the pack and applied once more to the finished weight-gradient sum:
    the stored weights are the fp32 values that the folded factor turns into +-4 and +-8 exactly, and the expected
    gradient of the stored weights is float32(1 / sqrt(2)) * float32(exact integer gradient), one rounding."""
    assert _run_sdf('skip.' + name, core)


@pytest.mark.parametrize('core', mx.CORES)
@pytest.mark.parametrize('name', list(mx.SDF_CLAMP_CASES))
def test_sdf_clamp_exact(name, core):
    """The bounding-sphere clamp on integer points with dyadic radius and scale: the decision sph < sdf per point (never
    within 2^-10 of a tie), the clamped sdf and the normal -scale x / |x| as numpy restates them in fp32, one rounding per
    operation (points of integer and power-of-two norm among them; the origin, clamped, has sdf = scale r and normals
    0), and parameter gradients to which clamped points hand on their feature gradient alone."""
    assert _run_sdf('clamp.' + name, core)


@pytest.mark.parametrize('core', mx.CORES)
@pytest.mark.parametrize('name', list(mx.SDF_GROUP_CASES))
def test_sdf_point_groups_exact(name, core):
    """evaluate(x, n_clamp, n_feat, split = s) over three workgroups, the last ragged: the first n_clamp points clamped,
    the first n_feat with features (the matrix-product output layer in their workgroups, the sdf row as a dot product in
    the others), the upstream gradients of d sdf / d x from two tensors split at s -- at and off the multiples of 16 and
    64.  Both forms of the output layer and both tensors carry the same exact integers, so every choice gives the bits
    of the reference.  (evaluate() keeps the clamped flags to itself: they show in the gradients.)"""
    name = 'group.' + name
    case, ok = _certified(name, core)
    assert ok, (name, core)
    net = _sdf_net(case, core)
    ref = mx.reference(case)
    n_clamp, n_feat, s = mx.groups(case)
    P = case.args['P']
    sdf, feat, grad_a, grad_b = net.evaluate(case.inputs['x'].cuda(), n_clamp, n_feat, split=s)
    assert sdf.shape == (s, 1) and feat.shape == (n_feat, case.args['F'])
    assert grad_a.shape == (s, 3) and grad_b.shape == (P - s, 3)
    _same(name, core, 'sdf', sdf, ref['sdf'][:s])
    _same(name, core, 'feat', feat, ref['feat'])
    _same(name, core, 'grad [:split]', grad_a, ref['grad'][:s])
    _same(name, core, 'grad [split:]', grad_b, ref['grad'][s:])
    (a, none), (C_a, C_b), B = case.up['a'], case.up['C'], case.up['B']
    assert none is None
    loss = (a.cuda() * sdf).sum() + (B[:n_feat].cuda() * feat).sum() + (C_a.cuda() * grad_a).sum() + \
        (C_b.cuda() * grad_b).sum()
    loss.backward()
    params = dict(net.named_parameters())
    assert set(params) == set(case.state)
    for k, p in params.items():
        _same(name, core, k, p.grad, ref[k])


@pytest.mark.parametrize('core', mx.CORES)
@pytest.mark.parametrize('name', list(mx.SDF_CASES))
def test_sdf_network_exact(name, core):
    """forward(), gradient_sdf(), get_sdf_vals() and the double backward of <a, sdf> + <B, feat> + <C, d sdf/dx> to every
    weight and bias: widths 64, 48, 100, 256 (17 out tiles, K = 17 transposed), two and three hidden layers, P of every
    wave and workgroup edge.  Needs exp2 to give 1 for -0 and 0 below -288 (softplus is then ReLU exactly)."""
    _run_sdf('sdf.' + name, core)


def _grid_net(case, core):
    from monosdf_amd.model.network import ImplicitNetworkGrid
    a, g = case.args, mx.grid_conf(case)
    net = ImplicitNetworkGrid(a['F'], 0.0, 3, 1, [a['width']] * a['hidden'], geometric_init=False, skip_in=(),
                              weight_norm=False, multires=0, base_size=g['base_size'], end_size=g['end_size'],
                              logmap=g['logmap'], num_levels=g['num_levels'], level_dim=g['level_dim'],
                              divide_factor=g['divide_factor'])
    state = {k: v.clone() for k, v in case.state.items()}
    state['encoding.offsets'] = net.encoding.offsets.clone()
    net.load_state_dict(state, strict=True)
    net = net.cuda()
    net.set_precision(core)
    return net


def _entry_points(prof):
    """The hash-grid entry points among the recorded calls, the binned forms under their plain names."""
    return {n[:-3] if n.endswith('_ws') else n for n in prof if n.startswith('msdf_hash_')}


@pytest.mark.parametrize('run', list(mx.GRID_RUNS))
@pytest.mark.parametrize('name', list(mx.GRID_CASES))
def test_hash_grid_model_exact(name, run, monkeypatch):
    """ImplicitNetworkGrid end to end -- encoder, network, the grid part of d sdf/dx, the double backward with the whole
    table gradient -- on levels of scale 8 with points on multiples of 1/8, in every aux layout (half, full and empty
    pieces of the level-major loads, one and two tiles, rows padded from 5, 6, 10, 12, 18 and 30 columns, hashed levels
    with colliding corners) and on every path: the fp32 core with the Jacobian inside the SDF kernels, with
    ops.FUSE_JACOBIAN off, with ops.HASH_SCATTER = 'atomic' (separate autograd nodes), and rows on the bf16 cores; four
    or eight features per level take rows on the fp32 core too, one feature per level the separate nodes.  All paths
    compute the same exact numbers, so all must give the same bits; the entry points each run calls are checked against
    the path it is meant to take."""
    from monosdf_amd import _lib, ops
    name = 'grid.' + name
    core, fuse, scatter = mx.GRID_RUNS[run]
    case, ok = _certified(name, core)
    assert ok, (name, core)
    path = mx.assert_grid_reaches(name, run)
    monkeypatch.setattr(ops, 'FUSE_JACOBIAN', fuse)
    monkeypatch.setattr(ops, 'HASH_SCATTER', scatter)
    prof = {}
    monkeypatch.setattr(_lib, 'PROFILE', prof)
    monkeypatch.setattr(_lib, 'PROFILE_NAMES', None)
    what = '%s (%s)' % (core, path)
    net = _grid_net(case, core)
    ref = mx.reference(case)
    x = case.inputs['x'].cuda()
    out = net(x)
    _same(name, what, 'forward().sdf', out['sdf'], ref['sdf'])
    _same(name, what, 'forward().feature', out['feature'], ref['feat'])
    _same(name, what, 'gradient_sdf()', net.gradient_sdf(x), ref['grad'])
    with torch.no_grad():
        _same(name, what, 'get_sdf_vals()', net.get_sdf_vals(x), ref['sdf'])
    prof.clear()
    sdf, feat, grad = net.get_outputs(x)
    for k, t in (('sdf', sdf), ('feat', feat), ('grad', grad)):
        _same(name, what, k, t, ref[k])
    up = {k: v.cuda() for k, v in case.up.items()}
    loss = (up['a'] * sdf).sum() + (up['B'] * feat).sum()
    if case.args['second_order']:
        loss = loss + (up['C'] * grad).sum()
    loss.backward()
    params = dict(net.named_parameters())
    assert set(params) == set(case.state)
    for k, p in params.items():
        _same(name, what, k, p.grad, ref[k])
    called = _entry_points(prof)
    must, must_not = mx.PATH_CALLS[path]
    if not case.args['second_order']:
        must = tuple(n for n in must if n != 'msdf_hash_encode_second_backward')
    assert set(must) <= called and not set(must_not) & called, (name, run, path, sorted(called))
    if not case.args['second_order']:
        # one feature per level has no second backward (the reference has none either): the library says so
        sdf, feat, grad = net.get_outputs(x)
        with pytest.raises(RuntimeError, match='unsupported'):
            grad.sum().backward()


def test_every_core_runs_every_kind():
    """fp32 and bf16x6 are certified on every case; bf16x3 on at least one full colour case (forward, backward, weight
    gradients), one full SDF case and the probes that need no more than its three plane products."""
    for core in ('fp32', 'bf16x6'):
        bad = [n for n, c in mx.ALL_CASES.items() if not mx.certificate(c, core).ok]
        assert not bad, (core, bad)
    ok3 = [n for n, c in mx.ALL_CASES.items() if mx.certificate(c, 'bf16x3').ok]
    for kind in ('color.', 'sdf.', 'probe.', 'grid.', 'skip.', 'clamp.', 'group.'):
        assert any(n.startswith(kind) for n in ok3), kind
    assert {'probe.w2f1g1', 'probe.w1f2g1', 'probe.w1f1g2'} <= set(ok3)
    assert {n for n in mx.ALL_CASES if n.startswith('grid.')} <= set(ok3)
