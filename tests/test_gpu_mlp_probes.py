"""Softplus, the rebuilt sigmoid, the second-order term and the encoding slots of the fused MLP kernels, value by value.

tests/mlp_probe_cases.py builds networks that route one hidden unit or one encoding slot into each compared number without
rounding, and derives a bound for each number from the rounding steps of the kernel's formula.  Here the real modules
(ImplicitNetwork, RenderingNetwork, set_precision) run them on all three matrix cores; every comparison is with a float64
reference, per element, and logs the worst measured error beside its bound (errlog).  No bound was set from what the GPU
returns.  bf16x3 runs every case: under its own bounds (softplus100_lean's stated differences, 2^-16 of a 24-bit value
per two-plane product) where they differ, else under the same ones."""
import numpy as np
import pytest
import torch

import mlp_probe_cases as mp

pytestmark = pytest.mark.gpu


def _check(errlog, test, case, key, got, ref, bound):
    """|got - ref| <= bound per element (bound 0: equal); logs the error and the bound where their ratio is worst."""
    got = got.detach().cpu().double().numpy()
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (test, case, key, got.shape, ref.shape)
    assert np.isfinite(got).all(), (test, case, key, 'not finite at', np.argwhere(~np.isfinite(got))[:3].tolist())
    err = np.abs(got - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print('%s %s %s: max error %.3e (bound there %.3e, ratio %.3f)' % (test, case, key, err[i], bound[i], ratio[i]))
    errlog(test, case, key, err[i], bound[i])
    assert ratio[i] <= 1.0, '%s %s %s: at %r got %r, reference %r: error %.3e above the derived bound %.3e' % (
        test, case, key, i, got[i], ref[i], err[i], bound[i])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().cuda()


def _sdf_net(core, width, multires, state):
    from monosdf_amd.model.network import ImplicitNetwork
    net = ImplicitNetwork(width, 0.0, 3, 1, [width, width], geometric_init=False, skip_in=(), weight_norm=False,
                          multires=multires)
    net = net.cuda()
    net.set_precision(core)
    net.load_state_dict(state, strict=True)
    return net


def _plane(core, magnitude):
    return mp.PLANE2 * np.abs(magnitude) if core == 'bf16x3' else 0.0


@pytest.mark.parametrize('core', mp.CORES)
def test_softplus_value(core, errlog):
    """h = softplus100(a1) (bf16x3: softplus100_lean) at 311 x 64 pre-activations -- 0, the grid step, both sides of
    e = 1e-4, of 1 + e == 1 and of 100 a = 20, the subnormal and underflow range of e, +-200, a sweep at eight scales --
    through forward(), get_outputs() and, with a one-hot sdf row, both kernels behind get_sdf_vals()."""
    assert not mp.certificate('softplus')
    lean = core == 'bf16x3'
    test = 'probe_softplus.' + core
    x = _t(mp.SP_X)
    _, a1 = mp.sp_preactivations(mp.SP_X)
    ref = mp.softplus64(a1)
    bound = mp.bound_h(a1, lean)
    net = _sdf_net(core, mp.WIDTH, 0, mp.sp_state(np.ones(mp.WIDTH)))
    # the features pass the output layer's product (1 * h): two planes on bf16x3
    _check(errlog, test, 'h', 'forward()', net(x)[:, 1:], ref, bound + _plane(core, ref))
    _check(errlog, test, 'h', 'get_outputs()', net.get_outputs(x)[1], ref, bound + _plane(core, ref))
    got_f, got_g = [], []
    for j in mp.ONE_HOT_UNITS:
        net.load_state_dict(mp.sp_state(mp.one_hot(j)), strict=True)
        got_g.append(net.get_sdf_vals(x)[:, 0])
        with torch.no_grad():
            got_f.append(net.get_sdf_vals(x)[:, 0])
    cols = list(mp.ONE_HOT_UNITS)
    # the sdf row as a plain fp32 dot product over the activation: no plane
    _check(errlog, test, 'h', 'get_sdf_vals(), forward kernel', torch.stack(got_f, 1), ref[:, cols], bound[:, cols])
    _check(errlog, test, 'h', 'get_sdf_vals(), forward + gradient kernel', torch.stack(got_g, 1), ref[:, cols], bound[:, cols])


@pytest.mark.parametrize('core', mp.CORES)
def test_sigmoid_through_the_gradient_sweep(core, errlog):
    """s = 1 - exp2(-c h) of scale_by_sigmoid (GradSweepHooks): with a three-hot sdf row d sdf / d x_c = 2^-k s(a1_j), one
    unit per channel.  Absolute bound, at most 6 (bf16x3: 7) x 2^-24."""
    assert not mp.certificate('softplus')
    lean = core == 'bf16x3'
    test = 'probe_softplus.' + core
    x = _t(mp.SP_X)
    _, a1 = mp.sp_preactivations(mp.SP_X)
    net = _sdf_net(core, mp.WIDTH, 0, mp.sp_state(np.ones(mp.WIDTH)))
    got_a, got_b, ref, bound = [], [], [], []
    for units in mp.THREE_HOT:
        assert [j % 3 for j in units] == [0, 1, 2]
        net.load_state_dict(mp.sp_state(mp.three_hot(units)), strict=True)
        got_a.append(net.gradient_sdf(x))
        got_b.append(net.get_outputs(x)[2])
        u = list(units)
        s = mp.sigmoid64(100 * a1[:, u])
        ref.append(mp.UNIT_SCALE[u] * s)
        # p = s goes through the transposed product of layer 1: two planes on bf16x3
        bound.append(mp.UNIT_SCALE[u] * (mp.bound_s(a1[:, u], lean) + _plane(core, s)))
    ref, bound = np.concatenate(ref, 1), np.concatenate(bound, 1)
    _check(errlog, test, 's', 'gradient_sdf()', torch.cat(got_a, 1), ref, bound)
    _check(errlog, test, 's', 'get_outputs() gradient', torch.cat(got_b, 1), ref, bound)


@pytest.mark.parametrize('core', mp.CORES)
def test_sigmoid_and_second_order_term_through_the_double_backward(core, errlog):
    """One-hot upstream tensors: with a non-zero at one point, d <a, sdf> / d lin1.bias[j] = s(a1_j); with C = (1, 1, 1) at
    one point, d <C, grad> / d lin1.bias[j] = 2^-k_j 100 s (1 - s) -- SweepDownHooks::tile with p-bar rebuilt as
    q-bar rcp(s), both sides of its s > 0 switch among the hot points -- for all 64 units at once, over 47 hot points.
    The diagonal of lin1.weight's gradient is the bias gradient times a0, plus s where C is the hot tensor."""
    assert not mp.certificate('softplus')
    lean = core == 'bf16x3'
    test = 'probe_softplus.' + core
    xh = mp.SP_X[mp.SP_HOT]
    a0, a1 = mp.sp_preactivations(xh)
    n = len(xh)
    x = _t(xh)
    net = _sdf_net(core, mp.WIDTH, 0, mp.sp_state(np.ones(mp.WIDTH)))
    zero_B = torch.zeros(n, mp.WIDTH, device='cuda')
    got = {k: [] for k in ('b_a', 'w_a', 'b_C', 'w_C')}
    for i in range(n):
        for which in 'aC':
            a, C = torch.zeros(n, 1, device='cuda'), torch.zeros(n, 3, device='cuda')
            if which == 'a':
                a[i] = 1.0
            else:
                C[i] = 1.0
            net.zero_grad(set_to_none=True)
            sdf, feat, grad = net.get_outputs(x)
            ((a * sdf).sum() + (zero_B * feat).sum() + (C * grad).sum()).backward()
            got['b_' + which].append(net.lin1.bias.grad.clone())
            got['w_' + which].append(net.lin1.weight.grad.diagonal().clone())
    got = {k: torch.stack(v, 0) for k, v in got.items()}
    s = mp.sigmoid64(100 * a1)
    t = mp.UNIT_SCALE * 100 * s * mp.sigmoid64(-100 * a1)
    ds, dt = mp.bound_s(a1, lean), mp.bound_t(a1, mp.UNIT_SCALE, lean)
    _check(errlog, test, 's', 'lin1.bias gradient of <a, sdf>', got['b_a'], s, ds)
    _check(errlog, test, 'second_order', 'lin1.bias gradient of <C, grad>', got['b_C'], t, dt)
    # the weight-gradient product: one rounding per term; on bf16x3 two planes of s (or t) times two planes of a0, the
    # pair of second planes dropped (mp.plane_lo), and s times q-bar = 1, one plane
    lolo = 2.0 ** -8 * mp.plane_lo(a0) if lean else 0.0
    _check(errlog, test, 's', 'lin1.weight diagonal gradient of <a, sdf>', got['w_a'], s * a0,
           a0 * ds + mp.U * s * a0 + _plane(core, s * a0) + s * lolo)
    _check(errlog, test, 'second_order', 'lin1.weight diagonal gradient of <C, grad>', got['w_C'], t * a0 + s,
           a0 * dt + ds + 2 * mp.U * (t * a0 + s) + _plane(core, t * a0) + t * lolo + _plane(core, s))


@pytest.mark.parametrize('core', mp.CORES)
@pytest.mark.parametrize('multires', mp.PE_MULTIRES)
def test_position_encoding_slots(multires, core, errlog):
    """Every slot of pe_values / pe_jacobian_transpose / pe_jacobian for multires 6, 7 (45 slots, the widest) and 1: the
    value through the features, dval and its channel through gradient_sdf() with one one-hot state per slot (exactly 0
    in the other two channels), and 100 s (1 - s) dval through the double backward behind a probe layer."""
    assert not mp.certificate('pe', multires)
    lean = core == 'bf16x3'
    test = 'probe_encoding.' + core
    case = 'multires%d' % multires
    n = mp.pe_slots(multires)
    W = mp.PE_WIDTH
    x = _t(mp.PE_X[multires])
    slots = [mp.pe_reference(multires, j)[0] for j in range(n)]
    net = _sdf_net(core, W, multires, mp.pe_state(multires, np.ones(W), False))
    # values: feat[:, j] = a0_j = w slot + 1.25 (the idle units: 1.25); on bf16x3 a0 passes a product on two planes
    ref = np.full((len(mp.PE_X[multires]), W), mp.PE_BIAS)
    bound = np.zeros_like(ref)
    for j, s in enumerate(slots):
        ref[:, j] = s.a0
        bound[:, j] = mp.pe_da0(s, core) + (_plane(core, s.a0) if j >= 3 else 0.0)
    _check(errlog, test, case, 'slot values, forward()', net(x)[:, 1:], ref, bound)
    # derivatives: one state per slot
    got, ref, bound = [], [], []
    for j, s in enumerate(slots):
        net.load_state_dict(mp.pe_state(multires, mp.one_hot(j, W), False), strict=True)
        got.append(net.gradient_sdf(x))
        r, b = np.zeros((len(s.val), 3)), np.zeros((len(s.val), 3))
        r[:, s.c] = mp.pe_weight(j) * s.dval
        b[:, s.c] = mp.pe_weight(j) * mp.bound_pe(s.dval) if j >= 3 else 0.0
        ref.append(r)
        bound.append(b)
    _check(errlog, test, case, 'slot derivatives and channels, gradient_sdf()', torch.cat(got, 1), np.concatenate(ref, 1),
           np.concatenate(bound, 1))
    # pe_jacobian: d <C, grad> / d lin1.bias[j] = 2^-6 100 s (1 - s)(a1_j) w_j dval_j, C = (1, 1, 1) at one point
    xh = mp.PE_X[multires][mp.PE_HOT]
    nh = len(xh)
    net.load_state_dict(mp.pe_state(multires, np.ones(W), True), strict=True)
    xg = _t(xh)
    got = []
    for i in range(nh):
        C = torch.zeros(nh, 3, device='cuda')
        C[i] = 1.0
        net.zero_grad(set_to_none=True)
        sdf, feat, grad = net.get_outputs(xg)
        ((0 * sdf).sum() + (0 * feat).sum() + (C * grad).sum()).backward()
        got.append(net.lin1.bias.grad.clone())
    ref, bound = np.zeros((nh, W)), np.zeros((nh, W))
    sc = 2.0 ** -mp.PE_K
    for j, s in enumerate(slots):
        w = mp.pe_weight(j)
        val, dval, a0 = s.val[mp.PE_HOT], s.dval[mp.PE_HOT], s.a0[mp.PE_HOT]
        a1 = sc * w * val
        pbar = sc * w * dval
        sig = mp.sigmoid64(100 * a1)
        t = 100 * sig * (1 - sig) * pbar
        hot = mp.PeSlot(j, val, dval, s.c, a0, None, None, None)
        da1 = sc * mp.pe_da0(hot, core) + (mp.acc_rounding(a1, core) if j >= 3 else 0.0)
        ref[:, j] = t
        # dval: 4 ulp = 8 U relative, its product with C one more U; on bf16x3 it passes layer 0's product on two planes
        bound[:, j] = mp.bound_t(a1, pbar, lean, da1) + np.abs(t) * (2 * mp.ULP_SINCOS + 1) * mp.U + \
            (_plane(core, t) if j >= 3 else 0.0)
    _check(errlog, test, case, 'second-order term times dval, lin1.bias gradient of <C, grad>', torch.stack(got, 0), ref, bound)


def _color_net(core, mode, m, hdr, state):
    from monosdf_amd.model.network import RenderingNetwork
    net = RenderingNetwork(mp.COLOR_F, mode, 9 if mode == 'idr' else 3, 3, [mp.WIDTH], weight_norm=False, multires_view=m,
                           per_image_code=False, if_hdr=hdr)
    net = net.cuda()
    net.set_precision(core)
    net.load_state_dict(state, strict=True)
    return net


@pytest.mark.parametrize('core', mp.CORES)
@pytest.mark.parametrize('case', list(mp.VIEW_CASES))
def test_view_encoding_columns(case, core, errlog):
    """Every lead column of the colour network's first layer -- x | PE(v) | normal for idr, PE(v) for nerf, multires_view 4
    and 2 -- read back through rgb = relu(column + 2), three columns per state; 7 samples per ray at P = 217 (ray = pt / 7);
    the normal's gradient in its dense row (columns 30 .. 32 at multires_view 4: across a quarter boundary)."""
    mode, m = mp.VIEW_CASES[case]
    assert not mp.certificate('view', mode, m)
    test = 'probe_view_encoding.' + core
    pts, nrm, dirs = mp.view_inputs(m)
    val, _, pre, _, bnd, n0 = mp.view_columns(mode, m)
    bound = mp.view_bound(val, pre, bnd, core)
    lead = mp.view_lead(mode, m)
    net = _color_net(core, mode, m, True, mp.view_state(mode, m, 0))
    g_rgb = _t(np.tile(mp.VIEW_G, (mp.COLOR_P, 1)))
    got_rgb, got_nrm = [], []
    for st in range(mp.view_states(mode, m)):
        net.load_state_dict(mp.view_state(mode, m, st), strict=True)
        feat = torch.zeros(mp.COLOR_P, mp.COLOR_F, device='cuda', requires_grad=True)
        normals = _t(nrm).requires_grad_()
        rgb = net(_t(pts), normals, _t(dirs), feat, None, if_pixel_input=True, samples_per_ray=mp.COLOR_SPR)['rgb']
        (rgb * g_rgb).sum().backward()
        got_rgb.append(rgb)
        if mode == 'idr':
            got_nrm.append(normals.grad)
        else:
            assert normals.grad is None
        assert not feat.grad.any()
    pad = 3 * mp.view_states(mode, m) - lead
    ref = np.concatenate([pre, np.zeros((mp.COLOR_P, pad))], 1)
    _check(errlog, test, case, 'rgb', torch.cat(got_rgb, 1), ref, np.concatenate([bound, np.zeros((mp.COLOR_P, pad))], 1))
    if mode == 'idr':
        assert n0 == 6 + 6 * m
        want = np.concatenate([np.tile(mp.view_g_nrm(mode, m, st), (mp.COLOR_P, 1)) for st in range(mp.view_states(mode, m))], 1)
        _check(errlog, test, case, 'normals.grad', torch.cat(got_nrm, 1), want, 0.0)


@pytest.mark.parametrize('core', mp.CORES)
def test_colour_sigmoid_output(core, errlog):
    """y = 1 / (1 + __expf(-o)) and its backward g y (1 - y) at o = 0, +-2^-20, a sweep over [-20, 20], +-88, +-89 (exp(-o)
    overflows: y must be 0, not NaN) and +-110."""
    assert not mp.certificate('sigmoid')
    test = 'probe_colour_sigmoid.' + core
    feat64, o, g = mp.sigmoid_inputs()
    n = len(o)
    net = _color_net(core, 'nerf', 0, False, mp.sigmoid_state())
    feat = _t(feat64).requires_grad_()
    z = torch.zeros(n, 3, device='cuda')
    rgb = net(z, z, z, feat, None, if_pixel_input=True)['rgb']
    (rgb * _t(g)).sum().backward()
    y = mp.sigmoid64(o)
    dy, dg = mp.bound_color_sigmoid(o, g)
    _check(errlog, test, 'sigmoid', 'rgb', rgb, y, dy)
    ref = g * y * mp.sigmoid64(-o) * (o != 0)          # relu(f) - relu(-f) has no slope at f = 0 (nor has torch's)
    # a-bar (24 bits) passes the first layer's transposed product: two planes on bf16x3
    _check(errlog, test, 'sigmoid', 'feat.grad', feat.grad[:, :3], ref, dg + _plane(core, ref))
    assert not feat.grad[:, 3:].any()
