"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the reference's
golden vectors.  Tolerance: 1e-4 of each tensor's max-abs (BASELINE.json north_star:
"within 1e-4 rel fp32"); sampler-dependent cases get 5e-4 because the inverse CDF amplifies
last-bit differences of the prefix sums (the oracle itself differs from the reference by up
to 2e-4 there when the summation order changes).
"""
import numpy as np
import pytest
import torch

from harness import build_model, case_model, check_param_grads, oracle_state, run_pass, to_device as _cuda
from helpers import ALL_CASES, Case, check, digest, hash_table_gradients, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


# the matrix cores of the fused MLP kernels: fp32 and bf16x6 (fp32-grade products from three bf16 planes) are held to
# the SAME rows of the frozen tolerance table (tests/helpers.py: a '.bf16x6' test reads the '.fp32' row), bf16x3 (opt-in,
# 2^-16 products) has rows of its own
@pytest.fixture(params=['fp32', 'bf16x3', 'bf16x6'])
def precision(request):
    return request.param


@pytest.mark.parametrize('name', ['mlp_w64_eval', 'mlp_w256_eval', 'gridless_w128_train'])
def test_sdf_network_stages(name, precision, errlog):
    from oracle import monosdf_oracle as mo
    c = Case(name)
    m = case_model(c, training=False, precision=precision)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(1000 + 37, 3, generator=g) * 2 - 1) * 1.3       # some points outside the sphere (clamp)
    st = oracle_state(c.state)
    sdf_o, feat_o, grad_o = mo.get_outputs(st, c.conf, x, create_graph=False)
    sdf, feat, grad = m.implicit_network.get_outputs(x.cuda())
    test = 'sdf_stages.' + precision
    check(errlog, test, name, 'sdf', rel_err(sdf, sdf_o))
    check(errlog, test, name, 'feature', rel_err(feat, feat_o))
    check(errlog, test, name, 'grad_x', rel_err(grad, grad_o))
    with torch.no_grad():
        vals = m.implicit_network.get_sdf_vals(x.cuda())
    check(errlog, test, name, 'get_sdf_vals', rel_err(vals, mo.get_sdf_vals(st, c.conf, x)))
    gu = m.implicit_network.gradient_sdf(x.cuda())
    check(errlog, test, name, 'gradient_sdf', rel_err(gu, mo.gradient_sdf(st, c.conf, x, create_graph=False)))


@pytest.mark.parametrize('name', ['mlp_w64_eval', 'mlp_w256_eval', 'gridless_w128_train'])
def test_sdf_network_double_backward(name, precision, errlog):
    """d/d params of  <a, sdf> + <B, feat> + <C, grad sdf>  (second order through grad sdf)."""
    from oracle import monosdf_oracle as mo
    c = Case(name)
    m = case_model(c, training=True, precision=precision)
    g = torch.Generator().manual_seed(5)
    P = 777
    x = (torch.rand(P, 3, generator=g) * 2 - 1) * 1.2
    F = c.conf['feature_vector_size']
    ca, cb, cc = torch.randn(P, 1, generator=g), torch.randn(P, F, generator=g) * 0.1, torch.randn(P, 3, generator=g)
    st = oracle_state(c.state, grad=True)
    sdf_o, feat_o, grad_o = mo.get_outputs(st, c.conf, x)
    loss_o = (ca * sdf_o).sum() + (cb * feat_o).sum() + (cc * grad_o).sum()
    names = [n for n in st if n.startswith('implicit_network.lin')]
    g_o = torch.autograd.grad(loss_o, [st[n] for n in names])
    sdf, feat, grad = m.implicit_network.get_outputs(x.cuda())
    loss = (ca.cuda() * sdf).sum() + (cb.cuda() * feat).sum() + (cc.cuda() * grad).sum()
    # the probe is a signed sum of ~50k terms: its error bound scales with the sum of their magnitudes
    scale = ((ca * sdf_o).abs().sum() + (cb * feat_o).abs().sum() + (cc * grad_o).abs().sum()).item()
    assert abs(loss.item() - loss_o.item()) < 1e-4 * max(1.0, scale)
    loss.backward()
    # second-order parameter gradients (the bf16x3 core drops the lo*lo term of every product, 2^-16 relative)
    check_param_grads(errlog, 'sdf_double_backward.' + precision, name, m, dict(zip(names, g_o)), names)


def test_color_network_forward_backward(precision, errlog):
    from oracle import monosdf_oracle as mo
    for name in ['mlp_w64_eval', 'mlp_w256_eval', 'mlp_w64_code_train']:
        c = Case(name)
        m = case_model(c, training=True, precision=precision)
        g = torch.Generator().manual_seed(7)
        n_rays, S = 12, 9
        P = n_rays * S
        F = c.conf['feature_vector_size']
        pts = torch.randn(P, 3, generator=g)
        nrm = torch.randn(P, 3, generator=g)
        feat = torch.randn(P, F, generator=g)
        dirs = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=1)
        idx = torch.arange(n_rays) % 5
        w = torch.randn(P, 3, generator=g)
        st = oracle_state(c.state, grad=True)
        nrm_o, feat_o = nrm.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        dirs_pp = dirs.unsqueeze(1).repeat(1, S, 1).reshape(-1, 3)
        rgb_o = mo.color_network(st, c.conf, pts, nrm_o, dirs_pp, feat_o, idx, True)
        names = [n for n in st if n.startswith('rendering_network.')]
        g_o = torch.autograd.grad((w * rgb_o).sum(), [st[n] for n in names] + [nrm_o, feat_o])
        nrm_g, feat_g = nrm.cuda().requires_grad_(True), feat.cuda().requires_grad_(True)
        rgb = m.rendering_network(pts.cuda(), nrm_g, dirs.cuda(), feat_g, idx.cuda(), if_pixel_input=True,
                                  samples_per_ray=S)['rgb']
        test = 'color_network.' + precision
        check(errlog, test, name, 'rgb', rel_err(rgb, rgb_o))
        (w.cuda() * rgb).sum().backward()
        check_param_grads(errlog, test, name, m, dict(zip(names, g_o)), names)
        check(errlog, test, name, 'd/d normals', rel_err(nrm_g.grad, g_o[-2]))
        check(errlog, test, name, 'd/d features', rel_err(feat_g.grad, g_o[-1]))


def test_camera_rays_kernel():
    """get_camera_params with the pose and with the identity, one launch."""
    from oracle import monosdf_oracle as mo
    from monosdf_amd import ops
    g = torch.Generator().manual_seed(11)
    for n in (1, 63, 1024 + 5):
        uv = torch.rand(1, n, 2, generator=g) * 384
        K = torch.eye(4)[None].clone()
        K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2], K[0, 0, 1] = 300.0, 310.0, 190.5, 188.25, 0.7
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        pose = torch.eye(4)[None].clone()
        pose[0, :3, :3], pose[0, :3, 3] = q, torch.tensor([0.3, -0.2, 0.5])
        d_o, c_o = mo.camera_rays(uv, pose, K)
        dc_o, _ = mo.camera_rays(uv, torch.eye(4)[None], K)
        d, dc, c = ops.camera_rays(uv[0].cuda(), pose[0].cuda(), K[0].cuda())
        assert rel_err(d, d_o[0]) < 1e-6 and rel_err(dc, dc_o[0]) < 1e-6
        assert torch.equal(c.cpu(), c_o.expand(n, 3))
    with pytest.raises(NotImplementedError):
        ops.camera_rays(uv[0].cuda(), torch.zeros(7).cuda(), K[0].cuda())


def test_monosdf_loss_against_reference_fixtures():
    """the fused training loss against values + gradients recorded from the reference class."""
    from test_loss_oracle import GOLDEN, GRAD_KEYS, SCALARS, load_case
    from monosdf_amd.model.loss import MonoSDFLoss
    assert len(GOLDEN) == 5
    for path in GOLDEN:
        out, gt, ref, grads, kw, step = load_case(path)
        leaves = {k: (v.cuda().requires_grad_(True) if k in GRAD_KEYS else v.cuda()) for k, v in out.items()}
        mod = MonoSDFLoss(rgb_loss='torch.nn.L1Loss', **kw)
        mod.step = step
        res = mod(leaves, gt, if_pixel_input=True)            # ground truth arrives on the host, as from the loader
        for k in SCALARS:
            assert abs(res[k].item() - ref[k]) <= 1e-5 * max(1.0, abs(ref[k])), (path, k, res[k].item(), ref[k])
        res['loss'].backward()
        for k in GRAD_KEYS:
            assert rel_err(leaves[k].grad, grads[k]) < TOL, (path, k, rel_err(leaves[k].grad, grads[k]))
        assert mod.step == step + 1
    with pytest.raises(AssertionError):
        mod(leaves, gt, if_pixel_input=False)


def test_compositor_forward_backward(errlog):
    from oracle import monosdf_oracle as mo
    from monosdf_amd import ops
    g = torch.Generator().manual_seed(11)
    for (N, S, white) in [(33, 98, False), (5, 130, True), (7, 17, False)]:
        z = torch.sort(torch.rand(N, S, generator=g) * 3.5, -1)[0]
        sdf = (torch.randn(N, S, generator=g) * 0.2).requires_grad_(True)
        rgb = torch.rand(N, S, 3, generator=g).requires_grad_(True)
        nrm = torch.randn(N, S, 3, generator=g).requires_grad_(True)
        beta = torch.tensor(0.07, requires_grad=True)
        ds = torch.rand(N, 1, generator=g) + 0.5
        bg = [0.9, 0.8, 0.7]
        dens = mo.laplace_density(sdf, beta)
        w_o = mo.transmittance_weights(z, dens)[0]
        rgbv_o = (w_o.unsqueeze(-1) * rgb).sum(1)
        dep_o = ds * ((w_o * z).sum(1, keepdim=True) / (w_o.sum(1, keepdim=True) + 1e-8))
        if white:
            rgbv_o = rgbv_o + (1 - w_o.sum(-1, keepdim=True)) * torch.tensor(bg)
        nm_o = (w_o.unsqueeze(-1) * (nrm / (nrm.norm(2, -1, keepdim=True) + 1e-6))).sum(1)
        c1, c2, c3, c4 = (torch.randn(N, 3, generator=g), torch.randn(N, 1, generator=g),
                          torch.randn(N, 3, generator=g), torch.randn(N, S, generator=g) * 0.1)
        loss_o = (c1 * rgbv_o).sum() + (c2 * dep_o).sum() + (c3 * nm_o).sum() + (c4 * w_o).sum()
        g_o = torch.autograd.grad(loss_o, [sdf, rgb, nrm, beta])
        leaf = lambda t: t.detach().cuda().requires_grad_(True)
        sdf_g, rgb_g, nrm_g, beta_g = leaf(sdf), leaf(rgb), leaf(nrm), leaf(beta)
        w, rgbv, dep, nm = ops.CompositeFunction.apply(z.cuda(), sdf_g, rgb_g, nrm_g, beta_g, ds.cuda(), white, bg)
        case = 'N%d_S%d' % (N, S)
        for k, a, b in [('weights', w, w_o), ('rgb_values', rgbv, rgbv_o), ('depth', dep, dep_o), ('normal_map', nm, nm_o)]:
            check(errlog, 'compositor', case, k, rel_err(a, b))
        loss = (c1.cuda() * rgbv).sum() + (c2.cuda() * dep).sum() + (c3.cuda() * nm).sum() + (c4.cuda() * w).sum()
        loss.backward()
        for k, a, b in zip(['d/d sdf', 'd/d rgb', 'd/d normals', 'd/d beta'], [sdf_g, rgb_g, nrm_g, beta_g], g_o):
            check(errlog, 'compositor', case, k, rel_err(a.grad, b))


def test_hash_encoder_kernels():
    from oracle import hashgrid_oracle as hg
    from monosdf_amd import _lib
    g = torch.Generator().manual_seed(13)
    for ic in [dict(num_levels=16, level_dim=2, logmap=19, base_size=16, end_size=2048),
               dict(num_levels=4, level_dim=2, logmap=10, base_size=16, end_size=64),
               dict(num_levels=6, level_dim=4, logmap=12, base_size=8, end_size=128),
               dict(num_levels=3, level_dim=8, logmap=11, base_size=4, end_size=32)]:
        geo = hg.level_geometry(ic)
        B, L, C = 513, geo['L'], geo['C']
        x = torch.rand(B, 3, generator=g)
        x[:7] = torch.tensor([0.0, 1.0, 0.5])          # cell borders
        x[7:11] = torch.tensor([1.2, 0.5, -0.1])       # out of range -> zeros
        emb = (torch.rand(geo['n_entries'], C, generator=g) - 0.5)
        out_o, dy_o = hg.encode_forward(x, emb, geo, True)
        offs = torch.tensor(geo['offsets'], dtype=torch.int32).cuda()
        xg, eg = x.cuda(), emb.cuda()
        out = torch.empty(L, B, C, device='cuda')
        dy = torch.empty(B, L * 3 * C, device='cuda')
        st = _lib.stream_ptr()
        _lib.call('msdf_hash_encode_forward', _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs), _lib.ptr(out), B, 3, C, L,
                  geo['S'], geo['H'], 1, _lib.ptr(dy), st)
        assert rel_err(out, out_o) < 2e-6 and rel_err(dy, dy_o) < 2e-6
        grad = torch.randn(L, B, C, generator=g)
        grad_g = grad.cuda()           # keep device tensors alive until the kernels have been enqueued
        ge_o = hg.encode_backward_grid(grad, x, geo, geo['n_entries'])
        gi_o = hg.encode_backward_input(grad, dy_o, geo)
        ggi = torch.randn(B, 3, generator=g)
        ggi_g = ggi.cuda()
        # atomic, and the same sums through the binned scatter (per-slice LDS accumulation instead of one atomic per corner)
        r = hash_table_gradients(eg, offs, geo['S'], geo['H'], xg, grad_g, grad_g, ggi_g,
                                 ('atomic', 'atomic_second', 'ws', 'ws_second'))
        ge, gi, gg, g2 = r['atomic'], r['atomic_inputs'], r['atomic_second_grad'], r['atomic_second']
        ge_b, gi_b, gg_b, g2_b = r['ws'], r['ws_inputs'], r['ws_second_grad'], r['ws_second']
        n_entries, ws, nbytes = geo['n_entries'], r['workspace'], r['nbytes']
        assert rel_err(ge, ge_o) < 1e-5 and rel_err(gi, gi_o) < 1e-5
        gg_o = hg.second_backward_grad(ggi, dy_o, geo)
        g2_o = hg.second_backward_embedding(grad, x, ggi, geo, geo['n_entries'])
        assert rel_err(gg, gg_o) < 1e-5 and rel_err(g2, g2_o) < 1e-5
        assert rel_err(ge_b, ge_o) < 1e-5 and rel_err(gi_b, gi_o) < 1e-5
        assert rel_err(gg_b, gg_o) < 1e-5 and rel_err(g2_b, g2_o) < 1e-5
        # ... accumulating into a table that already holds values (the reference's kernels ADD, hashgrid.py:75-76)
        _lib.call('msdf_hash_encode_backward_ws', _lib.ptr(grad_g), _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs),
                  _lib.ptr(g2_b), B, 3, C, L, geo['S'], geo['H'], 0, _lib.ptr(dy), None, n_entries,
                  _lib.ptr(ws), nbytes, st)
        assert rel_err(g2_b, g2_o + ge_o) < 1e-5
        # ... and both gradients in ONE scatter
        grad2 = torch.randn(L, B, C, generator=g)
        grad2_g = grad2.cuda()
        fused = hash_table_gradients(eg, offs, geo['S'], geo['H'], xg, grad_g, grad2_g, ggi_g, ('fused',))['fused']
        want = ge_o + hg.second_backward_embedding(grad2, x, ggi, geo, geo['n_entries'])
        assert rel_err(fused, want) < 1e-5
        # calc_grad_inputs = 2: dy_dx level-major [L, B, 3 C] in all three entry points, same numbers
        out_l, dy_l = torch.empty(L, B, C, device='cuda'), torch.empty(L, B, 3 * C, device='cuda')
        _lib.call('msdf_hash_encode_forward', _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs), _lib.ptr(out_l), B, 3, C, L,
                  geo['S'], geo['H'], 2, _lib.ptr(dy_l), st)
        assert torch.equal(out_l, out) and torch.equal(dy_l.permute(1, 0, 2).reshape(B, L * 3 * C), dy)
        gi_l, gg_l = torch.zeros_like(xg), torch.zeros(L, B, C, device='cuda')
        _lib.call('msdf_hash_encode_backward', _lib.ptr(grad_g), _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs), None,
                  B, 3, C, L, geo['S'], geo['H'], 2, _lib.ptr(dy_l), _lib.ptr(gi_l), st)
        _lib.call('msdf_hash_encode_second_backward_ws', _lib.ptr(grad_g), _lib.ptr(xg), None, _lib.ptr(offs), B, 3, C, L,
                  geo['S'], geo['H'], 2, _lib.ptr(dy_l), _lib.ptr(ggi_g), _lib.ptr(gg_l), None, n_entries, None, 0, st)
        assert torch.equal(gi_l, gi) and torch.equal(gg_l, gg)
        with pytest.raises(RuntimeError):          # a workspace that is too small is refused, not overrun
            _lib.call('msdf_hash_encode_backward_ws', _lib.ptr(grad_g), _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs),
                      _lib.ptr(ge_b), B, 3, C, L, geo['S'], geo['H'], 0, _lib.ptr(dy), None, n_entries,
                      _lib.ptr(ws), nbytes - 1, st)


def test_hash_node_forms_equal_the_reference_order_kernels():
    """The node forms (msdf_hash_node_*) are the reference-order kernels with the elementwise steps around them folded
    in and another tensor layout: through raw ctypes, bit for bit against the reference-order entry points fed with the
    tensor expressions the module would run (x01, the chain-rule factor, the scaled grad_grad_inputs), both layouts;
    msdf_hash_transpose round trip."""
    from oracle import hashgrid_oracle as hg
    from monosdf_amd import _lib
    g = torch.Generator().manual_seed(29)
    for ic in [dict(num_levels=16, level_dim=2, logmap=19, base_size=16, end_size=2048),
               dict(num_levels=3, level_dim=8, logmap=11, base_size=4, end_size=32),
               dict(num_levels=6, level_dim=4, logmap=12, base_size=8, end_size=128)]:
        geo = hg.level_geometry(ic)
        B, L, C = 777, geo['L'], geo['C']
        pitch = ((L * C + 15) // 16) * 16
        df = 1.1
        xw = ((torch.rand(B, 3, generator=g) * 2 - 1) * 1.15).cuda()       # some points leave the cube
        emb = (torch.rand(geo['n_entries'], C, generator=g) - 0.5).cuda()
        offs = torch.tensor(geo['offsets'], dtype=torch.int32).cuda()
        st = _lib.stream_ptr()
        x01 = ((xw / df + 1.0) / 2.0).contiguous()                         # the module's expression, on the device
        out = torch.empty(L, B, C, device='cuda')
        dy = torch.empty(L, B, 3 * C, device='cuda')
        _lib.call('msdf_hash_encode_forward', _lib.ptr(x01), _lib.ptr(emb), _lib.ptr(offs), _lib.ptr(out), B, 3, C, L,
                  geo['S'], geo['H'], 2, _lib.ptr(dy), st)
        for p_ in (0, pitch):
            x01_n = torch.empty(B, 3, device='cuda')
            feat = torch.full((L, B, C) if p_ == 0 else (B, p_), float('nan'), device='cuda')
            dy_n = torch.empty(L, B, 3 * C, device='cuda')
            _lib.call('msdf_hash_node_forward', _lib.ptr(xw), df, _lib.ptr(x01_n), _lib.ptr(emb), _lib.ptr(offs),
                      _lib.ptr(feat), p_, B, C, L, geo['S'], geo['H'], _lib.ptr(dy_n), st)
            assert torch.equal(x01_n, x01) and torch.equal(dy_n, dy)
            want = out if p_ == 0 else torch.nn.functional.pad(out.permute(1, 0, 2).reshape(B, L * C), (0, p_ - L * C))
            assert torch.equal(feat, want)
        # transposes: [L,B,C] -> rows -> [L,B,C], one and two tensors per launch
        rows = torch.full((B, pitch), float('nan'), device='cuda')
        _lib.call('msdf_hash_transpose', _lib.ptr(out), _lib.ptr(rows), None, None, L, B, C, pitch, 1, st)
        assert torch.equal(rows, torch.nn.functional.pad(out.permute(1, 0, 2).reshape(B, L * C), (0, pitch - L * C)))
        back = torch.empty(2, L, B, C, device='cuda')
        rows2 = (rows * 2).contiguous()
        _lib.call('msdf_hash_transpose', _lib.ptr(rows), _lib.ptr(back[0]), _lib.ptr(rows2), _lib.ptr(back[1]), L, B, C,
                  pitch, 0, st)
        assert torch.equal(back[0], out) and torch.equal(back[1], out * 2)
        # input gradient: nrm + (sum g dy) * k, as the tensor expression rounds it
        k = 0.5 / df
        g_rows = torch.randn(B, pitch, generator=g).cuda()
        g_lm = g_rows[:, :L * C].reshape(B, L, C).permute(1, 0, 2).contiguous()
        through = torch.empty(B, 3, device='cuda')
        _lib.call('msdf_hash_encode_backward', _lib.ptr(g_lm), _lib.ptr(x01), _lib.ptr(emb), _lib.ptr(offs), None, B, 3,
                  C, L, geo['S'], geo['H'], 2, _lib.ptr(dy), _lib.ptr(through), st)
        nrm = torch.randn(B, 3, generator=g).cuda()
        want = nrm + through * k
        for p_, gp in ((pitch, g_rows), (0, g_lm)):
            got = nrm.clone()
            _lib.call('msdf_hash_node_input_gradient', _lib.ptr(gp), p_, _lib.ptr(dy), B, C, L, float(k), _lib.ptr(got), st)
            assert torch.equal(got, want)
        # second-order term: gg = [g_a; g_b] * k, grad_grad = sum_d gg dy
        ns = 500
        g_a, g_b = torch.randn(ns, 3, generator=g).cuda(), torch.randn(B - ns, 3, generator=g).cuda()
        gg = torch.cat([g_a, g_b]) * k
        ggrad = torch.empty(L, B, C, device='cuda')
        _lib.call('msdf_hash_encode_second_backward_ws', _lib.ptr(g_lm), _lib.ptr(x01), None, _lib.ptr(offs), B, 3, C, L,
                  geo['S'], geo['H'], 2, _lib.ptr(dy), _lib.ptr(gg), _lib.ptr(ggrad), None, geo['n_entries'], None, 0, st)
        for p_ in (0, pitch):
            gg_n = torch.empty(B, 3, device='cuda')
            gr_n = torch.full((L, B, C) if p_ == 0 else (B, p_), float('nan'), device='cuda')
            _lib.call('msdf_hash_node_second_grad', _lib.ptr(g_a), _lib.ptr(g_b), ns, float(k), _lib.ptr(gg_n), _lib.ptr(dy),
                      _lib.ptr(gr_n), p_, B, C, L, st)
            want = ggrad if p_ == 0 else torch.nn.functional.pad(ggrad.permute(1, 0, 2).reshape(B, L * C), (0, p_ - L * C))
            assert torch.equal(gg_n, gg) and torch.equal(gr_n, want)
        # a missing half is zeros
        gg_n = torch.empty(B, 3, device='cuda')
        gr_n = torch.empty(L, B, C, device='cuda')
        _lib.call('msdf_hash_node_second_grad', _lib.ptr(g_a), None, ns, float(k), _lib.ptr(gg_n), _lib.ptr(dy),
                  _lib.ptr(gr_n), 0, B, C, L, st)
        assert torch.equal(gg_n[:ns], g_a * k) and not gg_n[ns:].any() and not gr_n[:, ns:].any()


def test_hash_encoder_single_feature_levels():
    """level_dim = 1 (the reference's kernels are instantiated for 1, 2, 4, 8): forward with dy_dx and the first-order
    backward, atomic and binned; the second-order kernels need C > 1 in the reference too (hashencoder.cu:431)."""
    from oracle import hashgrid_oracle as hg
    from monosdf_amd import _lib
    g = torch.Generator().manual_seed(17)
    geo = hg.level_geometry(dict(num_levels=5, level_dim=1, logmap=9, base_size=4, end_size=48))
    B, L, C = 301, geo['L'], geo['C']
    x = torch.rand(B, 3, generator=g)
    emb = torch.rand(geo['n_entries'], C, generator=g) - 0.5
    out_o, dy_o = hg.encode_forward(x, emb, geo, True)
    offs = torch.tensor(geo['offsets'], dtype=torch.int32).cuda()
    xg, eg = x.cuda(), emb.cuda()
    out, dy = torch.empty(L, B, C, device='cuda'), torch.empty(B, L * 3 * C, device='cuda')
    st = _lib.stream_ptr()
    _lib.call('msdf_hash_encode_forward', _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs), _lib.ptr(out), B, 3, C, L,
              geo['S'], geo['H'], 1, _lib.ptr(dy), st)
    assert rel_err(out, out_o) < 2e-6 and rel_err(dy, dy_o) < 2e-6
    grad = torch.randn(L, B, C, generator=g)
    grad_g = grad.cuda()
    ge_o = hg.encode_backward_grid(grad, x, geo, geo['n_entries'])
    gi_o = hg.encode_backward_input(grad, dy_o, geo)
    ge, gi = torch.zeros_like(eg), torch.zeros_like(xg)
    _lib.call('msdf_hash_encode_backward', _lib.ptr(grad_g), _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs), _lib.ptr(ge),
              B, 3, C, L, geo['S'], geo['H'], 1, _lib.ptr(dy), _lib.ptr(gi), st)
    assert rel_err(ge, ge_o) < 1e-5 and rel_err(gi, gi_o) < 1e-5
    n_entries = geo['n_entries']
    nbytes = _lib.load().msdf_hash_scatter_workspace_bytes(B, C, L, n_entries)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    ge_b = torch.zeros_like(eg)
    _lib.call('msdf_hash_encode_backward_ws', _lib.ptr(grad_g), _lib.ptr(xg), _lib.ptr(eg), _lib.ptr(offs),
              _lib.ptr(ge_b), B, 3, C, L, geo['S'], geo['H'], 0, _lib.ptr(dy), None, n_entries, _lib.ptr(ws), nbytes, st)
    assert rel_err(ge_b, ge_o) < 1e-5


def test_hash_table_gradient_return_codes():
    """The return-code table of include/monosdf_hip.h (hash-grid block) against the seven table-gradient entry points:
    every refusal gives its documented code, in the documented order, and leaves grad_embeddings (a sentinel) untouched;
    B == 0 leaves the "+=" forms' table alone and zeroes the "=" forms'.  Host-side returns and a memset only: every
    buffer is nevertheless a valid operand of its call (B = 1,061: two place workgroups, the second partial)."""
    import ctypes
    from monosdf_amd import _lib
    from monosdf_amd.hashencoder.hashgrid import HashEncoder
    enc = HashEncoder(input_dim=3, num_levels=4, level_dim=2, base_resolution=4, log2_hashmap_size=13,
                      desired_resolution=64).cuda()
    B, L, C = 1061, 4, 2
    OK, ARG, UNSUPPORTED = 0, 1, 3
    g = torch.Generator(device='cuda').manual_seed(31)
    x = torch.rand(B, 3, device='cuda', generator=g)
    grad, grad2 = torch.randn(2, L, B, C, device='cuda', generator=g)
    gg = torch.randn(B, 3, device='cuda', generator=g)
    offs, n = enc.offsets, enc.embeddings.shape[0]
    S, H = enc.log2_scale, int(enc.base_resolution)
    lib, st = _lib.load(), _lib.stream_ptr()
    nbytes = lib.msdf_hash_scatter_workspace_bytes(B, C, L, n)
    base = dict(grad=grad, grad2=grad2, x=x, offs=offs, table=torch.full((n, C), 7.0, device='cuda'), gg=gg,
                dy=torch.zeros(B, L * 3 * C, device='cuda'), gi=torch.zeros(B, 3, device='cuda'),
                ggrad=torch.zeros(L, B, C, device='cuda'), ws=torch.empty(nbytes, dtype=torch.uint8, device='cuda'),
                B=B, D=3, C=C, pitch=0, n=n, nbytes=nbytes)
    FIRST = ('msdf_hash_encode_backward', 'msdf_hash_encode_backward_ws')
    SECOND = ('msdf_hash_encode_second_backward', 'msdf_hash_encode_second_backward_ws')
    FUSED = ('msdf_hash_encode_backward_fused', 'msdf_hash_encode_backward_fused_out')
    NODE = 'msdf_hash_node_scatter'
    ALL = FIRST + SECOND + FUSED + (NODE,)
    BINNED = (FIRST[1], SECOND[1]) + FUSED + (NODE,)

    def status(name, **kw):
        a = dict(base, **kw)
        p = lambda k: ctypes.c_void_p(a[k]) if isinstance(a[k], int) else _lib.ptr(a[k])      # None -> NULL
        dims = (a['B'], a['D'], a['C'], L, S, H)
        if name in FIRST:
            args = (p('grad'), p('x'), None, p('offs'), p('table')) + dims + (1, p('dy'), p('gi'))
        elif name in SECOND:
            args = (p('grad2'), p('x'), None, p('offs')) + dims + (1, p('dy'), p('gg'), p('ggrad'), p('table'))
        elif name in FUSED:
            args = (p('grad'), p('grad2'), p('x'), p('offs'), p('table')) + dims + (p('gg'),)
        else:
            args = (p('grad'), p('grad2'), a['pitch'], p('x'), p('offs'), p('table'), a['B'], a['C'], L, S, H, p('gg'))
        if name in BINNED:
            args += (a['n'], p('ws'), a['nbytes'])
        return getattr(lib, name)(*args, st)

    def refused(names, code, **kw):
        for name in names:
            assert status(name, **kw) == code, (name, kw.keys(), code)

    # 1, 2: D and C, before any pointer is looked at
    refused(FIRST + SECOND + FUSED, UNSUPPORTED, D=2, table=None)
    refused(ALL, UNSUPPORTED, C=3, table=None)
    refused(SECOND + FUSED + (NODE,), UNSUPPORTED, C=1, B=0)
    # 3: the always-required pointers, before B == 0
    for k in ('table', 'grad', 'grad2', 'gg'):
        refused(FUSED, ARG, B=0, **{k: None})
    refused((NODE,), ARG, B=0, table=None)
    # 4: no points -- "+=" forms leave the table alone, with every other pointer NULL where the contract allows it
    none = dict(grad=None, grad2=None, x=None, offs=None, gg=None, dy=None, gi=None, ggrad=None, ws=None, nbytes=0)
    refused(FIRST + SECOND, OK, B=0, **none)
    refused(FUSED[:1], OK, B=0, x=None, offs=None, ws=None, nbytes=0)
    # 5: a NULL operand of a requested output; the pitch of point-major rows
    for names, k in ((FIRST, 'grad'), (FIRST, 'x'), (FIRST, 'offs'), (FIRST, 'dy'), (FIRST, 'gi'), (SECOND, 'grad2'),
                     (SECOND, 'x'), (SECOND, 'offs'), (SECOND, 'gg'), (SECOND, 'dy'), (FUSED, 'x'), (FUSED, 'offs'),
                     ((NODE,), 'grad'), ((NODE,), 'grad2'), ((NODE,), 'gg'), ((NODE,), 'x'), ((NODE,), 'offs')):
        refused(names, ARG, **{k: None})
    refused((NODE,), ARG, pitch=L * C - 1)
    # 6: 2^31 floats of table, 2^31 corner records -- before the workspace is looked at
    refused(BINNED, UNSUPPORTED, n=2 ** 30, ws=None)
    refused(BINNED, UNSUPPORTED, B=2 ** 26, ws=None)
    # 7: the workspace
    refused(BINNED, ARG, ws=None)
    refused(BINNED, ARG, nbytes=nbytes - 1)
    refused(BINNED, ARG, ws=base['ws'].data_ptr() + 4)
    assert torch.equal(base['table'], torch.full((n, C), 7.0, device='cuda'))
    # 4 again, the "=" forms: an all-zero table (the node form with the NULL operands of empty tensors)
    for name, kw in ((FUSED[1], {}), (NODE, none)):
        table = torch.full((n, C), 7.0, device='cuda')
        assert status(name, B=0, table=table, **kw) == OK and not table.any(), name


@pytest.mark.parametrize('name', [n for n in ALL_CASES if 'eval' in n and 'image' not in n])
def test_sampler_against_golden(name, errlog):
    """get_z_vals alone against the reference's z_vals: 1 to 5 rounds, converged and not (every exit of the
    loop, ray_sampler.py:125,179-207).  z is compared as a fraction of the sampler's far bound (3.85)."""
    c = Case(name)
    m = case_model(c, precision='fp32')
    rays = _cuda(c.inputs)
    z, _ = m.ray_sampler.get_z_vals(rays['ray_dirs'], rays['ray_cam_loc'], m)
    assert m.ray_sampler.last_rounds == c.rounds
    assert z.shape == c.out['z_vals'].shape
    assert torch.all(z[:, 1:] >= z[:, :-1])
    check(errlog, 'sampler_golden', name, 'z_vals', (z.cpu() - c.out['z_vals']).abs().max().item() / 3.85)


PER_SAMPLE = ('weights', 'sdf', 'z_vals', 'depth_vals', 'rgb')


@pytest.mark.parametrize('name', ALL_CASES)
def test_full_forward_against_golden(name, precision, errlog):
    c = Case(name)
    m = case_model(c, precision=precision)
    out = run_pass(m, c.inputs, c.indices, c.noise, c.pixel)
    assert set(out) == set(c.out)
    assert m.ray_sampler.last_rounds == c.rounds
    for k, ref in c.out.items():
        assert out[k].shape == ref.shape, k
        if precision == 'bf16x3' and c.rounds > 1 and k in PER_SAMPLE:
            # opt-in core, multi-round case: its SDF values sit 1.2e-5 ... 1.4e-5 from the reference's (13 x the fp32
            # core), enough to move single samples across the surface at beta <= 0.01; the per-sample tensors would need
            # bars of 10-30 %, so this core is held to the per-ray composites (rgb_values, depth_values, normal_map) there
            continue
        check(errlog, 'forward_golden.' + precision, name, k, rel_err(out[k], ref))


@pytest.mark.parametrize('name', [n for n in ALL_CASES if 'train' in n])
def test_full_gradients_against_golden(name, precision, errlog):
    from oracle import monosdf_oracle as mo
    c = Case(name)
    m = case_model(c, precision=precision)
    out = run_pass(m, c.inputs, c.indices, c.noise, c.pixel)
    loss = mo.probe_loss(out)
    test = 'gradients_golden.' + precision
    check(errlog, test, name, 'loss', abs(loss.item() - c.loss) / max(1.0, abs(c.loss)))
    loss.backward()
    check_param_grads(errlog, test, name, m, c.grads, list(c.grads))
    params = dict(m.named_parameters())
    for n, ref in c.gdig.items():
        d = digest(params[n].grad)
        check(errlog, test, name, n + '(digest)', abs(d[0] - ref[0]).item() / (ref[1].item() + 1e-9))
    for n, ref in c.gtab.items():
        # table gradient at the full table size (16 levels, 2^19 entries per hashed level): which level received what,
        # where every contribution landed (+-1 projections), and the largest entries by index
        from oracle import synth
        got = synth.table_fingerprint(params[n].grad, c.state[n.replace('embeddings', 'offsets')].numpy())
        rms = float(np.sqrt(ref['level_sq'].double().sum()))
        check(errlog, test, name, n + '(level |g|)',
              float(np.abs(got['level_abs'] - ref['level_abs'].numpy()).max() / ref['level_abs'].max()))
        check(errlog, test, name, n + '(level g^2)',
              float(np.abs(got['level_sq'] - ref['level_sq'].numpy()).max() / ref['level_sq'].max()))
        check(errlog, test, name, n + '(projections)', float(np.abs(got['proj'] - ref['proj'].numpy()).max() / rms))
        flat = params[n].grad.detach().reshape(-1).cpu().double().numpy()
        top = ref['top_idx'].numpy()
        check(errlog, test, name, n + '(largest entries)',
              float(np.abs(flat[top] - ref['top_val'].numpy()).max() / np.abs(ref['top_val'].numpy()).max()))


def test_full_image_render_chunked(errlog):
    """configs[3] at reduced size: chunked eval render == oracle's chunked render (one pose, uv grid)."""
    from oracle import monosdf_oracle as mo
    from monosdf_amd.utils import render
    c = Case('mlp_w64_image_eval')
    m = case_model(c, precision='fp32')
    n_side = 12
    ys, xs = torch.meshgrid(torch.arange(n_side), torch.arange(n_side), indexing='ij')
    uv = torch.stack([xs.flatten() * 30.0 + 10.0, ys.flatten() * 30.0 + 12.0], -1)[None].float()
    inputs = {'uv': uv, 'pose': c.inputs['pose'], 'intrinsics': c.inputs['intrinsics']}
    total = n_side * n_side
    ref = mo.render_image(c.state, c.conf, inputs, c.indices, total, split_n_pixels=50)
    out = render.render_image(m, _cuda(inputs), c.indices.cuda(), total, split_n_pixels=50)
    for k in ref:
        assert out[k].shape == ref[k].shape
        check(errlog, 'render_image', 'mlp_w64_image_eval_12x12', k, rel_err(out[k], ref[k]))


def test_sdf_volume_coarse_to_fine(golden_dir, errlog):
    """configs[4] at reduced size (one 128^3 block) against the volume the REFERENCE's plots.get_surface_sliding
    handed to marching cubes (tests/golden/volume_w64_128.npz, oracle/make_golden_volume.py): every 4th voxel, one
    full plane through the surface, the moments of the whole array and the number of voxels inside the finest
    threshold.  A voxel whose coarse |sdf| sits within rounding of a refinement threshold may be refined on one
    side and not on the other: those are counted, not compared."""
    from test_oracle_golden import volume_fixture, volume_moments
    from monosdf_amd.utils import render
    z, spec, conf, state = volume_fixture(golden_dir)
    c = Case('mlp_w64_eval')
    assert spec['width'] == 64 and spec['jitter'] == c.spec['jitter']
    m = case_model(c, precision='fp32')
    lo, hi = spec['grid_boundary']
    with torch.no_grad():
        fn = lambda p: m.implicit_network(p)[:, 0]
        blocks = list(render.sdf_volume(fn, resolution=spec['resolution'], grid_boundary=(lo, hi), shard=False))
    assert len(blocks) == 1
    origin, spacing, vol = blocks[0]
    assert np.allclose(spacing, z['spacing'], rtol=1e-6)
    k = spec['stride']
    scale = np.abs(z['sub']).max()
    for name, got, ref in (('every 4th voxel', vol[::k, ::k, ::k], z['sub']),
                           ('plane z=mid', vol[:, :, vol.shape[0] // 2], z['plane'])):
        diff = np.abs(got - ref) / scale
        flipped = float((diff > 1e-4).mean())              # refined here, not there (or the reverse)
        check(errlog, 'sdf_volume', 'volume_w64_128', name + ': threshold voxels', flipped, 1e-3)
        check(errlog, 'sdf_volume', 'volume_w64_128', name, float(diff[diff <= 1e-4].max()))
    mom, ref_mom = volume_moments(vol), z['moments']
    check(errlog, 'sdf_volume', 'volume_w64_128', 'moments', float(np.abs(mom - ref_mom).max() / np.abs(ref_mom).max()))
    thr = 2 * (hi - lo) / spec['resolution'] * 8 / 8
    near = int((np.abs(vol) < thr).sum())
    assert abs(near - int(z['near_count'])) <= 1e-3 * int(z['near_count']), (near, int(z['near_count']))


def test_configs0_uniform_sampler_plumbing(golden_dir, errlog):
    """BASELINE.json configs[0] (512 rays x 64 uniform samples, 8x256) through the HIP sub-modules, composed the way
    MonoSDFNetwork.forward composes them (reference network.py:532-562,603-611), against the fixture recorded from
    the reference's own UniformSampler + ImplicitNetwork + RenderingNetwork + volume_rendering."""
    from test_oracle_golden import plumbing_fixture
    from monosdf_amd.model.ray_sampler import UniformSampler
    z, spec, conf, state, rays = plumbing_fixture(golden_dir)
    m = build_model(conf, state, training=False)
    r = _cuda(rays)
    dirs, cam = r['ray_dirs'], r['ray_cam_loc']
    us = UniformSampler(conf['scene_bounding_sphere'], 0.0, spec['n_samples'], take_sphere_intersection=True)
    zv, near, far = us.get_z_vals(dirs, cam, m)
    n, s = zv.shape
    assert (n, s) == (512, 64)
    pts = (cam.unsqueeze(1) + zv.unsqueeze(2) * dirs.unsqueeze(1)).reshape(-1, 3)
    dirs_flat = dirs.unsqueeze(1).repeat(1, s, 1).reshape(-1, 3)
    sdf, feat, grad = m.implicit_network.get_outputs(pts)
    rgb = m.rendering_network(pts, grad, dirs_flat, feat, torch.arange(n).cuda())['rgb'].reshape(-1, s, 3)
    w = m.volume_rendering(zv, sdf)
    rgb_values = torch.sum(w.unsqueeze(-1) * rgb, 1)
    depth = r['ray_dirs_tmp'][:, 2:] * (torch.sum(w * zv, 1, keepdims=True) / (w.sum(dim=1, keepdims=True) + 1e-8))
    normals = grad / (grad.norm(2, -1, keepdim=True) + 1e-6)
    nmap = torch.sum(w.unsqueeze(-1) * normals.reshape(-1, s, 3), 1)
    nmap = (r['ray_pose'][:, :3, :3].transpose(1, 2) @ nmap.unsqueeze(-1)).squeeze(-1)
    t = lambda k: torch.from_numpy(z[k])
    case = 'plumbing_uniform64'
    check(errlog, 'configs0', case, 'z_vals', (zv.cpu() - t('out.z_vals')).abs().max().item() / 3.85)
    check(errlog, 'configs0', case, 'far', (far.cpu() - t('out.far')).abs().max().item() / 3.85)
    for k, v in (('rgb_values', rgb_values), ('depth_values', depth), ('normal_map', nmap)):
        check(errlog, 'configs0', case, k, rel_err(v, t('out.' + k)))
    for k, v in (('sdf', sdf.reshape(n, s)), ('weights', w), ('rgb', rgb)):
        check(errlog, 'configs0', case, k, rel_err(v[::8], t('sub.' + k)))


def test_fused_probe_loss_matches_torch_autograd():
    from oracle import monosdf_oracle as mo
    from monosdf_amd import ops
    g = torch.Generator().manual_seed(21)
    N = 300
    vals = {'rgb_values': torch.rand(N, 3, generator=g) - 0.3, 'normal_map': torch.randn(N, 3, generator=g),
            'depth_values': torch.rand(N, 1, generator=g) + 0.5, 'grad_theta': torch.randn(2 * N, 3, generator=g),
            'grad_theta_nei': torch.randn(2 * N, 3, generator=g)}
    ref_in = {k: v.clone().requires_grad_(True) for k, v in vals.items()}
    l_ref = mo.probe_loss(ref_in)
    g_ref = torch.autograd.grad(l_ref, list(ref_in.values()))
    gpu_in = {k: v.cuda().requires_grad_(True) for k, v in vals.items()}
    l = ops.probe_loss(gpu_in)
    assert abs(l.item() - l_ref.item()) < 1e-5 * abs(l_ref.item())
    (2.0 * l).backward()
    for (k, t), gr in zip(gpu_in.items(), g_ref):
        assert rel_err(t.grad, 2.0 * gr) < 1e-5, k


@pytest.mark.parametrize('n_rays', [1, 5, 67])
def test_ragged_batches_against_oracle(n_rays, precision, errlog):
    """Batches that fill neither a wave (16 points) nor a workgroup (64): 1, 5 and 67 rays, training mode,
    forward + backward against the oracle on the same rays and the same random draws."""
    from oracle import config, monosdf_oracle as mo, synth
    conf = config.mlp_config(width=64, depth=8)
    state = synth.make_state(conf, seed=3, jitter=0.3)
    rays = synth.make_rays(n_rays, seed=4, random_pose=True)
    noise = synth.make_noise(conf, n_rays, 128, seed=5)
    model = build_model(conf, state, precision=precision)
    idx = torch.arange(n_rays)
    out = run_pass(model, rays, idx, noise, loss=mo.probe_loss)
    st = oracle_state(state, grad=True)
    ref = mo.render(st, conf, rays, idx, True, True, noise)
    mo.probe_loss(ref).backward()
    test, case = 'ragged.' + precision, '%d_rays' % n_rays
    for k in ('rgb_values', 'depth_values', 'normal_map', 'grad_theta', 'weights', 'sdf'):
        assert out[k].shape == ref[k].shape, k
        check(errlog, test, case, k, rel_err(out[k], ref[k]))
    names = ['implicit_network.lin4.weight_v', 'implicit_network.lin0.bias', 'rendering_network.lin1.weight_g',
             'density.beta']
    check_param_grads(errlog, test, case, model, {n: st[n].grad for n in names}, names)


def test_ddp_wrapped_training_step_matches_plain():
    """The reference wraps the model in DistributedDataParallel(device_ids=[rank], broadcast_buffers=False,
    find_unused_parameters=True) (monosdf_train.py:228-229): one RCCL-backed step (world size 1) must give the
    gradients of the unwrapped model -- the custom autograd nodes and the side stream sit below DDP's hooks."""
    import os
    import torch.distributed as dist
    from monosdf_amd.model.loss import MonoSDFLoss
    c = Case('mlp_w64_train')
    plain = case_model(c, training=True, precision='fp32')
    wrapped_inner = case_model(c, training=True, precision='fp32')
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29533')
    created = not dist.is_initialized()
    if created:
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        ddp = torch.nn.parallel.DistributedDataParallel(wrapped_inner, device_ids=[0], broadcast_buffers=False,
                                                        find_unused_parameters=True)
        gt = None
        losses = []
        for m in (plain, ddp):
            inner = m.module if hasattr(m, 'module') else m
            inner._noise = _cuda(c.noise)
            out = m(_cuda(c.inputs), c.indices.cuda(), if_pixel_input=c.pixel)
            N = out['rgb_values'].shape[0]
            if gt is None:
                g = torch.Generator().manual_seed(1)
                gt = {'rgb': torch.rand(1, N, 3, generator=g), 'depth': torch.rand(1, N, 1, generator=g) * 0.04,
                      'normal': torch.randn(1, N, 3, generator=g), 'mask': torch.ones(1, N, 1)}
            loss = MonoSDFLoss(rgb_loss='torch.nn.L1Loss', eikonal_weight=0.05)(out, gt, if_pixel_input=True)['loss']
            loss.backward()
            losses.append(loss.item())
        assert losses[0] == losses[1]
        gp = dict(plain.named_parameters())
        for name, p in wrapped_inner.named_parameters():
            assert (p.grad is None) == (gp[name].grad is None), name
            if p.grad is not None:
                assert torch.equal(p.grad, gp[name].grad), name
    finally:
        if created:
            dist.destroy_process_group()
