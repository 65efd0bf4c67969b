"""The SDF node's permuted evaluation order and its reuse of the hidden activations the sampler's first round computed
(ops.SdfReuse, msdf_sdf_forward_save, msdf_fg_args_t.n_reuse): bit-identical with the reuse on and off, in every
speculation mode, and equal to the oracle at the parity tolerance.

Ray counts: 2 (32 N = 64: exactly one reused workgroup), 3 (n_reuse = 64 and a straddling workgroup that is
recomputed), 5 and 16 (several reused workgroups, a partly filled last one).  Networks: 64 wide with and without the
skip layer, 256 wide (the kernels' specialised K = 16 / 17 products)."""
import functools

import pytest
import torch

from harness import assert_same_step, oracle_state, run_pass, shared_weights, step_record, switched, to_device
from helpers import check, rel_err
from reuse_cases import N_EVAL, N_EXTRA, NETS, OUT_KEYS, conf_state as _conf_state, inputs as _inputs, model as _model

pytestmark = pytest.mark.gpu

RAYS = (2, 3, 5, 16)
CASES = [(net, n) for net in sorted(NETS) for n in RAYS]


@functools.lru_cache(maxsize=None)
def _run(net, n, reuse_on, beta=0.1, speculate=True, table=False):
    """One training step of a fresh model: outputs, loss, parameter gradients, rounds, repeated passes."""
    from monosdf_amd import ops
    from oracle import monosdf_oracle as mo
    rays, noise = _inputs(net, n, beta, table)
    m = _model(net, beta)
    m.speculate_rounds = speculate
    with switched(ops, 'REUSE_SAMPLER_H', reuse_on):
        out = run_pass(m, rays, torch.arange(n), noise)
        loss = mo.probe_loss(out)
        loss.backward()
    torch.cuda.synchronize()
    return step_record(m, out, loss, OUT_KEYS)


@pytest.mark.parametrize('net,n', CASES)
def test_reuse_on_and_off_are_bit_identical(net, n):
    """(a) every entry of the output dict, the loss and every parameter gradient."""
    on, off = _run(net, n, True), _run(net, n, False)
    assert on['rounds'] == off['rounds'] == 1 and on['repeats'] == 0
    assert len(on['grads']) >= 20
    assert_same_step(on, off)


@pytest.mark.parametrize('net,n', CASES)
def test_outputs_agree_with_the_oracle(net, n, errlog):
    """(f) at the parity tolerance of the full-forward tests (1e-4 of the tensor's largest magnitude)."""
    from oracle import monosdf_oracle as mo
    conf, state = _conf_state(net, 0.1)
    rays, noise = _inputs(net, n, 0.1, False)
    ref = mo.render(oracle_state(state), conf, rays, torch.arange(n), True, True, noise)
    out = _run(net, n, True)['out']
    for k in ('rgb_values', 'depth_values', 'normal_map', 'grad_theta', 'weights', 'sdf'):
        check(errlog, 'sdf_reuse', '%s.%d' % (net, n), k, rel_err(out[k], ref[k].detach()))


@pytest.mark.parametrize('net,n', CASES)
def test_two_round_state_in_every_speculation_mode(net, n):
    """(d) a state that needs more than one round: one round speculated (which saves activations the node must then
    NOT use) and the pass repeated; the rounds decided one by one (the first still saves); all rounds enqueued (nothing
    saved).  The three agree bit for bit with each other and with the reuse switched off."""
    beta = 0.01
    hist = _run(net, n, True, beta, True, True)
    assert hist['rounds'] == 2 and hist['repeats'] == 1
    sync, every = _run(net, n, True, beta, False, True), _run(net, n, True, beta, 'all', True)
    assert sync['rounds'] == every['rounds'] == hist['rounds'] and sync['repeats'] == every['repeats'] == 0
    assert_same_step(hist, sync)
    assert_same_step(hist, every)
    assert_same_step(hist, _run(net, n, False, beta, True, True))


@pytest.mark.parametrize('net,n', CASES)
def test_saved_rows_coordinates_and_skipped_products(net, n):
    """(b) the saving forward kernel returns msdf_sdf_forward_lm's sdf; (c) the rows it saves are the rows the forward
    + gradient kernel writes for the same points when it computes everything; (e) those points' coordinates in x_all
    are the first round's; the row map is the stated permutation; the reusing launch leaves the workspace the computing
    launch leaves; and the reused workgroups really read the staged rows (a row overwritten behind the sampler shows in
    the node's output, a row of a recomputed workgroup does not)."""
    from monosdf_amd import ops, plan as planlib
    from monosdf_amd.model.ray_sampler import ErrorBoundSampler
    rays, noise = _inputs(net, n, 0.1, False)
    m = _model(net, 0.1)
    m._noise = to_device(noise)
    dev = torch.device('cuda', torch.cuda.current_device())
    sdfnet, smp = m.implicit_network, m.ray_sampler
    S = smp.N_samples + N_EXTRA + 2
    P, n_ext = n * S + 4 * n, n * N_EXTRA
    d, o = rays['ray_dirs'].cuda().contiguous(), rays['ray_cam_loc'].cuda().contiguous()
    with shared_weights(sdfnet, dev):
        fused, _, _, wpack, bpack = sdfnet.packed(dev)
        beta0 = ops.effective_beta(m.density.beta, m.density.beta_min_f)
        reuse = sdfnet.sdf_reuse(dev, n, S, N_EXTRA, 4 * n, True)
        assert reuse.n_reuse == n_ext // 64 * 64 and reuse.P == P
        z_vals, _, x_all = smp.sample(d, o, m, speculate=1, beta0=beta0, sdf_reuse=reuse)
        assert smp.confirm() and smp.last_rounds == 1
        assert int(reuse.flags[1]) == 0 and int(reuse.h_saved[0]) == 1
        # the row map: a permutation, the eikonal block in place, a ray's other samples in sorted order
        rm = reuse.row_map.long()
        assert sorted(rm.tolist()) == list(range(P))
        assert torch.equal(rm[n * S:], torch.arange(n * S, P, device=dev))
        other = rm[n_ext:n * S].view(n, S - N_EXTRA)
        assert bool((other[:, 1:] > other[:, :-1]).all())
        assert torch.equal(other // S, torch.arange(n, device=dev)[:, None].expand(n, S - N_EXTRA))
        # (e) the extra rows are the first round's points, bit for bit
        cols = noise['extra_idx'].cuda()
        pts = reuse.round_pts
        assert torch.equal(x_all[rm[:n_ext]], pts.view(n, N_EVAL, 3)[:, cols].reshape(n_ext, 3))
        # (b)
        radius, scale = sdfnet.sdf_bounding_sphere, sdfnet.sphere_scale
        plain = ops.sdf_forward_nograd(fused, wpack, bpack, pts, None, radius, scale)
        scratch = sdfnet.sdf_reuse(dev, n, S, N_EXTRA, 4 * n, True)
        scratch.h_saved.zero_()
        slots = ErrorBoundSampler.column_slots(noise['extra_idx'], N_EVAL).cuda()
        saving = ops.sdf_forward_save(fused, wpack, bpack, pts, radius, scale, None, scratch, slots, N_EVAL)
        assert torch.equal(plain, saving) and int(scratch.h_saved[0]) == 1
        # (c) reuse switched off for this launch: the node writes every row of H itself, at the points' own rows
        staged = reuse.stage.clone()
        n_reuse, reuse.n_reuse = reuse.n_reuse, 0
        sdf_all, feat, nrm, _ = sdfnet.evaluate(x_all, n * S, n * S, save=True, split=n * S, reuse=reuse)
        woff, _ = planlib.sdf_workspace(fused.mp, reuse.P_pad)
        plan = fused.plan
        assert reuse.stage_pad == (n_ext + 63) // 64 * 64
        for l in range(plan.n_layers - 1):
            L = plan.layer[l]
            w = 16 * L.ot
            lo = woff['H'] + L.hpre * reuse.P_pad
            H = reuse.ws[lo:lo + P * w].view(P, w)[rm[:n_ext]]
            so = L.hpre * reuse.stage_pad
            assert torch.equal(staged[so:so + n_ext * w].view(n_ext, w), H), l
            assert torch.equal(scratch.stage[so:so + n_ext * w].view(n_ext, w), H), l
        ws_computed = reuse.ws.clone()
        # the reusing launch leaves the same workspace (H moved from the staged rows, PM and IN0 computed) ...
        reuse2 = sdfnet.sdf_reuse(dev, n, S, N_EXTRA, 4 * n, True)
        z2, _, x2 = smp.sample(d, o, m, speculate=1, beta0=beta0, sdf_reuse=reuse2)
        assert smp.confirm() and torch.equal(x2, x_all) and torch.equal(reuse2.row_map, reuse.row_map)
        sdf2, feat2, nrm2, _ = sdfnet.evaluate(x2, n * S, n * S, save=True, split=n * S, reuse=reuse2)
        for k, nxt in (('H', 'PM'), ('PM', 'IN0'), ('IN0', 'QB')):       # every row of the three, padded tail included
            assert torch.equal(reuse2.ws[woff[k]:woff[nxt]], ws_computed[woff[k]:woff[nxt]]), k
        assert torch.equal(sdf2, sdf_all) and torch.equal(feat2, feat) and torch.equal(nrm2, nrm)
        # ... and really takes the staged rows: zero the last hidden activation of grid row 0 (reused) and of the first
        # row behind the reused workgroups (staged, but computed by the node) behind a fresh sampler pass
        reuse3 = sdfnet.sdf_reuse(dev, n, S, N_EXTRA, 4 * n, True)
        smp.sample(d, o, m, speculate=1, beta0=beta0, sdf_reuse=reuse3)
        assert smp.confirm()
        L = plan.layer[plan.n_layers - 2]
        so = L.hpre * reuse3.stage_pad
        for r in (0, n_reuse):
            if r < n_ext:
                reuse3.stage[so + r * 16 * L.ot:so + (r + 1) * 16 * L.ot] = 0.0
        sdf3, feat3, nrm3, _ = sdfnet.evaluate(x_all, n * S, n * S, save=True, split=n * S, reuse=reuse3)
        # (the features: sdf and normal of a point outside the bounding sphere are the clamp's either way)
        changed = (feat3 != feat).any(dim=1).nonzero().flatten().tolist()
        assert changed == [int(rm[0])]
        same = torch.ones(n * S, dtype=torch.bool, device=dev)
        same[rm[0]] = False
        assert torch.equal(sdf3[same], sdf_all[same]) and torch.equal(nrm3[same], nrm[same])
