"""The dispatch rotation of the SDF forward + gradient kernel (msdf_fg_args_t.wg_first, ops.FG_REUSE_LAST): block b
evaluates workgroup (b + wg_first) mod n_wg, so that the workgroups that reuse the sampler's activations -- the short
ones -- start last.  Only the order in which workgroups start may change: outputs, loss, every parameter gradient and
the workspace (H, PM, IN0) are bit-identical with the rotation on and off and for any wg_first.

Ray counts (P = 102 N points, 64 per workgroup, n_reuse = floor(32 N / 64) 64), the smallest at which the index
arithmetic can go wrong: 2 (4 workgroups, one reusing, wg_first = 1, the partly filled last one holds the eikonal
rows), 3 (n_reuse = 64 and the workgroup behind it straddles dense-set and other rows), 6 (10 workgroups, 3 reusing,
the last one mixes rows with and without features: the workgroup-uniform feature test and the per-point guard under a
rotated index).  Networks: 64 and 256 wide (the kernels' specialised K = 16 / 17 products), both with the skip layer."""
import ctypes as C
import functools

import pytest
import torch

from harness import assert_same_step, run_pass, shared_weights, step_record, switched, to_device
from reuse_cases import N_EXTRA, OUT_KEYS, inputs as _inputs, model as _model

pytestmark = pytest.mark.gpu

NETS = ('w256_skip', 'w64_skip')
RAYS = (2, 3, 6)
CASES = [(net, n) for net in NETS for n in RAYS]
WS_BLOCKS = (('H', 'PM'), ('PM', 'IN0'), ('IN0', 'QB'))       # a block of the workspace and the one behind it


class _Recorder:
    """Records the argument struct of every msdf_sdf_fwd_grad launch (a copy) while active."""

    def __init__(self):
        self.fg = []

    def __enter__(self):
        from monosdf_amd import _lib
        self._lib, self._call = _lib, _lib.call

        def call(name, *args):
            if name == 'msdf_sdf_fwd_grad':
                a = _lib.FgArgs()
                C.memmove(C.byref(a), C.byref(args[1]._obj), C.sizeof(_lib.FgArgs))
                self.fg.append(a)
            return self._call(name, *args)
        _lib.call = call
        return self

    def __exit__(self, *exc):
        self._lib.call = self._call


@functools.lru_cache(maxsize=None)
def _step(net, n, reuse_last, beta=0.1, table=False):
    """One training step of a fresh model: outputs, loss, parameter gradients, the SDF node's workspace, the rounds and
    the rotation its forward + gradient launch was given."""
    from monosdf_amd import ops, plan as planlib
    from oracle import monosdf_oracle as mo
    rays, noise = _inputs(net, n, beta, table)
    m = _model(net, beta)
    m.speculate_rounds = True
    sdfnet = m.implicit_network
    made, make = [], sdfnet.sdf_reuse
    sdfnet.sdf_reuse = lambda *a, **k: made.append(make(*a, **k)) or made[-1]
    with switched(ops, 'FG_REUSE_LAST', reuse_last), _Recorder() as rec:
        out = run_pass(m, rays, torch.arange(n), noise)
        loss = mo.probe_loss(out)
        loss.backward()
    torch.cuda.synchronize()
    reuse = made[-1]                    # the pass that was kept
    woff, _ = planlib.sdf_workspace(reuse.mlp.mp, reuse.P_pad)
    return dict(step_record(m, out, loss, OUT_KEYS),
                ws={k: reuse.ws[woff[k]:woff[nxt]].clone() for k, nxt in WS_BLOCKS},
                wg_first=[a.wg_first for a in rec.fg], n_reuse=reuse.n_reuse, n_wg=reuse.P_pad // 64,
                taken=int(reuse.flags[1]) == 0 and int(reuse.h_saved[0]) == 1)


def _assert_same_step(a, b):
    assert_same_step(a, b)
    assert len(a['grads']) >= 20
    for k in a['ws']:
        assert a['ws'][k].numel() > 0 and torch.equal(a['ws'][k], b['ws'][k]), k


def _assert_geometry(r, n):
    assert r['n_wg'] == (102 * n + 63) // 64 and r['n_reuse'] == 32 * n // 64 * 64 > 0


@pytest.mark.parametrize('net,n', CASES)
def test_one_round_step_rotated_and_not(net, n):
    """The reuse is taken (one sampler round): the rotated launch starts the reusing workgroups last."""
    on, off = _step(net, n, True), _step(net, n, False)
    for r in (on, off):
        _assert_geometry(r, n)
        assert r['rounds'] == 1 and r['repeats'] == 0 and r['taken']
    assert on['wg_first'] == [on['n_reuse'] // 64] and off['wg_first'] == [0]
    _assert_same_step(on, off)


@pytest.mark.parametrize('net,n', CASES)
def test_two_round_step_rotated_and_not(net, n):
    """A state that needs two rounds (one speculated, the pass repeated): the reuse is armed but not taken, every
    workgroup computes everything, and the rotation still changes nothing."""
    on, off = _step(net, n, True, 0.01, True), _step(net, n, False, 0.01, True)
    for r in (on, off):
        _assert_geometry(r, n)
        assert r['rounds'] == 2 and r['repeats'] == 1 and not r['taken']
    assert on['wg_first'] == [on['n_reuse'] // 64] * 2 and off['wg_first'] == [0] * 2
    _assert_same_step(on, off)


def test_entry_point_with_every_rotation():
    """msdf_sdf_fwd_grad itself at N = 6 in the one-round state, on the buffers of a launch the node made: wg_first of 0,
    1 and n_wg - 1 write the same outputs and workspace; -1 and n_wg are MSDF_ERR_ARG; a non-zero value with a bf16 plan
    is MSDF_ERR_UNSUPPORTED (nothing is launched)."""
    from monosdf_amd import _lib, ops, plan as planlib
    net, n = 'w256_skip', 6
    rays, noise = _inputs(net, n, 0.1, False)
    m = _model(net, 0.1)
    m._noise = to_device(noise)
    dev = torch.device('cuda', torch.cuda.current_device())
    sdfnet, smp = m.implicit_network, m.ray_sampler
    S = smp.N_samples + N_EXTRA + 2
    P, n_wg = n * S + 4 * n, (n * S + 4 * n + 63) // 64
    d, o = rays['ray_dirs'].cuda().contiguous(), rays['ray_cam_loc'].cuda().contiguous()
    with shared_weights(sdfnet, dev):
        fused = sdfnet.packed(dev)[0]
        beta0 = ops.effective_beta(m.density.beta, m.density.beta_min_f)
        reuse = sdfnet.sdf_reuse(dev, n, S, N_EXTRA, 4 * n, True)
        _, _, x_all = smp.sample(d, o, m, speculate=1, beta0=beta0, sdf_reuse=reuse)
        assert smp.confirm() and smp.last_rounds == 1
        assert int(reuse.flags[1]) == 0 and int(reuse.h_saved[0]) == 1 and reuse.n_reuse == 192 and reuse.P == P
        with _Recorder() as rec:
            held = sdfnet.evaluate(x_all, n * S, n * S, save=True, split=n * S, reuse=reuse)   # keeps the buffers alive
        torch.cuda.synchronize()
        (a,) = rec.fg
        assert a.wg_first == 3 and a.P_pad == 64 * n_wg == 640 and a.n_feat == n * S == 588
        sdf_node, feat_node, nrm_node, nrm_b_node = [t.detach().clone() for t in held]
        woff, _ = planlib.sdf_workspace(fused.mp, reuse.P_pad)
        fn = _lib.load().msdf_sdf_fwd_grad
        stream = _lib.stream_ptr()
        results = {}
        for w in (0, 1, n_wg - 1):
            # every buffer the launch writes is overwritten first: what is compared is what this launch wrote
            for t in held:
                t.detach().fill_(-7.0)
            reuse.ws[woff['H']:woff['QB']].fill_(-7.0)
            a.wg_first = w
            assert fn(C.byref(fused.plan), C.byref(a), stream) == 0, w
            torch.cuda.synchronize()
            results[w] = [t.detach().clone() for t in held] + [reuse.ws[woff[k]:woff[nxt]].clone() for k, nxt in WS_BLOCKS]
        for w in (1, n_wg - 1):
            for got, want in zip(results[w], results[0]):
                assert torch.equal(got, want), w
        for got, want in zip(results[0][:4], (sdf_node, feat_node, nrm_node, nrm_b_node)):
            assert torch.equal(got, want) and not bool((got == -7.0).all())
        for w in (-1, n_wg):
            a.wg_first = w
            assert fn(C.byref(fused.plan), C.byref(a), stream) == 1, w          # MSDF_ERR_ARG
        a.wg_first = 1
        assert fn(C.byref(fused.mp.build_b16(2)), C.byref(a), stream) == 3      # MSDF_ERR_UNSUPPORTED
