"""Time the SDF forward+gradient launch of the bench shape (8x256 network, 1024 rays, training mode, one sampler round so
that the dense-set workgroups reuse the sampler's activations) for several dispatch rotations msdf_fg_args_t.wg_first:
which order of the short (reusing) and long workgroups ends first?  The launch is the one the SDF node makes -- its
argument struct is recorded and msdf_sdf_fwd_grad called again on the same buffers with only wg_first changed.
(diagnostic; prints ms per launch by HIP events, REPEATS x LAUNCHES launches per setting, settings interleaved)"""
import ctypes as C
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench                                     # noqa: E402
from monosdf_amd import _lib, ops                # noqa: E402
from monosdf_amd.model.network import MonoSDFNetwork   # noqa: E402

N, LAUNCHES, REPEATS = 1024, 10, 7
torch.manual_seed(0)
dev = torch.device('cuda', 0)
model = MonoSDFNetwork(bench.model_conf()).to(dev).train()
net, smp = model.implicit_network, model.ray_sampler
rays = bench.make_rays(N, 1, dev)
S = smp.N_samples + smp.N_samples_extra + 2
net.share(dev)
fused = net.packed(dev)[0]
reuse = net.sdf_reuse(dev, N, S, smp.N_samples_extra, 4 * N, True)
beta = ops.effective_beta(model.density.beta, model.density.beta_min_f)
_, _, x_all = smp.sample(rays['ray_dirs'], rays['ray_cam_loc'], model, speculate=1, beta0=beta, sdf_reuse=reuse)
assert smp.confirm() and smp.last_rounds == 1, 'the reuse path needs a one-round state'
assert int(reuse.flags[1]) == 0 and int(reuse.h_saved[0]) == 1

recorded, call = [], _lib.call


def recording(name, *args):
    if name == 'msdf_sdf_fwd_grad':
        recorded.append(args[1]._obj)
    return call(name, *args)


_lib.call = recording
held = net.evaluate(x_all, N * S, N * S, save=True, split=N * S, reuse=reuse)      # owns the output buffers
_lib.call = call
a, = recorded
fn, stream = _lib.load().msdf_sdf_fwd_grad, _lib.stream_ptr()
n_wg, short = a.P_pad // 64, a.n_reuse // 64
settings = [('grid order', 0), ('short last', short), ('split -96', short - 96), ('split +96', short + 96)]
print('%d workgroups, %d of them reusing; %d x %d launches per setting' % (n_wg, short, REPEATS, LAUNCHES))


def timed(w):
    a.wg_first = w
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        status = fn(C.byref(fused.plan), C.byref(a), stream)
        assert status == 0, status
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


for _, w in settings:                           # warm-up
    timed(w)
ms = {w: [] for _, w in settings}
for _ in range(REPEATS):
    for _, w in settings:
        ms[w].append(timed(w))
for name, w in settings:
    v = sorted(ms[w])
    print('%-11s wg_first %4d   median %.4f  min %.4f  max %.4f ms   [%s]' % (
        name, w, v[len(v) // 2], v[0], v[-1], ' '.join('%.4f' % t for t in ms[w])))
net.unshare()
