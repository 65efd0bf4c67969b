"""Times of the mesh evaluation on one MI355X: the brute-force nearest-neighbour search (msdf_nn_search, HIP events
after a warm-up) at 2e5 x 2e5 (the Replica protocol's sample counts) and 1e6 x 1e6, and evaluate_scannet /
evaluate_replica end to end on synthetic surfaces.

    python scripts/bench_meshmetrics.py [--repeats 5] [--no-large] [--out profiles/meshmetrics_bench.json]

Reports pairs/s and the fraction of the vector ALU's fp32 issue peak: the compiled inner loop of nn_search_k
(hipcc --save-temps on csrc/nnsearch.hip with the Makefile's flags, the loop under "Inner Loop Header") holds, per 8
reference records x 4 queries = 32 pairs, 297 vector-ALU instructions: 96 v_sub_f32, 32 v_mul_f32, 64 v_fmac_f32,
32 v_cmp_lt_f32, 64 v_cndmask_b32 (8 per pair) and 9 v_mov_b32 (the index constants).  A SIMD issues one wave64
fp32 instruction every 2 cycles (its 157.3 TFLOP/s fp32 vector peak is 1024 SIMDs x 32 lanes x 2 FLOP x 2.4 GHz), so
the peak is 1024 x 2.4e9 / 2 wave-instructions/s at the nominal clock.  If scipy is importable, cKDTree(...).query(...,
workers=16) on the same clouds is timed beside the search (the reference's CPU path); if not, the key is null.
Kernel-level times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/bench_meshmetrics.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_32_PAIRS = 297            # nn_search_k inner loop, counted in the compiled ISA (see above)
USEFUL_PER_PAIR = 8                # 3 subtract, 1 multiply, 2 fma, 1 compare, 2 select
N_SIMD = 256 * 4
CLOCK_HZ = 2.4e9                   # nominal; the clock held under load is lower
ISSUE_PEAK = N_SIMD * CLOCK_HZ / 2  # wave64 fp32 VALU instructions per second


def surface_cloud(n, seed, device):
    """Points on a room-like surface at scene scale: the six walls of a 6 x 4 x 3 m box centred at (8, -6, 3),
    displaced by a few centimetres of noise."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    u = torch.rand(n, 3, device=device, generator=g)
    wall = torch.randint(0, 6, (n,), device=device, generator=g)
    axis, side = wall % 3, (wall // 3).float()
    u[torch.arange(n, device=device), axis] = side
    u = u + 0.01 * torch.randn(n, 3, device=device, generator=g)
    size = torch.tensor([6.0, 4.0, 3.0], device=device)
    centre = torch.tensor([8.0, -6.0, 3.0], device=device)
    return ((u - 0.5) * size + centre).float().contiguous()


def time_search(lib, _lib, ref, qry, repeats):
    R, Q = ref.shape[0], qry.shape[0]
    ws = torch.empty(int(lib.msdf_nn_workspace_bytes(R, Q, 0)), dtype=torch.uint8, device=ref.device)
    dist = torch.empty(Q, dtype=torch.float32, device=ref.device)
    idx = torch.empty(Q, dtype=torch.int32, device=ref.device)

    def run():
        _lib.call('msdf_nn_search', _lib.ptr(ref), R, _lib.ptr(qry), Q, 0, _lib.ptr(ws), _lib.ptr(dist),
                  _lib.ptr(idx), _lib.stream_ptr())
    run()                                              # warm-up: code object, clocks
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t = float(np.median(ms)) * 1e-3
    pairs = float(R) * float(Q)
    out = {'n_ref': R, 'n_query': Q, 'n_splits': int(lib.msdf_nn_split_count(R, Q, 0)),
           'seconds': round(t, 6), 'seconds_all': [round(m * 1e-3, 6) for m in ms],
           'pairs_per_s': round(pairs / t, 1),
           'fraction_of_valu_issue_peak': round(pairs * VALU_PER_32_PAIRS / 32 / 64 / t / ISSUE_PEAK, 4),
           'fraction_of_valu_issue_peak_useful_8_per_pair': round(pairs * USEFUL_PER_PAIR / 64 / t / ISSUE_PEAK, 4)}
    return out, dist, idx


def time_ckdtree(ref, qry, dist_gpu):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    r, q = ref.cpu().numpy().astype(np.float64), qry.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(r)
    t1 = time.perf_counter()
    d, _ = tree.query(q, workers=16)
    t2 = time.perf_counter()
    return {'build_s': round(t1 - t0, 4), 'query_s_workers16': round(t2 - t1, 4), 'total_s': round(t2 - t0, 4),
            'max_abs_distance_difference_to_gpu': float(np.abs(d - dist_gpu.cpu().numpy()).max())}


def _wall(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)), 5), [round(t, 5) for t in ts]


def sphere_mesh(radius, n):
    from monosdf_amd.utils.mesh import marching_cubes
    g = torch.linspace(-1.2, 1.2, n, device='cuda', dtype=torch.float64)
    x, y, z = torch.meshgrid(g, g, g, indexing='ij')
    step = float(g[1] - g[0])
    v, f, _ = marching_cubes(((x * x + y * y + z * z).sqrt() - radius).float(), 0.0, (step, step, step))
    return (v - 1.2).contiguous(), f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-large', action='store_true', help='skip the 1e6 x 1e6 search')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_meshmetrics.py needs a GPU')
    from monosdf_amd import _lib
    from monosdf_amd.utils import mesh_eval
    lib = _lib.load()
    out = {'what': 'mesh evaluation: brute-force nearest neighbours (msdf_nn_search, HIP events) and the two protocols',
           'device': torch.cuda.get_device_name(0),
           'valu_instructions_per_pair': round(VALU_PER_32_PAIRS / 32, 3),
           'valu_issue_peak_wave_instructions_per_s': ISSUE_PEAK}
    for name, n in (('search_200k', 200000),) + (() if args.no_large else (('search_1m', 1000000),)):
        ref, qry = surface_cloud(n, 1, 'cuda'), surface_cloud(n, 2, 'cuda')
        res, dist, _ = time_search(lib, _lib, ref, qry, args.repeats)
        res['ckdtree'] = time_ckdtree(ref, qry, dist)
        out[name] = res
        print(name, json.dumps(res), file=sys.stderr, flush=True)
    # the protocols end to end: marching-cubes meshes of two spheres (radius 1.00 and 1.03)
    (pv, pf), (gv, gf) = sphere_mesh(1.03, 481), sphere_mesh(1.00, 481)
    t, ts = _wall(lambda: mesh_eval.evaluate_scannet(pv, gv), args.repeats)
    out['evaluate_scannet'] = {'pred_vertices': int(pv.shape[0]), 'gt_vertices': int(gv.shape[0]),
                               'down_sampled': [int(mesh_eval.voxel_down_sample(pv, 0.02).shape[0]),
                                                int(mesh_eval.voxel_down_sample(gv, 0.02).shape[0])],
                               'seconds': t, 'seconds_all': ts, 'metrics': mesh_eval.evaluate_scannet(pv, gv)}
    t, ts = _wall(lambda: mesh_eval.evaluate_replica((pv, pf), (gv, gf)), args.repeats)
    out['evaluate_replica'] = {'n_samples': 200000, 'rec_faces': int(pf.shape[0]), 'gt_faces': int(gf.shape[0]),
                               'seconds': t, 'seconds_all': ts,
                               'metrics': mesh_eval.evaluate_replica((pv, pf), (gv, gf))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
