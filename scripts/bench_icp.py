"""Times of one point-to-point ICP (monosdf_amd/utils/mesh_align.py) on one MI355X, stage by stage (HIP events after a
warm-up), on a synthetic pair at the sizes of a marching-cubes mesh: two independent draws of N points from one bumpy
sphere of radius 2 (a room's worth of surface), the source turned by 2 degrees and shifted by 0.02.

    python scripts/bench_icp.py [--sizes 200000 2000000] [--repeats 5] [--brute-at 200000] [--out profiles/icp_bench.json]

Per size: the target's grid build (once per alignment), then the four stages of ONE iteration at the start transform --
transform, search (query cells, sort, grid query), accumulate, solve -- their sum, and a whole icp() call (wall clock,
with its number of evaluations, fitness and rmse).  At --brute-at the same iteration's search is also timed by the
brute-force nearest_neighbors, the baseline.  Prints one JSON line and writes it to --out.
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


def bumpy_sphere(n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    d = torch.randn(n, 3, device='cuda', generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    r = 2.0 + 0.15 * torch.sin(5.0 * d[:, 0]) * torch.cos(4.0 * d[:, 1]) + 0.1 * torch.sin(7.0 * d[:, 2])
    return (d * r[:, None]).float().contiguous()


def rigid(axis, degrees, shift):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = shift
    return M


def timed(fn, repeats, before=None):
    """median HIP-event milliseconds of fn() after one warm-up call (``before()`` runs untimed in front of every call),
    and its last result."""
    def once():
        if before is not None:
            before()
        return fn()
    out = once()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'ms': round(float(np.median(ms)), 4), 'ms_all': [round(m, 4) for m in ms]}, out


def one_size(n, repeats, max_dist, brute):
    from monosdf_amd.utils import mesh_align as al
    from monosdf_amd.utils import mesh_args as ma
    from monosdf_amd.utils import mesh_eval as me
    from monosdf_amd.utils.point_grid import PointGrid
    tgt = bumpy_sphere(n, 1)
    motion = ma.upload(rigid((1.0, 2.0, 3.0), 2.0, (0.012, -0.012, 0.01)))
    src = (bumpy_sphere(n, 2).double() @ motion[:3, :3].T + motion[:3, 3]).float().contiguous()
    out = {'n_source': n, 'n_target': n, 'max_dist': max_dist}
    pivots, t_lo, t_hi = al._pivots('bench_icp', src, tgt)
    out['grid_build'], grid = timed(lambda: PointGrid(tgt, t_lo, t_hi, max_dist / me.GRID_CELL_FRACTION), repeats)
    out['grid'] = {'cell': round(grid.grid[3], 6), 'cells': list(grid.grid[4:])}
    state0 = al._new_state(np.eye(4), 30, src.device)
    state = state0.clone()
    ws = ma.workspace('bench_icp', 'msdf_icp_workspace_bytes', n, device=src.device)
    y = torch.empty_like(src)
    out['transform'], _ = timed(lambda: ma.call('msdf_icp_transform', src, n, state, y), repeats)
    out['search'], (_, idx) = timed(lambda: grid.query(y, max_dist, int32=True), repeats)
    out['search']['with_neighbour'] = int((idx >= 0).sum())
    out['accumulate'], _ = timed(lambda: ma.call('msdf_icp_accumulate', src, y, tgt, idx, n, n, pivots, state, ws),
                                 repeats)
    out['solve'], _ = timed(lambda: ma.call('msdf_icp_solve', ws, n, pivots, 30, 1e-6, 1e-6, state), repeats,
                            before=lambda: state.copy_(state0))
    out['iteration_ms'] = round(sum(out[k]['ms'] for k in ('transform', 'search', 'accumulate', 'solve')), 4)
    if brute:
        out['search_brute_force'], (_, idx_b) = timed(lambda: me.nearest_neighbors(tgt, y), max(1, repeats // 2))
        out['search_brute_force']['equal_where_within'] = bool(torch.equal(idx_b[idx >= 0], idx[idx >= 0].long()))
        out['iteration_brute_force_ms'] = round(out['iteration_ms'] - out['search']['ms'] +
                                                out['search_brute_force']['ms'], 4)
    seconds = []
    for _ in range(2):                                   # the second call has the allocator's blocks of the first
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T, fitness, rmse, log, evaluations = al.icp(src, tgt, max_dist, return_log=True)
        torch.cuda.synchronize()
        seconds.append(round(time.perf_counter() - t0, 4))
    found = np.abs(T - np.linalg.inv(motion.cpu().numpy())).max()
    out['icp'] = {'seconds': seconds[-1], 'seconds_all': seconds, 'evaluations': evaluations, 'fitness': fitness,
                  'inlier_rmse': rmse, 'largest_gap_from_the_inverse_motion': float(found)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[200000, 2000000])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--max-dist', type=float, default=0.1)
    ap.add_argument('--brute-at', type=int, default=200000, help='the size at which the brute-force search is timed too')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_icp.py needs a GPU')
    out = {'what': 'point-to-point ICP, one iteration stage by stage (HIP events, warm-up, median of %d); icp: wall '
                   'clock of the whole call' % args.repeats,
           'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for n in args.sizes:
        out['sizes'][str(n)] = one_size(n, args.repeats, args.max_dist, n == args.brute_at)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
