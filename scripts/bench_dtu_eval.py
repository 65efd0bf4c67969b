"""Times of the DTU evaluation protocol on one MI355X, stage by stage (HIP events after a warm-up), on a synthetic
scene at the protocol's sizes: a sphere of radius 150 mm meshed by marching cubes at 1.2 mm cells (the triangle size
of a 512^3 extraction of a DTU scene), 64 views of 1200 x 1600, density 0.2 mm, an stl cloud of 3e6 points.

    python scripts/bench_dtu_eval.py [--repeats 3] [--small] [--out profiles/dtu_eval_bench.json]
                                     [--grid-out profiles/gridnn_bench.json]

Stages: dilate_masks (all views, one launch), mask_vertices, sample_lattice, radius_thin (with its number of rounds),
the two closing brute-force searches, and evaluate_dtu end to end (wall clock).  Under 'grid_search': the same two
queries through nearest_neighbors_within (--max-dist, default 20 mm) next to those brute-force times, on the same
clouds -- the whole call, its build (cells, sort, records, start table) and its query (query cells, sort, kernel)
apart, whether the result equals the brute-force one where that is within max_dist, a sweep of the cell side over
max_dist / {4, 8, 16, 32, 64}, the second query again with a tenth of its queries moved 3 max_dist away from every
reference point (brute force and grid), and evaluate_dtu end to end with search='grid'.  If sklearn is importable, the
reference's form of the thinning (NearestNeighbors(algorithm='kd_tree').radius_neighbors plus the Python loop) is timed
on the CPU on a REDUCED cloud (--cpu-points, default 200,000 points of the same cloud) next to radius_thin on that
same reduced cloud, and the two masks are compared; it is reported as exactly that, not as a time of the full size.
Prints one JSON line.
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


def sphere_mesh(radius, cell):
    from monosdf_amd.utils.mesh import marching_cubes
    half = radius + 4 * cell
    n = int(np.ceil(2 * half / cell)) + 1
    g = (torch.arange(n, device='cuda', dtype=torch.float32) * cell - half)
    d2 = (g * g)[:, None, None] + (g * g)[None, :, None] + (g * g)[None, None, :]
    v, f, _ = marching_cubes((d2.sqrt() - radius).contiguous(), 0.0, (cell, cell, cell))
    return (v - half).contiguous(), f


def ring_cameras(n_views, distance, focal, height, width):
    """[n,3,4] float64 projections of cameras on a ring around the origin, looking at it."""
    K = np.array([[focal, 0, (width - 1) / 2], [0, focal, (height - 1) / 2], [0, 0, 1.0]])
    out = []
    for k in range(n_views):
        t = 2 * np.pi * k / n_views
        z = -np.array([np.cos(t), 0.25 * np.sin(3 * t), np.sin(t)])
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        out.append(K @ np.concatenate([R, (R @ (distance * z))[:, None]], 1))
    return np.stack(out)


def timed(fn, repeats):
    """median HIP-event milliseconds of fn() after one warm-up call, and its last result."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'ms': round(float(np.median(ms)), 3), 'ms_all': [round(m, 3) for m in ms]}, out


def grid_stages(reference, query, max_dist, cell, repeats):
    """nearest_neighbors_within(reference, query, max_dist, cell): the whole call, and its two halves apart."""
    from monosdf_amd.utils import mesh_args as ma
    from monosdf_amd.utils import mesh_eval as me
    from monosdf_amd.utils.point_grid import PointGrid
    whole, result = timed(lambda: me.nearest_neighbors_within(reference, query, max_dist, cell=cell), repeats)
    _, lo, hi = ma.finite_bounds('bench_dtu_eval', reference)
    build, grid = timed(lambda: PointGrid(reference, lo, hi, cell), repeats)
    search, _ = timed(lambda: grid.query(query, max_dist), repeats)
    return {'cell_asked': cell, 'cell': round(grid.grid[3], 6), 'cells': list(grid.grid[4:]), 'ms': whole['ms'],
            'ms_all': whole['ms_all'], 'build_ms': build['ms'], 'query_ms': search['ms']}, result


def equal_within(result, brute, max_dist):
    """Whether a bounded result is the brute-force one where that is within max_dist and (+inf, -1) elsewhere."""
    near = brute[0] <= torch.tensor(max_dist, dtype=torch.float32, device=brute[0].device)
    inf = torch.full_like(brute[0], float('inf'))
    return bool(torch.equal(result[0], torch.where(near, brute[0], inf)) and
                torch.equal(result[1], torch.where(near, brute[1], torch.full_like(brute[1], -1))))


def sklearn_thin(points, radius):
    try:
        import sklearn.neighbors as skln
    except ImportError:
        return None
    data = points.astype(np.float64)
    t0 = time.perf_counter()
    engine = skln.NearestNeighbors(n_neighbors=1, radius=radius, algorithm='kd_tree',
                                   n_jobs=min(16, os.cpu_count() or 1))
    engine.fit(data)
    idxs = engine.radius_neighbors(data, radius=radius, return_distance=False)
    t1 = time.perf_counter()
    mask = np.ones(len(data), bool)
    for curr, near in enumerate(idxs):
        if mask[curr]:
            mask[near] = 0
            mask[curr] = 1
    t2 = time.perf_counter()
    return mask, {'radius_neighbors_s': round(t1 - t0, 3), 'python_loop_s': round(t2 - t1, 3),
                  'total_s': round(t2 - t0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='a tenth of the linear size: a quick check of the script')
    ap.add_argument('--cpu-points', type=int, default=200000, help='size of the reduced cloud for the sklearn form')
    ap.add_argument('--out', default=None)
    ap.add_argument('--max-dist', type=float, default=20.0, help='the bound of the grid search, millimetres')
    ap.add_argument('--grid-out', default=None, help="where the 'grid_search' part goes as a line of its own")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dtu_eval.py needs a GPU')
    from monosdf_amd.utils import mesh_dtu as md
    from monosdf_amd.utils.mesh_eval import nearest_neighbors
    radius_mm, cell, density = (15.0 if args.small else 150.0), 1.2, 0.2
    n_views, height, width = (4 if args.small else 64), 1200, 1600
    n_stl = 30000 if args.small else 3000000
    out = {'what': 'DTU evaluation protocol, stage by stage (HIP events; evaluate_dtu: wall clock)',
           'device': torch.cuda.get_device_name(0), 'sphere_radius_mm': radius_mm, 'cell_mm': cell,
           'density_mm': density, 'views': n_views, 'image': [height, width]}
    verts, faces = sphere_mesh(radius_mm, cell)
    out['mesh'] = {'vertices': int(verts.shape[0]), 'faces': int(faces.shape[0])}

    # cull: masks of the sphere's silhouette, eroded a little so that the dilation has something to restore
    proj = ring_cameras(n_views, 4 * radius_mm, 2000.0, height, width)
    yy, xx = torch.meshgrid(torch.arange(height, device='cuda'), torch.arange(width, device='cuda'), indexing='ij')
    silhouette = 2000.0 * radius_mm / np.sqrt((4 * radius_mm) ** 2 - radius_mm ** 2) - 8.0
    disc = ((xx - (width - 1) / 2) ** 2 + (yy - (height - 1) / 2) ** 2) <= silhouette ** 2
    masks = (disc.to(torch.uint8) * 255)[None].repeat(n_views, 1, 1).contiguous()
    out['dilate_masks'], dilated = timed(lambda: md.dilate_masks(masks, 12), args.repeats)
    out['mask_vertices'], kept = timed(lambda: md.mask_vertices(verts, proj, dilated), args.repeats)
    out['mask_vertices']['kept'] = int(kept.sum())

    out['sample_lattice'], samples = timed(lambda: md.sample_lattice(verts, faces, density), args.repeats)
    out['sample_lattice']['points'] = int(samples.shape[0])
    cloud = torch.cat([verts, samples])
    del samples
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    order = torch.randperm(cloud.shape[0], generator=gen, device='cuda')
    out['radius_thin'], (keep, rounds) = timed(lambda: md.radius_thin(cloud, density, order, return_rounds=True),
                                              args.repeats)
    out['radius_thin'].update({'points': int(cloud.shape[0]), 'kept': int(keep.sum()), 'rounds': rounds})
    data_down = cloud[keep]

    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    d = torch.randn(n_stl, 3, device='cuda', generator=g)
    stl = ((radius_mm + 0.3) * d / d.norm(dim=1, keepdim=True)).float().contiguous()
    out['search_d2s'], brute_d2s = timed(lambda: nearest_neighbors(stl, data_down), 1)
    out['search_d2s'].update({'n_ref': int(stl.shape[0]), 'n_query': int(data_down.shape[0])})
    above = stl[stl[:, 2] > 0].contiguous()
    out['search_s2d'], brute_s2d = timed(lambda: nearest_neighbors(data_down, above), 1)
    out['search_s2d'].update({'n_ref': int(data_down.shape[0]), 'n_query': int(above.shape[0])})

    # the same two queries through the grid, on the same clouds
    md_mm = args.max_dist
    gs = out['grid_search'] = {'what': 'nearest_neighbors_within beside the brute-force searches of this run (HIP '
                               'events, warm-up, median of %d; evaluate_dtu: wall clock)' % args.repeats,
                               'device': out['device'], 'max_dist_mm': md_mm,
                               'brute_d2s_ms': out['search_d2s']['ms'], 'brute_s2d_ms': out['search_s2d']['ms'],
                               'n_d2s': [int(stl.shape[0]), int(data_down.shape[0])],
                               'n_s2d': [int(data_down.shape[0]), int(above.shape[0])]}
    def save_grid():                                     # after every part: a later failure keeps the earlier ones
        if args.grid_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.grid_out)), exist_ok=True)
            with open(args.grid_out, 'w') as f:
                f.write(json.dumps(gs) + '\n')
    sweep = {}
    for fraction in (4, 8, 16, 32, 64):
        d2s, res_d2s = grid_stages(stl, data_down, md_mm, md_mm / fraction, args.repeats)
        s2d, res_s2d = grid_stages(data_down, above, md_mm, md_mm / fraction, args.repeats)
        d2s['equal_to_brute'] = equal_within(res_d2s, brute_d2s, md_mm)
        s2d['equal_to_brute'] = equal_within(res_s2d, brute_s2d, md_mm)
        sweep['max_dist/%d' % fraction] = {'d2s': d2s, 's2d': s2d}
        del res_d2s, res_s2d
        gs['cell_sweep'] = sweep
        save_grid()
    from monosdf_amd.utils import mesh_eval
    gs['default_cell'] = 'max_dist/%d' % mesh_eval.GRID_CELL_FRACTION
    del brute_d2s
    # a tenth of the second query's points moved radially 3 max_dist outwards: no neighbour within max_dist
    far = above.clone()
    far[::10] *= (radius_mm + 0.3 + 3 * md_mm) / (radius_mm + 0.3)
    brute_far_ms, brute_far = timed(lambda: nearest_neighbors(data_down, far), 1)
    grid_far, res_far = grid_stages(data_down, far, md_mm, md_mm / mesh_eval.GRID_CELL_FRACTION, args.repeats)
    grid_far.update({'equal_to_brute': equal_within(res_far, brute_far, md_mm), 'brute_ms': brute_far_ms['ms'],
                     'queries_without_neighbour': int((res_far[1] < 0).sum()), 'n_query': int(far.shape[0])})
    gs['s2d_a_tenth_far'] = grid_far
    save_grid()
    del brute_far, res_far, far, brute_s2d

    box = radius_mm + 10.0
    bb = np.array([[-box] * 3, [box] * 3], np.float32)
    n_grid = int(2 * box / 10.0) + 1
    obs = np.ones((n_grid,) * 3, np.uint8)
    obs[:, :, : n_grid // 4] = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metrics = md.evaluate_dtu((verts, faces), stl, obs, bb, 10.0, [0.0, 0.0, 1.0, 0.0], density=density, seed=0,
                              max_dist=md_mm)
    torch.cuda.synchronize()
    out['evaluate_dtu'] = {'seconds': round(time.perf_counter() - t0, 3), 'metrics': metrics}
    seconds = []
    for _ in range(2):                                   # the second call has the allocator's blocks of the first
        t0 = time.perf_counter()
        by_grid = md.evaluate_dtu((verts, faces), stl, obs, bb, 10.0, [0.0, 0.0, 1.0, 0.0], density=density, seed=0,
                                  max_dist=md_mm, search='grid')
        torch.cuda.synchronize()
        seconds.append(round(time.perf_counter() - t0, 3))
    gs['evaluate_dtu'] = {'brute_seconds': out['evaluate_dtu']['seconds'], 'grid_seconds': seconds[-1],
                          'grid_seconds_all': seconds, 'metrics_equal': by_grid == metrics, 'metrics': by_grid}

    # the reference's CPU form of the thinning on a reduced cloud: the points of the cloud nearest to one pole
    n_cpu = min(args.cpu_points, cloud.shape[0])
    near_pole = torch.argsort(-cloud[:, 2])[:n_cpu]
    reduced = cloud[near_pole].contiguous()
    reduced = reduced[torch.randperm(n_cpu, generator=gen, device='cuda')].contiguous()
    res = sklearn_thin(reduced.cpu().numpy(), density)
    if res is None:
        out['thinning_reduced_cloud_sklearn_cpu'] = None
    else:
        mask, cpu = res
        gpu, (keep_r, rounds_r) = timed(lambda: md.radius_thin(reduced, density, return_rounds=True), args.repeats)
        out['thinning_reduced_cloud_sklearn_cpu'] = dict(
            cpu, points=n_cpu, cpu_threads=os.cpu_count() if not os.environ.get('OMP_NUM_THREADS') else
            int(os.environ['OMP_NUM_THREADS']), gpu_radius_thin_ms=gpu['ms'], gpu_rounds=rounds_r,
            masks_equal=bool(np.array_equal(mask, keep_r.cpu().numpy())), kept=int(mask.sum()))
    line = json.dumps(out)
    print(line)
    save_grid()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
