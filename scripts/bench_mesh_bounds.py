"""Times of the oriented bounding box and the Replica crop on one MI355X, on a synthetic room shell.

    python scripts/bench_mesh_bounds.py [--points 1000000] [--repeats 5] [--out profiles/mesh_bounds_bench.json]

Cloud: --points samples of the six walls of a 6 x 4 x 2.8 room with Gaussian noise of 2 mm, rotated and moved, stored
in fp32 (the recipe of tests/obb_numpy.room_shell).  After one warm-up pass of ``oriented_bounds``:
  * one pass with a host clock around every stage (each ends in a host copy, so in a device synchronise): the support
    call of every hull round, the host hull work of every round, the candidate search (its host preparation, the
    kernel and the read-back), with the rounds, F, h, K, E and the (normal, edge) pairs that the kernel measures;
  * msdf_obb_support alone by HIP events (median of --repeats) on the final hull's F planes and on 2048 random planes,
    as a rate against its count of 3 F N fp64 multiply-adds and the fp64 vector peak;
  * ``oriented_bounds`` and ``crop_to_oriented_bounds`` (a reconstruction of as many vertices and twice as many faces)
    end to end, median of --repeats by a host clock.
Where scipy imports, the baseline on the host: scipy.spatial.ConvexHull of the same cloud and the whole numpy
restatement (tests/obb_numpy.oriented_bounds: that hull, a 2-D hull per normal, a box per edge), once each, and the
two volumes compared.  No time or ratio here is a pass condition.  Writes one JSON document.
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

# fp64 on the vector ALU runs at half the fp32 vector rate of the MI355X (157.3 TFLOP/s by specification)
FP64_VECTOR_PEAK_TFLOPS = 157.3 / 2


def room_shell(n, seed=5, sides=(6.0, 4.0, 2.8), sigma=0.002):
    rng = np.random.default_rng(seed)
    sides = np.asarray(sides)
    p = rng.uniform(-0.5, 0.5, (n, 3)) * sides
    wall = rng.integers(0, 3, n)
    sign = rng.integers(0, 2, n) * 2 - 1
    p[np.arange(n), wall] = sign * sides[wall] / 2
    p += rng.normal(0.0, sigma, (n, 3))
    q, r = np.linalg.qr(np.random.default_rng(seed + 1).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return (p @ q.T + np.array([0.3, -0.2, 1.4])).astype(np.float32)


def _events(fn, repeats):
    samples = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b))
    return float(np.median(samples)), [round(s, 4) for s in samples]


def _wall(fn, repeats):
    samples = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(samples)), [round(s, 3) for s in samples]


def support_rate(pts, planes, repeats):
    """msdf_obb_support on the planes, by events -> a dict with the time and the rate."""
    from monosdf_amd.utils import mesh_args as ma
    dev, N, D = pts.device, pts.shape[0], len(planes)
    pl = ma.upload(planes, dev, np.float64)
    ws = ma.workspace('bench', 'msdf_obb_support_workspace_bytes', N, D, device=dev)
    value = torch.empty(D, dtype=torch.float64, device=dev)
    index = torch.empty(D, dtype=torch.int32, device=dev)

    def run():
        ma.call('msdf_obb_support', pts, N, pl, D, ws, value, index)

    run()
    ms, every = _events(run, repeats)
    fma = 3.0 * D * N
    tflops = 2.0 * fma / (ms * 1e-3) / 1e12
    return {'planes': D, 'points': N, 'ms': round(ms, 4), 'ms_all': every, 'fp64_fma': fma,
            'tflops_fp64': round(tflops, 3), 'share_of_fp64_vector_peak': round(tflops / FP64_VECTOR_PEAK_TFLOPS, 4),
            'workspace_bytes': int(ws.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_bounds_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_bounds.py needs a GPU')
    from monosdf_amd.utils import mesh_bounds as mb
    host = room_shell(args.points)
    pts = torch.from_numpy(host).cuda()
    N = pts.shape[0]
    mb.oriented_bounds(pts)                                            # warm-up: code objects, allocator

    stats = {}
    tol = mb._cloud('bench', pts)[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    to_origin, extents = mb._oriented_bounds('bench', pts, tol, stats)
    one_pass_ms = (time.perf_counter() - t0) * 1e3
    doc = {'what': 'oriented bounding box and Replica crop of a synthetic room shell; stage times of one pass by a '
                   'host clock (every stage ends in a host copy), msdf_obb_support by HIP events, end-to-end times '
                   'by a host clock around a synchronise; medians of %d after a warm-up pass' % args.repeats,
           'device': torch.cuda.get_device_name(0), 'points': N, 'extents': [float(e) for e in extents],
           'rounds': stats['rounds'], 'F': stats['F'], 'h': stats['h'], 'K': stats['K'], 'E': stats['E'],
           'silhouette_pairs': stats['silhouette_pairs'], 'faces_per_support_call': stats['faces'],
           'support_ms_per_round': [round(t, 3) for t in stats['support_ms']],
           'host_hull_ms_per_round': [round(t, 3) for t in stats['host_ms']],
           'candidates_ms': round(stats['candidates_ms'], 3), 'one_pass_ms': round(one_pass_ms, 3),
           'fp64_vector_peak_tflops': FP64_VECTOR_PEAK_TFLOPS,
           'fp64_vector_peak_source': 'half the fp32 vector rate of the specification (157.3 TFLOP/s); not measured'}

    planes = mb.convex_hull(pts)[2].cpu().numpy()
    rng = np.random.default_rng(0)
    many = rng.normal(size=(2048, 4))
    many[:, :3] /= np.linalg.norm(many[:, :3], axis=1, keepdims=True)
    doc['support_kernel'] = [support_rate(pts, planes, args.repeats), support_rate(pts, many, args.repeats)]

    ms, every = _wall(lambda: mb.oriented_bounds(pts), args.repeats)
    doc['oriented_bounds_ms'], doc['oriented_bounds_ms_all'] = round(ms, 3), every
    faces = torch.from_numpy(rng.integers(0, N, (2 * N, 3))).cuda()
    rec = (pts * 1.04 + 0.01, faces)                                  # sticks out of the box scaled by 1.05 in places
    kept = mb.crop_to_oriented_bounds(rec, (pts, faces))
    ms_crop, every = _wall(lambda: mb.crop_to_oriented_bounds(rec, (pts, faces)), args.repeats)
    doc['crop_ms'], doc['crop_ms_all'] = round(ms_crop, 3), every
    doc['crop_without_bounds_ms'] = round(ms_crop - ms, 3)
    doc['crop_kept_vertices'], doc['crop_kept_faces'] = int(len(kept.vertices)), int(len(kept.faces))

    try:
        from scipy.spatial import ConvexHull
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import obb_numpy
    except ImportError:
        doc['scipy_baseline'] = None
    else:
        t0 = time.perf_counter()
        hull = ConvexHull(host.astype(np.float64))
        t1 = time.perf_counter()
        volume = obb_numpy.oriented_bounds(host)[0]
        t2 = time.perf_counter()
        got = float(np.prod(extents))
        doc['scipy_baseline'] = {'convex_hull_ms': round((t1 - t0) * 1e3, 1), 'restatement_ms': round((t2 - t1) * 1e3, 1),
                                 'hull_vertices': int(len(hull.vertices)),
                                 'vertex_set_equal': bool(np.array_equal(np.sort(hull.vertices),
                                                                         mb.convex_hull(pts)[0].cpu().numpy())),
                                 'volume_relative_difference': abs(got - volume) / volume}
    text = json.dumps(doc, indent=1)
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
