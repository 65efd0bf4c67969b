"""Times of the mesh re-fusion on one MI355X (HIP events after a warm-up, median of --repeats): the depth rasteriser
(msdf_raster_depth), the TSDF integration (msdf_tsdf_integrate) and refuse() end to end, on a synthetic room: the
marching-cubes mesh of a 6 x 4 x 3 m box with a sphere in it (about 1e6 faces), 100 views of 968 x 1296 pixels from
inside it, 1 cm voxels.

    python scripts/bench_refuse.py [--repeats 5] [--views 100] [--size 968 1296] [--voxel 0.01] [--small]
                                   [--out profiles/refuse_bench.json]

--small: a quarter of the resolution everywhere (a quick check that the script runs).  Reported beside the times: the
triangles x views and the covered pixels of the raster, the voxels x views of the integration and the bytes it must
move at least (one depth gather per voxel and view that projects into an image, two stores per voxel).
Kernel-level times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/bench_refuse.py`.
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

ROOM = np.array([6.0, 4.0, 3.0])


def room_mesh(step):
    """Marching cubes of min(distance to the walls, distance to a sphere) - the room seen from inside: CUDA tensors."""
    from monosdf_amd.utils.mesh import marching_cubes
    half = ROOM / 2 + 0.1
    axes = [torch.arange(-h, h + step, step, device='cuda', dtype=torch.float64) for h in half]
    x, y, z = torch.meshgrid(*axes, indexing='ij')
    walls = torch.minimum(torch.minimum(ROOM[0] / 2 - x.abs(), ROOM[1] / 2 - y.abs()), ROOM[2] / 2 - z.abs())
    ball = ((x - 1.0) ** 2 + (y + 0.5) ** 2 + (z + 0.7) ** 2).sqrt() - 0.8
    v, f, _ = marching_cubes(torch.minimum(walls, ball).float(), 0.0, (step, step, step))
    return (v - torch.tensor(half, device='cuda', dtype=torch.float32)).contiguous(), f


def camera_poses(n, seed):
    rng = np.random.default_rng(seed)
    poses = []
    for _ in range(n):
        pos = rng.uniform(-0.35, 0.35, 3) * ROOM
        while np.linalg.norm(pos - [1.0, -0.5, -0.7]) < 1.0:
            pos = rng.uniform(-0.35, 0.35, 3) * ROOM
        z = rng.normal(size=3)
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [1.0, 0.0, 0.0])
        x /= np.linalg.norm(x)
        p = np.eye(4)
        p[:3, :3], p[:3, 3] = np.stack([x, np.cross(z, x), z], 1), pos
        poses.append(p)
    return np.stack(poses)


def timed(fn, repeats):
    fn()                                               # warm-up: code object, clocks
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)) * 1e-3, 6), [round(m * 1e-3, 6) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--size', type=int, nargs=2, default=(968, 1296))
    ap.add_argument('--voxel', type=float, default=0.01)
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_refuse.py needs a GPU')
    from monosdf_amd.utils import mesh_refuse as mr
    from monosdf_amd.utils.mesh import Mesh
    h, w = args.size
    voxel, step, n = args.voxel, 0.0125, args.views
    if args.small:
        h, w, voxel, step, n = h // 4, w // 4, voxel * 4, step * 4, max(1, n // 4)
    K = (w * 0.9, w * 0.9, w / 2 - 0.5, h / 2 - 0.5)
    verts, faces = room_mesh(step)
    poses = camera_poses(n, 0)
    out = {'what': 'mesh re-fusion: depth raster, TSDF integration (HIP events) and refuse() end to end (wall clock)',
           'device': torch.cuda.get_device_name(0), 'vertices': int(verts.shape[0]), 'faces': int(faces.shape[0]),
           'views': n, 'height': h, 'width': w, 'voxel_length': voxel}
    t, ts = timed(lambda: mr.render_depth(verts, faces, poses, K, h, w), args.repeats)
    depth = mr.render_depth(verts, faces, poses, K, h, w)
    out['raster'] = {'seconds': t, 'seconds_all': ts, 'triangle_views_per_s': round(faces.shape[0] * n / t, 1),
                     'covered_pixels': int((depth > 0).sum()), 'pixels': n * h * w}
    print('raster', json.dumps(out['raster']), file=sys.stderr, flush=True)
    origin, dims = mr.fusion_grid(verts.min(0).values.double().cpu().numpy(),
                                  verts.max(0).values.double().cpu().numpy(), voxel)
    block = tuple(min(d, 513) for d in dims)           # one block of refuse()
    t, ts = timed(lambda: mr.tsdf_integrate(depth, poses, K, origin, block, voxel, None), args.repeats)
    n_vox = block[0] * block[1] * block[2]
    out['integrate'] = {'dims': list(block), 'seconds': t, 'seconds_all': ts,
                        'voxel_views_per_s': round(n_vox * n / t, 1),
                        'bytes_at_least': n_vox * 8 + n_vox * n * 4,
                        'bytes_at_least_per_s': round((n_vox * 8 + n_vox * n * 4) / t, 1)}
    print('integrate', json.dumps(out['integrate']), file=sys.stderr, flush=True)
    del depth
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fused = mr.refuse((verts, faces), poses, K, h, w, voxel_length=voxel)
    torch.cuda.synchronize()
    out['refuse'] = {'seconds_wall_one_run': round(time.perf_counter() - t0, 3), 'volume_dims': list(dims),
                     'vertices_out': int(len(fused.vertices)), 'faces_out': int(len(fused.faces))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
