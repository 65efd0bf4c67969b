"""Times of the mesh export on one MI355X: the bench model's SDF volume (sdf_volume), get_surface_sliding over the same
block, and the two marching-cubes entry points alone (HIP events), with the classify pass's HBM roofline.

    python scripts/bench_mesh.py [--resolution 512] [--repeats 5] [--out FILE]

Bench model = bench.model_conf() (ImplicitNetwork 8x256, geometric init, seed 0), grid function
implicit_network.raw_sdf (INTEGRATION.md "Meshing grid"), grid_boundary (-1.1, 1.1), level 0.  Prints one JSON line.
Kernel-level times (classify / scan / emit separately) come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_mesh.py`.
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

HBM_PEAK = 8.0e12          # bytes/s, MI355X_MICROARCH.md (spec; ~6.3e12 achievable by a float4 copy)


def _median_wall(fn, repeats):
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), [round(t, 5) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh.py needs a GPU')
    import bench
    from monosdf_amd import _lib
    from monosdf_amd.model.network import MonoSDFNetwork
    from monosdf_amd.utils import render
    from monosdf_amd.utils.mesh import get_surface_sliding, marching_cubes

    torch.manual_seed(0)
    model = MonoSDFNetwork(bench.model_conf()).cuda().eval()
    sdf = lambda p: model.implicit_network.raw_sdf(p)
    bound = (-1.1, 1.1)
    res = args.resolution

    def volume():
        return list(render.sdf_volume(sdf, res, bound, shard=False))

    def surface():
        return get_surface_sliding(None, 0, sdf, resolution=res, grid_boundary=list(bound), return_mesh=True)

    volume()                                        # warm-up: code objects, pinned buffer, allocator
    mesh = surface()
    t_vol, all_vol = _median_wall(volume, args.repeats)
    t_surf, all_surf = _median_wall(surface, args.repeats)

    # the two entry points alone on the first block's device volume, HIP events around each call
    origin, spacing, vol = next(render.sdf_volume_device(sdf, res, bound, shard=False))
    marching_cubes(vol, 0.0, spacing)
    prof = {}
    _lib.PROFILE = prof
    try:
        t_mc, all_mc = _median_wall(lambda: marching_cubes(vol, 0.0, spacing), args.repeats)
    finally:
        _lib.PROFILE = None
    torch.cuda.synchronize()
    ev = {k: float(np.median([a.elapsed_time(b) for a, b in v])) * 1e3 for k, v in prof.items()}   # microseconds
    verts, faces, _ = marching_cubes(vol, 0.0, spacing)
    n = vol.numel()
    vol_bytes = 4 * n
    n_words = (n + 63) // 64
    count_bytes = vol_bytes + 40 * n_words * 3      # volume once; workspace written, read by the scan, rewritten
    out = {
        'what': 'mesh export of the bench model, grid function raw_sdf, resolution %d (%d block(s) of %d^3)' % (
            res, (res // vol.shape[0]) ** 3, vol.shape[0]),
        'device': torch.cuda.get_device_name(0),
        'sdf_volume_s': round(t_vol, 4), 'sdf_volume_s_all': all_vol,
        'get_surface_sliding_s': round(t_surf, 4), 'get_surface_sliding_s_all': all_surf,
        'surface_over_volume': round(t_surf / t_vol, 4),
        'mesh': {'vertices': int(len(mesh.vertices)), 'faces': int(len(mesh.faces))},
        'block': {'voxels': n, 'vertices': int(verts.shape[0]), 'faces': int(faces.shape[0])},
        'marching_cubes_call_s': round(t_mc, 6),
        'msdf_mc_count_us': round(ev['msdf_mc_count'], 1),
        'msdf_mc_emit_us': round(ev['msdf_mc_emit'], 1),
        'count_roofline': {
            'volume_bytes': vol_bytes,
            'floor_us_volume_once': round(vol_bytes / HBM_PEAK * 1e6, 1),
            'count_bytes_model': count_bytes,
            'fraction_of_hbm_peak': round(count_bytes / (ev['msdf_mc_count'] * 1e-6) / HBM_PEAK, 3),
            'note': 'msdf_mc_count = classify + 3 scan kernels; the classify kernel alone is in the rocprofv3 stats',
        },
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
