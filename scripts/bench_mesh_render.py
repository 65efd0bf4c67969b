"""Times of the mesh renderer on one MI355X (HIP events after a warm-up, median of --repeats), stage by stage, on the
synthetic room of scripts/bench_refuse.py: the marching-cubes mesh of a 6 x 4 x 3 m box with a sphere in it (about
1e6 faces), 8 views of 1080 x 1920 pixels from inside it.

    python scripts/bench_mesh_render.py [--repeats 5] [--views 8] [--size 1080 1920] [--small]
                                        [--out profiles/mesh_render_bench.json]

Stages: render_depth (msdf_raster_depth, the 32-bit depth-only rasteriser, on the same input for comparison),
visibility (msdf_rnd_visibility, cull back and none), vertex_normals (the host's sort and msdf_rnd_vertex_normals),
shade (msdf_rnd_shade), render_frames (all of them and the conversion to bytes), depth_l1 and views_see.  --small: a
quarter of the resolution everywhere (a quick check that the script runs).  The numbers are recorded, not judged: there
is no earlier implementation to compare against.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=(1080, 1920))
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_render.py needs a GPU')
    from bench_refuse import camera_poses, room_mesh, timed
    from monosdf_amd.utils import mesh_refuse as mr
    from monosdf_amd.utils import mesh_render as mrd
    h, w = args.size
    step, n = 0.0125, args.views
    if args.small:
        h, w, step = h // 4, w // 4, step * 4
    K = (w * 0.5, w * 0.5, w / 2 - 0.5, h / 2 - 0.5)
    verts, faces = room_mesh(step)
    poses = camera_poses(n, 0)
    out = {'what': 'mesh renderer, stage by stage (HIP events, median of repeats, seconds)',
           'device': torch.cuda.get_device_name(0), 'vertices': int(verts.shape[0]), 'faces': int(faces.shape[0]),
           'views': n, 'height': h, 'width': w, 'stages': {}}

    def stage(name, fn, **extra):
        t, ts = timed(fn, args.repeats)
        out['stages'][name] = dict(seconds=t, seconds_all=ts, **extra)
        print(name, json.dumps(out['stages'][name]), file=sys.stderr, flush=True)

    px = n * h * w
    stage('render_depth', lambda: mr.render_depth(verts, faces, poses, K, h, w), pixels=px)
    for cull in ('none', 'back'):
        stage('visibility_' + cull, lambda: mrd.visibility(verts, faces, poses, K, h, w, cull=cull), pixels=px)
    depth, face = mrd.visibility(verts, faces, poses, K, h, w, cull='back')
    out['covered_pixels_cull_back'] = int((face >= 0).sum())
    out['depth_equal_to_render_depth_cull_none'] = bool(torch.equal(
        mrd.visibility(verts, faces, poses, K, h, w)[0], mr.render_depth(verts, faces, poses, K, h, w)))
    stage('vertex_normals', lambda: mrd.vertex_normals(verts, faces))
    normals = mrd.vertex_normals(verts, faces)
    stage('shade', lambda: mrd.shade(face, depth, verts, faces, poses, K, normals=normals), pixels=px)
    stage('render_frames', lambda: mrd.render_frames((verts, faces), poses, K, h, w, views_per_call=n), pixels=px)
    other = mr.render_depth(verts + 0.01, faces, poses, K, h, w)
    stage('depth_l1', lambda: mrd.depth_l1(depth, other), pixels=px, bytes=8 * px)
    cloud = verts[::4].contiguous()
    many = camera_poses(256, 1)
    stage('views_see', lambda: mrd.views_see(cloud, many, K, h, w), points=int(cloud.shape[0]), views=256)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
