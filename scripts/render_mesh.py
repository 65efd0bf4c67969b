"""Shaded frames of a mesh along a camera trajectory, on the GPU: what render/render_trajectory_open3d.py and
render_tntvideos_open3d.py of the reference produce with open3d and an OpenGL window (monosdf_amd/utils/mesh_render.py;
parity with open3d's shader is unverified).

    python scripts/render_mesh.py MESH.ply OUT_DIR --cameras DIR_OF_tmpN.json [--options render.json]
    python scripts/render_mesh.py MESH.ply OUT_DIR --poses DIR|FILE --intrinsic FILE --size H W [--options render.json]
                                  [--cull none|back|front] [--flat] [--every N] [--views-per-call 8]

--cameras: a directory of open3d PinholeCameraParameters files ``tmpN.json`` (the reference's trajectories), taken in
ascending N; each brings its own pose; intrinsics and image size are those of the first.  --poses / --intrinsic / --size:
camera-to-world matrices and intrinsics as scripts/refuse_mesh.py reads them.  --options: an open3d RenderOption file
(default: the values of the reference's render/render.json: four lights, white background, back faces hidden).
Writes OUT_DIR/render_%d.jpg through PIL, numbered from 0 in trajectory order.
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mesh')
    ap.add_argument('out_dir')
    ap.add_argument('--cameras', default=None, help='directory of open3d camera files tmpN.json')
    ap.add_argument('--poses', default=None, help='ScanNet pose directory or Replica traj.txt')
    ap.add_argument('--intrinsic', default=None, help='with --poses: a 3x3 / 4x4 matrix or fx fy cx cy')
    ap.add_argument('--size', type=int, nargs=2, default=None, metavar=('H', 'W'), help='with --poses: image size')
    ap.add_argument('--options', default=None, help='open3d RenderOption JSON (default: render.json\'s values)')
    ap.add_argument('--cull', choices=('none', 'back', 'front'), default=None, help='default: what --options says')
    ap.add_argument('--flat', action='store_true', help='face normals instead of smooth vertex normals')
    ap.add_argument('--every', type=int, default=1)
    ap.add_argument('--views-per-call', type=int, default=8)
    args = ap.parse_args()
    if (args.cameras is None) == (args.poses is None):
        ap.error('give --cameras, or --poses with --intrinsic and --size')
    if args.poses is not None and (args.intrinsic is None or args.size is None):
        ap.error('--poses needs --intrinsic and --size')
    from PIL import Image
    from monosdf_amd.utils import mesh_args, mesh_refuse, mesh_render
    from monosdf_amd.utils.mesh import read_ply
    if args.cameras is not None:
        names = [n for n in os.listdir(args.cameras) if re.fullmatch(r'\D*\d+\.json', n)]
        names.sort(key=lambda n: int(re.findall(r'\d+', n)[-1]))
        cams = [mesh_render.read_o3d_camera(os.path.join(args.cameras, n)) for n in names[::args.every]]
        if not cams:
            ap.error('no camera files in %s' % args.cameras)
        poses = np.stack([c[0] for c in cams])
        K, (h, w) = cams[0][1][:4], cams[0][1][4:]
    else:
        poses = mesh_refuse.read_poses(args.poses, args.every)
        K, (h, w) = mesh_refuse.read_intrinsics(args.intrinsic), args.size
    options = mesh_render.RenderOptions() if args.options is None else mesh_render.RenderOptions.from_json(args.options)
    os.makedirs(args.out_dir, exist_ok=True)
    v, f, _ = mesh_args.mesh_tensors('render_mesh', read_ply(args.mesh))     # uploaded and checked once
    chunk = max(1, args.views_per_call)
    for a in range(0, len(poses), chunk):                        # a chunk of frames on the host at a time
        frames = mesh_render.render_frames((v, f), poses[a:a + chunk], K, h, w, options=options,
                                           base_color=options.default_mesh_color, flat=args.flat,
                                           views_per_call=chunk, cull=args.cull).cpu().numpy()
        for k, frame in enumerate(frames):
            Image.fromarray(frame).save(os.path.join(args.out_dir, 'render_%d.jpg' % (a + k)))
    print('%d frames of %d x %d in %s' % (len(poses), h, w, args.out_dir))


if __name__ == '__main__':
    main()
