"""Re-fuse or cull a reconstructed mesh with the cameras that saw the scene, on the GPU, before it is scored.

    python scripts/refuse_mesh.py IN.ply OUT.ply --poses DIR|FILE --intrinsic FILE --size H W
                                  [--every 10] [--voxel 0.01] [--mode refuse|cull] [--scale-mat cameras.npz]

refuse: refuse() of scannet_eval/evaluate.py:111-137 (postprocess/refuse.py at --voxel 0.001): depth maps of the mesh
from every --every-th pose, fused into a TSDF volume, a new mesh extracted: surface no camera saw is gone.
cull:   replica_eval/cull_mesh.py: faces whose vertices lie in no camera frustum are dropped.
--poses: a directory of ScanNet `N.txt` files (one 4x4 camera-to-world matrix each, taken in ascending N) or a Replica
`traj.txt` (16 numbers per line).  --intrinsic: a text file with the 3x3 / 4x4 intrinsic matrix (ScanNet's
intrinsic_color.txt) or the four numbers fx fy cx cy.  --size: image height and width (ScanNet 968 1296, Replica 680 1200).
--scale-mat: a cameras.npz whose `scale_mat_0` takes IN.ply from the normalised training frame to the world frame of
the poses, applied first.  OUT.ply feeds scripts/eval_mesh.py as it is.  Prints one JSON line with the sizes.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mesh_in')
    ap.add_argument('mesh_out')
    ap.add_argument('--poses', required=True, help='directory of N.txt poses, or a traj.txt')
    ap.add_argument('--intrinsic', required=True, help='text file: intrinsic matrix, or fx fy cx cy')
    ap.add_argument('--size', type=int, nargs=2, required=True, metavar=('H', 'W'))
    ap.add_argument('--every', type=int, default=10, help='use every N-th pose (the reference: 10 for refuse)')
    ap.add_argument('--voxel', type=float, default=0.01, help='refuse: voxel length (truncation is 3 voxels)')
    ap.add_argument('--depth-trunc', type=float, default=5.0, help='refuse: depths beyond this are ignored')
    ap.add_argument('--view-chunk', type=int, default=None, help='refuse: depth maps held at a time (default: all)')
    ap.add_argument('--mode', choices=('refuse', 'cull'), default='refuse')
    ap.add_argument('--scale-mat', default=None)
    args = ap.parse_args()
    from monosdf_amd.utils import mesh_eval, mesh_refuse
    mesh = mesh_eval.read_ply(args.mesh_in)
    if args.scale_mat:
        mesh.apply_transform(np.load(args.scale_mat)['scale_mat_0'])
    poses = mesh_refuse.read_poses(args.poses, every=max(1, args.every))
    K = mesh_refuse.read_intrinsics(args.intrinsic)
    h, w = args.size
    if args.mode == 'refuse':
        out = mesh_refuse.refuse(mesh, poses, K, h, w, voxel_length=args.voxel, depth_trunc=args.depth_trunc,
                                 view_chunk=args.view_chunk)
    else:
        out = mesh_refuse.cull_to_frustums(mesh, poses, K, h, w)
    out.export(args.mesh_out, 'ply')
    print(json.dumps({'mode': args.mode, 'views': int(len(poses)), 'vertices_in': int(len(mesh.vertices)),
                      'faces_in': int(len(mesh.faces)), 'vertices_out': int(len(out.vertices)),
                      'faces_out': int(len(out.faces))}))


if __name__ == '__main__':
    main()
