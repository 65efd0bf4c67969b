"""Rigidly align one mesh to another by point-to-point ICP on their vertices, on the GPU.

    python scripts/align_mesh.py SRC.ply TGT.ply OUT.ply [--max-dist 0.1] [--init FILE] [--save-transform FILE]

What get_align_transformation() of replica_eval/eval_recon.py does through open3d before calc_3d_metric(align=True)
scores a mesh (monosdf_amd/utils/mesh_align.py; parity with open3d is unverified).  --init: a 4 x 4 start transform, a
text file of four rows or an .npy (default: the identity, as the reference).  OUT.ply is SRC.ply moved by the
transform found (vertices and normals); --save-transform writes the 4 x 4 as text (.npy: as an array).  Prints one
JSON line: the transform, fitness, inlier rmse and the number of evaluations.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('src')
    ap.add_argument('tgt')
    ap.add_argument('out')
    ap.add_argument('--max-dist', type=float, default=0.1, help='the correspondence distance')
    ap.add_argument('--init', default=None, help='a 4 x 4 start transform (text or .npy)')
    ap.add_argument('--save-transform', default=None)
    args = ap.parse_args()
    from monosdf_amd.utils import mesh_align, mesh_eval
    src, tgt = mesh_eval.read_ply(args.src), mesh_eval.read_ply(args.tgt)
    init = None
    if args.init:
        init = np.load(args.init) if args.init.endswith('.npy') else np.loadtxt(args.init)
    T, fitness, rmse, _, evaluations = mesh_align.icp(src.vertices.astype(np.float32), tgt.vertices.astype(np.float32),
                                                      args.max_dist, init=init, return_log=True)
    src.apply_transform(T).export(args.out)
    if args.save_transform:
        if args.save_transform.endswith('.npy'):
            np.save(args.save_transform, T)
        else:
            np.savetxt(args.save_transform, T, fmt='%.17g')
    print(json.dumps({'transformation': T.tolist(), 'fitness': fitness, 'inlier_rmse': rmse,
                      'evaluations': evaluations}))


if __name__ == '__main__':
    main()
