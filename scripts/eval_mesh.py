"""Metrics of a reconstructed mesh against a ground-truth mesh, on the GPU, as one JSON line.

    python scripts/eval_mesh.py PRED.ply GT.ply --protocol scannet|replica [--scale-mat cameras.npz]

scannet: evaluate() of scannet_eval/evaluate.py (vertex clouds, 2 cm voxel down-sample, 5 cm threshold).
replica: the metrics of calc_3d_metric() of replica_eval/eval_recon.py (200,000 surface samples per mesh, 5 cm).
--scale-mat: a cameras.npz whose `scale_mat_0` takes the predicted mesh from the normalised training frame to the
world frame (evaluation/eval.py applies it before it writes the mesh; pass it when PRED.ply was written without).
The meshes must be aligned already: ICP and the bounding-box crop are not done here (monosdf_amd/utils/mesh_eval.py).
The reference scores the re-fused (ScanNet) or frustum-culled (Replica) mesh: make PRED.ply with scripts/refuse_mesh.py.
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
    ap.add_argument('pred')
    ap.add_argument('gt')
    ap.add_argument('--protocol', choices=('scannet', 'replica'), required=True)
    ap.add_argument('--scale-mat', default=None)
    ap.add_argument('--threshold', type=float, default=0.05)
    ap.add_argument('--down-sample', type=float, default=0.02, help='scannet: voxel size (0: none)')
    ap.add_argument('--n-samples', type=int, default=200000, help='replica: surface samples per mesh')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    from monosdf_amd.utils import mesh_eval
    pred, gt = mesh_eval.read_ply(args.pred), mesh_eval.read_ply(args.gt)
    if args.scale_mat:
        pred.apply_transform(np.load(args.scale_mat)['scale_mat_0'])
    if args.protocol == 'scannet':
        out = mesh_eval.evaluate_scannet(pred, gt, threshold=args.threshold, down_sample=args.down_sample)
    else:
        out = mesh_eval.evaluate_replica(pred, gt, n_samples=args.n_samples, dist_th=args.threshold, seed=args.seed)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
