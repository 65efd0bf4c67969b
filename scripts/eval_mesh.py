"""Metrics of a reconstructed mesh against a ground-truth mesh, on the GPU, as one JSON line.

    python scripts/eval_mesh.py PRED.ply GT.ply --protocol scannet|replica [--scale-mat cameras.npz] [--crop] [--align]
                                         [--depth-l1 [--unseen FILE.npy] [--n-imgs N]]
    python scripts/eval_mesh.py PRED.ply --protocol dtu --dtu-dir DTU --scan 24 [--cameras cameras.npz --masks DIR|NPY]
                                         [--search brute|grid]

scannet: evaluate() of scannet_eval/evaluate.py (vertex clouds, 2 cm voxel down-sample, 5 cm threshold).
replica: the metrics of calc_3d_metric() of replica_eval/eval_recon.py (200,000 surface samples per mesh, 5 cm).
dtu: evaluate_single_scene.py + eval.py of dtu_eval (monosdf_amd/utils/mesh_dtu.py): with --cameras and --masks the mesh
(in the normalised training frame) is first culled to the dilated object masks and taken to the world frame by
`scale_mat_0`; without them PRED.ply must be culled and in the world frame already.  --dtu-dir holds the official
ObsMask/ and Points/stl/ folders.  Prints d2s, s2d and their mean in millimetres.  --search grid runs the two closing
distance queries through the grid-bounded search (nearest_neighbors_within): the same numbers, sooner.
--scale-mat: a cameras.npz whose `scale_mat_0` takes the predicted mesh from the normalised training frame to the
world frame (evaluation/eval.py applies it before it writes the mesh; pass it when PRED.ply was written without).
--align (replica) first moves PRED onto GT by point-to-point ICP on the vertices, as calc_3d_metric(align=True) does
(monosdf_amd/utils/mesh_align.py; parity with open3d's ICP is unverified); without it the meshes must be aligned
already.  --crop (replica) then crops PRED to the oriented bounding box of GT scaled by 1.05, as calc_3d_metric() always
does (monosdf_amd/utils/mesh_bounds.py); without it PRED is scored as it came.
--depth-l1 (replica) adds `depth_l1_cm`, the 2D metric of calc_2d_metric(): both meshes rendered from --n-imgs (1000)
random views inside the room, redrawn while they see a point of --unseen (the scene's `*_pc_unseen.npy`), mean absolute
depth difference in centimetres (monosdf_amd/utils/mesh_render.py; parity with open3d's renderer is unverified).  With
--align PRED is aligned for it as for the 3D metrics.  Without the flag the output is unchanged.
The reference scores the re-fused (ScanNet) or frustum-culled (Replica) mesh: make PRED.ply with scripts/refuse_mesh.py.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def evaluate_dtu(ap, args):
    from monosdf_amd.utils import mesh_dtu, mesh_eval
    if args.dtu_dir is None or args.scan is None:
        ap.error('--protocol dtu needs --dtu-dir and --scan')
    if (args.cameras is None) != (args.masks is None):
        ap.error('the mask cull needs both --cameras and --masks')
    pred = mesh_eval.read_ply(args.pred)
    if args.cameras:
        masks = mesh_dtu.read_masks(args.masks)
        pred = mesh_dtu.cull_to_masks(pred, mesh_dtu.dtu_projections(args.cameras, len(masks)), masks)
        pred.apply_transform(np.load(args.cameras)['scale_mat_0'])
    elif args.scale_mat:
        pred.apply_transform(np.load(args.scale_mat)['scale_mat_0'])
    scene = mesh_dtu.read_dtu_scene(args.dtu_dir, args.scan)
    return mesh_dtu.evaluate_dtu(pred, scene['stl_points'], scene['obs_mask'], scene['bb'], scene['res'],
                                 scene['plane'], density=args.density, seed=args.seed, search=args.search)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('pred')
    ap.add_argument('gt', nargs='?', default=None, help='scannet, replica: the ground-truth mesh')
    ap.add_argument('--protocol', choices=('scannet', 'replica', 'dtu'), required=True)
    ap.add_argument('--dtu-dir', default=None, help='dtu: the official evaluation data (ObsMask/, Points/stl/)')
    ap.add_argument('--scan', type=int, default=None, help='dtu: the scan number')
    ap.add_argument('--cameras', default=None, help='dtu: the scene\'s cameras.npz, for the mask cull')
    ap.add_argument('--masks', default=None, help='dtu: the scene\'s mask directory or an .npy stack [n, H, W]')
    ap.add_argument('--density', type=float, default=0.2, help='dtu: sampling and thinning distance')
    ap.add_argument('--search', choices=('brute', 'grid'), default='brute',
                    help='dtu: the two closing nearest-neighbour queries by brute force or through the grid')
    ap.add_argument('--scale-mat', default=None)
    ap.add_argument('--threshold', type=float, default=0.05)
    ap.add_argument('--down-sample', type=float, default=0.02, help='scannet: voxel size (0: none)')
    ap.add_argument('--n-samples', type=int, default=200000, help='replica: surface samples per mesh')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--crop', action='store_true',
                    help='replica: crop PRED to the oriented bounding box of GT scaled by 1.05 first')
    ap.add_argument('--align', action='store_true',
                    help='replica: move PRED onto GT by point-to-point ICP on the vertices first')
    ap.add_argument('--depth-l1', action='store_true',
                    help='replica: add the depth L1 of calc_2d_metric() in centimetres')
    ap.add_argument('--unseen', default=None, help='replica, --depth-l1: .npy cloud no view may see')
    ap.add_argument('--n-imgs', type=int, default=1000, help='replica, --depth-l1: views')
    args = ap.parse_args()
    from monosdf_amd.utils import mesh_eval
    if args.depth_l1 and args.protocol != 'replica':
        ap.error('--depth-l1 belongs to --protocol replica')
    if (args.unseen is not None or args.n_imgs != 1000) and not args.depth_l1:
        ap.error('--unseen and --n-imgs belong to --depth-l1')
    if args.crop and args.protocol != 'replica':
        ap.error('--crop belongs to --protocol replica')
    if args.align and args.protocol != 'replica':
        ap.error('--align belongs to --protocol replica')
    if args.protocol == 'dtu':
        print(json.dumps(evaluate_dtu(ap, args)))
        return
    if args.gt is None:
        ap.error('--protocol %s needs PRED.ply and GT.ply' % args.protocol)
    pred, gt = mesh_eval.read_ply(args.pred), mesh_eval.read_ply(args.gt)
    if args.scale_mat:
        pred.apply_transform(np.load(args.scale_mat)['scale_mat_0'])
    if args.protocol == 'scannet':
        out = mesh_eval.evaluate_scannet(pred, gt, threshold=args.threshold, down_sample=args.down_sample)
    else:
        out = mesh_eval.evaluate_replica(pred, gt, n_samples=args.n_samples, dist_th=args.threshold, seed=args.seed,
                                           crop=args.crop, align=args.align)
        if args.depth_l1:
            from monosdf_amd.utils import mesh_render
            out['depth_l1_cm'] = mesh_render.evaluate_depth_l1(
                pred, gt, n_imgs=args.n_imgs, unseen=None if args.unseen is None else np.load(args.unseen),
                align=args.align, seed=args.seed)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
