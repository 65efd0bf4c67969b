"""Merge the monocular cue patches of a scan into one depth map and one normal map per image, on the GPU.

    python scripts/merge_highres_cues.py PATCH_DIR OUT_DIR [--grid 7 14] [--patch 384] [--stride 128] [--batch 4]

PATCH_DIR holds the reference's layout (preprocess/generate_high_res_map.py --mode merge_patches):
%06d_%02d_%02d_depth.npy, %06d_%02d_%02d_normal.npy (row, column) and %06d_mid_depth.npy, %06d_mid_normal.npy.
OUT_DIR receives %06d_depth.npy, %06d_normal.npy and the previews %06d_depth.png, %06d_normal.png
(utils/highres_cues.merge_scan).  Creating the patches, the RGB resize and cameras.npz are not part of this tool.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('patch_dir')
    ap.add_argument('out_dir')
    ap.add_argument('--grid', type=int, nargs=2, default=(7, 14), metavar=('ROWS', 'COLS'))
    ap.add_argument('--patch', type=int, default=384)
    ap.add_argument('--stride', type=int, default=128)
    ap.add_argument('--batch', type=int, default=4, help='images per launch')
    ap.add_argument('--no-previews', action='store_true')
    args = ap.parse_args()
    from monosdf_amd.utils import highres_cues
    t0 = time.perf_counter()
    done = highres_cues.merge_scan(args.patch_dir, args.out_dir, rows=args.grid[0], cols=args.grid[1],
                                   patch=args.patch, stride=args.stride, batch=args.batch,
                                   previews=not args.no_previews)
    h, w = highres_cues.mosaic_size(args.grid[0], args.grid[1], args.patch, args.stride)
    print('merged %d images of %d x %d into %s in %.1f s' % (len(done), h, w, args.out_dir, time.perf_counter() - t0))


if __name__ == '__main__':
    main()
