"""Remove floaters from a mesh on the GPU: merge duplicate vertices, split into connected components, keep the
largest or those above a size.

    python scripts/clean_mesh.py IN.ply OUT.ply [--merge DIGITS] [--connectivity edge|edge_any|vertex]
                                 [--keep-largest [area|faces]] [--min-faces N] [--min-area A]

The steps run in that order, each only when its option is given (utils/mesh_clean.py).  --merge: vertices whose
coordinates agree after rounding to DIGITS decimals become one (trimesh's merge_vertices uses 8; a mesh that
get_surface_sliding concatenated from blocks needs a coarser value, such as 5, to close the block seams).
--connectivity: 'edge' is trimesh's split rule.  --keep-largest: the component of largest area (default) or face
count.  --min-faces / --min-area: drop the components below either bound.  Prints the component count and the five
largest components by area, before and after, as one JSON line; OUT.ply feeds scripts/eval_mesh.py as it is.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def describe(mesh, connectivity):
    """Component count and the five largest components by area."""
    import torch
    from monosdf_amd.utils import mesh_clean
    labels, n = mesh_clean.face_components(mesh, connectivity)
    out = {'vertices': int(len(mesh.vertices)), 'faces': int(len(mesh.faces)), 'components': n, 'largest_by_area': []}
    if n:
        count, area = mesh_clean.component_sizes(mesh, labels, n)
        top = torch.sort(area, descending=True, stable=True)[1][:5]
        out['largest_by_area'] = [{'component': int(i), 'faces': int(count[i]), 'area': float(area[i])} for i in top]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mesh_in')
    ap.add_argument('mesh_out')
    ap.add_argument('--merge', type=int, default=None, metavar='DIGITS')
    ap.add_argument('--connectivity', choices=('edge', 'edge_any', 'vertex'), default='edge')
    ap.add_argument('--keep-largest', nargs='?', const='area', default=None, choices=('area', 'faces'))
    ap.add_argument('--min-faces', type=int, default=None)
    ap.add_argument('--min-area', type=float, default=None)
    args = ap.parse_args()
    from monosdf_amd.utils import mesh_clean
    from monosdf_amd.utils.mesh import read_ply
    mesh = read_ply(args.mesh_in)
    if args.merge is not None:
        mesh = mesh_clean.merge_vertices(mesh, args.merge)
    report = {'connectivity': args.connectivity, 'merge_digits': args.merge, 'before': describe(mesh, args.connectivity)}
    if args.keep_largest is not None:
        mesh = mesh_clean.largest_component(mesh, args.connectivity, args.keep_largest)
    if args.min_faces is not None or args.min_area is not None:
        mesh = mesh_clean.remove_small_components(mesh, args.min_faces, args.min_area, args.connectivity)
    report['after'] = describe(mesh, args.connectivity)
    mesh.export(args.mesh_out, 'ply')
    print(json.dumps(report))


if __name__ == '__main__':
    main()
