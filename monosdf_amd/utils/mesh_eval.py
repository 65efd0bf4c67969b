"""Mesh evaluation on the GPU: what the reference's scripts compute after the mesh export.

* ``nearest_neighbors``: exact brute-force 1-nearest-neighbour search (csrc/nnsearch.hip, ABI msdf_nn_*), in place of
  sklearn's ``KDTree(...).query`` (scannet_eval/evaluate.py:16-26) and scipy's ``cKDTree(...).query``
  (replica_eval/eval_recon.py:25-43, 96-106).
* ``nearest_neighbors_within``: the same answer, bit for bit, for the queries that have a reference point within
  ``max_dist``, through a uniform grid (utils/point_grid.py's ``PointGrid``, built and queried once per call;
  csrc/gridnn.hip): the search of the DTU protocol's two closing queries, which use only the distances below
  ``max_dist``.  ``grid_dims`` and the two ``GRID_*`` defaults of that module are importable from here too.
* ``voxel_down_sample``: the rule of open3d's ``PointCloud.voxel_down_sample`` (evaluate.py:36-38; ABI msdf_voxel_*).
* ``sample_surface``, ``face_normals``: trimesh.sample.sample_surface and Trimesh.face_normals (eval_recon.py:138-158).
* ``evaluate_scannet``: ``evaluate`` (evaluate.py:29-56).  ``evaluate_replica``: the metrics of ``calc_3d_metric``
  (eval_recon.py:138-177).
* ``read_ply``: utils/mesh.py's PLY reader, importable from here as before.

Everything runs on CUDA tensors; there is no CPU path.  Arguments are checked by utils/mesh_args.py: every function
that takes a mesh validates it once (``mesh_tensors``) and hands it on to the unchecked ``_face_cross``.
The oriented-bounding-box crop that ``calc_3d_metric`` applies first (eval_recon.py:121-136) is in
utils/mesh_bounds.py; ``evaluate_replica(..., crop=True)`` runs it.
The ICP alignment (``get_align_transformation``, which ``calc_3d_metric(align=True)`` runs first) is in
utils/mesh_align.py; ``evaluate_replica(..., align=True)`` runs it.
Out of scope: the coloured error clouds that ``calc_3d_metric`` writes, ``calc_2d_metric``, and an unbounded grid- or
tree-accelerated search: the means of the ScanNet and Replica protocols need every distance, their brute-force searches take milliseconds, and brute force is the exact baseline
that ``nearest_neighbors_within`` is checked against.  View culling and TSDF re-fusion (``refuse``), which the reference applies to the predicted mesh
before it calls these metrics, are in utils/mesh_refuse.py; the DTU protocol and its mask culling are in
utils/mesh_dtu.py.
"""
import numpy as np
import torch

from . import mesh_args as ma
from .mesh import read_ply                                   # noqa: F401 (public here too)
from .point_grid import GRID_CELL_FRACTION, GRID_MAX_CELLS, PointGrid, grid_dims    # noqa: F401 (public here too)


def nearest_neighbors(reference, query, n_splits=0):
    """For every ``query[i]`` the closest point of ``reference``: ``(dist [Q] float32, idx [Q] int64)``, exact, by
    brute force on the GPU.  reference [R,3], query [Q,3]: float32 CUDA tensors on one device.

    The squared distance is dx^2 + dy^2 + dz^2 of the three fp32 differences (relative error of ``dist`` about 2.4e-7
    wherever the clouds lie).  Of several reference points at the same fp32 squared distance the smallest index wins.
    The same inputs give bitwise the same outputs every call and for every ``n_splits`` (over how many slices of the
    reference cloud the work is spread; 0 = chosen from the sizes).  ValueError for an empty reference cloud and for
    non-finite coordinates (one device reduction and one host read)."""
    name = 'nearest_neighbors'
    ma.check_tensor(name, 'reference', reference)
    ma.check_tensor(name, 'query', query)
    dev = ma.same_device(name, reference=reference, query=query)
    R, Q = reference.shape[0], query.shape[0]
    if R == 0:
        raise ValueError('%s: the reference cloud is empty' % name)
    ref, qry = reference.contiguous(), query.contiguous()
    if not bool((torch.isfinite(ref).all() & torch.isfinite(qry).all()).item()):
        raise ValueError('%s: non-finite coordinates' % name)
    dist = torch.empty(Q, dtype=torch.float32, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q > 0:
        with torch.cuda.device(dev):
            ws = ma.workspace(name, 'msdf_nn_workspace_bytes', R, Q, int(n_splits), device=dev)
            ma.call('msdf_nn_search', ref, R, qry, Q, int(n_splits), ws, dist, idx)
    return dist, idx.long()


def nearest_neighbors_within(reference, query, max_dist, cell=None, max_cells=None):
    """``nearest_neighbors(reference, query)`` for the queries that have a reference point within ``max_dist``:
    ``(dist [Q] float32, idx [Q] int64)``.  With (d, i) what ``nearest_neighbors`` returns for a query: bitwise (d, i)
    if d <= float32(max_dist), else (+inf, -1).  reference [R,3], query [Q,3]: float32 CUDA tensors on one device.

    Exact, through a uniform grid over the reference cloud's bounding box: the reference points are sorted by cell
    (a stable ``torch.sort``), a dense table holds every cell's first point, and a query scans the cube of cells within
    1, 2, 4, ... cells of its own until no point outside the cube can be as near as the best inside it, or the cube
    reaches ``max_dist`` (csrc/gridnn.hip has the argument).  ``cell``: the cell side (default ``max_dist`` / 16);
    ``max_cells``: the cap of the cell count (default 2^25), to which the cell side is enlarged.  Both change the speed
    only: the result does not depend on them, and is bitwise the same every call (no atomics).  A query with no
    neighbour within ``max_dist`` walks every cube up to that distance: the search is fast where most queries have a
    near neighbour.  ValueError for an empty reference cloud, non-finite coordinates, a ``max_dist`` that is not
    positive and finite (as a float32 too), and a ``cell`` or ``max_cells`` that is given and not positive."""
    name = 'nearest_neighbors_within'
    ma.check_tensor(name, 'reference', reference)
    ma.check_tensor(name, 'query', query)
    dev = ma.same_device(name, reference=reference, query=query)
    md = ma.search_distance(name, max_dist)
    h = md / GRID_CELL_FRACTION if cell is None else ma.positive_number(name, 'cell', cell)
    cap = GRID_MAX_CELLS if max_cells is None else ma.positive_number(name, 'max_cells', max_cells)
    R, Q = reference.shape[0], query.shape[0]
    if R == 0:
        raise ValueError('%s: the reference cloud is empty' % name)
    ref, qry = reference.contiguous(), query.contiguous()
    _, lo_h, hi_h = ma.finite_bounds(name, ref)
    if Q > 0 and not bool(torch.isfinite(qry).all().item()):
        raise ValueError('%s: non-finite coordinates' % name)
    if Q == 0:
        return (torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
    with torch.cuda.device(dev):
        return PointGrid(ref, lo_h, hi_h, h, cap).query(qry, md)


_VOXEL_AXIS_MAX = 2 ** 21            # cells per axis the 63-bit voxel key holds


def voxel_down_sample(points, voxel_size):
    """One point per occupied voxel, the mean of the points in it: points [N,3] float32 CUDA -> [M,3].

    The rule of open3d's ``PointCloud.voxel_down_sample``: voxel of a point = floor((p - (min_bound - v/2)) / v) per
    axis with min_bound the per-axis minimum of the cloud.  Arithmetic: the voxel coordinate in fp32 with separately
    rounded operations, the sum of a voxel in fp64 in ascending original point index, rounded once to fp32.  Output
    order: ascending (ix, iy, iz).  No floating-point atomics: the same cloud gives bitwise the same output every call.
    Parity with open3d's own binning is UNVERIFIED: open3d is not available where this is built and the reference
    holds no recorded output of it, so the rule is pinned by the numpy restatement of the tests only (a point within
    rounding of a voxel face may fall on the other side there, and open3d's output order is its hash map's)."""
    name = 'voxel_down_sample'
    ma.check_tensor(name, 'points', points)
    v = float(np.float32(voxel_size))
    if not v > 0.0:
        raise ValueError('%s: voxel_size must be positive, got %r' % (name, voxel_size))
    n = points.shape[0]
    dev = points.device
    if n == 0:
        return points.new_empty(0, 3)
    pts = points.contiguous()
    lo, lo_h, hi_h = ma.finite_bounds(name, pts)
    if float(((hi_h - lo_h) / v).max()) + 2.0 >= _VOXEL_AXIS_MAX:
        raise ValueError('%s: more than 2^21 voxels along an axis (extent %g, voxel %g)' %
                         (name, float((hi_h - lo_h).max()), v))
    with torch.cuda.device(dev):
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        ma.call('msdf_voxel_keys', pts, n, lo.contiguous(), v, keys)
        sorted_keys, order = torch.sort(keys, stable=True)
        head = torch.ones(n, dtype=torch.bool, device=dev)
        head[1:] = sorted_keys[1:] != sorted_keys[:-1]
        seg_start = head.nonzero().squeeze(1).contiguous()
        m = seg_start.shape[0]
        out = torch.empty(m, 3, dtype=torch.float32, device=dev)
        ma.call('msdf_voxel_mean', pts, order, seg_start, n, m, out)
    return out


def _face_cross(vertices, faces):
    """origin, the two edge vectors and their cross product per face, in fp64.  Indexes with ``faces`` as they are:
    only for a mesh that ``mesh_args.mesh_tensors`` has passed."""
    tri = vertices.double()[faces.long()]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    return tri[:, 0], e1, e2, torch.linalg.cross(e1, e2)


def face_normals(vertices, faces):
    """Unit normals by the right-hand rule, [F,3] float32; zero for degenerate (zero-area) faces.  ValueError for a
    face index outside [0, V) and for non-finite vertices (as in every function here that takes a mesh)."""
    return _face_normals(*ma.mesh_tensors('face_normals', (vertices, faces))[:2])


def _face_normals(vertices, faces):
    c = _face_cross(vertices, faces)[3]
    norm = c.norm(dim=1, keepdim=True)
    return torch.where(norm > 0, c / torch.where(norm > 0, norm, torch.ones_like(norm)),
                       torch.zeros_like(c)).float()


def sample_surface(vertices, faces, count, generator=None):
    """``count`` points uniform on the surface, as trimesh.sample.sample_surface: a face drawn with probability
    proportional to its area, a uniform point in it (the unit square folded onto the triangle).
    -> (points [count,3] float32, face_index [count] int64).  Degenerate (zero-area) faces are never drawn.
    ``generator``: a torch.Generator on the vertices' device; the same seed gives the same samples."""
    return _sample_surface(*ma.mesh_tensors('sample_surface', (vertices, faces))[:2], count, generator)


def _sample_surface(vertices, faces, count, generator):
    dev = vertices.device
    origin, e1, e2, c = _face_cross(vertices, faces)
    cum = torch.cumsum(0.5 * c.norm(dim=1), 0)
    if faces.shape[0] == 0 or not float(cum[-1]) > 0.0:
        raise ValueError('sample_surface: the mesh has no area')
    u = torch.rand(count, 3, dtype=torch.float64, device=dev, generator=generator)
    # pick in [0, total): face i is drawn for cum[i-1] <= pick < cum[i], an empty interval for a zero-area face
    pick = torch.minimum(u[:, 0] * cum[-1], torch.nextafter(cum[-1], torch.zeros_like(cum[-1])))
    face_index = torch.searchsorted(cum, pick, right=True)
    a, b = u[:, 1], u[:, 2]
    fold = a + b > 1.0
    a, b = torch.where(fold, 1.0 - a, a), torch.where(fold, 1.0 - b, b)
    pts = origin[face_index] + a[:, None] * e1[face_index] + b[:, None] * e2[face_index]
    return pts.float(), face_index


def _fscore(p, r):
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def evaluate_scannet(pred_vertices, gt_vertices, threshold=0.05, down_sample=0.02):
    """``evaluate`` of scannet_eval/evaluate.py:29-56 on two vertex clouds (float32 CUDA tensors [N,3]; numpy arrays
    and Mesh objects are uploaded): both voxel-down-sampled (``down_sample`` = 0 / None: not), nearest neighbours both
    ways, then with the reference's keys, as Python floats:
      'Acc'   mean distance from the predicted points to the target cloud      'Prec'  share of them < threshold
      'Comp'  mean distance from the target points to the predicted cloud      'Recal' share of them < threshold
      'F-score' 2 Prec Recal / (Prec + Recal), 0.0 when both are zero.
    The down-sample follows open3d's rule but its parity with open3d is unverified (see voxel_down_sample)."""
    dev = ma.device_of(pred_vertices, gt_vertices)
    pred = ma.cloud_tensor('evaluate_scannet', 'pred_vertices', pred_vertices, dev)
    gt = ma.cloud_tensor('evaluate_scannet', 'gt_vertices', gt_vertices, dev)
    if down_sample:
        pred, gt = voxel_down_sample(pred, down_sample), voxel_down_sample(gt, down_sample)
    if pred.shape[0] == 0 or gt.shape[0] == 0:
        raise ValueError('evaluate_scannet: an empty cloud')
    dist1, _ = nearest_neighbors(pred, gt)              # target -> predicted
    dist2, _ = nearest_neighbors(gt, pred)              # predicted -> target
    vals = torch.stack([dist2.double().mean(), dist1.double().mean(), (dist2 < threshold).double().mean(),
                        (dist1 < threshold).double().mean()]).tolist()
    acc, comp, prec, recal = vals
    return {'Acc': acc, 'Comp': comp, 'Prec': prec, 'Recal': recal, 'F-score': _fscore(prec, recal)}


def evaluate_replica(rec, gt, n_samples=200000, dist_th=0.05, seed=0, return_samples=False, crop=False, align=False):
    """The metrics of ``calc_3d_metric`` (replica_eval/eval_recon.py:138-177).  ``rec``, ``gt``: Mesh objects or
    (vertices [V,3], faces [F,3]) pairs (CUDA tensors, or numpy arrays, which are uploaded).  ``n_samples``
    area-weighted surface samples of each mesh (``seed`` fixes them), nearest neighbours both ways, then:
      'accuracy'  mean distance rec -> gt, cm            'precision'         share of rec samples within dist_th, %
      'completion' mean distance gt -> rec, cm           'completion_ratio'  share of gt samples within dist_th, %
      'fscore'    2 P R / (P + R) of those two, %, 0.0 when both are zero
      'chamfer'   (accuracy + completion) / 2, cm
      'normal_acc' / 'normal_comp'  mean |cos| between the face normal of a rec / gt sample and the face normal of its
                  nearest neighbour in the other cloud, %;  'normal_avg' their mean.
    The reference draws a second set of samples for the normals; here one set serves both.  ``crop``: True crops
    ``rec`` to the oriented bounding box of ``gt`` scaled by 1.05 first, as ``calc_3d_metric`` always does
    (eval_recon.py:121-136; utils/mesh_bounds.crop_to_oriented_bounds); False (the default) scores ``rec`` as it came.
    ``align``: True first moves ``rec`` onto ``gt`` by point-to-point ICP on the vertices, before the crop, the order
    of ``calc_3d_metric(align=True)`` (eval_recon.py:51-65, 113-117; utils/mesh_align.align_mesh, whose parity with
    open3d's ICP is unverified); False (the default) takes the meshes as aligned.  ``return_samples``: also a dict with
    'rec_points', 'rec_faces', 'gt_points', 'gt_faces' (the samples and the face each came from), 'rec_normals',
    'gt_normals' (per sample)."""
    name = 'evaluate_replica'
    if align:
        from .mesh_align import align_mesh
        rec = align_mesh(rec, gt)[0]
    if crop:
        from .mesh_bounds import crop_to_oriented_bounds
        rec = crop_to_oriented_bounds(rec, gt)
    rv, rf, _ = ma.mesh_tensors(name, rec, ma.device_of(*ma.mesh_parts(gt)))
    gv, gf, _ = ma.mesh_tensors(name, gt, rv.device)
    ma.same_device(name, rec=rv, gt=gv)
    gen = torch.Generator(device=rv.device)
    gen.manual_seed(int(seed))
    rp, rfi = _sample_surface(rv, rf, n_samples, gen)
    gp, gfi = _sample_surface(gv, gf, n_samples, gen)
    rn, gn = _face_normals(rv, rf)[rfi], _face_normals(gv, gf)[gfi]
    d_acc, i_gt = nearest_neighbors(gp, rp)             # rec -> gt
    d_comp, i_rec = nearest_neighbors(rp, gp)           # gt -> rec
    n_acc = (rn.double() * gn.double()[i_gt]).sum(1).abs().mean()
    n_comp = (gn.double() * rn.double()[i_rec]).sum(1).abs().mean()
    vals = torch.stack([d_acc.double().mean(), d_comp.double().mean(), (d_acc < dist_th).double().mean(),
                        (d_comp < dist_th).double().mean(), n_acc, n_comp]).tolist()
    acc, comp, prec, ratio, n_acc, n_comp = vals
    out = {'accuracy': acc * 100, 'completion': comp * 100, 'precision': prec * 100, 'completion_ratio': ratio * 100,
           'fscore': _fscore(prec, ratio) * 100, 'chamfer': (acc * 100 + comp * 100) / 2,
           'normal_acc': n_acc * 100, 'normal_comp': n_comp * 100, 'normal_avg': (n_acc + n_comp) * 0.5 * 100}
    if return_samples:
        return out, {'rec_points': rp, 'rec_faces': rfi, 'rec_normals': rn,
                     'gt_points': gp, 'gt_faces': gfi, 'gt_normals': gn}
    return out
