"""The DTU evaluation protocol on the GPU: the reference's dtu_eval/evaluate_single_scene.py (``cull_scan``) and
dtu_eval/eval.py (csrc/dtueval.hip, ABI msdf_dtu_*; the closing distance queries are ``mesh_eval.nearest_neighbors``
or, with ``search='grid'``, the grid-bounded ``mesh_eval.nearest_neighbors_within``).

* ``dilate_masks``: skimage's ``binary_dilation(mask, disk(12))`` of every view's object mask
  (evaluate_single_scene.py:80-82), all views in one launch on bit-packed rows.
* ``dtu_projections``, ``mask_vertices``, ``cull_to_masks``: every vertex projected into every view and looked up in the
  dilated mask; vertices that fall outside a mask are dropped with their faces (evaluate_single_scene.py:57-97).
* ``sample_lattice``: the deterministic per-triangle lattice sampler (eval.py:54-71) in place of a multiprocessing pool.
* ``radius_thin``: the greedy thinning of eval.py:86-94 (sklearn ``radius_neighbors`` plus a Python loop over every
  point) as a parallel iteration that reaches the same, unique, set.
* ``evaluate_dtu``: the rest of eval.py: bounding box, observation mask, the two one-sided Chamfer means.
* ``read_dtu_scene``, ``read_masks``: the official ObsMask / Plane / stl files; a scene's mask images or an ``.npy`` stack.

Everything runs on CUDA tensors; there is no CPU path.  Arguments are checked by utils/mesh_args.py: every function
that takes a mesh validates it once (``mesh_tensors``) and hands it on to the unchecked ``_lattice``.  Every rule is
integer, boolean, separately rounded fp32 or fp64, with no floating-point atomics: the same inputs give bitwise the
same outputs every call, and the numpy restatements of tests/dtu_numpy.py are matched exactly.  The two closing queries
take nearly all of the protocol's time by brute force; ``evaluate_dtu(..., search='grid')`` gives the same metrics through
the search bounded by ``max_dist``.  Not built: the two coloured error clouds ``vis_*_d2s.ply`` / ``vis_*_s2d.ply`` that
eval.py also writes.
"""
import glob
import os

import numpy as np
import torch

from . import mesh_args as ma
from .mesh import read_ply
from .mesh_eval import nearest_neighbors, nearest_neighbors_within

MAX_RADIUS = 32                      # pixels: the dilation kernel reads a word and its two neighbours
_CELL_AXIS_MAX = 2 ** 21             # cells per axis the 63-bit cell key holds
_CELL_SLACK = 1.0 + 2.0 ** -10       # cell side over radius: rounding of the cell coordinate is ~1e-9 of a cell


def _check_images(name, arg, t):
    """[n, H, W] uint8 / bool masks -> contiguous uint8 (a bool tensor viewed, not copied)."""
    ma.check_tensor(name, arg, t, (torch.uint8, torch.bool), '[n, H, W]')
    if t.shape[1] < 1 or t.shape[2] < 1 or t.numel() > 2 ** 37:
        raise ValueError('%s: %s must be [n, H, W] with H, W >= 1 and at most 2^37 pixels, got %s' %
                         (name, arg, tuple(t.shape)))
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).contiguous()


def dilate_masks(masks, radius=12):
    """``binary_dilation(mask, disk(radius))`` of every view: masks [n, H, W] uint8 / bool CUDA -> uint8 [n, H, W] of
    0 / 1.  A pixel is set iff it is non-zero (the reference's ``mask / 256.`` then ``binary_dilation``); the
    structuring element is skimage's ``disk``: the offsets with dx^2 + dy^2 <= radius^2; pixels outside the image are
    unset.  0 <= radius <= 32."""
    r = int(radius)
    if r != radius or r < 0 or r > MAX_RADIUS:
        raise ValueError('dilate_masks: radius must be an integer in [0, %d], got %r' % (MAX_RADIUS, radius))
    m = _check_images('dilate_masks', 'masks', masks)
    n, h, w = m.shape
    out = torch.empty(n, h, w, dtype=torch.uint8, device=m.device)
    if n > 0:
        with torch.cuda.device(m.device):
            ws = ma.workspace('dilate_masks', 'msdf_dtu_dilate_workspace_bytes', n, h, w, device=m.device)
            ma.call('msdf_dtu_dilate', m, n, h, w, r, ws, out)
    return out


def dtu_projections(cameras, n_views):
    """[n_views, 3, 4] float64 projections from a DTU ``cameras.npz`` (a path or a mapping with ``world_mat_i`` and
    ``scale_mat_i``): P = (world_mat_i @ scale_mat_i)[:3], divided by |P[2, :3]| sign(det P[:, :3]), so that
    P (x, 1) = (u z, v z, z) with z the camera depth.  The same matrix as K[:3, :3] @ world_to_camera[:3, :4] with
    K[2, 2] = 1 that the reference recomposes from ``load_K_Rt_from_P``, without cv2.  The matrices are read as
    float32, as the reference reads them."""
    cams = np.load(cameras) if isinstance(cameras, (str, os.PathLike)) else cameras
    out = np.empty((int(n_views), 3, 4), np.float64)
    for i in range(int(n_views)):
        try:
            world, scale = cams['world_mat_%d' % i], cams['scale_mat_%d' % i]
        except KeyError as e:
            raise ValueError('dtu_projections: the cameras hold no %s' % e)
        P = (np.asarray(world, np.float32) @ np.asarray(scale, np.float32)).astype(np.float64)[:3, :4]
        s = np.linalg.norm(P[2, :3]) * np.sign(np.linalg.det(P[:, :3]))
        if not np.isfinite(s) or s == 0:
            raise ValueError('dtu_projections: view %d has a singular projection' % i)
        out[i] = P / s
    return out


def _projection_rows(name, projections):
    if isinstance(projections, torch.Tensor):
        projections = projections.detach().cpu().numpy()
    p = np.asarray(projections, dtype=np.float64)
    if p.ndim != 3 or p.shape[1:] != (3, 4):
        raise ValueError('%s: projections must be [n, 3, 4], got %s' % (name, p.shape))
    if not np.isfinite(p).all():
        raise ValueError('%s: non-finite projection' % name)
    return np.ascontiguousarray(p.reshape(-1, 12), dtype=np.float32)


def mask_vertices(vertices, projections, dilated):
    """For every vertex whether the masks keep it: bool [V] on the vertices' device.  vertices [V,3] float32 CUDA;
    projections [n,3,4] (numpy or tensor; formed in fp64, used in fp32; see ``dtu_projections``); dilated [n,H,W]
    uint8 / bool CUDA (``dilate_masks``).  Per vertex and view, in separately rounded fp32:
    (u, v, z) = ((P0 x + P1 y) + P2 z) + P3 per row, px = u / (z + 1e-6), py = v / (z + 1e-6); *valid* iff
    0 < px < W-1 and 0 < py < H-1; pixel = (rint(px), rint(py)), half to even.  A vertex is kept iff in every view it
    is not valid or the dilated mask is set at its pixel.  There is no depth-sign test: the reference has none.  One
    lane per vertex loops over the views and stops at the first that culls it.

    The reference renormalises px, py to [-1, 1] and samples through ``grid_sample(mode='nearest',
    align_corners=True)``, which scales them back: a vertex within fp32 rounding of a pixel boundary or of the image
    edge may fall on the other side there."""
    name = 'mask_vertices'
    ma.check_tensor(name, 'vertices', vertices, shape='[V, 3]')
    proj = _projection_rows(name, projections)
    d = _check_images(name, 'dilated', dilated)
    ma.same_device(name, vertices=vertices, dilated=d)
    if d.shape[0] != proj.shape[0]:
        raise ValueError('%s: %d projections for %d masks' % (name, proj.shape[0], d.shape[0]))
    v = vertices.contiguous()
    keep = torch.ones(v.shape[0], dtype=torch.uint8, device=v.device)
    if v.shape[0] > 0 and d.shape[0] > 0:
        with torch.cuda.device(v.device):
            ma.call('msdf_dtu_mask_vertices', v, v.shape[0], ma.upload(proj, v.device), d.shape[0], d, d.shape[1],
                    d.shape[2], keep)
    return keep.bool()


@torch.no_grad()
def cull_to_masks(mesh, projections, masks, radius=12):
    """``cull_scan`` of dtu_eval/evaluate_single_scene.py without its final rescale: the masks [n,H,W] (uint8 / bool;
    numpy arrays are uploaded) are dilated by ``disk(radius)``, the vertices that ``mask_vertices`` does not keep are
    DROPPED, with every face that does not have all three vertices kept, and the faces are reindexed -- trimesh's
    ``update_vertices`` / ``update_faces``.  This differs from ``mesh_refuse.cull_to_frustums``, which drops faces only
    and keeps all vertices.  ``mesh``: a Mesh or a (vertices, faces) pair.  -> Mesh (with the kept vertices' normals
    when a Mesh came in).  The caller takes the result to the world frame with ``Mesh.apply_transform(scale_mat)``."""
    name = 'cull_to_masks'
    v, f, nrm = ma.mesh_tensors(name, mesh, ma.device_of(masks))
    if isinstance(masks, np.ndarray):
        masks = ma.upload((masks != 0).view(np.uint8), v.device)
    keep = mask_vertices(v, projections, dilate_masks(masks, radius))
    # a (vertices, faces) pair comes back as what was culled, a mesh object with its own vertices and normals
    return ma.kept_mesh(v if nrm is None else mesh.vertices, nrm, keep, ma.compact_faces(keep, f))


def sample_lattice(vertices, faces, density=0.2):
    """The deterministic sampler of eval.py:54-71: vertices [V,3] float32, faces [F,3] int32 / int64, CUDA ->
    float32 [M,3].  In fp64 on the fp32 vertices, the reference's expressions in the reference's order:
    v1 = p1 - p0, v2 = p2 - p0, l = sqrt((x^2 + y^2) + z^2), area2 = |v1 x v2| (a face with area2 == 0 is skipped),
    thr = density sqrt(l1 l2 / area2), n1 = floor(l1 / thr), n2 = floor(l2 / thr); candidates
    a = (i + 0.5) / max(n1, 1e-7) for i = 0..n1 and b = (j + 0.5) / max(n2, 1e-7) for j = 0..n2, kept iff a + b < 1;
    point = (v1 a + v2 b) + p0, rounded once to fp32.  Output order: face ascending, then i, then j.  The vertices
    themselves are not included: the caller concatenates them, as the reference does.  ValueError at 2^31 points."""
    dens = ma.positive_number('sample_lattice', 'density', density)
    return _lattice(*ma.mesh_tensors('sample_lattice', (vertices, faces))[:2], dens)


def _lattice(v, f, dens):
    dev = v.device
    nv, nf = v.shape[0], f.shape[0]
    if nf == 0:
        return v.new_empty(0, 3)
    with torch.cuda.device(dev):
        offsets = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
        counts = offsets[1:]
        ma.call('msdf_dtu_lattice_count', v, nv, f, nf, dens, counts)
        largest = int(counts.max())
        counts.cumsum_(0)                                    # offsets: the exclusive scan, the total last
        total = int(offsets[-1])
        if largest >= 2 ** 31 or total >= 2 ** 31:
            raise ValueError('sample_lattice: 2^31 points or more (density %g): sample the mesh in parts' % dens)
        out = torch.empty(total, 3, dtype=torch.float32, device=dev)
        if total > 0:
            ma.call('msdf_dtu_lattice_emit', v, nv, f, nf, dens, offsets, total, out)
    return out


def radius_thin(points, radius, order=None, return_rounds=False):
    """The thinning of eval.py:86-94: the points are visited in ``order``; a point still marked is kept and unmarks
    every point within ``radius`` of it.  points [N,3] float32 CUDA -> bool [N], True for the kept points.
    ``order``: None (index order) or an int64 permutation on the points' device, ``order[k]`` the k-th point visited.
    Distance rule, fp64 on the fp32 coordinates: ((dx dx + dy dy) + dz dz) <= radius radius, which is what sklearn's
    KD-tree decides on float32-valued input.

    The kept set is the lexicographically first maximal independent set of the graph {d^2 <= r^2} under the order: it
    is unique, so it is computed in parallel.  Every point is undecided, kept or removed; in a round every undecided
    point looks at its neighbours that come earlier in the order: one kept -> removed; else one undecided -> it waits;
    else -> kept.  The earliest undecided point is decided every round.  A shuffled order needs about log N rounds, a
    sorted chain one round per point (still correct).  Neighbours come from a uniform grid of cells a little larger
    than the radius (27 cells per point); the host reads the undecided count once per round.
    ``return_rounds``: also the number of rounds that ran."""
    name = 'radius_thin'
    r = ma.positive_number(name, 'radius', radius)
    if order is not None:
        if not isinstance(order, torch.Tensor) or order.dtype != torch.int64 or order.dim() != 1:
            raise ValueError('%s: order must be a 1-D int64 tensor' % name)
        if isinstance(points, torch.Tensor) and points.dim() == 2 and order.shape[0] != points.shape[0]:
            raise ValueError('%s: order has %d entries for %d points' % (name, order.shape[0], points.shape[0]))
    ma.check_tensor(name, 'points', points)
    dev = points.device
    n = points.shape[0]
    pts = points.contiguous()
    rank = None
    if order is not None:
        ma.same_device(name, points=points, order=order)
        if n > 0:
            inside = (order >= 0) & (order < n)
            hit = torch.zeros(n, dtype=torch.bool, device=dev)
            hit[order[inside]] = True
            if not bool((inside.all() & hit.all()).item()):
                raise ValueError('%s: order is not a permutation of 0..%d' % (name, n - 1))
            rank = torch.empty(n, dtype=torch.int64, device=dev)
            rank[order] = torch.arange(n, dtype=torch.int64, device=dev)
    keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    rounds = 0
    if n > 0:
        _, lo_h, hi_h = ma.finite_bounds(name, pts)
        # two points within r differ by less than one cell per axis, rounding included; at most 2^21 - 4 cells an axis
        cell = max(r * _CELL_SLACK, float((hi_h - lo_h).max()) / (_CELL_AXIS_MAX - 4))
        with torch.cuda.device(dev):
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            ma.call('msdf_dtu_thin_keys', pts, n, *lo_h.tolist(), cell, keys)
            sorted_keys, perm = torch.sort(keys, stable=True)
            ws = ma.workspace(name, 'msdf_dtu_thin_workspace_bytes', n, device=dev)
            ma.call('msdf_dtu_thin_prepare', pts, perm, rank, sorted_keys, n, ws)
            undecided = torch.empty(1, dtype=torch.int32, device=dev)
            while True:
                ma.call('msdf_dtu_thin_round', ws, n, r, undecided)
                rounds += 1
                if int(undecided.item()) == 0:
                    break
            ma.call('msdf_dtu_thin_finish', ws, perm, n, keep)
    return (keep.bool(), rounds) if return_rounds else keep.bool()


def _mean_below(dist, max_dist):
    d = dist.double()
    near = d[d < max_dist]
    return float(near.mean()) if near.numel() else float('nan')


@torch.no_grad()
def evaluate_dtu(mesh_or_points, stl_points, obs_mask, bb, res, plane, density=0.2, patch=60, max_dist=20, seed=0,
                 order=None, return_clouds=False, search='brute'):
    """dtu_eval/eval.py from the sampling on.  ``mesh_or_points``: a Mesh or a (vertices, faces) pair (the reference's
    mesh mode) or a bare [N,3] cloud (its pcd mode), in the DTU world frame (millimetres); ``stl_points`` [S,3] the
    scan's reference cloud; ``obs_mask`` [X,Y,Z] (non-zero = observed), ``bb`` [2,3] and ``res`` from
    ``ObsMask{scan}_10.mat``; ``plane`` the 4 coefficients of ``Plane{scan}.mat``.  numpy arrays are uploaded.

    cloud = vertices ++ ``sample_lattice(vertices, faces, density)``; it is thinned by ``radius_thin(cloud, density,
    order)`` with ``order`` a ``torch.randperm`` from a device generator seeded with ``seed`` unless one is given (the
    reference shuffles unseeded, so its own result is not reproducible either); ``data_down = cloud[keep]`` stays in
    the cloud's order, which the means do not depend on.  ``data_in``: the points with bb[0] - patch <= p <
    bb[1] + 2 patch on all axes (the bounds in fp32, as the reference forms them).  ``data_in_obs``: those whose grid
    index rint((p - bb[0]) / res) (fp64, half to even) lies inside ``obs_mask`` and is set there.
    'd2s': the mean distance from data_in_obs to the stl cloud over the distances < max_dist; 's2d': the mean distance
    from ``stl_above``, the stl points with plane . (x, 1) > 0, to data_in (not data_in_obs), likewise; 'overall':
    their mean.  -> a dict of Python floats (nan where no distance is below max_dist).  ``return_clouds``: also a dict
    with 'data_pcd', 'order', 'keep', 'data_in', 'data_in_obs', 'stl_above', 'dist_d2s', 'dist_s2d' (tensors).

    ``search``: 'brute' (the default) sends the two closing queries through ``nearest_neighbors``; 'grid' sends them
    through ``nearest_neighbors_within(..., max_dist)``, which needs ``max_dist`` positive and finite.  The distances
    below ``max_dist`` are the same bits in the same order, so the three metrics are equal as Python floats; with
    'grid', 'dist_d2s' and 'dist_s2d' hold +inf wherever the brute-force distance exceeds ``max_dist``."""
    name = 'evaluate_dtu'
    if search not in ('brute', 'grid'):
        raise ValueError("%s: search must be 'brute' or 'grid', got %r" % (name, search))
    dev = ma.device_of(stl_points, obs_mask)
    if isinstance(mesh_or_points, (tuple, list)) or hasattr(mesh_or_points, 'faces'):
        v, f, _ = ma.mesh_tensors(name, mesh_or_points, dev)
        cloud = torch.cat([v, _lattice(v, f, ma.positive_number(name, 'density', density))])
    else:
        cloud = ma.cloud_tensor(name, 'points', mesh_or_points, dev)
    dev = cloud.device
    stl = ma.cloud_tensor(name, 'stl_points', stl_points, dev)
    obs = obs_mask if isinstance(obs_mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(obs_mask))
    if obs.dim() != 3:
        raise ValueError('%s: obs_mask must be [X, Y, Z], got %s' % (name, tuple(obs.shape)))
    obs = obs.to(dev) != 0
    bb32 = np.asarray(bb.detach().cpu().numpy() if isinstance(bb, torch.Tensor) else bb).astype(np.float32)
    if bb32.shape != (2, 3):
        raise ValueError('%s: bb must be [2, 3], got %s' % (name, bb32.shape))
    res = float(np.asarray(res, np.float64).reshape(-1)[0])
    if not res > 0:
        raise ValueError('%s: res must be positive, got %r' % (name, res))
    pl = np.asarray(plane.detach().cpu().numpy() if isinstance(plane, torch.Tensor) else plane, np.float64).reshape(-1)
    if pl.shape != (4,):
        raise ValueError('%s: plane must hold 4 coefficients' % name)
    n = cloud.shape[0]
    if order is None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        order = torch.randperm(n, generator=gen, device=dev)
    keep = radius_thin(cloud, density, order)
    data_down = cloud[keep]
    lower = ma.upload((bb32[0] - np.float32(patch)).astype(np.float64), dev)
    upper = ma.upload((bb32[1] + np.float32(patch * 2)).astype(np.float64), dev)
    down64 = data_down.double()
    inbound = ((down64 >= lower) & (down64 < upper)).all(dim=1)
    data_in = data_down[inbound]
    grid = torch.round((data_in.double() - ma.upload(bb32[0].astype(np.float64), dev)) / res).long()
    shape = torch.tensor(list(obs.shape), dtype=torch.int64, device=dev)
    grid_in = ((grid >= 0) & (grid < shape)).all(dim=1)
    g = grid[grid_in]
    in_obs = obs[g[:, 0], g[:, 1], g[:, 2]]
    data_in_obs = data_in[grid_in][in_obs]
    if stl.shape[0] == 0:
        raise ValueError('%s: the stl cloud is empty' % name)
    if search == 'grid':
        def nearest(reference, query):
            return nearest_neighbors_within(reference, query, max_dist)
    else:
        nearest = nearest_neighbors
    dist_d2s = nearest(stl, data_in_obs)[0]
    s64 = stl.double()
    above = ((s64[:, 0] * pl[0] + s64[:, 1] * pl[1]) + s64[:, 2] * pl[2]) + pl[3] > 0
    stl_above = stl[above]
    if data_in.shape[0] > 0:
        dist_s2d = nearest(data_in, stl_above)[0]
    else:
        dist_s2d = torch.full((stl_above.shape[0],), float('inf'), dtype=torch.float32, device=dev)
    d2s, s2d = _mean_below(dist_d2s, max_dist), _mean_below(dist_s2d, max_dist)
    out = {'d2s': d2s, 's2d': s2d, 'overall': (d2s + s2d) / 2}
    if return_clouds:
        return out, {'data_pcd': cloud, 'order': order, 'keep': keep, 'data_in': data_in, 'data_in_obs': data_in_obs,
                     'stl_above': stl_above, 'dist_d2s': dist_d2s, 'dist_s2d': dist_s2d}
    return out


def read_masks(path):
    """Object masks [n, H, W] uint8 from an ``.npy`` stack or a directory of images (sorted by name; the first channel,
    as the reference takes it); images need PIL."""
    if os.path.isfile(path):
        m = np.load(path)
        if m.ndim == 4:
            m = m[..., 0]
        if m.ndim != 3:
            raise ValueError('read_masks: %s holds an array of shape %s, not [n, H, W]' % (path, m.shape))
        return np.ascontiguousarray(m != 0).view(np.uint8)
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError('read_masks: reading mask images needs PIL; pass an .npy stack [n, H, W] instead')
    files = sorted(glob.glob(os.path.join(path, '*.png')))
    if not files:
        raise ValueError('read_masks: no *.png under %s' % path)
    out = []
    for p in files:
        a = np.asarray(Image.open(p))
        out.append((a[..., 0] if a.ndim == 3 else a) != 0)
    return np.ascontiguousarray(np.stack(out)).view(np.uint8)


def read_dtu_scene(dataset_dir, scan):
    """The official evaluation files of one scan -> dict with 'stl_points' [S,3] float64 (``Points/stl/
    stl{scan:03}_total.ply``), 'obs_mask' [X,Y,Z], 'bb' [2,3] float32, 'res' float (``ObsMask/ObsMask{scan}_10.mat``)
    and 'plane' [4] (``ObsMask/Plane{scan}.mat``): the arguments of ``evaluate_dtu``.  The .mat files need scipy."""
    try:
        from scipy.io import loadmat
    except ImportError:
        raise RuntimeError('read_dtu_scene: reading ObsMask / Plane .mat files needs scipy (scipy.io.loadmat); '
                           'without it pass the arrays to evaluate_dtu yourself')
    scan = int(scan)
    obs = loadmat(os.path.join(dataset_dir, 'ObsMask', 'ObsMask%d_10.mat' % scan))
    plane = loadmat(os.path.join(dataset_dir, 'ObsMask', 'Plane%d.mat' % scan))['P']
    stl = read_ply(os.path.join(dataset_dir, 'Points', 'stl', 'stl%03d_total.ply' % scan))
    return {'stl_points': stl.vertices, 'obs_mask': np.asarray(obs['ObsMask']),
            'bb': np.asarray(obs['BB']).astype(np.float32), 'res': float(np.asarray(obs['Res']).reshape(-1)[0]),
            'plane': np.asarray(plane, np.float64).reshape(-1)}
