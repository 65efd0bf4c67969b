"""Oriented bounding box of a mesh on the GPU and the crop of the Replica protocol that uses it.

* ``support``: for every plane the farthest point of a cloud and its signed distance, in fp64 (csrc/obb.hip, ABI
  msdf_obb_* of include/monosdf_obb.h).  The only step here that touches every point.
* ``convex_hull``: the 3-D convex hull by rounds: the hull of a few extreme points is built on the host in fp64
  (``HostHull``, incremental beneath-beyond), ``support`` finds for every face the farthest point of the whole cloud,
  the points beyond a face are inserted, until no face has a point beyond it.  The host only ever sees hull vertices.
* ``oriented_bounds``: the search of ``trimesh.bounds.oriented_bounds`` (replica_eval/eval_recon.py:122): of all boxes
  with one face parallel to a hull face and one side parallel to an edge of the hull's projection onto that face, the
  one of smallest volume.  An edge of the projected hull is a silhouette edge of the 3-D hull seen along the normal,
  so no 2-D hulls are built (msdf_obb_candidates).
* ``crop_to_oriented_bounds``: lines 122-136 of ``calc_3d_metric``: the reconstructed vertices outside the
  ground-truth mesh's box scaled by 1.05 are dropped with the faces that touch one.

Everything runs on CUDA tensors; there is no CPU path, and neither scipy nor trimesh is imported.  Arguments are
checked by utils/mesh_args.py.  No floating-point atomics: the same input gives bitwise the same output every call.

Parity with trimesh is UNVERIFIED: trimesh is not available where this is built and the reference holds no recorded
output of it, so the rule is pinned by the numpy restatement of the tests (tests/obb_numpy.py) only.  One known
difference: trimesh rounds the spherical angles of the candidate normals to one decimal before it searches; this search
takes every distinct face normal, so its box is never larger than the one of trimesh's rule.  The order of the axes
(extents ascending, rotation right-handed) is believed to be trimesh's ``ordered=True``.
"""
import time

import numpy as np
import torch

from . import mesh_args as ma

TOL_SCALE = 1e-12                     # tol = this times the largest absolute coordinate
MAX_ROUNDS = 100                      # hull rounds before convex_hull gives up (measured: 4 ... 8)
_WORKSPACE_TARGET = 64 << 20          # planes go to msdf_obb_support in batches whose workspace stays about this
_SLICE = 2048                         # points per slice of msdf_obb_support (OBB_SLICE)

# the seed directions of convex_hull: axes, face diagonals and body diagonals of the cube, both signs
_SEED = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, 1], [0, 1, -1],
                  [1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1]], dtype=np.float64)


# ---------------------------------------------------------------- the support function

def _support(name, pts, planes):
    """pts: float32 CUDA [N,3], checked, N >= 1; planes: float64 host array [D,4] -> (value float64 [D],
    index int64 [D]) as host arrays."""
    dev, N, D = pts.device, pts.shape[0], len(planes)
    value = torch.empty(D, dtype=torch.float64, device=dev)
    index = torch.empty(D, dtype=torch.int32, device=dev)
    if D:
        pl = ma.upload(planes, dev, np.float64)
        batch = max(256, _WORKSPACE_TARGET // (12 * ((N + _SLICE - 1) // _SLICE)))
        with torch.cuda.device(dev):
            ws = ma.workspace(name, 'msdf_obb_support_workspace_bytes', N, min(D, batch), device=dev)
            for a in range(0, D, batch):
                b = min(D, a + batch)
                ma.call('msdf_obb_support', pts, N, pl[a:b], b - a, ws, value[a:b], index[a:b])
    return value.cpu().numpy(), index.cpu().numpy().astype(np.int64)


def support(points, planes):
    """For every plane the farthest point of the cloud: points [N,3] float32 CUDA, planes [D,4] float64 (a, b, c, w;
    a CUDA tensor or a host array) -> (value [D] float64, index [D] int64) CUDA tensors.

    value[d] = max over the points of fma(c, z, fma(b, y, a * x)) + w, evaluated in fp64 on the exact fp64 values of
    the fp32 coordinates; index[d] = the point that attains it, the smallest index among points of equal fp64 value.
    Bitwise the same every call.  ValueError for an empty cloud; non-finite inputs are refused (one device reduction
    and one host read)."""
    name = 'support'
    ma.check_tensor(name, 'points', points)
    if isinstance(planes, torch.Tensor):
        ma.check_tensor(name, 'planes', planes, (torch.float64,), '[D, 4]')
        ma.same_device(name, points=points, planes=planes)
        planes = planes.cpu().numpy()
    planes = np.asarray(planes, dtype=np.float64)
    if planes.ndim != 2 or planes.shape[1] != 4:
        raise ValueError('%s: planes must be [D, 4], got %s' % (name, planes.shape))
    if points.shape[0] == 0:
        raise ValueError('%s: the cloud is empty' % name)
    pts = points.contiguous()
    if not (bool(torch.isfinite(pts).all()) and np.isfinite(planes).all()):
        raise ValueError('%s: non-finite coordinates' % name)
    value, index = _support(name, pts, planes)
    return ma.upload(value, pts.device), ma.upload(index, pts.device)


# ---------------------------------------------------------------- the host part of the hull

def _unit_planes(a, b, c):
    """The planes through the triangles (a, b, c) [m,3] each, by the right-hand rule: ([m,4] unit normal and offset,
    [m] the norm of the cross product)."""
    n = np.cross(b - a, c - a)
    norm = np.linalg.norm(n, axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        n = n / norm[:, None]
    return np.concatenate([n, -(n * a).sum(1, keepdims=True)], axis=1), norm


class HostHull:
    """Incremental (beneath-beyond) convex hull in fp64 on the host.  Starts from a tetrahedron; ``add`` inserts one
    point: the faces it lies more than ``tol`` above are removed and the hole is closed by the cone from the point to
    the horizon edges.  A point that sees no face changes nothing.  Faces are rows of local point numbers (the order
    of insertion, tetrahedron first) with outward orientation; ``planes`` holds their unit outward normal and offset."""

    def __init__(self, simplex, tol):
        simplex = np.asarray(simplex, dtype=np.float64).reshape(4, 3)
        self.tol = float(tol)
        self.points = [p for p in simplex]
        faces = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
        other = np.array([3, 2, 0, 1])                              # the vertex a face leaves out
        planes, norm = _unit_planes(*(simplex[faces[:, k]] for k in range(3)))
        if not (norm > 0).all():
            raise ValueError('HostHull: a flat simplex')
        below = (planes[:, :3] * simplex[other]).sum(1) + planes[:, 3]
        if not ((below < 0).all() or (below > 0).all()):
            raise ValueError('HostHull: a flat simplex')
        if below[0] > 0:                                            # inside out: turn every face round
            faces = faces[:, ::-1]
            planes = -planes
        self._cap = 64
        self.f = np.zeros((self._cap, 3), dtype=np.int64)
        self.pl = np.zeros((self._cap, 4))
        self.alive = np.zeros(self._cap, dtype=bool)
        self.n = 0
        self._append(faces, planes)

    def _append(self, faces, planes):
        m = len(faces)
        while self.n + m > self._cap:
            self._cap *= 2
            for attr in ('f', 'pl', 'alive'):
                old = getattr(self, attr)
                new = np.zeros((self._cap,) + old.shape[1:], dtype=old.dtype)
                new[:self.n] = old[:self.n]
                setattr(self, attr, new)
        self.f[self.n:self.n + m] = faces
        self.pl[self.n:self.n + m] = planes
        self.alive[self.n:self.n + m] = True
        self.n += m

    def _compact(self):
        keep = self.alive[:self.n]
        m = int(keep.sum())
        self.f[:m], self.pl[:m] = self.f[:self.n][keep], self.pl[:self.n][keep]
        self.alive[:m], self.alive[m:self.n] = True, False
        self.n = m

    def add(self, p):
        """Insert the point; -> its local number, or -1 when it sees no face (or would close the hole with a face of
        no area) and the hull is as it was."""
        p = np.asarray(p, dtype=np.float64)
        n = self.n
        visible = self.alive[:n] & (self.pl[:n, :3] @ p + self.pl[:n, 3] > self.tol)
        if not visible.any():
            return -1
        vf = self.f[:n][visible]
        a = np.concatenate([vf[:, 0], vf[:, 1], vf[:, 2]])
        b = np.concatenate([vf[:, 1], vf[:, 2], vf[:, 0]])
        big = len(self.points) + 1
        horizon = ~np.isin(b * big + a, a * big + b)               # the face across the edge is not visible
        a, b = a[horizon], b[horizon]
        coords = np.asarray(self.points)
        planes, norm = _unit_planes(coords[a], coords[b], np.broadcast_to(p, (len(a), 3)))
        if not (norm > 0).all():
            return -1
        number = len(self.points)
        self.points.append(p)
        self.alive[:n][visible] = False
        self._append(np.stack([a, b, np.full(len(a), number)], axis=1), planes)
        if self.n > 4 * max(64, int(self.alive[:self.n].sum())):
            self._compact()
        return number

    def result(self):
        """(faces [F,3] of local point numbers, planes [F,4]) of the hull as it stands."""
        keep = self.alive[:self.n]
        return self.f[:self.n][keep].copy(), self.pl[:self.n][keep].copy()


def host_hull(points, tol):
    """The hull of a small host cloud [m,3] by ``HostHull`` alone: the simplex from the two points farthest apart among
    the axis extremes, the farthest from their line and the farthest from their plane, then every point in ascending
    order.  -> (faces [F,3] into ``points``, planes [F,4]).  ValueError for a cloud within ``tol`` of a plane."""
    pts = np.asarray(points, dtype=np.float64)
    simplex = _simplex_rows(pts, tol)
    hull = HostHull(pts[simplex], tol)
    ids = list(simplex)
    for i in range(len(pts)):
        if i not in simplex and hull.add(pts[i]) >= 0:
            ids.append(i)
    faces, planes = hull.result()
    return np.asarray(ids, dtype=np.int64)[faces], planes


def _line_distance(pts, p0, p1):
    d = (p1 - p0) / np.linalg.norm(p1 - p0)
    r = pts - p0
    return np.linalg.norm(r - (r @ d)[:, None] * d, axis=1)


def _simplex_rows(pts, tol):
    """Four rows of the host cloud that span a volume, or ValueError."""
    if len(pts) < 4:
        raise ValueError('host_hull: fewer than 4 points')
    ext = np.unique(np.concatenate([pts.argmin(0), pts.argmax(0)]))
    gap = np.linalg.norm(pts[ext][:, None] - pts[ext][None], axis=2)
    i, j = np.unravel_index(np.argmax(gap), gap.shape)
    if not gap[i, j] > tol:
        raise ValueError('host_hull: the points coincide')
    i, j = int(ext[i]), int(ext[j])
    line = _line_distance(pts, pts[i], pts[j])
    k = int(np.argmax(line))
    if not line[k] > tol:
        raise ValueError('host_hull: the points lie on a line')
    plane = _unit_planes(pts[i][None], pts[j][None], pts[k][None])[0][0]
    off = np.abs(pts @ plane[:3] + plane[3])
    l = int(np.argmax(off))
    if not off[l] > tol:
        raise ValueError('host_hull: the points lie in a plane')
    return [i, j, k, l]


# ---------------------------------------------------------------- the hull of a device cloud

def _gather(pts, index):
    """Rows ``index`` (host int64) of the device cloud as a host fp64 array."""
    return pts[ma.upload(index, pts.device)].double().cpu().numpy()


def _cloud(name, points):
    """The argument of convex_hull / oriented_bounds -> (float32 CUDA [N,3] contiguous, tol).  ValueError for fewer
    than 4 points and for non-finite coordinates."""
    if isinstance(points, tuple) and len(points) == 2:
        points = points[0]
    pts = ma.cloud_tensor(name, 'points', points).contiguous()
    if pts.shape[0] < 4:
        raise ValueError('%s: %d points: a hull needs at least 4' % (name, pts.shape[0]))
    _, lo, hi = ma.finite_bounds(name, pts)
    return pts, TOL_SCALE * float(torch.maximum(lo.abs(), hi.abs()).max())


def _flat(name, tol):
    return ValueError('%s: the cloud lies within %.3g of one plane: it has no volume' % (name, tol))


def _seed(name, pts, tol):
    """-> (index [m] int64 host: the extreme points of the seed directions with the simplex in the first four rows,
    their coordinates [m,3]).  Two of the extremes farthest apart, the extreme farthest from their line (or, when the
    extremes are collinear, the cloud's farthest point in four directions across the line), and the cloud's farthest
    point from the plane of the three, either side, by a support call of its own."""
    planes = np.zeros((2 * len(_SEED), 4))
    unit = _SEED / np.linalg.norm(_SEED, axis=1, keepdims=True)
    planes[:, :3] = np.concatenate([unit, -unit])
    index = np.unique(_support(name, pts, planes)[1])
    xyz = _gather(pts, index)
    gap = np.linalg.norm(xyz[:, None] - xyz[None], axis=2)
    i, j = np.unravel_index(np.argmax(gap), gap.shape)
    if not gap[i, j] > tol:
        raise _flat(name, tol)
    p0, p1 = xyz[i], xyz[j]
    line = _line_distance(xyz, p0, p1)
    k = int(np.argmax(line))
    if line[k] > tol:
        third, p2 = int(index[k]), xyz[k]
    else:
        d = (p1 - p0) / np.linalg.norm(p1 - p0)
        e1 = np.cross(d, np.eye(3)[int(np.argmin(np.abs(d)))])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(d, e1)
        across = np.array([e1, -e1, e2, -e2])
        value, where = _support(name, pts, np.concatenate([across, -(across @ p0)[:, None]], axis=1))
        if not value.max() > tol:
            raise _flat(name, tol)
        third = int(where[int(np.argmax(value))])
        p2 = _gather(pts, np.array([third]))[0]
    plane = _unit_planes(p0[None], p1[None], p2[None])[0]
    value, where = _support(name, pts, np.concatenate([plane, -plane]))
    if not value.max() > tol:
        raise _flat(name, tol)
    fourth = int(where[int(np.argmax(value))])
    first = [int(index[i]), int(index[j]), third, fourth]
    index = np.array(first + [int(s) for s in index if int(s) not in first], dtype=np.int64)
    return index, _gather(pts, index)


def _convex_hull(name, pts, tol, stats=None):
    """-> (faces [F,3] int64 into the cloud, planes [F,4]) as host arrays.  ``stats``: a dict that receives 'rounds',
    and the lists 'support_ms', 'host_ms', 'faces' per round (the benchmark's; timing synchronises)."""
    index, xyz = _seed(name, pts, tol)
    hull = HostHull(xyz[:4], tol)
    ids = [int(i) for i in index[:4]]
    known = set(ids)
    for i, p in zip(index[4:], xyz[4:]):
        if hull.add(p) >= 0:
            ids.append(int(i))
        known.add(int(i))
    rounds = 0
    while True:
        faces, planes = hull.result()
        t0 = time.perf_counter()
        value, where = _support(name, pts, planes)
        t1 = time.perf_counter()
        beyond = np.unique(where[value > tol])
        if len(beyond) == 0:
            break
        rounds += 1
        if rounds > MAX_ROUNDS:
            raise RuntimeError('%s: no hull after %d rounds' % (name, MAX_ROUNDS))
        added = 0
        for i, p in zip(beyond, _gather(pts, beyond)):
            if hull.add(p) >= 0:
                ids.append(int(i))
                added += 1
        if added == 0:
            raise RuntimeError('%s: points beyond the hull that cannot be inserted (degenerate input)' % name)
        if stats is not None:
            stats.setdefault('support_ms', []).append((t1 - t0) * 1e3)
            stats.setdefault('host_ms', []).append((time.perf_counter() - t1) * 1e3)
            stats.setdefault('faces', []).append(len(faces))
    if stats is not None:
        stats['rounds'] = rounds
        stats.setdefault('support_ms', []).append((t1 - t0) * 1e3)       # the closing call that found nothing
        stats.setdefault('faces', []).append(len(faces))
    return np.asarray(ids, dtype=np.int64)[faces], planes


def convex_hull(points):
    """The convex hull of a cloud: points [N,3] float32 CUDA (a numpy array is uploaded, of a mesh object the vertices
    are taken) -> (vertex_index [h] int64 ascending, faces [F,3] int64 into ``points`` with outward orientation,
    planes [F,4] float64: unit outward normal and offset), CUDA tensors.

    With tol = 1e-12 times the largest absolute coordinate: no input point lies more than tol beyond any face plane
    (the loop ends on exactly that answer of ``support``), and every vertex is an input point.  A point is inserted
    only when it is the farthest of the whole cloud beyond some face, which makes it a vertex of the true hull; a
    point within tol of the hull's surface may or may not become a vertex.  ValueError for fewer than 4 points, for
    non-finite coordinates and for a cloud that lies within tol of one plane."""
    name = 'convex_hull'
    pts, tol = _cloud(name, points)
    faces, planes = _convex_hull(name, pts, tol)
    dev = pts.device
    return ma.upload(np.unique(faces), dev), ma.upload(faces, dev), ma.upload(planes, dev)


# ---------------------------------------------------------------- the box

def hull_normals(planes):
    """The distinct face normals of a hull, host [K,3]: opposite normals merged to one hemisphere (the first non-zero
    component positive), exact duplicates removed, in ascending (x, y, z) order."""
    n = np.array(planes[:, :3], dtype=np.float64)
    lead = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    n[lead < 0] *= -1.0
    return np.unique(n + 0.0, axis=0)                               # + 0.0: -0.0 and 0.0 are one value, make them one


def hull_edges(faces):
    """The edges of a closed hull, host: faces [F,3] -> (edges [E,2] with a < b, the face on which the edge runs a -> b
    [E], the face on which it runs b -> a [E]).  ValueError unless every edge has exactly those two faces."""
    F = len(faces)
    a = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
    b = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
    face = np.tile(np.arange(F), 3)
    big = int(faces.max()) + 1
    key = a * big + b
    order = np.argsort(key, kind='stable')
    forward = a < b
    back = b[forward] * big + a[forward]
    at = np.searchsorted(key[order], back)
    if (3 * F) % 2 or len(np.unique(key)) != 3 * F or at.max(initial=0) >= 3 * F or \
            not np.array_equal(key[order][at], back) or 2 * int(forward.sum()) != 3 * F:
        raise ValueError('hull_edges: the faces do not form a closed surface')
    return np.stack([a[forward], b[forward]], axis=1), face[forward], face[order][at]


def _frame(n, d):
    """The right-handed frame (n, u, n x u) of a face normal and an edge vector, host: u = the part of d across n,
    orthogonalised twice."""
    n = n / np.linalg.norm(n)
    u = d - (d @ n) * n
    u /= np.linalg.norm(u)
    u -= (u @ n) * n
    u /= np.linalg.norm(u)
    w = np.cross(n, u)
    return np.stack([n, u, w / np.linalg.norm(w)])


def _oriented_bounds(name, pts, tol, stats=None):
    dev = pts.device
    faces, planes = _convex_hull(name, pts, tol, stats)
    t0 = time.perf_counter()
    vertex_index = np.unique(faces)
    local = np.searchsorted(vertex_index, faces)
    normals = hull_normals(planes)
    edges, f1, f2 = hull_edges(local)
    K, E, h = len(normals), len(edges), len(vertex_index)
    verts = pts[ma.upload(vertex_index, dev)].double().contiguous()
    volume = torch.empty(K, dtype=torch.float64, device=dev)
    edge = torch.empty(K, dtype=torch.int32, device=dev)
    extents = torch.empty(K, 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ma.call('msdf_obb_candidates', verts, h, ma.upload(normals, dev), K, ma.upload(edges, dev, np.int32),
                ma.upload(np.concatenate([planes[f1, :3], planes[f2, :3]], axis=1), dev), E, volume, edge, extents)
    volume_h, edge_h = volume.cpu().numpy(), edge.cpu().numpy()
    k = int(np.argmin(volume_h))                                    # the first of equal minima
    if edge_h[k] < 0 or not np.isfinite(volume_h[k]):
        raise RuntimeError('%s: no candidate box (degenerate hull)' % name)
    xyz = verts.cpu().numpy()
    e0, e1 = edges[int(edge_h[k])]
    axes = _frame(normals[k], xyz[e1] - xyz[e0])
    t1 = time.perf_counter()
    # the chosen frame measured over ALL points: the box contains the cloud whatever the hull did
    side = np.zeros((6, 4))
    side[:3, :3], side[3:, :3] = axes, -axes
    value = _support(name, pts, side)[0]
    size, centre = value[:3] + value[3:], 0.5 * (value[:3] - value[3:])
    order = np.argsort(size, kind='stable')
    rot, size, centre = axes[order], size[order], centre[order]
    if np.linalg.det(rot) < 0:
        rot[2], centre[2] = -rot[2], -centre[2]
    to_origin = np.eye(4)
    to_origin[:3, :3], to_origin[:3, 3] = rot, -centre
    if stats is not None:
        stats.update(F=len(faces), h=h, K=K, E=E, candidates_ms=(t1 - t0) * 1e3,
                     silhouette_pairs=_silhouette_pairs(normals, planes, f1, f2),
                     candidate_volume=float(volume_h[k]))
    return to_origin, size


def _silhouette_pairs(normals, planes, f1, f2, eps=1e-12):
    """How many (normal, edge) pairs msdf_obb_candidates measures: the benchmark's count."""
    total = 0
    for a in range(0, len(normals), 256):
        s1, s2 = normals[a:a + 256] @ planes[f1, :3].T, normals[a:a + 256] @ planes[f2, :3].T
        total += int((((s1 <= eps) & (s2 >= -eps)) | ((s1 >= -eps) & (s2 <= eps))).sum())
    return total


def oriented_bounds(mesh_or_points):
    """The oriented bounding box of a cloud -> (to_origin [4,4] float64, extents [3] float64), host arrays as the
    other transforms of this package.  ``mesh_or_points``: a mesh object or a (vertices, faces) pair (the vertices are
    used), a numpy array, or a float32 CUDA tensor [N,3].  ``to_origin`` takes the cloud to a frame in which the box
    is centred at the origin with its sides along the axes; extents ascending along x, y, z, the rotation
    right-handed (determinant +1).

    The rule is the search space of ``trimesh.bounds.oriented_bounds``: of all boxes with one face parallel to a face
    of the convex hull and, in that face's plane, one side parallel to an edge of the projected hull, the one of
    smallest volume (of equal volumes: the smallest normal in ascending (x, y, z) order of the normals turned to one
    hemisphere, then the smallest edge).  The chosen frame is then measured over every input point by ``support``, so
    the box contains the cloud up to the rounding of that evaluation.  Parity with trimesh is unverified (see the
    module's docstring).  Errors as ``convex_hull``."""
    name = 'oriented_bounds'
    pts, tol = _cloud(name, mesh_or_points)
    return _oriented_bounds(name, pts, tol)


# ---------------------------------------------------------------- the crop

def crop_to_oriented_bounds(rec, gt, margin=1.05):
    """Lines 122-136 of ``calc_3d_metric`` (replica_eval/eval_recon.py) -> Mesh: ``rec`` without the vertices outside
    the oriented bounding box of ``gt`` scaled by ``margin``, and without the faces that touch one.  ``rec``, ``gt``:
    Mesh objects or (vertices, faces) pairs (CUDA tensors, or numpy arrays, which are uploaded).

    Both vertex sets go through ``oriented_bounds(gt)[0]`` in fp64; lo, hi = the per-axis minimum and maximum of the
    transformed ``gt`` vertices times ``margin``; a ``rec`` vertex stays when it is strictly inside on every axis, a
    face when its three vertices stay.  The vertices come back in their original frame and order, the faces
    re-indexed; vertex normals follow their vertices when a mesh object came in.  Nothing left gives an empty Mesh."""
    name = 'crop_to_oriented_bounds'
    rv, rf, normals = ma.mesh_tensors(name, rec, ma.device_of(*ma.mesh_parts(gt)))
    gv = ma.mesh_tensors(name, gt, rv.device)[0]
    dev = ma.same_device(name, rec=rv, gt=gv)
    to_origin = ma.upload(oriented_bounds(gv)[0], dev)
    rot, shift = to_origin[:3, :3], to_origin[:3, 3:]
    g = (rot @ gv.double().T + shift).T
    r = (rot @ rv.double().T + shift).T
    lo, hi = g.min(dim=0).values * float(margin), g.max(dim=0).values * float(margin)
    keep = ((r - lo[None]) > 0).all(dim=1) & ((r - hi[None]) < 0).all(dim=1)
    return ma.kept_mesh(ma.mesh_parts(rec)[0], normals, keep, ma.compact_faces(keep, rf))
