"""numpy / scipy restatement of utils/mesh_bounds.py by an independent route, and the constructed clouds of its tests.

* ``support``: the support function in the evaluation order of include/monosdf_obb.h, (c z + (b y + a x)) + w in fp64.
  numpy has no fused multiply-add, so each product is rounded on its own: equal to the kernel for integer-valued
  inputs, within the rounding bound of ``support_bound`` otherwise.
* ``hull``: scipy.spatial.ConvexHull.
* ``oriented_bounds``: the rule of trimesh.bounds.oriented_bounds stated the long way: per distinct hull normal the 2-D
  ConvexHull of the projected hull vertices, per edge of it the box, the minimum volume.  No silhouette test.
* ``crop``: lines 122-136 of replica_eval/eval_recon.py.
"""
import numpy as np


# ---------------------------------------------------------------- restatements

def support(points, planes):
    """points [N,3] (any float dtype), planes [D,4] float64 -> (value [D] float64, index [D] int64: the first
    maximum)."""
    p = np.asarray(points, dtype=np.float64)
    q = np.asarray(planes, dtype=np.float64)
    value = np.empty(len(q))
    index = np.empty(len(q), dtype=np.int64)
    for d, (a, b, c, w) in enumerate(q):
        s = (c * p[:, 2] + (b * p[:, 1] + a * p[:, 0])) + w
        index[d] = int(np.argmax(s))                                # the first of equal maxima
        value[d] = s[index[d]]
    return value, index


def support_bound(points, planes):
    """[D, N]: 4 * 2^-53 * (|a x| + |b y| + |c z| + |w|), the four rounding steps of one evaluation."""
    p = np.abs(np.asarray(points, dtype=np.float64))
    q = np.abs(np.asarray(planes, dtype=np.float64))
    return 4.0 * 2.0 ** -53 * (q[:, :3] @ p.T + q[:, 3:])


def hull(points):
    """-> (vertex index ascending, volume, equations [F,4]) of scipy's hull of the fp64 values of the points."""
    from scipy.spatial import ConvexHull
    h = ConvexHull(np.asarray(points, dtype=np.float64))
    return np.sort(h.vertices).astype(np.int64), float(h.volume), h.equations.copy()


def faces_volume(points, faces):
    """The volume enclosed by outward-oriented faces: the sum of the signed tetrahedra against the centroid."""
    p = np.asarray(points, dtype=np.float64)
    p = p - p[np.unique(faces)].mean(0)
    a, b, c = (p[faces[:, k]] for k in range(3))
    return float((np.cross(a, b) * c).sum() / 6.0)


def hemisphere(normals):
    n = np.array(normals, dtype=np.float64)
    lead = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    n[lead < 0] *= -1.0
    return np.unique(n + 0.0, axis=0)


def oriented_bounds(points):
    """-> (volume, extents ascending [3], to_origin [4,4]) of the smallest box of trimesh's search space, through 2-D
    hulls.  ``to_origin``: the chosen frame measured over all points, extents ascending, right-handed; the sign of an
    axis is whatever the 2-D hull's edge gave."""
    from scipy.spatial import ConvexHull
    p = np.asarray(points, dtype=np.float64)
    h = ConvexHull(p)
    hv = p[h.vertices]
    best, best_ext, frame = np.inf, None, None
    for n in hemisphere(h.equations[:, :3]):
        n = n / np.linalg.norm(n)
        x = np.cross(n, np.eye(3)[int(np.argmin(np.abs(n)))])
        x /= np.linalg.norm(x)
        y = np.cross(n, x)
        flat = np.stack([hv @ x, hv @ y], axis=1)
        along = hv @ n
        en = along.max() - along.min()
        ring = ConvexHull(flat)
        for i, j in ring.simplices:
            d = flat[j] - flat[i]
            d /= np.linalg.norm(d)
            su, sv = flat @ d, flat @ np.array([-d[1], d[0]])
            eu, ev = su.max() - su.min(), sv.max() - sv.min()
            if en * eu * ev < best:
                best, best_ext = en * eu * ev, np.sort([en, eu, ev])
                u = d[0] * x + d[1] * y
                frame = np.stack([n, u, np.cross(n, u)])
    s = p @ frame.T
    size, centre = s.max(0) - s.min(0), 0.5 * (s.max(0) + s.min(0))
    order = np.argsort(size, kind='stable')
    rot, centre = frame[order], centre[order]
    if np.linalg.det(rot) < 0:
        rot[2], centre[2] = -rot[2], -centre[2]
    to_origin = np.eye(4)
    to_origin[:3, :3], to_origin[:3, 3] = rot, -centre
    return float(best), best_ext, to_origin


def crop(rec_vertices, rec_faces, gt_vertices, to_origin, margin=1.05):
    """-> (kept-vertex mask [V], the kept faces re-indexed [F',3], the transformed rec and gt vertices, lo, hi)."""
    T = np.asarray(to_origin, dtype=np.float64)
    g = (T[:3, :3] @ np.asarray(gt_vertices, dtype=np.float64).T + T[:3, 3:]).T
    r = (T[:3, :3] @ np.asarray(rec_vertices, dtype=np.float64).T + T[:3, 3:]).T
    lo, hi = g.min(axis=0) * margin, g.max(axis=0) * margin
    mask = np.concatenate(((r - lo[None]) > 0, (r - hi[None]) < 0), axis=1).all(axis=1)
    faces = np.asarray(rec_faces)
    face_mask = mask[faces].all(axis=1)
    return mask, (np.cumsum(mask) - 1)[faces[face_mask]].reshape(-1, 3), r, g, lo, hi


# ---------------------------------------------------------------- constructed clouds (fp32, from seeds)

def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


CUBOID_SIDES = np.array([1.0, 2.0, 3.0])


def cuboid_cloud(seed=11, interior=300):
    """The 8 corners of a rotated 3 x 2 x 1 cuboid centred at the origin, then ``interior`` points inside 0.8 of it."""
    rng = np.random.default_rng(seed)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * (CUBOID_SIDES / 2)
    inside = rng.uniform(-0.4, 0.4, (interior, 3)) * CUBOID_SIDES
    return (np.concatenate([corners, inside]) @ rotation(seed).T).astype(np.float32)


def room_shell(n, seed=5, sides=(6.0, 4.0, 2.8), sigma=0.002):
    """``n`` points on the six walls of a room of the given sides with Gaussian noise ``sigma``, rotated and moved."""
    rng = np.random.default_rng(seed)
    sides = np.asarray(sides)
    p = rng.uniform(-0.5, 0.5, (n, 3)) * sides
    wall = rng.integers(0, 3, n)
    sign = rng.integers(0, 2, n) * 2 - 1
    p[np.arange(n), wall] = sign * sides[wall] / 2
    p += rng.normal(0.0, sigma, (n, 3))
    return (p @ rotation(seed + 1).T + np.array([0.3, -0.2, 1.4])).astype(np.float32)


def gaussian(n, seed=7):
    return np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32)


def sphere(n=200, seed=3):
    p = np.random.default_rng(seed).normal(size=(n, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


def tetrahedron():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)


def five():
    """A tetrahedron and a point inside it."""
    return np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2], [0.4, 0.5, 0.3]], dtype=np.float32)


def lattice(n=5):
    """The n x n x n integer lattice in ascending (x, y, z) order: exact coplanarity everywhere."""
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)


HULL_CLOUDS = {
    'tetrahedron': tetrahedron,
    'five': five,
    'sphere': sphere,
    'gaussian': lambda: gaussian(2000),
    'room': lambda: room_shell(5000),
}


def tolerance(points):
    return 1e-12 * float(np.abs(points).max())


def crop_case(seed=21):
    """(rec vertices fp32, rec faces, gt vertices fp32, gt faces): the ground truth is a room shell with triangles
    between neighbouring samples; the reconstruction is a lattice sheet stack that sticks out of the ground truth's
    box on every side, triangulated along the lattice so that faces straddle the boundary."""
    gt_v = room_shell(3000, seed)
    rng = np.random.default_rng(seed)
    gt_f = rng.integers(0, len(gt_v), (500, 3))
    R, t = rotation(seed + 1), np.array([0.3, -0.2, 1.4])
    nx, ny, nz = 23, 17, 9
    gx, gy, gz = np.meshgrid(np.linspace(-3.47, 3.47, nx), np.linspace(-2.43, 2.43, ny), np.linspace(-1.73, 1.73, nz),
                             indexing='ij')
    local = np.stack([gx, gy, gz], axis=-1).reshape(-1, 3)
    rec_v = (local @ R.T + t).astype(np.float32)
    idx = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    rec_f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)])
    return rec_v, rec_f.astype(np.int64), gt_v, gt_f.astype(np.int64)
