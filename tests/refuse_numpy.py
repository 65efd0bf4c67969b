"""numpy restatements of the mesh re-fusion (csrc/refuse.hip, utils/mesh_refuse.py) for the tests, and the scenes they
share.  The ray-caster is fp64 brute force (every pixel against every triangle); the TSDF and frustum rules are fp32
with every operation rounded separately, the arithmetic of the kernels.  All of them take the world-to-camera rows as
the kernels get them: the fp64 inverse of the pose rounded to fp32 (``w2c_rows``)."""
import numpy as np

F32 = np.float32


def w2c_rows(poses):
    """[n,4,4] camera-to-world -> [n,3,4] float32 world-to-camera rows (fp64 inverse, rounded once)."""
    return np.linalg.inv(np.asarray(poses, np.float64))[:, :3, :].astype(F32)


def icosphere(subdivisions, radius, centre):
    """Vertices (fp32-rounded, as float64) and faces of an icosahedron subdivided ``subdivisions`` times: 20 * 4^s faces,
    outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.array(v) * radius + np.asarray(centre, np.float64)
    return verts.astype(F32).astype(np.float64), np.array(f, np.int64)


def box_mesh(lo, hi):
    """The 12 triangles of an axis-aligned box, outward winding."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (k >> d) & 1 else lo)[d] for d in range(3)] for k in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v.astype(F32).astype(np.float64), np.array(f, np.int64)


def join(*meshes):
    off, vs, fs = 0, [], []
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def pose_from(rotation, position):
    p = np.eye(4)
    p[:3, :3], p[:3, 3] = rotation, position
    return p


def look_at(position, target, up=(0.0, 0.0, 1.0)):
    """OpenCV-style camera-to-world pose at ``position`` with +z toward ``target`` (x right, y down)."""
    position, target = np.asarray(position, np.float64), np.asarray(target, np.float64)
    z = target - position
    z /= np.linalg.norm(z)
    up = np.asarray(up, np.float64)
    if abs(z @ up) > 0.99:
        up = np.array([1.0, 0.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    return pose_from(np.stack([x, np.cross(z, x), z], 1), position)


def room_scene(seed=0, n_cameras=8):
    """The shared test scene: a closed box with an icosphere (2 subdivisions, 320 faces) in it and cameras inside the
    box with random rotations.  -> (vertices, faces, poses [n,4,4])."""
    v, f = join(box_mesh((-2, -1.5, -2), (2, 1.5, 2)), icosphere(2, 0.5, (0.3, -0.2, 0.8)))
    rng = np.random.default_rng(seed)
    pos = rng.uniform((-0.8, -0.48, -1.6), (0.8, 0.48, 0.0), (n_cameras, 3))
    poses = np.stack([pose_from(random_rotation(rng), p) for p in pos])
    return v, f, poses


def raycast(vertices, faces, poses, K, height, width, znear=0.05, zfar=100.0, pixel_center=0.5):
    """fp64 brute force.  -> (depth [n,H,W] float64, 0 = no hit; exempt [n,H,W] bool; grazing [n,H,W] bool).
    exempt: some triangle met in front of the camera has a barycentric coordinate within 1e-4 of 0 (the ray passes
    within that of one of its edges), or a hit lies within 1e-5 of znear, or the nearest face meets the ray at
    |cos| < 0.05 (``grazing``, a subset)."""
    fx, fy, cx, cy = K
    rows = w2c_rows(poses).astype(np.float64)
    vertices = np.asarray(vertices, np.float64)
    n = len(rows)
    depth = np.zeros((n, height, width))
    exempt = np.zeros((n, height, width), bool)
    grazing = np.zeros((n, height, width), bool)
    jj, ii = np.meshgrid(np.arange(width), np.arange(height))
    d = np.stack([(jj + pixel_center - cx) / fx, (ii + pixel_center - cy) / fy, np.ones_like(jj, np.float64)],
                 -1).reshape(-1, 3)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    for k in range(n):
        if len(faces) == 0:
            continue
        vc = vertices @ rows[k, :, :3].T + rows[k, :, 3]
        a, b, c = vc[faces[:, 0]], vc[faces[:, 1]], vc[faces[:, 2]]
        nrm = np.cross(b - a, c - a)
        area2 = (nrm * nrm).sum(1)
        ok = area2 > 0
        a, b, c, nrm, area2 = a[ok], b[ok], c[ok], nrm[ok], area2[ok]
        nd = d @ nrm.T                                             # [P, F]
        with np.errstate(divide='ignore', invalid='ignore'):
            t = (nrm * a).sum(1)[None] / nd
            p = t[..., None] * d[:, None, :]
            bary = np.stack([(np.cross(b[None] - p, c[None] - p) * nrm[None]).sum(-1),
                             (np.cross(c[None] - p, a[None] - p) * nrm[None]).sum(-1),
                             (np.cross(a[None] - p, b[None] - p) * nrm[None]).sum(-1)], -1) / area2[None, :, None]
        bmin = np.where(np.isfinite(t), bary.min(-1), -np.inf)
        front = np.isfinite(t) & (t > 0)
        hit = front & (bmin >= 0) & (t >= znear) & (t <= zfar)
        tt = np.where(hit, t, np.inf)
        near = tt.argmin(1)
        z = tt[np.arange(len(d)), near]
        found = np.isfinite(z)
        cos = np.abs(dn @ (nrm / np.sqrt(area2)[:, None]).T)[np.arange(len(d)), near]
        graze = found & (cos < 0.05)
        edge = (front & (bmin >= -1e-4) & (bmin <= 1e-4)).any(1)
        plane = (front & (bmin >= 0) & (np.abs(t - znear) < 1e-5)).any(1)
        depth[k] = np.where(found, z, 0.0).reshape(height, width)
        grazing[k] = graze.reshape(height, width)
        exempt[k] = (edge | plane | graze).reshape(height, width)
    return depth, exempt, grazing


def tsdf_fp32(depth, poses, K, origin, dims, voxel_length, sdf_trunc, depth_trunc=5.0):
    """The integration rule in fp32, every operation rounded separately, views in order.
    -> (tsdf, weight [nx,ny,nz] float32, exempt [nx,ny,nz] bool).  exempt (decided in fp64): for some view
    fx x / z + cx + 0.5 or its y analogue lies within 1e-4 of an integer, or s lies within 1e-5 of -sdf_trunc."""
    fx, fy, cx, cy = (F32(x) for x in K)
    depth = np.asarray(depth, F32)
    n, H, W = depth.shape
    rows = w2c_rows(poses)
    vl, trunc, dtrunc = F32(voxel_length), F32(sdf_trunc), F32(depth_trunc)
    o = np.asarray(origin, F32)
    half, one = F32(0.5), F32(1.0)
    idx = np.meshgrid(*[np.arange(m) for m in dims], indexing='ij')
    x, y, z = (o[a] + vl * (idx[a].astype(F32) + half) for a in range(3))
    tsdf = np.zeros(dims, F32)
    w = np.zeros(dims, F32)
    exempt = np.zeros(dims, bool)
    for k in range(n):
        m = rows[k]
        pz = m[2, 0] * x + m[2, 1] * y + m[2, 2] * z + m[2, 3]
        px = m[0, 0] * x + m[0, 1] * y + m[0, 2] * z + m[0, 3]
        py = m[1, 0] * x + m[1, 1] * y + m[1, 2] * z + m[1, 3]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            uf = fx * px / pz + cx + half
            vf = fy * py / pz + cy + half
            ok = (pz > 0) & (uf >= 0) & (uf < F32(W)) & (vf >= 0) & (vf < F32(H))
            u = np.where(ok, uf, 0).astype(np.int64)
            v = np.where(ok, vf, 0).astype(np.int64)
            d = depth[k][v, u]
            ok &= (d > 0) & ~(d > dtrunc)
            rx, ry = (u.astype(F32) - cx) / fx, (v.astype(F32) - cy) / fy
            length = np.sqrt(rx * rx + ry * ry + one)
            s = (d - pz) * length
            ok &= ~(s <= -trunc)
            tau = np.minimum(one, s / trunc)
            new = (tsdf * w + tau) / (w + one)
        tsdf = np.where(ok, new, tsdf).astype(F32)
        w = np.where(ok, w + one, w).astype(F32)
        # the exemptions, in fp64 from the same fp32 inputs
        m64 = m.astype(np.float64)
        x64, y64, z64 = (a.astype(np.float64) for a in (x, y, z))
        qz = m64[2, 0] * x64 + m64[2, 1] * y64 + m64[2, 2] * z64 + m64[2, 3]
        qx = m64[0, 0] * x64 + m64[0, 1] * y64 + m64[0, 2] * z64 + m64[0, 3]
        qy = m64[1, 0] * x64 + m64[1, 1] * y64 + m64[1, 2] * z64 + m64[1, 3]
        with np.errstate(divide='ignore', invalid='ignore'):
            u64 = float(fx) * qx / qz + float(cx) + 0.5
            v64 = float(fy) * qy / qz + float(cy) + 0.5
            front = qz > 0
            near_int = front & ((np.abs(u64 - np.round(u64)) < 1e-4) | (np.abs(v64 - np.round(v64)) < 1e-4))
            inside = front & (u64 >= 0) & (u64 < W) & (v64 >= 0) & (v64 < H)
            ui = np.where(inside, u64, 0).astype(np.int64)
            vi = np.where(inside, v64, 0).astype(np.int64)
            d64 = depth[k][vi, ui].astype(np.float64)
            len64 = np.sqrt(((ui - float(cx)) / float(fx)) ** 2 + ((vi - float(cy)) / float(fy)) ** 2 + 1.0)
            s64 = (d64 - qz) * len64
            near_trunc = inside & (d64 > 0) & (np.abs(s64 + float(trunc)) < 1e-5)
        exempt |= near_int | near_trunc
    return tsdf, w, exempt


def face_keep(vertices, faces, weight):
    """A face is kept iff every lattice point in [floor(min), ceil(max)] per axis of its vertices has weight > 0."""
    tri = np.asarray(vertices, np.float64)[faces]
    lo = np.floor(tri.min(1)).astype(np.int64)
    hi = np.ceil(tri.max(1)).astype(np.int64)
    keep = np.ones(len(faces), bool)
    for k in range(len(faces)):
        block = weight[lo[k, 0]:hi[k, 0] + 1, lo[k, 1]:hi[k, 1] + 1, lo[k, 2]:hi[k, 2] + 1]
        keep[k] = bool((block > 0).all())
    return keep


def seen_fp32(vertices, poses, K, height, width):
    """The frustum test in fp32, every operation rounded separately.  -> (seen [V] bool, exempt [V] bool).  exempt
    (decided in fp64): for some view the vertex projects within 1e-4 px of the image border or |z - 1e-5| < 1e-7."""
    fx, fy, cx, cy = (F32(x) for x in K)
    v = np.asarray(vertices, F32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    eps = F32(1e-5)
    seen = np.zeros(len(v), bool)
    exempt = np.zeros(len(v), bool)
    for m in w2c_rows(poses):
        pz = m[2, 0] * x + m[2, 1] * y + m[2, 2] * z + m[2, 3]
        px = m[0, 0] * x + m[0, 1] * y + m[0, 2] * z + m[0, 3]
        py = m[1, 0] * x + m[1, 1] * y + m[1, 2] * z + m[1, 3]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            zz = pz - eps
            u, r = fx * px / zz + cx, fy * py / zz + cy
            seen |= (pz >= eps) & (u > 0) & (u < F32(width)) & (r > 0) & (r < F32(height))
            m64 = m.astype(np.float64)
            q = v.astype(np.float64) @ m64[:, :3].T + m64[:, 3]
            z64 = q[:, 2] - float(eps)
            u64, r64 = float(fx) * q[:, 0] / z64 + float(cx), float(fy) * q[:, 1] / z64 + float(cy)
            border = ((np.abs(u64) < 1e-4) | (np.abs(u64 - width) < 1e-4) | (np.abs(r64) < 1e-4) |
                      (np.abs(r64 - height) < 1e-4))
            exempt |= ((z64 > 0) & border) | (np.abs(z64) < 1e-7)
    return seen, exempt
