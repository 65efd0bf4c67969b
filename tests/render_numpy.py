"""numpy restatements of the mesh renderer (csrc/meshrender.hip, utils/mesh_render.py) for the tests.  The ray-caster
is the fp64 brute force of tests/refuse_numpy.py extended by the nearest face, culling and one more exemption; vertex
normals and depth L1 are fp64; the Phong rule is one function run in fp64 and in fp32; ``check_proj`` is fp32 with
every operation rounded separately.  All of them take the world-to-camera rows as the kernels get them
(``refuse_numpy.w2c_rows``).  The keyword arguments named ``mutant_*`` switch one rule to a wrong one: the CPU tests
check that each of them changes a result on the scenes of the GPU tests, so those scenes can tell the rules apart."""
import numpy as np

import refuse_numpy as rfn

F32 = np.float32
CULL = {'none': 0, 'back': 1, 'front': 2}


def raycast(vertices, faces, poses, K, height, width, znear=0.05, zfar=100.0, pixel_center=0.5, cull='none',
            mutant_tie_largest=False, mutant_cull_flipped=False):
    """fp64 brute force.  -> (depth [n,H,W] float64, 0 = no hit; face [n,H,W] int64, -1 = no hit; exempt [n,H,W] bool;
    back [n,H,W] bool: the nearest hit is seen from behind).
    A face (a, b, c) is front-facing for a ray d iff ((b - a) x (c - a)) . d < 0; ``cull`` 'back' drops the others,
    'front' drops those.  Of the faces at exactly the nearest depth the smallest index wins.
    exempt: as ``refuse_numpy.raycast`` (a ray within 1e-4 of an edge of some triangle in front of the camera, a hit
    within 1e-5 of znear, the nearest face met at |cos| < 0.05), decided over ALL faces whatever the culling, or the
    second-nearest accepted hit lies within 1e-4 relative of the nearest (a near tie: fp32 may order it the other
    way)."""
    fx, fy, cx, cy = K
    rows = rfn.w2c_rows(poses).astype(np.float64)
    vertices = np.asarray(vertices, np.float64)
    faces = np.asarray(faces, np.int64)
    n = len(rows)
    depth = np.zeros((n, height, width))
    face = np.full((n, height, width), -1, np.int64)
    exempt = np.zeros((n, height, width), bool)
    back = np.zeros((n, height, width), bool)
    jj, ii = np.meshgrid(np.arange(width), np.arange(height))
    d = np.stack([(jj + pixel_center - cx) / fx, (ii + pixel_center - cy) / fy, np.ones_like(jj, np.float64)],
                 -1).reshape(-1, 3)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    mode = CULL[cull]
    for k in range(n):
        if len(faces) == 0:
            continue
        vc = vertices @ rows[k, :, :3].T + rows[k, :, 3]
        valid = ((faces >= 0) & (faces < len(vertices))).all(1)
        fc = np.where(valid[:, None], faces, 0)
        a, b, c = vc[fc[:, 0]], vc[fc[:, 1]], vc[fc[:, 2]]
        nrm = np.cross(b - a, c - a)
        area2 = (nrm * nrm).sum(1)
        ok = np.flatnonzero((area2 > 0) & valid)
        a, b, c, nrm, area2 = a[ok], b[ok], c[ok], nrm[ok], area2[ok]
        nd = d @ nrm.T                                             # [P, F]
        with np.errstate(divide='ignore', invalid='ignore'):
            t = (nrm * a).sum(1)[None] / nd
            p = t[..., None] * d[:, None, :]
            bary = np.stack([(np.cross(b[None] - p, c[None] - p) * nrm[None]).sum(-1),
                             (np.cross(c[None] - p, a[None] - p) * nrm[None]).sum(-1),
                             (np.cross(a[None] - p, b[None] - p) * nrm[None]).sum(-1)], -1) / area2[None, :, None]
        bmin = np.where(np.isfinite(t), bary.min(-1), -np.inf)
        front_of_camera = np.isfinite(t) & (t > 0)
        facing = (nd > 0) if mutant_cull_flipped else (nd < 0)     # the face shows its front to the ray
        kept = np.ones_like(facing) if mode == 0 else (facing if mode == 1 else ~facing)
        hit = front_of_camera & (bmin >= 0) & (t >= znear) & (t <= zfar) & kept
        tt = np.where(hit, t, np.inf)
        z = tt.min(1)
        found = np.isfinite(z)
        at_min = tt == z[:, None]
        order = at_min[:, ::-1] if mutant_tie_largest else at_min
        near = order.argmax(1)
        if mutant_tie_largest:
            near = at_min.shape[1] - 1 - near
        rows_i = np.arange(len(d))
        cos = np.abs(dn @ (nrm / np.sqrt(area2)[:, None]).T)[rows_i, near]
        graze = found & (cos < 0.05)
        edge = (front_of_camera & (bmin >= -1e-4) & (bmin <= 1e-4)).any(1)
        plane = (front_of_camera & (bmin >= 0) & (np.abs(t - znear) < 1e-5)).any(1)
        second = np.where(at_min, np.inf, tt).min(1)
        with np.errstate(invalid='ignore'):
            tie = found & np.isfinite(second) & (second - z <= 1e-4 * z)
        depth[k] = np.where(found, z, 0.0).reshape(height, width)
        face[k] = np.where(found, ok[near], -1).reshape(height, width)
        back[k] = (found & (nd[rows_i, near] > 0)).reshape(height, width)
        exempt[k] = (edge | plane | graze | tie).reshape(height, width)
    return depth, face, exempt, back


def vertex_normals(vertices, faces):
    """Per vertex the sum of (b - a) x (c - a) over its faces in ascending face index, in fp64 from the fp32
    coordinates, over its length sqrt((x x + y y) + z z); (0, 0, 1) where that is zero or not finite; rounded once to
    fp32.  Faces with a repeated or out-of-range index add nothing."""
    v = np.asarray(vertices, F32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f = f[ok]
    a = v[f[:, 0]]
    u, w = v[f[:, 1]] - a, v[f[:, 2]] - a
    cr = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                   u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    s = np.zeros((len(v), 3))
    np.add.at(s, f.reshape(-1), np.repeat(cr, 3, axis=0))          # unbuffered, in order: ascending face per vertex
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        good = (length > 0) & np.isfinite(length)
        out = np.where(good[:, None], s / np.where(good, length, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    return out.astype(F32)


def light_frame(vertices):
    """Centre and largest extent of the bounding box, as the fp32 numbers the kernel gets."""
    v = np.asarray(vertices, F32).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return tuple(float(F32(x)) for x in (lo + hi) / 2), float(F32((hi - lo).max()))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _unit(v):
    length = np.sqrt(_dot(v, v))
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where((length > 0)[..., None], v / length[..., None], np.zeros_like(v))


def _rot(m, p):
    return np.stack([(m[r, 0] * p[..., 0] + m[r, 1] * p[..., 1]) + m[r, 2] * p[..., 2] for r in range(3)], -1)


def phong(dtype, face, depth, rows, K, vertices, faces, normals, table, centre, extent, base=(1.0, 1.0, 1.0),
          colors=None, flat=False, two_sided=False, pixel_center=0.5, mutant_unnormalised=False,
          mutant_world_lights=False, mutant_unclamped_specular=False):
    """The shading rule of include/monosdf_render.h in ``dtype`` (np.float64: the reference; np.float32: a copy
    whose distance from the reference measures what fp32 costs on a scene).  face, depth: [n,H,W] (depth fp32 as the
    renderer wrote it); rows: [n,3,4] fp32 world-to-camera; table: the 42 floats of ``RenderOptions.light_table``.
    -> rgb [n,H,W,3] ``dtype``."""
    T = dtype
    fx, fy, cx, cy = (T(x) for x in K)
    n, H, W = face.shape
    v = np.asarray(vertices, F32).astype(T)
    faces = np.asarray(faces, np.int64)
    table = np.asarray(table, F32).astype(T)
    nrm_v = None if normals is None else np.asarray(normals, F32).astype(T)
    col_v = None if colors is None else np.asarray(colors, F32).astype(T)
    centre = np.asarray(centre, T)
    extent, pc = T(extent), T(pixel_center)
    zero, one, two = T(0), T(1), T(2)
    out = np.empty((n, H, W, 3), T)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    dx = (jj.astype(T) + pc - cx) / fx
    dy = (ii.astype(T) + pc - cy) / fy
    d = np.stack([dx, dy, np.ones_like(dx)], -1)
    for k in range(n):
        m = np.asarray(rows[k], F32).astype(T)
        hit = face[k] >= 0
        tri = faces[np.where(hit, face[k], 0)]
        a, b, c = (_rot(m, v[tri[..., i]]) + m[:, 3] for i in range(3))
        w0, w1, w2 = _dot(d, _cross(a, b - a)), _dot(d, _cross(b, c - b)), _dot(d, _cross(c, a - c))
        with np.errstate(invalid='ignore', divide='ignore'):
            s = (w0 + w1) + w2
            wa, wb, wc = (w1 / s)[..., None], (w2 / s)[..., None], (w0 / s)[..., None]
        z = np.asarray(depth[k], F32).astype(T)
        P = z[..., None] * d
        if flat:
            N = _cross(b - a, c - a)
        else:
            na, nb, nc = (_rot(m, nrm_v[tri[..., i]]) for i in range(3))
            N = (wa * na + wb * nb) + wc * nc
        if not mutant_unnormalised:
            N = _unit(N)
        if two_sided:
            N = np.where((_dot(N, -P) < 0)[..., None], -N, N)
        e = _unit(-P)
        basec = np.broadcast_to(np.asarray(base, F32).astype(T), P.shape)
        if col_v is not None:
            basec = (wa * col_v[tri[..., 0]] + wb * col_v[tri[..., 1]]) + wc * col_v[tri[..., 2]]
        diffuse = np.broadcast_to(table[36:39], P.shape).copy()
        specular = np.zeros_like(P)
        r, u, fw = m[0, :3], -m[1, :3], -m[2, :3]
        if mutant_world_lights:
            r, u, fw = (np.asarray(x, T) for x in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))
        for i in range(4):
            L = table[9 * i:9 * i + 9]
            world = centre + extent * ((L[0] * r + L[1] * u) + L[2] * fw)
            lc = _rot(m, world) + m[:, 3]
            l = _unit(lc - P)
            nl = _dot(N, l)
            cos_t = np.clip(nl, zero, one)
            R = (two * nl)[..., None] * N - l
            er = _dot(e, R)
            cos_a = np.clip(er, zero, one)
            with np.errstate(invalid='ignore', divide='ignore'):
                spec = np.where(cos_a > 0, np.power(np.where(cos_a > 0, cos_a, one), L[8]), zero).astype(T)
                if mutant_unclamped_specular:                      # (e . R)^s of a negative e . R: positive for s = 10
                    spec = np.nan_to_num(np.power(er, L[8])).astype(T)
            diffuse += ((L[6] * cos_t)[..., None] * L[3:6]).astype(T)
            specular += ((L[7] * spec)[..., None] * L[3:6]).astype(T)
        rgb = np.clip(basec * diffuse + specular, zero, one)
        out[k] = np.where(hit[..., None], rgb, table[39:42])
    return out


def views_see(points, poses, K, height, width, mutant_strict=False):
    """``check_proj`` in fp32, every operation rounded separately -> bool [n]: with (x, y, z) = w2c p and q = z - 1e-5:
    q >= 0 and 0 < (fx x + cx z) / q < width and 0 < (fy y + cy z) / q < height."""
    fx, fy, cx, cy = (F32(x) for x in K)
    p = np.asarray(points, F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    eps = F32(1e-5)
    out = []
    for m in rfn.w2c_rows(poses):
        pz = m[2, 0] * x + m[2, 1] * y + m[2, 2] * z + m[2, 3]
        px = m[0, 0] * x + m[0, 1] * y + m[0, 2] * z + m[0, 3]
        py = m[1, 0] * x + m[1, 1] * y + m[1, 2] * z + m[1, 3]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            q = pz - eps
            u, r = (fx * px + cx * pz) / q, (fy * py + cy * pz) / q
            front = (q > 0) if mutant_strict else (q >= 0)
            out.append(bool((front & (u > 0) & (u < F32(width)) & (r > 0) & (r < F32(height))).any()))
    return np.array(out, bool)


def depth_l1(a, b):
    """Per view the mean over all pixels of |a - b|: the difference in fp32, the sum in fp64."""
    diff = np.abs(np.asarray(a, F32) - np.asarray(b, F32))
    return diff.astype(np.float64).reshape(len(diff), -1).sum(1) / float(diff[0].size)
