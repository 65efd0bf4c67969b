"""Numpy restatement of the marching-cubes kernels (csrc/mcubes.hip) over the generated table, for the tests.

Same classification (below = v < level), vertex order (linear voxel index, axis), face order (linear cell index,
table order), interpolation and normals, in fp32."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location('gen_mc_tables', os.path.join(ROOT, 'scripts', 'gen_mc_tables.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GEN = load_generator()
TABLES = _GEN.build_tables()
MAX_T = max(len(t) for t in TABLES)
TRI = np.full((256, MAX_T, 3), -1, np.int64)
for _c, _tris in enumerate(TABLES):
    for _t, _tri in enumerate(_tris):
        TRI[_c, _t] = _tri
TRI_COUNT = np.array([len(t) for t in TABLES], np.int64)
EDGE_AXIS = np.array(_GEN.EDGE_AXIS)
EDGE_OFF = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in _GEN.EDGE_C0])   # owner offset of each edge


def _gradient(vol, sp):
    """Central differences / spacing, one-sided on the border, fp32: [nx, ny, nz, 3]."""
    g = np.empty(vol.shape + (3,), np.float32)
    for a in range(3):
        v = np.moveaxis(vol, a, 0)
        d = np.empty_like(v)
        d[1:-1] = (v[2:] - v[:-2]) / np.float32(2 * sp[a])
        d[0] = (v[1] - v[0]) / np.float32(sp[a])
        d[-1] = (v[-1] - v[-2]) / np.float32(sp[a])
        g[..., a] = np.moveaxis(d, 0, a)
    return g


def marching_cubes(vol, level=0.0, spacing=(1.0, 1.0, 1.0)):
    """-> verts [V,3] f32, faces [F,3] int64, normals [V,3] f32."""
    vol = np.ascontiguousarray(vol, np.float32)
    nx, ny, nz = vol.shape
    lv = np.float32(level)
    sp = [np.float32(s) for s in spacing]
    below = vol < lv
    N = vol.size
    # vertices: crossing edges by (linear voxel index, axis)
    vid = np.full((N, 3), -1, np.int64)
    cross = np.zeros((N, 3), bool)
    for a in range(3):
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[a] = slice(0, vol.shape[a] - 1)
        sl1[a] = slice(1, None)
        c = np.zeros(vol.shape, bool)
        c[tuple(sl0)] = below[tuple(sl0)] != below[tuple(sl1)]
        cross[:, a] = c.reshape(-1)
    order = np.flatnonzero(cross.reshape(-1))            # lin * 3 + axis, ascending
    vid.reshape(-1)[order] = np.arange(order.size)
    lin, axis = order // 3, order % 3
    idx = np.stack(np.unravel_index(lin, vol.shape), 1)
    step = np.eye(3, dtype=np.int64)[axis]
    idx1 = idx + step
    v0 = vol[idx[:, 0], idx[:, 1], idx[:, 2]]
    v1 = vol[idx1[:, 0], idx1[:, 1], idx1[:, 2]]
    t = (lv - v0) / (v1 - v0)
    pos = idx.astype(np.float32)
    pos[np.arange(pos.shape[0]), axis] += t
    verts = (pos * np.array(sp, np.float32)).astype(np.float32)
    g = _gradient(vol, sp)
    g0 = g[idx[:, 0], idx[:, 1], idx[:, 2]]
    g1 = g[idx1[:, 0], idx1[:, 1], idx1[:, 2]]
    n = g0 + t[:, None] * (g1 - g0)
    norm = np.sqrt((n * n).sum(1, dtype=np.float32))
    normals = np.where(norm[:, None] > 0, n / np.where(norm > 0, norm, 1)[:, None], 0).astype(np.float32)
    # faces: cells by linear index, triangles in table order
    code = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        code |= below[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci = np.stack(np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing='ij'), -1).reshape(-1, 3)
    code = code.reshape(-1)
    keep = TRI_COUNT[code] > 0
    ci, code = ci[keep], code[keep]
    faces = []
    for t_ in range(MAX_T):
        sel = TRI_COUNT[code] > t_
        edges = TRI[code[sel], t_]                       # [n, 3]
        own = ci[sel][:, None, :] + EDGE_OFF[edges]      # [n, 3, 3]
        olin = (own[..., 0] * ny + own[..., 1]) * nz + own[..., 2]
        faces.append((vid[olin, EDGE_AXIS[edges]], np.flatnonzero(sel), t_))
    rows = np.concatenate([f[0] for f in faces]) if faces else np.zeros((0, 3), np.int64)
    cell = np.concatenate([f[1] for f in faces])
    tri = np.concatenate([np.full(f[1].size, f[2]) for f in faces])
    rows = rows[np.lexsort((tri, cell))]
    assert (rows >= 0).all()
    return verts, rows.reshape(-1, 3), normals


def edge_use(faces):
    """{(a, b): count} of directed mesh edges."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    keys, cnt = np.unique(e, axis=0, return_counts=True)
    return {tuple(k): int(c) for k, c in zip(keys, cnt)}


def euler(verts, faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    n_edges = np.unique(np.sort(e, 1), axis=0).shape[0]
    return np.unique(faces).size - n_edges + faces.shape[0]


def signed_volume(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


def area(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())
