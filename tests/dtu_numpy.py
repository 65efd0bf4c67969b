"""Numpy restatements of the DTU protocol's rules (reference: dtu_eval/evaluate_single_scene.py, dtu_eval/eval.py),
written for clarity and not for speed: what csrc/dtueval.hip and utils/mesh_dtu.py must reproduce exactly."""
import numpy as np

import nn_numpy as nnn


def disk_halfwidths(radius):
    """{dy: floor(sqrt(r^2 - dy^2))} in integers: the row runs of skimage's disk(r)."""
    out = {}
    for dy in range(-radius, radius + 1):
        w = 0
        while (w + 1) ** 2 + dy * dy <= radius * radius:
            w += 1
        out[dy] = w
    return out


def _shifted(m, dy, dx):
    """out[y, x] = m[y - dy, x - dx], unset where that lies outside the image."""
    h, w = m.shape[-2:]
    out = np.zeros_like(m)
    if abs(dy) >= h or abs(dx) >= w:
        return out
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[..., yd, xd] = m[..., ys, xs]
    return out


def dilate(masks, radius):
    """binary_dilation(mask != 0, disk(radius)) of [n, H, W] (or [H, W]) by OR-ing shifted copies -> bool."""
    m = np.asarray(masks) != 0
    out = np.zeros_like(m)
    for dy, hw in disk_halfwidths(radius).items():
        for dx in range(-hw, hw + 1):
            out |= _shifted(m, dy, dx)
    return out


def project(vertices, projections):
    """(px, py, valid) [n_views, V] in separately rounded fp32, for images of the size given to ``mask_vertices``."""
    v = np.asarray(vertices, np.float32)
    P = np.asarray(projections, np.float64).astype(np.float32).reshape(-1, 3, 4)
    x, y, z = v[:, 0][None], v[:, 1][None], v[:, 2][None]
    rows = []
    with np.errstate(all='ignore'):
        for k in range(3):
            p = [P[:, k, c][:, None] for c in range(4)]
            rows.append(((p[0] * x + p[1] * y) + p[2] * z) + p[3])
        den = rows[2] + np.float32(1e-6)
        px, py = rows[0] / den, rows[1] / den
    assert px.dtype == np.float32
    return px, py


def mask_vertices(vertices, projections, dilated, reasons=False):
    """kept [V] bool: in every view not valid or the dilated mask set at (rint(px), rint(py)).  ``reasons``: also
    whether some view's mask kept a valid vertex."""
    d = np.asarray(dilated) != 0
    n, h, w = d.shape
    px, py = project(vertices, projections)
    with np.errstate(invalid='ignore'):
        valid = (px > 0) & (px < np.float32(w - 1)) & (py > 0) & (py < np.float32(h - 1))
    ix = np.where(valid, np.rint(px), 0).astype(np.int64)
    iy = np.where(valid, np.rint(py), 0).astype(np.int64)
    hit = d[np.arange(n)[:, None], iy, ix]
    kept = (~valid | hit).all(0)
    if reasons:
        return kept, valid.any(0)
    return kept


def cull_mesh(vertices, faces, kept):
    """trimesh's update_vertices / update_faces: kept vertices, the faces with all three kept, reindexed."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    new_index = np.cumsum(kept) - 1
    fk = kept[faces].all(1)
    return np.asarray(vertices)[kept], new_index[faces[fk]]


def sample_lattice(vertices, faces, density=0.2):
    """eval.py:54-71 in fp64 on the fp32 vertices -> float32 [M, 3], in the order face, i, j."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    out = []
    for f in np.asarray(faces, np.int64).reshape(-1, 3):
        p0 = v[f[0]]
        v1, v2 = v[f[1]] - p0, v[f[2]] - p0
        l1 = np.sqrt((v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2])
        l2 = np.sqrt((v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2])
        c = np.array([v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]])
        area2 = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        if not area2 > 0:
            continue
        thr = density * np.sqrt(l1 * l2 / area2)
        n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
        a = (np.arange(int(n1) + 1) + 0.5) / max(n1, 1e-7)
        b = (np.arange(int(n2) + 1) + 0.5) / max(n2, 1e-7)
        keep = (a[:, None] + b[None, :]) < 1
        i, j = np.nonzero(keep)                              # row-major: i, then j
        out.append((v1[None] * a[i][:, None] + v2[None] * b[j][:, None]) + p0[None])
    if not out:
        return np.zeros((0, 3), np.float32)
    return np.concatenate(out).astype(np.float32)


def within(points, k, radius):
    """Which points lie within ``radius`` of point k: ((dx dx + dy dy) + dz dz) <= r r in fp64."""
    p = np.asarray(points, np.float32).astype(np.float64)
    d = p - p[k]
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= float(radius) * float(radius)


def radius_thin(points, radius, order=None):
    """eval.py:86-94 by brute force: visiting in ``order``, a point still marked is kept and unmarks all within r."""
    n = len(points)
    mask = np.ones(n, bool)
    for k in (range(n) if order is None else np.asarray(order)):
        if mask[k]:
            mask[within(points, k, radius)] = False
            mask[k] = True
    return mask


def thin_rounds(points, radius, order=None):
    """The parallel iteration on the host (synchronous rounds): -> (kept mask, number of rounds)."""
    n = len(points)
    rank = np.arange(n) if order is None else np.argsort(np.asarray(order))
    earlier = [np.flatnonzero(within(points, k, radius) & (rank < rank[k])) for k in range(n)]
    state = np.zeros(n, np.int8)                              # 0 undecided, 1 kept, 2 removed
    rounds = 0
    while (state == 0).any():
        new = state.copy()
        for k in np.flatnonzero(state == 0):
            s = state[earlier[k]]
            new[k] = 2 if (s == 1).any() else (0 if (s == 0).any() else 1)
        state = new
        rounds += 1
    return state == 1, rounds


def evaluate(cloud, order, stl, obs_mask, bb, res, plane, density=0.2, patch=60, max_dist=20):
    """eval.py:86-134 on a cloud (vertices ++ lattice samples, or a bare cloud) -> (metrics, stages)."""
    cloud = np.asarray(cloud, np.float32)
    keep = radius_thin(cloud, density, order)
    down = cloud[keep]
    bb = np.asarray(bb).astype(np.float32)
    lower, upper = bb[:1] - np.float32(patch), bb[1:] + np.float32(patch * 2)
    d64 = down.astype(np.float64)
    inbound = ((d64 >= lower.astype(np.float64)) & (d64 < upper.astype(np.float64))).sum(-1) == 3
    data_in = down[inbound]
    grid = np.rint((data_in.astype(np.float64) - bb[:1].astype(np.float64)) / float(res)).astype(np.int64)
    obs_mask = np.asarray(obs_mask)
    grid_in = ((grid >= 0) & (grid < np.array(obs_mask.shape)[None])).sum(-1) == 3
    g = grid[grid_in]
    in_obs = obs_mask[g[:, 0], g[:, 1], g[:, 2]] != 0
    data_in_obs = data_in[grid_in][in_obs]
    stl = np.asarray(stl, np.float32)
    dist_d2s = nnn.nearest(stl, data_in_obs)[0]
    s64, pl = stl.astype(np.float64), np.asarray(plane, np.float64).reshape(-1)
    above = ((s64[:, 0] * pl[0] + s64[:, 1] * pl[1]) + s64[:, 2] * pl[2]) + pl[3] > 0
    stl_above = stl[above]
    dist_s2d = nnn.nearest(data_in, stl_above)[0]
    d2s, s2d = dist_d2s[dist_d2s < max_dist].mean(), dist_s2d[dist_s2d < max_dist].mean()
    return ({'d2s': float(d2s), 's2d': float(s2d), 'overall': float((d2s + s2d) / 2)},
            {'keep': keep, 'data_in': data_in, 'data_in_obs': data_in_obs, 'stl_above': stl_above,
             'dist_d2s': dist_d2s, 'dist_s2d': dist_s2d})


# ---- inputs the CPU and the GPU tests share

def thin_cases():
    """name -> (points float32 [N,3], radius, order or None): the five inputs of the thinning tests."""
    rng = np.random.default_rng(7)
    cases = {}
    cases['random_cube'] = (rng.uniform(0, 1, (2500, 3)).astype(np.float32), 0.08, None)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing='ij'), -1).reshape(-1, 3)
    # spacing 0.5, r = 2.5: the offsets (3, 4, 0) and (5, 0, 0) are at exactly r, in fp32 and in fp64
    cases['lattice_pairs_at_r'] = ((g * 0.5).astype(np.float32), 2.5, rng.permutation(len(g)))
    g = np.stack(np.meshgrid(*[np.arange(10)] * 3, indexing='ij'), -1).reshape(-1, 3)
    cases['integer_lattice'] = (g.astype(np.float32), 1.0, rng.permutation(len(g)))
    chain = np.zeros((400, 3), np.float32)
    chain[:, 0] = np.arange(400) * 0.6
    cases['sorted_chain'] = (chain, 1.0, None)
    base = rng.uniform(0, 1, (100, 3)).astype(np.float32)
    cases['duplicates'] = (np.tile(base, (20, 1))[rng.permutation(2000)], 0.05, None)
    return cases


def ring_scene(seed, n_views=5, height=40, width=56, n_vertices=4000):
    """Cameras on a ring of radius 3 that look at a ball of radius 0.6 at the origin -> (projections [n,3,4] float64,
    masks [n,H,W] uint8: the ball's silhouette, vertices [V,3] float32: half in the cube [-4,4]^3, which reaches
    behind and beside the cameras, half in [-1,1]^3)."""
    rng = np.random.default_rng(seed)
    K = np.array([[50.0, 0, (width - 1) / 2], [0, 50.0, (height - 1) / 2], [0, 0, 1]])
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
    d = np.stack([(u - K[0, 2]) / 50.0, (v - K[1, 2]) / 50.0, np.ones_like(u, float)], -1)
    c = np.array([0.0, 0.0, 3.0])                              # the ball's centre in every camera's frame
    miss = np.linalg.norm(np.cross(np.broadcast_to(c, d.shape), d), axis=-1) / np.linalg.norm(d, axis=-1)
    mask = (miss < 0.6).astype(np.uint8)
    proj = []
    for k in range(n_views):
        t = 2 * np.pi * k / n_views + 0.3
        z = -np.array([np.cos(t), 0.2, np.sin(t)])            # viewing direction
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])                  # world -> camera
        proj.append(K @ np.concatenate([R, (R @ (3.0 * z))[:, None]], 1))
    verts = np.concatenate([rng.uniform(-4, 4, (n_vertices // 2, 3)), rng.uniform(-1, 1, (n_vertices // 2, 3))])
    return np.stack(proj), np.stack([mask] * n_views), verts[rng.permutation(len(verts))].astype(np.float32)
