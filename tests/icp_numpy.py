"""Float64 numpy restatement of the point-to-point ICP of include/monosdf_icp.h (csrc/icp.hip, utils/mesh_align.py),
with the constructed inputs that the CPU and the GPU tests share.

The search is ``gridnn_numpy.brute`` + ``within``: bit for bit what the device search answers.  The moved point is
rounded to fp32 where the kernel rounds it.  The sums are numpy's (pairwise) sums and the rotation is numpy's ``svd``
with the sign rule, so what separates the restatement from the kernels is summation order and the solver alone.
``icp(..., mistake=...)`` swaps in one of five plausible errors, which the tests show the inputs catch."""
import functools

import numpy as np

import gridnn_numpy as gn

MISTAKES = ('rmse_over_N', 'no_sign_rule', 'strict_max_dist', 'compose', 'fitness_only')
N_SUMS = 17


def transform(points, T):
    """fl32(((r0 x + r1 y) + r2 z) + t) per row of T, fp64 arithmetic on the fp32 coordinates."""
    p = np.asarray(points, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)],
                    axis=1).astype(np.float32)


def pivots(source, target):
    """c_s, c_t: the centres of the two bounding boxes in fp64."""
    s, t = np.asarray(source, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    return (s.min(axis=0) + s.max(axis=0)) / 2, (t.min(axis=0) + t.max(axis=0)) / 2


def correspondences(moved, target, max_dist, strict=False):
    """idx int64 [N] with -1: the nearest target point within float32(max_dist)."""
    dist, idx = gn.brute(target, moved)
    if strict:
        return np.where(dist < np.float32(max_dist), idx, -1)
    return gn.within(dist, idx, max_dist)[1]


def terms(source, moved, target, idx, cs, ct):
    """[n_k, 17]: what every correspondence adds to the 17 sums."""
    keep = idx >= 0
    p = np.asarray(source, np.float32).astype(np.float64)[keep] - cs
    qq = np.asarray(target, np.float32).astype(np.float64)[idx[keep]]
    q = qq - ct
    d = np.asarray(moved, np.float32).astype(np.float64)[keep] - qq
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.concatenate([np.ones((len(p), 1)), p, q, (p[:, :, None] * q[:, None, :]).reshape(-1, 9), r2[:, None]],
                          axis=1)


def sums(source, moved, target, idx, cs, ct):
    return terms(source, moved, target, idx, cs, ct).sum(axis=0) if (idx >= 0).any() else np.zeros(N_SUMS)


def rotation(H, sign_rule=True):
    """R that maximises tr(R H) over the proper rotations: numpy's svd, V diag(1, 1, det) U^T."""
    U, _, Vt = np.linalg.svd(H)
    if sign_rule and np.linalg.det(Vt.T @ U.T) < 0:
        Vt = Vt.copy()
        Vt[2] *= -1
    return Vt.T @ U.T


def measure(s, n_source, over_n=False):
    """(fitness, rmse) of the sums s."""
    if s[0] == 0:
        return 0.0, 0.0
    return s[0] / n_source, float(np.sqrt(s[16] / (n_source if over_n else s[0])))


def update(s, cs, ct, T, sign_rule=True):
    """Step 5: T_{k+1} from the sums; T itself when there is no correspondence."""
    if s[0] == 0:
        return T
    mp, mq = s[1:4] / s[0], s[4:7] / s[0]
    H = s[7:16].reshape(3, 3) / s[0] - np.outer(mp, mq)
    R = rotation(H, sign_rule)
    out = np.eye(4)
    out[:3, :3] = R
    out[:3, 3] = (ct + mq) - R @ (cs + mp)
    return out


def kabsch(src, dst, T=None):
    """The 4 x 4 of step 5 for two equal-length clouds; ``T`` (default identity) for n = 0."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    T = np.eye(4) if T is None else T
    if len(src) == 0:
        return T
    cs, ct = pivots(src, dst)
    return update(sums(src, src, dst, np.arange(len(src)), cs, ct), cs, ct, T)


def icp(source, target, max_dist=0.1, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
        mistake=None):
    """-> (T, fitness, rmse, log [evaluations, 3], per-evaluation list of (moved, idx))."""
    assert mistake is None or mistake in MISTAKES
    source, target = np.asarray(source, np.float32), np.asarray(target, np.float32)
    cs, ct = pivots(source, target)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    log, trace, pts = [], [], source
    for k in range(max_iteration + 1):
        moved = transform(pts, T if mistake != 'compose' or k == 0 else step)
        idx = correspondences(moved, target, max_dist, strict=mistake == 'strict_max_dist')
        s = sums(source, moved, target, idx, cs, ct)
        fitness, rmse = measure(s, len(source), over_n=mistake == 'rmse_over_N')
        log.append((fitness, rmse, s[0]))
        trace.append((moved, idx))
        if k >= 1 and abs(fitness - log[-2][0]) < relative_fitness and \
                (mistake == 'fitness_only' or abs(rmse - log[-2][1]) < relative_rmse):
            break
        if k == max_iteration:
            break
        if mistake == 'compose':
            # open3d's way: the update that maps the MOVED cloud onto its correspondences, composed with T, applied
            # to a cloud that is rounded to fp32 at every step
            ms, _ = pivots(moved, target)
            step = update(sums(moved, moved, target, idx, ms, ct), ms, ct, np.eye(4))
            T, pts = step @ T, moved
        else:
            T = update(s, cs, ct, T, sign_rule=mistake != 'no_sign_rule')
    return T, log[-1][0], log[-1][1], np.array(log), trace


# ---------------------------------------------------------------- the constructed inputs

def rigid(axis, degrees, shift):
    """4 x 4: the rotation by ``degrees`` about ``axis`` through the origin (Rodrigues), then ``shift``."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = shift
    return M


def surface(rng, count):
    """``count`` points of z = 0.3 sin 2.1 x + 0.2 y^2 + 0.15 x y over the square |x|, |y| <= 0.5, fp32."""
    xy = rng.uniform(-0.5, 0.5, (count, 2))
    z = 0.3 * np.sin(2.1 * xy[:, 0]) + 0.2 * xy[:, 1] ** 2 + 0.15 * xy[:, 0] * xy[:, 1]
    return np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)


MOTION = rigid((1.0, 2.0, 3.0), 6.0, np.array([0.02, -0.03, 0.0173]))      # |shift| = 0.04
MAX_DIST = 0.1
SEEDS = {'subset': 21, 'noisy': 22, 'tiny': 23}


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (source, target, the motion that was applied to the source or None): float32 clouds inside the unit box.
      'subset'  300 of 1200 surface points moved by MOTION: ICP must find its inverse
      'noisy'   the same with N(0, 0.002) added to the moved points
      'tiny'    64 of 256 points"""
    rng = np.random.default_rng(SEEDS[name])
    n_t, n_s = (256, 64) if name == 'tiny' else (1200, 300)
    target = surface(rng, n_t)
    pick = np.sort(rng.choice(n_t, n_s, replace=False))
    moved = target[pick].astype(np.float64) @ MOTION[:3, :3].T + MOTION[:3, 3]
    if name == 'noisy':
        moved = moved + rng.normal(0.0, 0.002, moved.shape)
    return moved.astype(np.float32), target, MOTION


@functools.lru_cache(maxsize=None)
def solved(name):
    """The restatement's answer for ``case(name)``, computed once and shared."""
    source, target, _ = case(name)
    return icp(source, target, MAX_DIST)


def mirrored_pair():
    """A generic slab, thin along x, and its mirror image in the plane x = 0: the best ORTHOGONAL map is the
    reflection, so the rotation must take the sign rule; the slab's thin axis is clearly the one to give up."""
    rng = np.random.default_rng(31)
    src = (rng.uniform(-0.5, 0.5, (40, 3)) * (0.1, 1.0, 1.0)).astype(np.float32)
    return src, src * np.array([-1, 1, 1], np.float32)


def coplanar_pair():
    """A cloud in the plane z = 0.25 and its image under a rotation about z by 90 degrees and an integer shift: every
    coordinate a multiple of 1/8, so the moved cloud is exact in fp32 and H has rank two."""
    rng = np.random.default_rng(32)
    src = np.concatenate([rng.integers(-4, 5, (30, 2)) / 8.0, np.full((30, 1), 0.25)], axis=1)
    R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, (1.0, -2.0, 0.5)
    return src.astype(np.float32), (src @ R.T + T[:3, 3]).astype(np.float32), T


def tie_pair():
    """One source point exactly max_dist = 0.25 from its only near target point, and three that match theirs."""
    target = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    source = target.copy()
    source[0] = (0.25, 0, 0)
    return source, target, 0.25


@functools.lru_cache(maxsize=None)
def mesh_pair():
    """-> (rec vertices, gt vertices, faces, the motion applied to rec): two sheets one above the other, each a
    jittered 20 x 20 grid of vertices (no lattice that could slide onto itself), centred in the unit box; ``rec`` is
    ``gt`` turned by 5 degrees about (2, -1, 3) through the origin."""
    rng = np.random.default_rng(41)
    g = (np.arange(20) + 0.5) / 20 - 0.5
    sheets, faces = [], []
    for s, lift in enumerate((-0.12, 0.13)):
        xy = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2) + rng.uniform(-0.015, 0.015, (400, 2))
        z = lift + (0.1 * np.sin(3.0 * xy[:, 0] + s) + 0.15 * xy[:, 1] ** 2 + 0.1 * (1 - 2 * s) * xy[:, 0] * xy[:, 1])
        sheets.append(np.concatenate([xy, z[:, None]], axis=1))
        i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(19), np.arange(19), indexing='ij'))
        a = 400 * s + 20 * i + j
        faces += [np.stack([a, a + 20, a + 1], 1), np.stack([a + 1, a + 20, a + 21], 1)]
    gt = np.concatenate(sheets).astype(np.float32)
    motion = rigid((2.0, -1.0, 3.0), 5.0, (0.0, 0.0, 0.0))
    rec = (gt.astype(np.float64) @ motion[:3, :3].T).astype(np.float32)
    return rec, gt, np.concatenate(faces).astype(np.int32), motion
