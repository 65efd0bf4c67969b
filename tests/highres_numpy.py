"""Float64 restatement of the high-resolution cue merge (preprocess/generate_high_res_map.py lines 44-174, 297-383):
the yardstick of the GPU tests (test_gpu_highres.py), itself pinned to the reference's recorded outputs by
test_highres_cpu.py.  One image at a time, everything in float64; `axis` 1 merges along x (rows, left to right),
axis 0 along y (row strips, top to bottom).

``store``: the dtype the running depth mosaic is rounded to after every step (None: float64 throughout, the
yardstick; np.float32: a model of the device, which forms every value in fp64 and stores fp32).
``fade`` and ``fit`` select deliberately wrong variants, which test_highres_cpu.py shows to miss the bar."""
import numpy as np


def linspace_weight(O):
    return np.linspace(1, 0, O)


def fit_depth(p, t):
    """Least-squares (scale, shift) of p onto t and the determinant (reference lines 44-64); 0, 0 where it is 0."""
    p = np.asarray(p, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    a00, a01, a11 = np.sum(p * p), np.sum(p), float(p.size)
    b0, b1 = np.sum(p * t), np.sum(t)
    det = a00 * a11 - a01 * a01
    if det != 0:
        return (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det, det
    return 0.0, 0.0, det


def _blend(M, Q, axis, O, fade):
    """M with Q cross-faded in along `axis` over the last O lines of M / first O of Q (any leading dims)."""
    M, Q = np.moveaxis(M, axis, -1), np.moveaxis(Q, axis, -1)
    w = linspace_weight(O)
    if fade == 'reversed':
        w = w[::-1]
    s1 = M.shape[-1] - O
    out = np.concatenate([M[..., :s1], M[..., s1:] * w + Q[..., :O] * (1 - w), Q[..., O:]], axis=-1)
    return np.moveaxis(out, -1, axis)


def _overlap(M, Q, axis, O):
    M, Q = np.moveaxis(M, axis, -1), np.moveaxis(Q, axis, -1)
    return M[..., M.shape[-1] - O:], Q[..., :O]


def depth_step(M, Q, axis, O, fade='forward', fit='patch'):
    m, q = _overlap(M, Q, axis, O)
    if fit == 'patch':
        scale, shift, det = fit_depth(q, m)
        Q = scale * Q + shift
    else:                                                   # wrong on purpose: the mosaic is fitted to the patch
        scale, shift, det = fit_depth(m, q)
        M = scale * M + shift
    return _blend(M, Q, axis, O, fade), (scale, shift), det


def merge_depth(patches, S, mid=None, store=None, fade='forward', fit='patch'):
    """patches [R, C, P, P], mid [P, P] or None -> dict(raw: the mosaic before the final normalisation, out: after,
    steps [n_steps, 2], det [n_steps])."""
    patches = np.asarray(patches, dtype=np.float64)
    R, C, P = patches.shape[:3]
    O = P - S
    keep = (lambda a: a) if store is None else (lambda a: a.astype(store).astype(np.float64))
    steps, dets, strips = [], [], []
    for r in range(R):
        M = patches[r, 0]
        for c in range(1, C):
            M, coef, det = depth_step(M, patches[r, c], 1, O, fade, fit)
            M = keep(M)
            steps.append(coef)
            dets.append(det)
        strips.append(M)
    M = strips[0]
    for r in range(1, R):
        M, coef, det = depth_step(M, strips[r], 0, O, fade, fit)
        M = keep(M)
        steps.append(coef)
        dets.append(det)
    if mid is not None:
        H, W = M.shape
        y0, x0 = H // 2 - P // 2, W // 2 - P // 2
        scale, shift, det = fit_depth(M[y0:y0 + P, x0:x0 + P], mid)
        M = keep(scale * M + shift)
        steps.append((scale, shift))
        dets.append(det)
    out = keep((M - M.min()) / (M.max() - M.min()))
    return dict(raw=M, out=out, steps=np.array(steps, dtype=np.float64).reshape(-1, 2), det=np.array(dets))


def best_rotation(A, B):
    """Reference lines 67-87 on A, B [n, 3] -> (R, the singular values, d = the sign of det(V U^T))."""
    H = np.dot(A.T, B)
    U, s, Vt = np.linalg.svd(H)
    R = np.dot(Vt.T, U.T)
    d = 1.0
    if np.linalg.det(R) < 0:
        Vt = Vt.copy()
        Vt[2, :] *= -1
        R = np.dot(Vt.T, U.T)
        d = -1.0
    return R, s, d


def normal_step(M, Q, axis, O):
    """M, Q [3, h, w]; axis 1 (rows of the image: along y) or 2 (along x)."""
    m, q = _overlap(M, Q, axis, O)
    R, s, d = best_rotation(q.reshape(3, -1).T, m.reshape(3, -1).T)
    Q = (R @ Q.reshape(3, -1)).reshape(Q.shape)
    out = _blend(M, Q, axis, O, 'forward')
    return out / (np.linalg.norm(out, axis=0) + 1e-15)[None], R, s, d


def merge_normals(patches, S, mid=None):
    """patches [R, C, 3, P, P] decoded unit normals, mid [3, P, P] or None -> dict(raw: the unit normals, out:
    (raw + 1) / 2, steps [n_steps, 3, 3], sv [n_steps, 3], d [n_steps])."""
    patches = np.asarray(patches, dtype=np.float64)
    R_, C, _, P = patches.shape[:4]
    O = P - S
    steps, svs, ds, strips = [], [], [], []

    def take(result):
        steps.append(result[1])
        svs.append(result[2])
        ds.append(result[3])
        return result[0]

    for r in range(R_):
        M = patches[r, 0]
        for c in range(1, C):
            M = take(normal_step(M, patches[r, c], 2, O))
        strips.append(M)
    M = strips[0]
    for r in range(1, R_):
        M = take(normal_step(M, strips[r], 1, O))
    if R_ == 1 and C == 1:
        # no step has divided anything: divided once here, so that every grid gives unit vectors in float64.  (The
        # reference's functions do not run on a 1 x 1 grid; its main loop would save the fp32 decode as it came.)
        M = M / (np.linalg.norm(M, axis=0) + 1e-15)[None]
    if mid is not None:
        H, W = M.shape[1:]
        y0, x0 = H // 2 - P // 2, W // 2 - P // 2
        rot, s, d = best_rotation(M[:, y0:y0 + P, x0:x0 + P].reshape(3, -1).T, np.asarray(mid, np.float64).reshape(3, -1).T)
        M = take(((rot @ M.reshape(3, -1)).reshape(M.shape), rot, s, d))
    return dict(raw=M, out=(M + 1.) / 2., steps=np.array(steps, dtype=np.float64).reshape(-1, 3, 3),
                sv=np.array(svs, dtype=np.float64).reshape(-1, 3), d=np.array(ds, dtype=np.float64))


def relative_gap(a, b, scale):
    """max |a - b| / max |scale|."""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(scale).max())
