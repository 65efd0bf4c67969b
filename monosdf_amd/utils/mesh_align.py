"""Rigid alignment of a reconstruction to a ground-truth scan on the GPU: the point-to-point ICP that
``get_align_transformation`` (replica_eval/eval_recon.py:51-65) runs through open3d before ``calc_3d_metric(align=True)``
scores a mesh.

* ``icp``: open3d's ``registration_icp`` with ``TransformationEstimationPointToPoint()`` and the default criteria
  (csrc/icp.hip, ABI msdf_icp_* of include/monosdf_icp.h, which states the rule).
* ``evaluate_registration``: fitness, inlier rmse and the correspondences of one transform.
* ``kabsch``: the best rigid map between two clouds in correspondence.  ``transform_points``: T applied as ICP applies it.
* ``align_mesh``: ICP on the vertices of two meshes, as ``get_align_transformation`` does, and the moved mesh.

Everything runs on CUDA tensors (numpy arrays are uploaded); there is no CPU path.  One iteration is six launches on the
current stream -- transform, the target grid's cell kernel, a sort, the grid query, the 17 sums, the solve -- and the
host reads nothing back inside it: the transform, the iteration count, the convergence test and the log live in one
small device struct, every ICP kernel returns at once when its ``done`` flag is set, and the host looks at the flag
once every ``check_every`` iterations.  The target's grid is one ``PointGrid`` (utils/point_grid.py, the object
``nearest_neighbors_within`` searches through), built once per alignment and queried every iteration.  No atomics: the
same inputs give bitwise the same result every call and for every ``check_every``.

Two deliberate differences from open3d: it composes ``update @ T`` on a cloud that it transforms in place, here T is
solved from the original points every iteration (the same optimum in exact arithmetic, no drift); it holds points in
fp64, here the searched point is fp32.  Parity with open3d is UNVERIFIED: open3d is not available where this is built
and the reference holds no recorded output of it, so the rule is pinned by the numpy restatement of the tests only.
"""
import numpy as np
import torch

from .. import _lib
from . import mesh_args as ma
from .point_grid import GRID_CELL_FRACTION, PointGrid

_T_DOUBLES, _FLAG_WORD = 18, 37      # the state: T[16], prev_fitness, prev_rmse, then int32 iteration, done, then the log


def _cloud(name, arg, cloud, device):
    t = ma.cloud_tensor(name, arg, cloud, device)
    if t.shape[0] == 0:
        raise ValueError('%s: %s is empty' % (name, arg))
    return t.contiguous()


def _matrix(name, arg, T):
    """A finite 4 x 4 with last row 0 0 0 1 -> float64 numpy; None -> the identity."""
    if T is None:
        return np.eye(4)
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    T = np.array(T, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all() or T[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise ValueError('%s: %s must be a finite 4 x 4 matrix with last row 0 0 0 1' % (name, arg))
    return T


def _new_state(T, max_iteration, device):
    n = int(_lib.load().msdf_icp_state_bytes(max_iteration))
    if n < 0:
        raise ValueError('icp: max_iteration %d out of range' % max_iteration)
    host = np.zeros(n // 8, dtype=np.float64)
    host[:16] = T.reshape(-1)
    return ma.upload(host, device)


def _read_state(state):
    """-> (T [4,4], evaluations, log [evaluations, 3]) of a finished run: one host copy."""
    host = state.cpu().numpy()
    iteration = int(host[_T_DOUBLES:_T_DOUBLES + 1].view(np.int32)[0])
    return host[:16].reshape(4, 4).copy(), iteration + 1, host[_T_DOUBLES + 1:].reshape(-1, 3)[:iteration + 1].copy()


def _pivots(name, src, tgt):
    """The centres of the two bounding boxes as one fp64 device tensor [6], and the target's bounds; ValueError for
    non-finite coordinates."""
    _, s_lo, s_hi = ma.finite_bounds(name, src)
    _, t_lo, t_hi = ma.finite_bounds(name, tgt)
    return torch.cat([(s_lo + s_hi) / 2, (t_lo + t_hi) / 2]).to(src.device), t_lo, t_hi


def _run(name, src, tgt, md, T, max_iteration, relative_fitness, relative_rmse, check_every):
    """The iterations.  src, tgt: checked, contiguous, non-empty, on one device -> (state, y, idx int32) after the last
    evaluation."""
    dev = src.device
    N, M = src.shape[0], tgt.shape[0]
    pivots, t_lo, t_hi = _pivots(name, src, tgt)
    with torch.cuda.device(dev):
        grid = PointGrid(tgt, t_lo, t_hi, md / GRID_CELL_FRACTION)           # once per alignment
        state = _new_state(T, max_iteration, dev)
        flags = state.view(torch.int32)
        ws = ma.workspace(name, 'msdf_icp_workspace_bytes', N, device=dev)
        y = torch.empty(N, 3, dtype=torch.float32, device=dev)
        idx = None
        for k in range(max_iteration + 1):
            ma.call('msdf_icp_transform', src, N, state, y)
            idx = grid.query(y, md, int32=True)[1]
            ma.call('msdf_icp_accumulate', src, y, tgt, idx, N, M, pivots, state, ws)
            ma.call('msdf_icp_solve', ws, N, pivots, max_iteration, relative_fitness, relative_rmse, state)
            if (k + 1) % check_every == 0 and k < max_iteration and int(flags[_FLAG_WORD]):
                break
    return state, y, idx


def icp(source, target, max_dist=0.1, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
        check_every=5, return_log=False):
    """Point-to-point ICP of ``source`` [N,3] onto ``target`` [M,3] (float32 CUDA tensors, or numpy arrays, which are
    uploaded): -> ``(transformation [4,4] float64 numpy, fitness, inlier_rmse)``, open3d's ``registration_icp`` with
    ``TransformationEstimationPointToPoint()``; the defaults are open3d's criteria and the reference's ``max_dist`` and
    identity ``init``.

    Evaluation k moves the source by the current T (fp64 arithmetic, rounded once to fp32), pairs every moved point
    with its nearest target point if that is within ``max_dist`` (bit for bit ``nearest_neighbors_within``), and forms
    fitness = pairs / N and the rmse over the pairs.  It stops when both changed by less than their criteria since the
    evaluation before, or after ``max_iteration`` updates; otherwise the next T is the best rigid map (always a proper
    rotation) of the ORIGINAL paired source points onto their partners.  No pair at all leaves T as it is.
    ``max_iteration=0`` evaluates ``init`` only.  ``check_every``: after how many iterations the host looks at the
    device's ``done`` flag; it changes the speed only.  ``return_log``: also ``(log [evaluations, 3] of (fitness, rmse,
    pairs), evaluations)``.  ValueError for an empty cloud, non-finite coordinates, a ``max_dist`` that is not positive
    and finite, an ``init`` that is not a finite 4 x 4 with last row 0 0 0 1, a negative ``max_iteration`` and a
    ``check_every`` below 1.  See the module docstring for the differences from open3d; parity with it is unverified."""
    name = 'icp'
    dev = ma.device_of(source, target)
    src = _cloud(name, 'source', source, dev)
    tgt = _cloud(name, 'target', target, src.device)
    ma.same_device(name, source=src, target=tgt)
    md = ma.search_distance(name, max_dist)
    T = _matrix(name, 'init', init)
    max_iteration, check_every = int(max_iteration), int(check_every)
    if max_iteration < 0:
        raise ValueError('%s: max_iteration must not be negative, got %d' % (name, max_iteration))
    if check_every < 1:
        raise ValueError('%s: check_every must be at least 1, got %d' % (name, check_every))
    state = _run(name, src, tgt, md, T, max_iteration, float(relative_fitness), float(relative_rmse), check_every)[0]
    T, evaluations, log = _read_state(state)
    out = (T, float(log[-1, 0]), float(log[-1, 1]))
    return out + (log, evaluations) if return_log else out


def evaluate_registration(source, target, max_dist, transformation=None):
    """open3d's ``evaluate_registration``: -> ``(fitness, inlier_rmse, idx [N] int64)`` of ``transformation`` (default
    the identity): evaluation 0 of ``icp``, with ``idx[i]`` the target point paired with source point i, -1 for none."""
    name = 'evaluate_registration'
    dev = ma.device_of(source, target)
    src = _cloud(name, 'source', source, dev)
    tgt = _cloud(name, 'target', target, src.device)
    ma.same_device(name, source=src, target=tgt)
    md = ma.search_distance(name, max_dist)
    state, _, idx = _run(name, src, tgt, md, _matrix(name, 'transformation', transformation), 0, 0.0, 0.0, 1)
    log = _read_state(state)[2]
    return float(log[0, 0]), float(log[0, 1]), idx.long()


def kabsch(src, dst):
    """The rigid 4 x 4 (float64 numpy) that best maps ``src[i]`` onto ``dst[i]`` in the least-squares sense, always with
    a proper rotation: one update of ``icp`` with every point paired with its namesake.  src, dst: [N,3] of one
    length."""
    name = 'kabsch'
    dev = ma.device_of(src, dst)
    a = _cloud(name, 'src', src, dev)
    b = _cloud(name, 'dst', dst, a.device)
    ma.same_device(name, src=a, dst=b)
    if a.shape[0] != b.shape[0]:
        raise ValueError('%s: %d points against %d' % (name, a.shape[0], b.shape[0]))
    n = a.shape[0]
    pivots = _pivots(name, a, b)[0]
    with torch.cuda.device(a.device):
        state = _new_state(np.eye(4), 1, a.device)
        ws = ma.workspace(name, 'msdf_icp_workspace_bytes', n, device=a.device)
        idx = torch.arange(n, dtype=torch.int32, device=a.device)
        ma.call('msdf_icp_accumulate', a, a, b, idx, n, n, pivots, state, ws)
        ma.call('msdf_icp_solve', ws, n, pivots, 1, 0.0, 0.0, state)
    return _read_state(state)[0]


def transform_points(points, T):
    """``points`` [N,3] moved by the 4 x 4 ``T`` as ``icp`` moves them: per row fl32(((r0 x + r1 y) + r2 z) + t), fp64
    arithmetic on the fp32 coordinates -> float32 CUDA [N,3]."""
    name = 'transform_points'
    pts = ma.cloud_tensor(name, 'points', points).contiguous()
    T = _matrix(name, 'T', T)
    out = torch.empty_like(pts)
    if pts.shape[0] > 0:
        with torch.cuda.device(pts.device):
            ma.call('msdf_icp_transform', pts, pts.shape[0], _new_state(T, 0, pts.device), out)
    return out


def align_mesh(rec, gt, max_dist=0.1):
    """``get_align_transformation`` (eval_recon.py:51-65) and what ``calc_3d_metric`` does with it: ICP of the vertices
    of ``rec`` onto the vertices of ``gt`` from the identity -> ``((vertices float32 [V,3], faces int32 [F,3]), T)``,
    the moved ``rec`` as CUDA tensors and the 4 x 4.  ``rec``, ``gt``: Mesh objects or (vertices, faces) pairs."""
    name = 'align_mesh'
    rv, rf, _ = ma.mesh_tensors(name, rec, ma.device_of(*ma.mesh_parts(gt)))
    gv = ma.mesh_tensors(name, gt, rv.device)[0]
    T = icp(rv, gv, max_dist)[0]
    return (transform_points(rv, T), rf), T
