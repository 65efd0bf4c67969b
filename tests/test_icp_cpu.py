"""CPU tests of the point-to-point ICP: the sizes and the host-side refusals of the msdf_icp_* entry points, the float64
restatement (tests/icp_numpy.py) on inputs whose answer is known, the five mistakes it can be made to commit, and the
conditions on the constructed inputs that the GPU tests (test_gpu_icp.py) rely on."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import gridnn_numpy as gn
import icp_numpy as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ('subset', 'noisy', 'tiny')


# ---------------------------------------------------------------- the library (header and table: test_abi_cpu.py)

def test_rotation_solver_has_one_definition():
    csrc = os.path.join(ROOT, 'monosdf_amd', 'csrc')
    defined = [f for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h')) and
               re.search(r'^(static )?__device__ void \w*solve_rotation\(', open(os.path.join(csrc, f)).read(), flags=re.M)]
    assert defined == ['rotation_solve.h']
    for user in ('highres.hip', 'icp.hip'):
        text = open(os.path.join(csrc, user)).read()
        assert '#include "rotation_solve.h"' in text and 'solve_rotation(' in text
    makefile = open(os.path.join(csrc, 'Makefile')).read()
    for obj in ('highres', 'icp'):
        assert re.search(r'^%s\.o: .*rotation_solve\.h' % obj, makefile, flags=re.M)


def test_library_exports_the_icp_entries():
    from monosdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    lib = _lib.load()
    big = 2 ** 31 - 1
    # the state: 18 fp64, two int32 and three fp64 per evaluation; the partials: 17 fp64 per slice of 2048 points
    assert lib.msdf_icp_state_bytes(0) == 152 + 24 and lib.msdf_icp_state_bytes(30) == 152 + 31 * 24
    assert lib.msdf_icp_workspace_bytes(0) == 256 and lib.msdf_icp_workspace_bytes(2048) == 256
    assert lib.msdf_icp_workspace_bytes(2049) == 2 * 17 * 8
    assert lib.msdf_icp_workspace_bytes(2 * 10 ** 6) == 977 * 17 * 8
    for it in (-1, 2 ** 20 + 1, 2 ** 40):
        assert lib.msdf_icp_state_bytes(it) == -1, it
    # refused on the host, before anything is launched: sizes outside [0, 2^31), null pointers with sizes > 0
    fake = ctypes.c_void_p(256)                            # never dereferenced on the host
    for n in (-1, big, 2 ** 40):
        assert lib.msdf_icp_workspace_bytes(n) == -1, n
        assert lib.msdf_icp_transform(fake, n, fake, fake, None) == 1, n
        assert lib.msdf_icp_accumulate(fake, fake, fake, fake, n, 1, fake, fake, fake, None) == 1, n
        assert lib.msdf_icp_accumulate(fake, fake, fake, fake, 1, n, fake, fake, fake, None) == 1, n
        assert lib.msdf_icp_solve(fake, n, fake, 30, 1e-6, 1e-6, fake, None) == 1, n
    assert lib.msdf_icp_transform(None, 5, fake, None, None) == 1
    assert lib.msdf_icp_transform(fake, 5, None, fake, None) == 1
    assert lib.msdf_icp_transform(None, 0, fake, None, None) == 0                  # nothing to do, nothing launched
    assert lib.msdf_icp_accumulate(None, None, None, None, 5, 5, fake, fake, None, None) == 1
    assert lib.msdf_icp_accumulate(fake, fake, fake, fake, 5, 5, None, fake, fake, None) == 1
    assert lib.msdf_icp_accumulate(fake, fake, fake, fake, 5, 5, fake, None, fake, None) == 1
    assert lib.msdf_icp_accumulate(None, None, None, None, 0, 5, fake, fake, None, None) == 0
    assert lib.msdf_icp_solve(None, 5, fake, 30, 1e-6, 1e-6, fake, None) == 1
    assert lib.msdf_icp_solve(fake, 5, None, 30, 1e-6, 1e-6, fake, None) == 1
    assert lib.msdf_icp_solve(fake, 5, fake, 30, 1e-6, 1e-6, None, None) == 1
    for it in (-1, 2 ** 20 + 1):
        assert lib.msdf_icp_solve(fake, 5, fake, it, 1e-6, 1e-6, fake, None) == 1, it


def test_python_surface_without_a_gpu():
    import inspect
    from monosdf_amd.utils import mesh_align as al, mesh_eval as me
    sig = inspect.signature(al.icp).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [
        ('max_dist', 0.1), ('init', None), ('max_iteration', 30), ('relative_fitness', 1e-6), ('relative_rmse', 1e-6),
        ('check_every', 5), ('return_log', False)]
    assert inspect.signature(me.evaluate_replica).parameters['align'].default is False
    for fn in (al.evaluate_registration, al.kabsch, al.transform_points, al.align_mesh):
        assert callable(fn)
    with pytest.raises(TypeError, match='^icp: source must be a CUDA tensor'):
        al.icp(__import__('torch').zeros(4, 3), np.zeros((4, 3), np.float32))


# ---------------------------------------------------------------- the restatement

def test_restated_search_is_the_brute_force_search():
    source, target, _ = inp.case('tiny')
    idx = inp.correspondences(source, target, 0.05)
    dist, want = gn.within(*gn.brute(target, source), 0.05)
    assert np.array_equal(idx, want) and (idx >= 0).any() and (idx < 0).any()
    assert np.array_equal(idx >= 0, dist <= np.float32(0.05))


def test_restated_transform_rounds_once():
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(50, 3)).astype(np.float32)
    T = inp.rigid((0.3, -1.0, 0.7), 33.0, (0.1, 0.2, -0.3))
    got = inp.transform(pts, T)
    exact = pts.astype(np.longdouble) @ T[:3, :3].astype(np.longdouble).T + T[:3, 3].astype(np.longdouble)
    assert got.dtype == np.float32
    assert (np.abs(got.astype(np.longdouble) - exact) <= np.spacing(np.abs(got)) * 0.5 * (1 + 1e-6)).all()


@pytest.mark.parametrize('name', ('subset', 'tiny'))
def test_restatement_recovers_a_known_rigid_motion(name):
    """The source is a subset of the target moved by a known motion and rounded to fp32 (coordinates below 1: a
    rounding of at most 3e-8 per coordinate), so T must be the motion's inverse to 1e-6 in every entry."""
    source, target, motion = inp.case(name)
    assert np.abs(source).max() < 1.0 and np.abs(target).max() < 1.0
    T, fitness, rmse, log, _ = inp.solved(name)
    err = np.abs(T - np.linalg.inv(motion)).max()
    print(name, 'evaluations', len(log), 'largest error of T', err, 'rmse', rmse)
    assert err <= 1e-6
    assert fitness == 1.0 and rmse < 1e-7 and 2 < len(log) <= 31
    R = T[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0


def test_kabsch_is_exact_on_a_mirrored_pair():
    """The best orthogonal map of the pair is the reflection; the best ROTATION is what svd with the sign rule gives,
    and it is better than every rotation near it."""
    src, dst = inp.mirrored_pair()
    T = inp.kabsch(src, dst)
    R = T[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14

    def cost(M):
        return ((src.astype(np.float64) @ M[:3, :3].T + M[:3, 3] - dst) ** 2).sum()
    rng = np.random.default_rng(2)
    for _ in range(20):
        near = inp.rigid(rng.normal(size=3), 0.5, rng.normal(size=3) * 1e-3) @ T
        assert cost(T) < cost(near)
    # without the sign rule: the reflection, which no rigid motion is
    cs, ct = inp.pivots(src, dst)
    s = inp.sums(src, src, dst, np.arange(len(src)), cs, ct)
    assert np.linalg.det(inp.update(s, cs, ct, np.eye(4), sign_rule=False)[:3, :3]) < 0


def test_kabsch_is_exact_on_a_coplanar_cloud_and_leaves_t_alone_for_nothing():
    src, dst, want = inp.coplanar_pair()
    assert (src[:, 2] == 0.25).all()
    T = inp.kabsch(src, dst)
    assert np.abs(T - want).max() <= 1e-14
    assert np.array_equal(inp.transform(src, T), dst)
    T0 = inp.rigid((1, 0, 0), 10.0, (1, 2, 3))
    assert inp.kabsch(np.zeros((0, 3)), np.zeros((0, 3)), T0) is T0
    assert inp.update(np.zeros(17), np.zeros(3), np.zeros(3), T0) is T0
    assert inp.measure(np.zeros(17), 5) == (0.0, 0.0)


# ---------------------------------------------------------------- five mistakes, each caught

def _with_strays(name):
    """The case with ten source points 5 units away: no correspondence for them, so fitness < 1."""
    source, target, _ = inp.case(name)
    return np.concatenate([source, source[:10] + np.float32(5.0)]), target


def test_mistake_rmse_over_n():
    source, target = _with_strays('tiny')
    good, bad = inp.icp(source, target, inp.MAX_DIST), inp.icp(source, target, inp.MAX_DIST, mistake='rmse_over_N')
    assert good[1] == bad[1] == 64 / 74
    assert bad[3][0, 1] == pytest.approx(good[3][0, 1] * np.sqrt(64 / 74), rel=1e-12)
    assert abs(bad[3][0, 1] - good[3][0, 1]) > 1e-3


def test_mistake_no_sign_rule():
    src, dst = inp.mirrored_pair()
    good = inp.icp(src, dst, 10.0, max_iteration=1)
    bad = inp.icp(src, dst, 10.0, max_iteration=1, mistake='no_sign_rule')
    assert np.linalg.det(good[0][:3, :3]) > 0 > np.linalg.det(bad[0][:3, :3])


def test_mistake_strict_max_dist():
    source, target, max_dist = inp.tie_pair()
    d = gn.brute(target, source)[0]
    assert d[0] == np.float32(max_dist) and (d[1:] == 0).all()
    good = inp.icp(source, target, max_dist, max_iteration=0)
    bad = inp.icp(source, target, max_dist, max_iteration=0, mistake='strict_max_dist')
    assert good[3][0].tolist() == [1.0, 0.125, 4.0] and bad[3][0].tolist() == [0.75, 0.0, 3.0]


@pytest.mark.parametrize('name', CASES)
def test_mistake_compose(name):
    """Composing the updates on a cloud rounded to fp32 at every step drifts: T ends further from the restatement than
    the 1e-9 the kernels are held to."""
    source, target, _ = inp.case(name)
    bad = inp.icp(source, target, inp.MAX_DIST, mistake='compose')
    gap = np.abs(bad[0] - inp.solved(name)[0]).max()
    print(name, 'composed T differs by', gap)
    assert gap > 1e-9


@pytest.mark.parametrize('name', CASES)
def test_mistake_fitness_only(name):
    source, target, _ = inp.case(name)
    bad = inp.icp(source, target, inp.MAX_DIST, mistake='fitness_only')
    good = inp.solved(name)
    assert len(bad[3]) == 2 < len(good[3])
    assert np.abs(bad[0] - good[0]).max() > 1e-3


# ---------------------------------------------------------------- conditions the GPU tests rely on

@pytest.mark.parametrize('name', CASES)
def test_whole_icp_cases_are_well_separated(name):
    """For every evaluation of the case: no source point's nearest and second-nearest target distances are within 1e-5
    relative (100 times the rounding of an fp32 distance), none's nearest distance is within 1e-5 relative of max_dist,
    and no |delta rmse| lies within 1 % of relative_rmse while |delta fitness| is below its criterion: a last-bit
    difference in T cannot change a correspondence, a count or the number of evaluations."""
    source, target, _ = inp.case(name)
    _, _, _, log, trace = inp.solved(name)
    tgt = target.astype(np.float64)
    gaps, margins = [], []
    for moved, idx in trace:
        d = np.linalg.norm(moved.astype(np.float64)[:, None] - tgt[None], axis=2)
        d.sort(axis=1)
        gaps.append(((d[:, 1] - d[:, 0]) / d[:, 1]).min())
        margins.append((np.abs(d[:, 0] - inp.MAX_DIST) / inp.MAX_DIST).min())
    print(name, 'evaluations', len(log), 'smallest gap', min(gaps), 'smallest margin', min(margins))
    assert min(gaps) > 1e-5 and min(margins) > 1e-5
    d_fit, d_rmse = np.abs(np.diff(log[:, 0])), np.abs(np.diff(log[:, 1]))
    close = (d_fit < 1e-6) & (np.abs(d_rmse - 1e-6) <= 1e-8)
    assert not close.any()
    assert d_fit[-1] < 1e-6 and d_rmse[-1] < 1e-6 and len(log) < 31      # stopped by the criteria, not by the count


def test_far_source_has_no_correspondence():
    source, target, _ = inp.case('tiny')
    T, fitness, rmse, log, _ = inp.icp(source + np.float32(10.0), target, inp.MAX_DIST)
    assert np.array_equal(T, np.eye(4)) and fitness == 0.0 and rmse == 0.0 and log.tolist() == [[0, 0, 0], [0, 0, 0]]


def test_mesh_pair_is_recovered_by_the_restatement():
    """The callers' test scores a mesh that ICP has moved back: on the restatement the motion is found to 1e-6, every
    vertex is paired with its own original, and the well-separatedness above holds at the last evaluation."""
    rec, gt, faces, motion = inp.mesh_pair()
    assert np.abs(rec).max() < 1.0 and faces.max() == len(gt) - 1 == 799
    T, fitness, rmse, log, trace = inp.icp(rec, gt, inp.MAX_DIST)
    print('mesh pair: evaluations', len(log), 'error of T', np.abs(T - np.linalg.inv(motion)).max(), 'rmse', rmse)
    assert np.abs(T - np.linalg.inv(motion)).max() <= 1e-6 and fitness == 1.0 and len(log) < 31
    assert np.array_equal(trace[-1][1], np.arange(len(gt)))
