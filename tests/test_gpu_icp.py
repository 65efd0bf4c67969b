"""GPU tests of utils/mesh_align.py and the msdf_icp_* kernels (csrc/icp.hip) against the float64 restatement
(tests/icp_numpy.py): the transform exactly, the 17 sums exactly on integer inputs and within the summation bound
otherwise, the solve, whole ICP runs row by row, the independence of the result from the host's schedule, and the
callers.  The conditions on the constructed inputs that the exact comparisons rely on are proved in test_icp_cpu.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import gridnn_numpy as gn
import icp_numpy as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

THREADS, LANE, WAVE, SLICE = 256, 8, 8 * 64, 2048         # ICP_THREADS, ICP_PPL, points per wave, ICP_SLICE (icp.hip)
SIZES_T = (1, 63, 64, 65, THREADS + 3)
SIZES_A = (1, LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3)
CASES = ('subset', 'noisy', 'tiny')


def _al():
    from monosdf_amd.utils import mesh_align
    return mesh_align


def _call(entry, *args):
    from monosdf_amd.utils import mesh_args
    mesh_args.call(entry, *args)


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _state(T=None, iteration=0, previous=(0.0, 0.0), done=0, max_iteration=30):
    from monosdf_amd import _lib
    host = np.zeros(_lib.load().msdf_icp_state_bytes(max_iteration) // 8)
    host[:16] = np.eye(4).reshape(-1) if T is None else np.asarray(T, np.float64).reshape(-1)
    host[16:18] = previous
    host[18:19].view(np.int32)[:] = (iteration, done)
    return _cuda(host)


def _read(state):
    host = state.cpu().numpy()
    iteration, done = host[18:19].view(np.int32).tolist()
    return {'T': host[:16].reshape(4, 4), 'previous': host[16:18].tolist(), 'iteration': iteration, 'done': done,
            'log': host[19:].reshape(-1, 3)}


IRRATIONAL = inp.rigid((1.0, math.sqrt(2.0), math.pi), 37.0, (math.sqrt(3.0), -math.e, 0.1))


# ---------------------------------------------------------------- msdf_icp_transform

@pytest.mark.parametrize('n', SIZES_T)
def test_transform_equals_the_fp64_expression(n):
    pts = np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32) * 3
    got = _al().transform_points(_cuda(pts), IRRATIONAL)
    assert got.dtype == torch.float32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), inp.transform(pts, IRRATIONAL))
    assert np.array_equal(_al().transform_points(pts, IRRATIONAL).cpu().numpy(), got.cpu().numpy())   # uploaded
    # a finished state: the launch changes nothing
    out = torch.full((n, 3), 7.0, device='cuda')
    _call('msdf_icp_transform', _cuda(pts), n, _state(IRRATIONAL, done=1), out)
    assert (out == 7.0).all()


# ---------------------------------------------------------------- msdf_icp_accumulate

def _accumulate(source, moved, target, idx, cs, ct, done=0):
    """-> [slices, 17]: the partials; NaN where the kernel wrote nothing."""
    n = len(source)
    part = torch.full(((n + SLICE - 1) // SLICE, inp.N_SUMS), float('nan'), dtype=torch.float64, device='cuda')
    pad = torch.full((64,), float('nan'), dtype=torch.float64, device='cuda')      # the workspace's minimum size
    ws = torch.cat([part.reshape(-1), pad])
    _call('msdf_icp_accumulate', _cuda(source, np.float32), _cuda(moved, np.float32), _cuda(target, np.float32),
          _cuda(idx, np.int32), n, len(target), _cuda(np.concatenate([cs, ct])), _state(done=done), ws)
    assert torch.isnan(ws[part.numel():]).all()
    return ws[:part.numel()].reshape(part.shape).cpu().numpy()


def _edges(n):
    """First and last point of a lane, of a wave and of a slice, and the cloud's last point."""
    e = [0, LANE - 1, LANE, 2 * LANE - 1, WAVE - 1, WAVE, WAVE + LANE - 1, SLICE - 1, SLICE, SLICE + LANE - 1,
         2 * SLICE - 1, 2 * SLICE, n - 1]
    return np.array(sorted({i for i in e if i < n}))


def _restated_partials(source, moved, target, idx, cs, ct):
    return np.stack([inp.sums(source[a:a + SLICE], moved[a:a + SLICE], target, idx[a:a + SLICE], cs, ct)
                     for a in range(0, len(source), SLICE)])


@pytest.mark.parametrize('n', SIZES_A)
def test_accumulate_exact_on_integers(n):
    """Integer coordinates and pivots: every term and every partial sum is an integer far below 2^53, so the sums are
    exact in any order and must equal the restatement's."""
    rng = np.random.default_rng(n)
    m = 37
    source, moved = (rng.integers(-8, 9, (n, 3)).astype(np.float32) for _ in range(2))
    target = rng.integers(-8, 9, (m, 3)).astype(np.float32)
    cs, ct = np.array([1.0, -2.0, 3.0]), np.array([-1.0, 0.0, 2.0])
    full = rng.integers(0, m, n)
    for label in ('all', 'random', 'edges', 'all but edges', 'none'):
        idx = full.copy()
        if label == 'random':
            idx[rng.random(n) < 0.3] = -1
        elif label == 'edges':
            idx[_edges(n)] = -1
        elif label == 'all but edges':
            idx[:] = -1
            idx[_edges(n)] = full[_edges(n)]
        elif label == 'none':
            idx[:] = -1
        got = _accumulate(source, moved, target, idx, cs, ct)
        want = _restated_partials(source, moved, target, idx, cs, ct)
        assert np.array_equal(got, want), (n, label)
        if label == 'none':
            assert (got == 0).all()
    # an index past the target cloud counts as no correspondence; a finished state writes nothing
    idx = full.copy()
    idx[0] = m
    want = _restated_partials(source, moved, target, np.where(idx == m, -1, idx), cs, ct)
    assert np.array_equal(_accumulate(source, moved, target, idx, cs, ct), want)
    assert np.isnan(_accumulate(source, moved, target, full, cs, ct, done=1)).all()


@pytest.mark.parametrize('n', (1, WAVE + 1, 2 * SLICE + 3))
def test_accumulate_within_the_summation_bound_on_reals(n):
    """The terms are formed as the restatement forms them (one rounding each), so against their exact sum (math.fsum)
    a partial may be off by the rounding of its k - 1 additions: (k - 1) 2^-53 sum |term|, k the correspondences of
    the slice."""
    rng = np.random.default_rng(200 + n)
    m = 500
    source = rng.normal(size=(n, 3)).astype(np.float32)
    moved = (source + rng.normal(size=(n, 3)) * 0.01).astype(np.float32)
    target = rng.normal(size=(m, 3)).astype(np.float32)
    idx = rng.integers(0, m, n)
    idx[rng.random(n) < 0.2] = -1
    cs, ct = inp.pivots(source, target)
    got = _accumulate(source, moved, target, idx, cs, ct)
    worst = 0.0
    for s, a in enumerate(range(0, n, SLICE)):
        terms = inp.terms(source[a:a + SLICE], moved[a:a + SLICE], target, idx[a:a + SLICE], cs, ct)
        exact = np.array([math.fsum(terms[:, c]) for c in range(inp.N_SUMS)])
        bound = max(len(terms) - 1, 0) * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(got[s] - exact)
        assert (err <= bound).all(), (n, s, err, bound)
        worst = max(worst, (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0)
        assert got[s, 0] == len(terms)
    print('accumulate n', n, 'largest error / bound', worst)


# ---------------------------------------------------------------- msdf_icp_solve

def _solve(source, moved, target, idx, state, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """Accumulate and solve once on ``state`` -> (what the state holds afterwards, the restated sums, pivots)."""
    cs, ct = inp.pivots(source, target)
    n = len(source)
    pivots = _cuda(np.concatenate([cs, ct]))
    ws = torch.zeros(max(32, ((n + SLICE - 1) // SLICE) * inp.N_SUMS), dtype=torch.float64, device='cuda')
    _call('msdf_icp_accumulate', _cuda(source, np.float32), _cuda(moved, np.float32), _cuda(target, np.float32),
          _cuda(idx, np.int32), n, len(target), pivots, state, ws)
    _call('msdf_icp_solve', ws, n, pivots, max_iteration, relative_fitness, relative_rmse, state)
    return _read(state), inp.sums(source, moved, target, idx, cs, ct), (cs, ct)


def _solve_inputs(name):
    if name == 'generic':
        source, target, _ = inp.case('subset')
        moved = inp.transform(source, IRRATIONAL @ np.linalg.inv(IRRATIONAL))      # the identity up to rounding
        return source, moved, target, inp.correspondences(moved, target, inp.MAX_DIST)
    if name == 'mirrored':
        source, target = inp.mirrored_pair()
    else:
        source, target, _ = inp.coplanar_pair()
    return source, source, target, np.arange(len(source))


@pytest.mark.parametrize('name', ('generic', 'mirrored', 'coplanar'))
def test_solve_against_the_restatement(name):
    """R and t to 1e-9 (the bar this solver is held to in test_gpu_highres.py), R orthogonal to 1e-14 and proper."""
    source, moved, target, idx = _solve_inputs(name)
    start = inp.rigid((0, 1, 0), 20.0, (5, 6, 7))
    got, s, (cs, ct) = _solve(source, moved, target, idx, _state(start))
    want = inp.update(s, cs, ct, start)
    fitness, rmse = inp.measure(s, len(source))
    R = got['T'][:3, :3]
    gap = np.abs(got['T'] - want).max()
    print('solve', name, 'largest gap of T', gap, '| R^T R - I |', np.abs(R.T @ R - np.eye(3)).max())
    assert gap <= 1e-9
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0
    assert got['T'][3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert got['iteration'] == 1 and got['done'] == 0
    assert got['log'][0, 2] == s[0] and got['log'][0, 0] == fitness and abs(got['log'][0, 1] - rmse) <= 1e-9
    assert got['previous'] == got['log'][0, :2].tolist()
    assert (got['log'][1:] == 0).all()
    if name == 'coplanar':
        assert np.abs(got['T'] - inp.coplanar_pair()[2]).max() <= 1e-14
    if name != 'generic':
        assert np.abs(_al().kabsch(_cuda(source), _cuda(target)) - inp.kabsch(source, target)).max() <= 1e-9


def test_solve_without_correspondences():
    source, target, _ = inp.case('tiny')
    start = inp.rigid((0, 1, 0), 20.0, (5, 6, 7))
    none = np.full(len(source), -1)
    state = _state(start)
    got = _solve(source, source, target, none, state)[0]
    assert np.array_equal(got['T'], start) and got['log'][0].tolist() == [0, 0, 0]
    assert got['iteration'] == 1 and got['done'] == 0 and got['previous'] == [0.0, 0.0]
    got = _solve(source, source, target, none, state)[0]                   # nothing changed since: converged
    assert np.array_equal(got['T'], start) and got['log'][1].tolist() == [0, 0, 0]
    assert got['iteration'] == 1 and got['done'] == 1
    before = state.clone()
    _solve(source, source, target, np.arange(len(source)), state)          # finished: nothing is written
    assert torch.equal(before, state)


def test_solve_sets_the_flag_on_the_right_side_of_both_criteria():
    source, moved, target, idx = _solve_inputs('generic')
    first = _solve(source, moved, target, idx, _state())[0]
    f, r = first['log'][0, :2]
    assert 0 < f <= 1 and r > 1e-4
    for d_fit, d_rmse, done in ((0.0, 0.5e-6, 1), (0.0, -0.5e-6, 1), (0.5e-6, 0.0, 1), (0.5e-6, 0.5e-6, 1),
                                (0.0, 2e-6, 0), (0.0, -2e-6, 0), (2e-6, 0.0, 0), (-2e-6, 0.0, 0), (2e-6, 2e-6, 0)):
        got = _solve(source, moved, target, idx, _state(iteration=1, previous=(f + d_fit, r + d_rmse)))[0]
        assert got['done'] == done, (d_fit, d_rmse)
        assert got['iteration'] == (1 if done else 2)
        assert np.array_equal(got['T'], np.eye(4)) == bool(done)
        assert got['log'][1].tolist() == first['log'][0].tolist() and (got['log'][0] == 0).all()
    # evaluation 0 never stops on the criteria; evaluation max_iteration always stops
    assert _solve(source, moved, target, idx, _state(previous=(f, r)))[0]['done'] == 0
    got = _solve(source, moved, target, idx, _state(iteration=3, previous=(0.0, 0.0), max_iteration=3), 3)[0]
    assert got['done'] == 1 and got['iteration'] == 3 and np.array_equal(got['T'], np.eye(4))
    # an iteration that is none of this run: the flag and nothing else
    for bad in (-1, 4):
        got = _solve(source, moved, target, idx, _state(iteration=bad, max_iteration=3), 3)[0]
        assert got['done'] == 1 and got['iteration'] == bad and (got['log'] == 0).all()


# ---------------------------------------------------------------- whole ICP

@pytest.mark.parametrize('name', CASES)
def test_icp_against_the_restatement(name):
    """Row by row: count and fitness equal, rmse to 1e-9, as many evaluations, T to 1e-9 per entry (clouds inside the
    unit box).  The restatement rounds to fp32 where the kernel does; summation order and the solver remain."""
    source, target, motion = inp.case(name)
    want_T, want_f, want_r, want_log, _ = inp.solved(name)
    T, fitness, rmse, log, evaluations = _al().icp(_cuda(source), _cuda(target), inp.MAX_DIST, return_log=True)
    assert T.dtype == np.float64 and T.shape == (4, 4) and log.shape == (evaluations, 3)
    assert evaluations == len(want_log)
    gap_r, gap_T = np.abs(log[:, 1] - want_log[:, 1]).max(), np.abs(T - want_T).max()
    print('icp', name, 'evaluations', evaluations, 'largest gap of rmse', gap_r, 'of T', gap_T,
          'from the known motion', np.abs(T - np.linalg.inv(motion)).max())
    assert np.array_equal(log[:, 2], want_log[:, 2]) and np.array_equal(log[:, 0], want_log[:, 0])
    assert gap_r <= 1e-9 and gap_T <= 1e-9
    assert fitness == log[-1, 0] == want_f and rmse == log[-1, 1] and abs(rmse - want_r) <= 1e-9
    if name != 'noisy':
        assert np.abs(T - np.linalg.inv(motion)).max() <= 1e-6


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_result_does_not_depend_on_the_schedule():
    al = _al()
    source, target, _ = inp.case('tiny')
    src, tgt = _cuda(source), _cuda(target)
    base = al.icp(src, tgt, inp.MAX_DIST, return_log=True)
    assert 2 < base[4] < 31
    for kwargs in ({'check_every': 1}, {'check_every': 30}, {}, {'max_iteration': 100, 'check_every': 7},
                   {'max_iteration': 100, 'check_every': 1000}):
        assert _same(base, al.icp(src, tgt, inp.MAX_DIST, return_log=True, **kwargs)), kwargs
    assert _same(base, al.icp(source, target, inp.MAX_DIST, return_log=True))              # uploaded
    # stopped by the count: the updates made so far
    cut = al.icp(src, tgt, inp.MAX_DIST, max_iteration=2, return_log=True)
    assert cut[4] == 3 and np.array_equal(cut[3], base[3][:3]) and not np.array_equal(cut[0], base[0])


EVALUATION = ['msdf_icp_transform', 'msdf_gnn_cells', 'msdf_gnn_query', 'msdf_icp_accumulate', 'msdf_icp_solve']


def test_icp_builds_the_grid_once_and_launches_nothing_else(monkeypatch):
    """The library calls of one icp(), in order: the target's cells and records once, then five calls per evaluation.
    The sequence was recorded with this wrapper on the commit before utils/point_grid.py existed."""
    from monosdf_amd import _lib
    entries, real = [], _lib.call

    def recording(name, *args):
        entries.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    source, target, _ = inp.case('tiny')
    evaluations = _al().icp(_cuda(source), _cuda(target), inp.MAX_DIST, max_iteration=3, check_every=1,
                            return_log=True)[4]
    assert evaluations == 4
    assert entries == ['msdf_gnn_cells', 'msdf_gnn_records'] + 4 * EVALUATION


def test_far_source_keeps_init():
    source, target, _ = inp.case('tiny')
    init = inp.rigid((1, 1, 0), 3.0, (0.01, 0.0, -0.01))
    T, fitness, rmse, log, evaluations = _al().icp(_cuda(source + np.float32(10.0)), _cuda(target), inp.MAX_DIST,
                                                   init=init, return_log=True)
    assert np.array_equal(T, init) and fitness == 0.0 and rmse == 0.0
    assert evaluations == 2 and log.tolist() == [[0, 0, 0], [0, 0, 0]]


def test_evaluate_registration_is_evaluation_zero():
    al = _al()
    source, target, _ = inp.case('subset')
    src, tgt = _cuda(source), _cuda(target)
    init = inp.rigid((0, 0, 1), -2.0, (0.0, 0.03, 0.0))
    for max_dist in (inp.MAX_DIST, 0.03):
        fitness, rmse, idx = al.evaluate_registration(src, tgt, max_dist, init)
        moved = inp.transform(source, init)
        want = inp.correspondences(moved, target, max_dist)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want)
        cs, ct = inp.pivots(source, target)
        f, r = inp.measure(inp.sums(source, moved, target, want, cs, ct), len(source))
        assert fitness == f and abs(rmse - r) <= 1e-9
        T, f0, r0, log, evaluations = al.icp(src, tgt, max_dist, init=init, max_iteration=0, return_log=True)
        assert np.array_equal(T, init) and (f0, r0) == (fitness, rmse) and evaluations == 1
    assert 0 < fitness < 1 and (want < 0).any()
    assert al.evaluate_registration(src, tgt, inp.MAX_DIST)[:2] == al.icp(src, tgt, inp.MAX_DIST, max_iteration=0)[1:]
    # the tie: a point exactly max_dist away is a correspondence
    source, target, max_dist = inp.tie_pair()
    fitness, rmse, idx = al.evaluate_registration(source, target, max_dist)
    assert (fitness, rmse, idx.tolist()) == (1.0, 0.125, [0, 1, 2, 3])


# ---------------------------------------------------------------- the callers

def test_evaluate_replica_aligns_first():
    from monosdf_amd.utils import mesh_eval as me
    al = _al()
    rec_v, gt_v, faces, motion = inp.mesh_pair()
    rec, gt = (_cuda(rec_v), _cuda(faces)), (_cuda(gt_v), _cuda(faces))
    (moved_v, moved_f), T = al.align_mesh(rec, gt)
    assert moved_v.dtype == torch.float32 and moved_v.shape == rec[0].shape and torch.equal(moved_f, rec[1])
    assert np.abs(T - np.linalg.inv(motion)).max() <= 1e-6
    assert np.array_equal(moved_v.cpu().numpy(), inp.transform(rec_v, T))
    kw = dict(n_samples=20000, seed=3)
    aligned = me.evaluate_replica(rec, gt, align=True, **kw)
    assert aligned == me.evaluate_replica((moved_v, moved_f), gt, **kw)
    straight = me.evaluate_replica(gt, gt, **kw)
    turned = me.evaluate_replica(rec, gt, **kw)
    print('chamfer: unrotated', straight['chamfer'], 'aligned', aligned['chamfer'], 'rotated', turned['chamfer'])
    assert abs(aligned['chamfer'] - straight['chamfer']) <= 0.01 * straight['chamfer']
    assert turned['chamfer'] > 1.5 * straight['chamfer']
    assert turned == me.evaluate_replica(rec, gt, align=False, **kw)
    assert me.evaluate_replica((rec_v, faces), (gt_v, faces), align=True, crop=True, **kw)['chamfer'] > 0     # uploaded


def test_nearest_neighbors_within_is_unchanged():
    from monosdf_amd.utils import mesh_eval as me
    reference, query, max_dist, cells = gn.small_cases()['lattice ties, duplicates']
    want = gn.within(*gn.brute(reference, query), max_dist)
    for cell in cells:
        dist, idx = me.nearest_neighbors_within(_cuda(reference), _cuda(query), max_dist, cell=cell)
        assert dist.dtype == torch.float32 and idx.dtype == torch.int64
        assert np.array_equal(dist.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(idx.cpu().numpy(), want[1])


def test_icp_refuses():
    al = _al()
    pts = torch.rand(10, 3, device='cuda')
    bad = pts.clone()
    bad[3, 1] = float('nan')
    with pytest.raises(ValueError, match='^icp: source is empty'):
        al.icp(pts[:0], pts)
    with pytest.raises(ValueError, match='^icp: target is empty'):
        al.icp(pts, pts[:0])
    with pytest.raises(ValueError, match='^icp: non-finite'):
        al.icp(bad, pts)
    with pytest.raises(ValueError, match='^icp: non-finite'):
        al.icp(pts, bad)
    for max_dist in (0.0, -1.0, float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='^icp: max_dist'):
            al.icp(pts, pts, max_dist)
    almost = np.eye(4)
    almost[3, 3] = 2.0
    for init in (np.eye(3), np.full((4, 4), np.nan), almost):
        with pytest.raises(ValueError, match='^icp: init'):
            al.icp(pts, pts, init=init)
    with pytest.raises(ValueError, match='^icp: max_iteration'):
        al.icp(pts, pts, max_iteration=-1)
    with pytest.raises(ValueError, match='^icp: check_every'):
        al.icp(pts, pts, check_every=0)
    with pytest.raises(ValueError, match='^evaluate_registration: transformation'):
        al.evaluate_registration(pts, pts, 0.1, np.eye(3))
    with pytest.raises(ValueError, match='^evaluate_registration: max_dist'):
        al.evaluate_registration(pts, pts, 0.0)
    with pytest.raises(ValueError, match='^kabsch: 10 points against 9'):
        al.kabsch(pts, pts[:9])
    with pytest.raises(ValueError, match='^kabsch: src is empty'):
        al.kabsch(pts[:0], pts[:0])
    with pytest.raises(ValueError, match='^transform_points: T'):
        al.transform_points(pts, almost)
    with pytest.raises(ValueError, match='^align_mesh: non-finite'):
        al.align_mesh((bad, torch.zeros(1, 3, dtype=torch.int32, device='cuda')),
                      (pts, torch.zeros(1, 3, dtype=torch.int32, device='cuda')))
    assert al.transform_points(pts[:0], np.eye(4)).shape == (0, 3)


def test_scripts_align_and_score(tmp_path, monkeypatch, capsys):
    """scripts/align_mesh.py writes the moved mesh and the transform that icp() finds; scripts/eval_mesh.py --align
    prints what evaluate_replica(align=True) returns."""
    import importlib
    import json
    from monosdf_amd.utils import mesh_eval as me
    from monosdf_amd.utils.mesh import Mesh
    rec_v, gt_v, faces, motion = inp.mesh_pair()
    src, tgt, out, saved = (str(tmp_path / n) for n in ('rec.ply', 'gt.ply', 'out.ply', 'T.txt'))
    Mesh(rec_v, faces).export(src)
    Mesh(gt_v, faces).export(tgt)
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'scripts'))
    monkeypatch.setattr(sys, 'argv', ['align_mesh.py', src, tgt, out, '--save-transform', saved])
    importlib.import_module('align_mesh').main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    T = _al().icp(rec_v, gt_v)[0]
    assert np.array_equal(np.array(line['transformation']), T) and np.array_equal(np.loadtxt(saved), T)
    assert line['fitness'] == 1.0 and line['evaluations'] == 5
    moved = me.read_ply(out)
    assert np.array_equal(moved.faces, faces) and np.abs(moved.vertices - gt_v).max() <= 1e-6
    monkeypatch.setattr(sys, 'argv', ['eval_mesh.py', src, tgt, '--protocol', 'replica', '--align', '--n-samples',
                                      '20000', '--seed', '3'])
    importlib.import_module('eval_mesh').main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == me.evaluate_replica(me.read_ply(src), me.read_ply(tgt), n_samples=20000, seed=3, align=True)
