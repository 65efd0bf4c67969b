"""GPU tests of the grid-bounded nearest-neighbour search (csrc/gridnn.hip, mesh_eval.nearest_neighbors_within): on
every input the result is ``torch.equal`` to the brute-force ``nearest_neighbors`` where that distance is at most
``max_dist`` and (+inf, -1) elsewhere, whatever the grid.  The inputs are constructed in tests/gridnn_numpy.py, whose
restatement of the method is compared with the kernel on the small ones as well."""
import os
import sys

import numpy as np
import pytest
import torch

import gridnn_numpy as gn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SMALL = gn.small_cases()


def _me():
    from monosdf_amd.utils import mesh_eval
    return mesh_eval


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _expected(ref, qry, max_dist):
    """From the brute-force kernel: (d, i) where d <= float32(max_dist), (+inf, -1) elsewhere."""
    d, i = _me().nearest_neighbors(ref, qry)
    keep = d <= torch.tensor(max_dist, dtype=torch.float32, device=d.device)
    return torch.where(keep, d, torch.full_like(d, float('inf'))), torch.where(keep, i, torch.full_like(i, -1))


def _check(ref, qry, max_dist, want=None, **grid):
    want = _expected(ref, qry, max_dist) if want is None else want
    dist, idx = _me().nearest_neighbors_within(ref, qry, max_dist, **grid)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == idx.shape == (qry.shape[0],)
    assert torch.equal(idx, want[1]), grid
    assert torch.equal(dist, want[0]), grid
    return want


@pytest.mark.parametrize('name', sorted(SMALL))
def test_small_inputs(name):
    """ring order, last ring, 3-4-5, lattice ties (with and without duplicated points), outside the box."""
    ref, qry, max_dist, cells = SMALL[name]
    r, q = _cuda(ref), _cuda(qry)
    want = _expected(r, q, max_dist)
    host = gn.within(*gn.brute(ref, qry), max_dist)            # the numpy brute force is the kernel's, bit for bit
    assert np.array_equal(want[0].cpu().numpy().view(np.uint32), host[0].view(np.uint32))
    assert np.array_equal(want[1].cpu().numpy(), host[1])
    for cell in cells:
        _check(r, q, max_dist, want, cell=cell)
    found = (want[1] >= 0).tolist()
    if name == 'ring order':
        assert want[1].tolist() == [1]
    if name == 'last ring':
        assert want[1].tolist() == [1] and 4.98 < want[0].item() < 5.0
    if name == '3-4-5':
        assert found == gn.THREE_FOUR_FIVE_REPORTED and want[0][:4].tolist() == [5.0] * 4
    if name == 'outside the box':
        assert found == [False, True, True, True, False]
    if name.startswith('lattice ties'):
        assert all(found)


def test_one_crowded_cell():
    ref, qry, max_dist, cells = gn.crowded_cell()
    want = _check(_cuda(ref), _cuda(qry), max_dist, cell=cells[0])
    idx = want[1].cpu().numpy()
    assert (idx[:300] >= 0).all() and (idx[300:500] == 5000).any() and (idx[500:] == -1).all()
    _check(_cuda(ref), _cuda(qry), max_dist, want)


def test_sizes_off_the_lane_grid():
    found = []
    for (R, Q), (ref, qry) in gn.off_lane_sizes().items():
        want = _check(_cuda(ref), _cuda(qry), 0.3)
        found.append(float((want[1] >= 0).float().mean()))
    assert min(found) < 0.5 and max(found) > 0.5


@pytest.fixture(scope='module')
def shells():
    inner, outer, max_dist = gn.sphere_shells()
    return _cuda(inner), _cuda(outer), max_dist


@pytest.mark.parametrize('shift', [0.0, 1000.0])
def test_two_sphere_shells(shift):
    inner, outer, max_dist = gn.sphere_shells(shift)
    inner, outer = _cuda(inner), _cuda(outer)
    want = _check(outer, inner, max_dist)
    none = float((want[1] < 0).float().mean())
    assert 0.1 < none < 0.5                                    # the inner points over the part that was cut away
    assert bool((_check(inner, outer, max_dist)[1] >= 0).all())


def test_result_does_not_depend_on_the_grid(shells):
    inner, outer, max_dist = shells
    want = _expected(outer, inner, max_dist)
    for cell in (None, max_dist / 64, max_dist, 4 * max_dist):
        for max_cells in (None, 8, 1):
            _check(outer, inner, max_dist, want, cell=cell, max_cells=max_cells)
    a = _me().nearest_neighbors_within(outer, inner, max_dist)
    b = _me().nearest_neighbors_within(outer, inner, max_dist)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_one_grid_answers_many_query_sets():
    """A PointGrid built once over 300 jittered lattice points and queried three times (65, 1 and 130 points: off the
    64-lane grid on both sides) gives each time, bit for bit, what a fresh nearest_neighbors_within gives and what the
    numpy brute force gives; queries up to 2 outside the lattice's box have no neighbour within max_dist = 1."""
    from monosdf_amd.utils import mesh_args as ma
    from monosdf_amd.utils.point_grid import GRID_CELL_FRACTION, PointGrid
    rng = np.random.default_rng(21)
    reference = (gn.lattice(rng)[:300] + rng.uniform(-0.2, 0.2, (300, 3))).astype(np.float32)
    max_dist = 1.0
    queries = [rng.uniform(-2.0, 8.0, (n, 3)).astype(np.float32) for n in (65, 1, 130)]
    queries[1][0] = (3.1, 2.9, 3.2)                            # inside the lattice: it has a neighbour
    ref = _cuda(reference)
    _, lo, hi = ma.finite_bounds('test', ref)
    grid = PointGrid(ref, lo, hi, max_dist / GRID_CELL_FRACTION)
    assert grid.n_ref == 300 and len(grid.grid) == 7
    records, starts = grid.records.clone(), grid.starts.clone()
    found = []
    for qry in queries:
        q = _cuda(qry)
        dist, idx = grid.query(q, max_dist)
        assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == idx.shape == (len(qry),)
        fresh = _me().nearest_neighbors_within(ref, q, max_dist)
        assert torch.equal(idx, fresh[1]) and torch.equal(dist, fresh[0])
        want = gn.within(*gn.brute(reference, qry), max_dist)
        assert np.array_equal(idx.cpu().numpy(), want[1])
        assert np.array_equal(dist.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        dist32, idx32 = grid.query(q, max_dist, int32=True)
        assert idx32.dtype == torch.int32 and torch.equal(idx32.long(), idx) and torch.equal(dist32, dist)
        found.append((want[1] >= 0).tolist())
    assert found[1] == [True] and not all(found[0]) and any(found[0]) and not all(found[2]) and any(found[2])
    assert torch.equal(grid.records, records) and torch.equal(grid.starts, starts)     # a query leaves the grid alone


def test_refusals(shells):
    inner, outer, _ = shells
    within = _me().nearest_neighbors_within
    with pytest.raises(ValueError, match='empty'):
        within(inner[:0], outer, 1.0)
    d, i = within(inner, outer[:0], 1.0)
    assert d.shape == i.shape == (0,) and d.dtype == torch.float32 and i.dtype == torch.int64 and d.is_cuda
    for bad in (inner, outer):
        broken = bad[:50].clone()
        broken[7, 1] = float('nan')
        with pytest.raises(ValueError, match='non-finite'):
            within(broken, outer[:10], 1.0)
        with pytest.raises(ValueError, match='non-finite'):
            within(inner[:10], broken, 1.0)
    broken[7, 1] = float('inf')
    with pytest.raises(ValueError, match='non-finite'):
        within(broken, outer[:10], 1.0)
    for max_dist in (0, 0.0, -1.0, float('nan'), float('inf'), 1e39, 'far'):
        with pytest.raises(ValueError, match='max_dist'):
            within(inner, outer, max_dist)
    for cell in (0, -0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='cell'):
            within(inner, outer, 1.0, cell=cell)
    for max_cells in (0, -4, float('nan')):
        with pytest.raises(ValueError, match='max_cells'):
            within(inner, outer, 1.0, max_cells=max_cells)
    with pytest.raises(TypeError, match='cpu'):
        within(inner.cpu(), outer, 1.0)
    with pytest.raises(TypeError, match='cpu'):
        within(inner, outer.cpu(), 1.0)
    with pytest.raises(TypeError, match='float32'):
        within(inner.double(), outer, 1.0)
    with pytest.raises(ValueError, match=r'\[N, 3\]'):
        within(inner[:, :2], outer, 1.0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='cuda:1'):
            within(inner, outer.to('cuda:1'), 1.0)


# ---------------------------------------------------------------- the protocol

def _icosphere(radius, subdivisions):
    t = (1 + 5 ** 0.5) / 2
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
             (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
             (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, float) / np.linalg.norm(p) for p in verts]
    for _ in range(subdivisions):
        middle_of, split = {}, []
        for tri in faces:
            mids = []
            for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                key = (min(a, b), max(a, b))
                if key not in middle_of:
                    m = verts[a] + verts[b]
                    verts.append(m / np.linalg.norm(m))
                    middle_of[key] = len(verts) - 1
                mids.append(middle_of[key])
            ab, bc, ca = mids
            split += [(tri[0], ab, ca), (tri[1], bc, ab), (tri[2], ca, bc), (ab, bc, ca)]
        faces = split
    return (np.array(verts) * radius).astype(np.float32), np.array(faces, np.int64)


def test_protocol_with_grid_search_gives_the_same_metrics():
    """The scene of the protocol tests: an icosphere of radius 30 against an stl cloud on radius 30.5, the box of ``bb``
    and ``patch`` cutting the sphere, so that stl points over the part cut away have no neighbour within max_dist."""
    from monosdf_amd.utils import mesh_dtu as md
    from monosdf_amd.utils.mesh import Mesh
    rng = np.random.default_rng(5)
    verts, faces = _icosphere(30.0, 2)
    d = rng.normal(size=(4000, 3))
    stl = (30.5 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    obs = np.zeros((21, 21, 21), np.uint8)
    obs[:11] = 1
    args = dict(obs_mask=obs, bb=np.array([[-20, -20, -20], [20, 20, 20]], np.float32), res=2.0,
                plane=np.array([0.0, 0.0, 1.0, 0.0]), density=2.0, patch=5, max_dist=3)
    brute, bc = md.evaluate_dtu(Mesh(verts, faces), stl, seed=3, return_clouds=True, **args)
    grid, gc = md.evaluate_dtu(Mesh(verts, faces), stl, seed=3, return_clouds=True, search='grid', **args)
    assert grid == brute and all(isinstance(v, float) and v == v for v in grid.values())
    assert bool((bc['dist_s2d'] >= 3).any()) and bool((bc['dist_s2d'] < 3).any())
    for k in ('dist_d2s', 'dist_s2d'):
        near = bc[k] <= 3
        assert bc[k].shape == gc[k].shape and torch.equal(gc[k][near], bc[k][near]), k
        assert bool(torch.isinf(gc[k][~near]).all()) and bool((gc[k][~near] > 0).all()), k
        assert torch.equal(torch.isinf(gc[k]), ~near), k
    for k in ('data_in', 'data_in_obs', 'stl_above', 'keep'):
        assert torch.equal(bc[k], gc[k]), k
    with pytest.raises(ValueError, match='max_dist'):
        md.evaluate_dtu(Mesh(verts, faces), stl, seed=3, search='grid', **dict(args, max_dist=0))
