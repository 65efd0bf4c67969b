"""CPU tests of the grid-bounded nearest-neighbour search: the numpy restatement of its method (tests/gridnn_numpy.py)
against the fp32 brute force on every constructed input of the GPU tests, the five mistakes that the small inputs
catch, the workspace size and the host-side refusals of the msdf_gnn_* entry points, and the refusals that need no
GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import gridnn_numpy as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL = gn.small_cases()
CATCHERS = ('ring order', 'last ring', 'lattice ties', 'lattice ties, duplicates', '3-4-5')


def _same(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


def _check(ref, qry, max_dist, **grid):
    want = gn.within(*gn.brute(ref, qry), max_dist)
    got = gn.grid_search(ref, qry, max_dist, **grid)
    assert got[0].dtype == np.float32 and _same(got, want), grid
    return want


def test_fused_step_rounds_once():
    """_fma32 against exact rational arithmetic, on operands picked so that the fp64 sum is inexact and rounding it
    to fp32 afterwards would round twice."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.uniform(1, 2, 2000).astype(np.float32)
    c = (rng.uniform(1, 2, 2000) * 2.0 ** rng.integers(-40, 30, 2000)).astype(np.float32)
    # a * a + c with c a half ulp of the sum's fp32 result away from a tie, nudged by a far smaller term
    a[:3] = np.float32(1 + 2.0 ** -12)
    c[:3] = np.float32([2.0 ** -60, 2.0 ** -24 + 2.0 ** -47, 2.0 ** -70])
    got = gn._fma32(a, a, c)
    for x, z, g in zip(a, c, got):
        exact = Fraction(float(x)) * Fraction(float(x)) + Fraction(float(z))
        lo = np.float32(float(exact))                           # Python rounds a Fraction to fp64 once ...
        near = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        err = [abs(Fraction(float(v)) - exact) for v in near]   # ... so choose among the fp32 neighbours exactly
        assert abs(Fraction(float(g)) - exact) == min(err), (x, z, g)


def test_brute_force_is_the_plain_minimum():
    """``brute`` (which evaluates the fused form only near each query's minimum) equals the minimum of the fused form
    over every pair, ties to the smallest index."""
    rng = np.random.default_rng(1)
    ref = np.round(rng.uniform(0, 3, (400, 3)) * 4).astype(np.float32) / 4          # a coarse lattice: many ties
    qry = rng.uniform(-1, 4, (150, 3)).astype(np.float32)
    d2 = gn.d2_fp32(qry[:, None, :], ref[None, :, :])
    idx = d2.argmin(axis=1)
    dist, got = gn.brute(ref, qry)
    assert np.array_equal(got, idx) and np.array_equal(dist, np.sqrt(d2[np.arange(len(qry)), idx]))
    assert (np.sort(d2, axis=1)[:, 0] == np.sort(d2, axis=1)[:, 1]).any()


@pytest.mark.parametrize('name', sorted(SMALL))
def test_restatement_equals_brute_force_small(name):
    ref, qry, max_dist, cells = SMALL[name]
    for cell in cells:
        want = _check(ref, qry, max_dist, cell=cell)
    if name == '3-4-5':
        assert (want[1] >= 0).tolist() == gn.THREE_FOUR_FIVE_REPORTED
        assert want[0][:4].tolist() == [5.0] * 4
    if name.startswith('lattice ties'):
        d2 = gn.d2_fp32(qry[:, None, :], ref[None, :, :])
        assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 8).sum() >= 216
    if name == 'outside the box':
        assert (want[1] >= 0).tolist() == [False, True, True, True, False]


def test_restatement_equals_brute_force_crowded_cell():
    ref, qry, max_dist, cells = gn.crowded_cell()
    want = _check(ref, qry, max_dist, cell=cells[0])
    assert (want[1][:300] >= 0).all() and (want[1][300:500] == 5000).any() and (want[1][500:] == -1).all()


def test_restatement_equals_brute_force_off_lane_sizes():
    found = []
    for (R, Q), (ref, qry) in gn.off_lane_sizes().items():
        want = _check(ref, qry, 0.3)
        assert len(want[0]) == Q
        found.append((want[1] >= 0).mean())
    assert min(found) < 0.5 and max(found) > 0.5


@pytest.mark.parametrize('shift', [0.0, 1000.0])
def test_restatement_equals_brute_force_sphere_shells(shift):
    inner, outer, max_dist = gn.sphere_shells(shift)
    want = _check(outer, inner, max_dist)
    none = (want[1] < 0).mean()
    print('inner -> outer: %d queries, %.3f with no neighbour' % (len(inner), none))
    assert 0.1 < none < 0.5
    assert (_check(inner, outer, max_dist)[1] >= 0).all()


def test_restatement_does_not_depend_on_the_grid():
    ref, qry, max_dist, _ = gn.crowded_cell()
    want = gn.grid_search(ref, qry, max_dist)
    for cell, max_cells in ((max_dist / 64, None), (max_dist, None), (4 * max_dist, None), (None, 8), (None, 1)):
        assert _same(gn.grid_search(ref, qry, max_dist, cell=cell, max_cells=max_cells), want), (cell, max_cells)
    assert gn.grid_dims([0, 0, 0], [1, 1, 1], 0.01, 1)[1] == [1, 1, 1]
    h, n = gn.grid_dims([0, 0, 0], [10, 5, 0], 0.1, 8)
    assert n[0] * n[1] * n[2] <= 8 < 101 * 51 and n[2] == 1 and h > 0.1


@pytest.mark.parametrize('mistake', gn.MISTAKES)
def test_each_mistake_is_caught(mistake):
    """Stopping at the first non-empty cube, a bound of (k + 1) h, kmax = floor(max_dist / h), ties in cell order and
    reporting without the max_dist test: each gives a wrong answer on one of the small inputs at least."""
    caught = []
    for name in CATCHERS:
        ref, qry, max_dist, cells = SMALL[name]
        want = gn.within(*gn.brute(ref, qry), max_dist)
        if any(not _same(gn.grid_search(ref, qry, max_dist, cell=c, mistake=mistake), want) for c in cells):
            caught.append(name)
    print(mistake, 'caught by', caught)
    assert caught


def test_python_grid_is_the_restatement_grid():
    from monosdf_amd.utils import mesh_eval as me
    for lo, hi, h, cap in (([0, 0, 0], [10, 5, 0], 0.1, 8), ([-3.5, 2, 1], [4, 2.25, 9], 0.3, 2 ** 25),
                           ([0, 0, 0], [1e4, 1e4, 1e4], 1e-3, 2 ** 25), ([1, 1, 1], [1, 1, 1], 5.0, 1)):
        got, want = me.grid_dims(lo, hi, h, cap), gn.grid_dims(lo, hi, h, cap)
        assert got[0] == want[0] and list(got[1]) == want[1]
    assert me.GRID_CELL_FRACTION == gn.CELL_FRACTION and me.GRID_MAX_CELLS == gn.MAX_CELLS


# ---------------------------------------------------------------- the library (header and table: test_abi_cpu.py)

def test_library_exports_the_gnn_entries():
    from monosdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    lib = _lib.load()
    assert lib.msdf_gnn_workspace_bytes(1) == 256 and lib.msdf_gnn_workspace_bytes(1000) == 16000
    assert lib.msdf_gnn_workspace_bytes(0) == -1 and lib.msdf_gnn_workspace_bytes(2 ** 31) == -1
    # argument errors are refused on the host, before any launch
    grid = (0.0, 0.0, 0.0, 1.0, 1, 1, 1)
    assert lib.msdf_gnn_query(None, None, 0, None, 1, None, *grid, 1.0, None, None, None) == 0
    assert lib.msdf_gnn_query(None, None, 1, None, 1, None, *grid, 1.0, None, None, None) == 1
    assert lib.msdf_gnn_query(None, None, 0, None, 0, None, *grid, 1.0, None, None, None) == 1
    for bad in ((0.0, 0.0, 0.0, 0.0, 1, 1, 1), (0.0, 0.0, 0.0, float('inf'), 1, 1, 1), (0.0, 0.0, 0.0, 1.0, 0, 1, 1),
                (0.0, float('nan'), 0.0, 1.0, 1, 1, 1), (0.0, 0.0, 0.0, 1.0, 2 ** 11, 2 ** 10, 2 ** 10)):
        assert lib.msdf_gnn_query(None, None, 0, None, 1, None, *bad, 1.0, None, None, None) == 1, bad
        assert lib.msdf_gnn_cells(None, 0, *bad, None, None) == 1, bad
    for max_dist in (0.0, -1.0, float('inf'), float('nan')):
        assert lib.msdf_gnn_query(None, None, 0, None, 1, None, *grid, max_dist, None, None, None) == 1
    assert lib.msdf_gnn_cells(None, 0, *grid, None, None) == 0 and lib.msdf_gnn_cells(None, 1, *grid, None, None) == 1
    assert lib.msdf_gnn_records(None, None, 1, None, None) == 1


def test_refusals_without_a_gpu():
    from monosdf_amd.utils import mesh_dtu as md
    from monosdf_amd.utils import mesh_eval as me
    pts = torch.zeros(4, 3)
    with pytest.raises(TypeError, match='cpu'):
        me.nearest_neighbors_within(pts, pts, 1.0)
    with pytest.raises(TypeError, match='cpu'):
        md.evaluate_dtu(pts, pts, np.ones((2, 2, 2)), np.zeros((2, 3)), 1.0, [0, 0, 1, 0], search='grid')
    with pytest.raises(ValueError, match='search'):
        md.evaluate_dtu(pts, pts, np.ones((2, 2, 2)), np.zeros((2, 3)), 1.0, [0, 0, 1, 0], search='tree')
