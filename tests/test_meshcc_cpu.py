"""CPU tests of the mesh connected components: the restatement (tests/meshcc_numpy.py) against scipy on every
constructed input and every rule, the two rule details that the named cases catch, the host-side refusals of the
msdf_mcc_* entry points, ``aligned_grid``, and the refusals that need no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import meshcc_cases as cases
import meshcc_numpy as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {c.name: c for c in cases.all_cases()}


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_has_its_structure(name):
    CASES[name].structure(CASES[name])


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_equals_scipy(name):
    sparse = pytest.importorskip('scipy.sparse')
    from scipy.sparse.csgraph import connected_components
    case = CASES[name]
    F = len(case.faces)
    for rule in cc.RULES:
        labels, count = cc.face_components(case.faces, len(case.vertices), rule)
        assert labels.dtype == np.int64 and labels.shape == (F,)
        if F == 0:
            assert count == 0
            continue
        rows, cols = cc.graph(case.faces, len(case.vertices), rule)
        adjacency = sparse.coo_matrix((np.ones(len(rows), bool), (rows, cols)), shape=(F, F)).tocsr()
        want_count, want = connected_components(adjacency, directed=False)
        assert count == want_count and np.array_equal(labels, want), (name, rule)


def test_runs_of_three_connect_nothing_under_edge():
    for name in ('three on an edge', 'degenerate face', 'soup'):
        case = CASES[name]
        right = cc.face_components(case.faces, len(case.vertices), 'edge')
        wrong = cc.face_components(case.faces, len(case.vertices), 'edge', mistake='runs of 3')
        assert wrong[1] < right[1], name
    assert cc.face_components(CASES['three on an edge'].faces, 8, 'edge')[1] == 3


def test_vertex_components_are_numbered_by_first_face():
    case = CASES['tetrahedra']
    right = cc.face_components(case.faces, len(case.vertices), 'vertex')
    wrong = cc.face_components(case.faces, len(case.vertices), 'vertex', mistake='root order')
    assert right[1] == wrong[1] == 1000 and not np.array_equal(right[0], wrong[0])
    first = [int(np.flatnonzero(right[0] == s)[0]) for s in range(right[1])]
    assert first == sorted(first) and first[0] == 0


def test_sizes_and_selection_restated():
    case = CASES['marching cubes']
    labels, n = cc.face_components(case.faces, len(case.vertices), 'edge')
    count, area = cc.component_sizes(cc.face_areas(case.vertices, case.faces), labels, n)
    assert count.sum() == len(case.faces) and cc.largest(area) == int(np.argmax(area))
    used, faces = cc.select(case.vertices, case.faces, labels == cc.largest(area))
    assert np.array_equal(used[faces], case.faces[labels == cc.largest(area)]) and len(used) < len(case.vertices)
    assert cc.largest(np.array([2.0, 5.0, 5.0])) == 1


# ---------------------------------------------------------------- the library (header and table: test_abi_cpu.py)

def test_library_exports_the_mcc_entries():
    from monosdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    lib = _lib.load()
    big = 2 ** 31 - 1
    # per entry: a size of 0 launches nothing (0), a null pointer with a size > 0 and a size outside [0, 2^31) are
    # refused on the host (1)
    for n, status in ((0, 0), (1, 1), (-1, 1), (big, 1), (2 ** 40, 1)):
        assert lib.msdf_mcc_edge_keys(None, n, None, None) == status, n
        assert lib.msdf_mcc_init(None, n, None) == status, n
        assert lib.msdf_mcc_link_edges(None, None, n, 0, None, None) == status, n
        assert lib.msdf_mcc_link_edges(None, None, n, 1, None, None) == status, n
        assert lib.msdf_mcc_link_vertices(None, n, None, None) == status, n
        assert lib.msdf_mcc_flatten(None, n, None) == status, n
        assert lib.msdf_mcc_segment_sum(None, None, n, None, None) == status, n
    assert lib.msdf_mcc_edge_keys(None, (2 ** 31 - 1) // 3 + 1, None, None) == 1          # 3 F is no size
    for rule in (-1, 2):
        assert lib.msdf_mcc_link_edges(None, None, 0, rule, None, None) == 1


# ---------------------------------------------------------------- aligned_grid

BOXES = {0: ([-0.2, -1.0, -0.7], [0.3, 1.5, 0.9]), 1: ([-2.0, 0.1, -1.0], [1.0, 0.35, 2.5]),
         2: ([0.0, -3.0, 0.5], [2.0, 0.25, 1.0])}


@pytest.mark.parametrize('shortest', sorted(BOXES))
def test_aligned_grid(shortest):
    from monosdf_amd.utils.mesh import aligned_grid
    lo, hi = (np.array(b) for b in BOXES[shortest])
    assert int(np.argmin(hi - lo)) == shortest
    for resolution, eps in ((64, 0.1), (17, 0.01)):
        axes = aligned_grid(lo, hi, resolution, eps)
        want = cc.aligned_grid(lo, hi, resolution, eps)
        assert len(axes) == 3
        for a in range(3):
            assert axes[a].dtype == np.float64 and np.array_equal(axes[a], want[a]), a
        short = axes[shortest]
        assert len(short) == resolution and short[0] == lo[shortest] - eps and short[-1] == hi[shortest] + eps
        step = (short[-1] - short[0]) / (resolution - 1)
        for a in range(3):
            if a != shortest:
                # cubic cells from lo - eps on, covering hi + eps and ending within two steps of it
                assert axes[a][0] == lo[a] - eps and len(axes[a]) > resolution
                assert np.allclose(np.diff(axes[a]), step, rtol=1e-9, atol=0)
                # (arange forms start + i * step: a point meant for hi + eps may land a few ulps either side)
                assert hi[a] + eps - 1e-12 <= axes[a][-1] < hi[a] + eps + 2 * step


def test_aligned_grid_refuses():
    from monosdf_amd.utils.mesh import aligned_grid
    with pytest.raises(ValueError, match='^aligned_grid'):
        aligned_grid([0, 0, 0], [1, 1, 1], 1)
    with pytest.raises(ValueError, match='^aligned_grid'):
        aligned_grid([0, 0, 0], [1, float('nan'), 1], 8)
    with pytest.raises(ValueError, match='^aligned_grid'):
        aligned_grid([0, 0, 0], [1, 0, 1], 8, eps=0.0)


# ---------------------------------------------------------------- refusals without a GPU

def test_merge_keys_follow_the_restatement_and_refuse_overflow():
    from monosdf_amd.utils import mesh_clean as mc
    rng = np.random.default_rng(3)
    v = rng.uniform(-3, 3, (500, 3))
    v[:4] = [[0.5e-8, 1.5e-8, 2.5e-8], [-0.5e-8, -1.5e-8, 1e-9], [1.0, 1.0 + 4e-9, 1.0 + 6e-9], [0, 0, 0]]
    for digits in (8, 5, 0):
        assert np.array_equal(mc.merge_keys(v, digits), cc.merge_keys(v, digits))
        assert torch.equal(mc.merge_keys(torch.from_numpy(v), digits), torch.from_numpy(cc.merge_keys(v, digits)))
    faces = np.array([[0, 1, 2]])
    big = np.array([[0, 0, 0], [1, 0, 0], [0, 2.0 ** 53 / 1e8, 0]])
    with pytest.raises(ValueError, match='^merge_vertices: .*2\\^53'):
        mc.merge_vertices((big, faces), digits=8)
    with pytest.raises(ValueError, match='^merge_vertices'):
        mc.merge_vertices((np.array([[0, 0, 0], [1, 0, 0], [0, float('inf'), 0]]), faces))
    assert mc.merge_keys(big / 2, 8).max() == 2 ** 52


def test_refusals_without_a_gpu():
    from monosdf_amd.utils import mesh_clean as mc
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    host = (np.zeros((4, 3)), np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match='^face_components: connectivity'):
        mc.face_components(host, 'faces')
    with pytest.raises(ValueError, match='^largest_component: connectivity'):
        mc.largest_component(host, connectivity='edges')
    with pytest.raises(ValueError, match='^largest_component: by'):
        mc.largest_component(host, by='volume')
    with pytest.raises(ValueError, match='^remove_small_components: connectivity'):
        mc.remove_small_components(host, min_faces=1, connectivity=None)
    with pytest.raises(ValueError, match='^remove_small_components: give'):
        mc.remove_small_components(host)
    for fn in (mc.face_components, mc.largest_component, mc.merge_vertices, mc.face_areas):
        with pytest.raises(TypeError, match='^%s: .*cpu' % fn.__name__):
            fn((v, f))
    with pytest.raises(TypeError, match='^remove_small_components: .*cpu'):
        mc.remove_small_components((v, f), min_faces=1)
    with pytest.raises(TypeError, match='^component_sizes: .*cpu'):
        mc.component_sizes((v, f), torch.zeros(2, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match='^face_components: face index'):
        mc.face_components((np.zeros((4, 3)), np.array([[0, 1, 4]])))
    with pytest.raises(ValueError, match='^merge_vertices: face index'):
        mc.merge_vertices((np.zeros((4, 3)), np.array([[0, 1, 4]])))
