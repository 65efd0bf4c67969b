"""CPU tests of the oriented bounds: the workspace size and the host-side refusals of the msdf_obb_* entry points, the
host hull (utils/mesh_bounds.HostHull) against scipy, the restatement (tests/obb_numpy.py) on a cuboid whose answer is
known, and the conditions on the constructed inputs that the GPU tests (test_gpu_obb.py) rely on."""
import os
import re
import sys

import numpy as np
import pytest

pytest.importorskip('scipy')

import obb_numpy as on

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---------------------------------------------------------------- the library (header and table: test_abi_cpu.py)

def test_library_exports_the_obb_entries():
    from monosdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    lib = _lib.load()
    # refused on the host, before anything is launched: sizes outside [0, 2^31), null pointers with sizes > 0, a
    # maximum over no points; no planes and no normals launch nothing
    big = 2 ** 31 - 1
    assert lib.msdf_obb_support_workspace_bytes(1, 1) == 256
    assert lib.msdf_obb_support_workspace_bytes(2049, 1000) == 2 * 1000 * 12
    for n, d in ((-1, 1), (1, -1), (big, 1), (1, big), (2 ** 40, 1)):
        assert lib.msdf_obb_support_workspace_bytes(n, d) == -1, (n, d)
        assert lib.msdf_obb_support(None, n, None, d, None, None, None, None) == 1, (n, d)
    assert lib.msdf_obb_support(None, 5, None, 0, None, None, None, None) == 0
    assert lib.msdf_obb_support(None, 0, None, 0, None, None, None, None) == 0
    assert lib.msdf_obb_support(None, 0, None, 3, None, None, None, None) == 1
    assert lib.msdf_obb_support(None, 5, None, 3, None, None, None, None) == 1
    assert lib.msdf_obb_candidates(None, 4, None, 0, None, None, 6, None, None, None, None) == 0
    assert lib.msdf_obb_candidates(None, 4, None, 2, None, None, 6, None, None, None, None) == 1
    for h, k, e in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (big, 1, 1), (1, big, 1), (1, 1, big)):
        assert lib.msdf_obb_candidates(None, h, None, k, None, None, e, None, None, None, None) == 1, (h, k, e)


def test_product_imports_neither_scipy_nor_trimesh():
    text = open(os.path.join(ROOT, 'monosdf_amd', 'utils', 'mesh_bounds.py')).read()
    assert not re.search(r'^\s*(import|from)\s+(scipy|trimesh)', text, flags=re.M)


# ---------------------------------------------------------------- the host hull on its own

@pytest.mark.parametrize('name', sorted(on.HULL_CLOUDS))
def test_host_hull_equals_scipy(name):
    from monosdf_amd.utils import mesh_bounds as mb
    pts = on.HULL_CLOUDS[name]()
    tol = on.tolerance(pts)
    faces, planes = mb.host_hull(pts, tol)
    want, volume, _ = on.hull(pts)
    assert np.array_equal(np.unique(faces), want)
    assert abs(on.faces_volume(pts, faces) - volume) <= 1e-12 * volume
    # outward unit normals, every point on or below every face
    assert np.allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0, rtol=0, atol=1e-14)
    assert on.support(pts, planes)[0].max() <= tol
    # closed: every edge once in each direction
    edges, f1, f2 = mb.hull_edges(np.searchsorted(want, faces))
    assert 2 * len(edges) == 3 * len(faces) and len(want) - len(edges) + len(faces) == 2


def test_host_hull_skips_inside_points_and_refuses_flat_input():
    from monosdf_amd.utils import mesh_bounds as mb
    hull = mb.HostHull(on.tetrahedron(), 1e-12)
    assert hull.add([0.1, 0.1, 0.1]) == -1 and len(hull.result()[0]) == 4
    assert hull.add([1.0, 1.0, 1.0]) == 4 and len(hull.result()[0]) == 6
    flat = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.3, 0.2, 0]], dtype=np.float64)
    for bad in (flat, flat[:, [0, 2, 2]], flat[:1].repeat(5, 0), flat[:3]):
        with pytest.raises(ValueError, match='^host_hull'):
            mb.host_hull(bad, 1e-12)
    with pytest.raises(ValueError, match='^HostHull'):
        mb.HostHull(flat[:4], 1e-12)


def test_hull_normals_merge_hemispheres_and_duplicates():
    from monosdf_amd.utils import mesh_bounds as mb
    planes = np.array([[0, 0, 1, 0], [0, 0, -1, 0], [0, -1, 0, 0], [0.6, 0.8, 0, 0], [-0.6, -0.8, 0, 0],
                       [0.6, 0.8, 0, 1], [-0.0, 1, 0, 2]], dtype=np.float64)
    got = mb.hull_normals(planes)
    assert np.array_equal(got, np.array([[0, 0, 1], [0, 1, 0], [0.6, 0.8, 0]]))
    assert not np.signbit(got).any()
    assert np.array_equal(got, on.hemisphere(planes[:, :3]))


# ---------------------------------------------------------------- the restatement on a known answer

def test_restatement_on_the_cuboid():
    """The cloud's hull is the cuboid of the 8 stored corners.  Storing a corner in fp32 moves each coordinate by at
    most half an ulp of the largest coordinate, u = 2^-24 (coordinates below 2 in magnitude), so a corner moves by
    delta <= sqrt(3) u = 1.04e-7.  (1) Along any fixed direction the width of the stored cloud differs from the exact
    cuboid's by at most 2 delta.  (2) Every candidate frame comes from a hull face through three stored corners and
    a hull edge; a plane through three points that moved by delta, whose triangle has no altitude below 2 / sqrt(5)
    (the 2 x 1 face's diagonal), tilts by at most 2 delta / 0.894, and the projection of a face diagonal seen edge-on
    enlarges that by at most the ratio of the sides, 3: theta <= 6.71 delta.  (3) In a frame tilted by theta the exact
    cuboid's width along an axis grows by at most (the sum of the other two sides) sin(theta) <= 5 theta.  Together:
    |extent - side| <= 2 delta + 5 * 6.71 delta < 36 delta = 3.7e-6.  Measured: 8e-8."""
    pts = on.cuboid_cloud()
    assert np.abs(pts).max() < 2.0
    delta = np.sqrt(3.0) * 2.0 ** -24
    bound = 36.0 * delta
    volume, extents, to_origin = on.oriented_bounds(pts)
    err = np.abs(extents - on.CUBOID_SIDES)
    print('cuboid: extents', extents, 'error', err, 'bound', bound)
    assert (err <= bound).all()
    assert abs(volume - 6.0) <= 6.0 * (3 * bound)
    assert np.array_equal(on.hull(pts)[0], np.arange(8))
    rot = to_origin[:3, :3]
    assert np.allclose(rot @ rot.T, np.eye(3), rtol=0, atol=1e-14) and abs(np.linalg.det(rot) - 1.0) < 1e-14
    q = pts.astype(np.float64) @ rot.T + to_origin[:3, 3]
    assert (np.abs(q) <= extents / 2 + 1e-14).all()


def test_restated_support_takes_the_first_maximum():
    pts = np.array([[1, 0, 0], [3, 0, 0], [3, 0, 0], [2, 5, 0]], dtype=np.float32)
    value, index = on.support(pts, np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, -2.0]]))
    assert value.tolist() == [3.5, 5.0, -1.0, -2.0] and index.tolist() == [1, 3, 0, 0]


# ---------------------------------------------------------------- conditions the GPU tests rely on

@pytest.mark.parametrize('name', sorted(on.HULL_CLOUDS))
def test_hull_clouds_have_no_point_near_a_face(name):
    """No point that is not a hull vertex lies within 100 tol of a hull face: whether it is a vertex cannot depend on
    the last bits of a plane."""
    pts = on.HULL_CLOUDS[name]()
    vertices, _, equations = on.hull(pts)
    rest = np.setdiff1d(np.arange(len(pts)), vertices)
    if len(rest):
        dist = pts[rest].astype(np.float64) @ equations[:, :3].T + equations[:, 3]
        assert dist.max() < -100 * on.tolerance(pts)
    if name == 'sphere':
        assert len(rest) == 0
    if name == 'five':
        assert rest.tolist() == [4]


def test_lattice_is_exactly_coplanar():
    pts = on.lattice()
    assert len(pts) == 125 and on.hull(pts)[1] == 64.0
    assert (pts[:, 0] == 4).sum() == 25


def test_crop_case_keeps_clear_of_the_box_faces():
    """No transformed vertex of the constructed reconstruction lies within 1e-6 of a face of the scaled box, so a
    last-bit difference in to_origin cannot flip a vertex; the reconstruction sticks out on all six sides, keeps
    something, and has faces that straddle the boundary."""
    rec_v, rec_f, gt_v, gt_f = on.crop_case()
    to_origin = on.oriented_bounds(gt_v)[2]
    mask, faces, r, g, lo, hi = on.crop(rec_v, rec_f, gt_v, to_origin)
    gap = np.minimum(np.abs(r - lo[None]), np.abs(r - hi[None])).min()
    print('crop case: smallest distance to a scaled box face', gap)
    assert gap > 1e-6
    assert ((r < lo[None]).any(axis=0) & (r > hi[None]).any(axis=0)).all()
    assert 0 < mask.sum() < len(mask)
    part = mask[rec_f].sum(axis=1)
    assert ((part > 0) & (part < 3)).any() and len(faces) == (part == 3).sum() > 0
    # the box is centred: its two faces along an axis are equally far from the origin (up to rounding)
    assert np.allclose(lo, -hi, rtol=0, atol=1e-12)
