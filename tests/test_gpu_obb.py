"""GPU tests of utils/mesh_bounds.py: the support kernel against numpy (exactly on integer inputs, within the rounding
bound otherwise), convex_hull against scipy, oriented_bounds against the 2-D-hull restatement (tests/obb_numpy.py),
the crop against its restatement, and evaluate_replica(crop=True).  The conditions on the constructed inputs that the
exact comparisons rely on are proved in test_obb_cpu.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytest.importorskip('scipy')

import obb_numpy as on

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SLICE, TILE = 2048, 128                                   # OBB_SLICE, OBB_TILE of csrc/obb.hip
SIZES_N = (1, 63, 64, 65, 257, 1025, 2 * SLICE + 3)       # the last: past a slice, three slices, the last one short
SIZES_D = (1, 63, 65, TILE + 1, 2 * TILE + 5)             # past an LDS tile; three tiles, the last no multiple of 4


def _mb():
    from monosdf_amd.utils import mesh_bounds
    return mesh_bounds


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _support(points, planes):
    value, index = _mb().support(_cuda(points, np.float32), planes)
    assert value.dtype == torch.float64 and index.dtype == torch.int64 and value.is_cuda and index.is_cuda
    return value.cpu().numpy(), index.cpu().numpy()


# ---------------------------------------------------------------- the support kernel

@pytest.mark.parametrize('n', SIZES_N)
def test_support_exact_on_integers(n):
    rng = np.random.default_rng(n)
    for d in SIZES_D:
        pts = rng.integers(-4, 5, (n, 3)).astype(np.float32)            # few values: repeated maxima everywhere
        planes = rng.integers(-3, 4, (d, 4)).astype(np.float64)
        want = on.support(pts, planes)
        got = _support(pts, planes)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, d)
        again = _support(pts, planes)
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), (n, d)
    # the maximum in the last point (behind it the pad positions of its lane and slice), then the same value in the
    # first point too: the smallest index wins
    planes = np.array([[1, 1, 1, 0], [1, 0, 0, 5], [0, 0, 2, -1]], dtype=np.float64)
    pts[-1] = 50
    value, index = _support(pts, planes)
    assert value.tolist() == [150.0, 55.0, 99.0] and index.tolist() == [n - 1] * 3
    pts[0] = 50
    value, index = _support(pts, planes)
    assert value.tolist() == [150.0, 55.0, 99.0] and index.tolist() == [0] * 3
    if n > 2:
        pts[0] = 0
        pts[n // 2] = 50
        assert _support(pts, planes)[1].tolist() == [n // 2] * 3


@pytest.mark.parametrize('n', SIZES_N)
def test_support_within_rounding_on_reals(n):
    """value: within 4 * 2^-53 * (|a x| + |b y| + |c z| + |w|) of the exact value -- the kernel's four rounding steps
    -- and numpy's own evaluation within the same, so twice that between them.  The reported point's value,
    recomputed, lies within that of the maximum."""
    rng = np.random.default_rng(100 + n)
    for d in SIZES_D:
        pts = rng.normal(size=(n, 3)).astype(np.float32) * 3
        planes = rng.normal(size=(d, 4))
        value, index = _support(pts, planes)
        want, _ = on.support(pts, planes)
        bound = on.support_bound(pts, planes)                           # [D, N]
        rows = np.arange(d)
        assert (index >= 0).all() and (index < n).all()
        err = np.abs(value - want)
        print('n', n, 'd', d, 'largest error / bound', (err / (2 * bound.max(axis=1))).max())
        assert (err <= 2 * bound.max(axis=1)).all(), (n, d)
        p = pts[index].astype(np.float64)
        at = (planes[:, 2] * p[:, 2] + (planes[:, 1] * p[:, 1] + planes[:, 0] * p[:, 0])) + planes[:, 3]
        assert (np.abs(at - value) <= 2 * bound[rows, index]).all(), (n, d)
        assert (want - at <= 2 * bound.max(axis=1)).all(), (n, d)


def test_support_refuses():
    mb = _mb()
    pts = torch.zeros(5, 3, device='cuda')
    with pytest.raises(TypeError, match='^support: .*cpu'):
        mb.support(torch.zeros(5, 3), np.zeros((1, 4)))
    with pytest.raises(ValueError, match='^support: planes'):
        mb.support(pts, np.zeros((2, 3)))
    with pytest.raises(ValueError, match='^support: .*empty'):
        mb.support(pts[:0], np.zeros((2, 4)))
    with pytest.raises(ValueError, match='^support: non-finite'):
        mb.support(pts, np.array([[0, 0, np.inf, 0]]))
    value, index = mb.support(pts, np.zeros((0, 4)))
    assert value.shape == (0,) and index.shape == (0,)


# ---------------------------------------------------------------- convex_hull

@functools.lru_cache(maxsize=None)
def _cloud(name):
    return on.HULL_CLOUDS[name]()


def _hull(pts):
    vertex_index, faces, planes = _mb().convex_hull(_cuda(pts, np.float32))
    assert vertex_index.dtype == faces.dtype == torch.int64 and planes.dtype == torch.float64
    assert faces.shape[1:] == (3,) and planes.shape == (faces.shape[0], 4)
    return vertex_index.cpu().numpy(), faces.cpu().numpy(), planes.cpu().numpy()


def _check_contract(pts, vertex_index, faces, planes):
    tol = on.tolerance(pts)
    assert np.array_equal(vertex_index, np.unique(faces)) and vertex_index.min() >= 0 and vertex_index.max() < len(pts)
    assert np.allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0, rtol=0, atol=1e-14)
    # containment through the support kernel: no point more than tol beyond a face
    assert _support(pts, planes)[0].max() <= tol
    # outward orientation: the right-hand normal of a face is its plane's
    p = pts.astype(np.float64)
    cross = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    assert ((cross * planes[:, :3]).sum(1) > 0).all()
    # the vertices lie on their faces' planes
    on_plane = (p[faces] * planes[:, None, :3]).sum(2) + planes[:, None, 3]
    assert np.abs(on_plane).max() <= 100 * tol + 16 * 2.0 ** -53 * np.abs(p).max()


@pytest.mark.parametrize('name', sorted(on.HULL_CLOUDS))
def test_convex_hull_equals_scipy(name):
    pts = _cloud(name)
    vertex_index, faces, planes = _hull(pts)
    want, volume, _ = on.hull(pts)
    assert np.array_equal(vertex_index, want)
    got = on.faces_volume(pts, faces)
    print(name, 'vertices', len(want), 'faces', len(faces), 'volume error', abs(got - volume) / volume)
    assert abs(got - volume) <= 1e-12 * volume
    _check_contract(pts, vertex_index, faces, planes)
    again = _hull(pts)
    assert np.array_equal(again[1], faces) and np.array_equal(again[2], planes)


def test_convex_hull_of_a_lattice():
    pts = on.lattice()
    vertex_index, faces, planes = _hull(pts)
    _check_contract(pts, vertex_index, faces, planes)
    assert abs(on.faces_volume(pts, faces) - 64.0) <= 1e-12 * 64.0


def test_convex_hull_refuses():
    mb = _mb()
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match='^convex_hull: .*at least 4'):
        mb.convex_hull(_cuda(on.tetrahedron()[:3]))
    bad = on.five().copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match='^convex_hull: non-finite'):
        mb.convex_hull(_cuda(bad))
    flat = rng.uniform(-1, 1, (100, 3)).astype(np.float32)
    flat[:, 2] = 0.5
    line = (np.outer(np.arange(-25, 25), [1.0, 2.0, -0.5]) / 32).astype(np.float32)     # exact in fp32
    same = np.full((10, 3), 0.25, dtype=np.float32)
    for cloud in (flat, flat[:, [2, 0, 1]], line, same):
        with pytest.raises(ValueError, match='^convex_hull: .*one plane'):
            mb.convex_hull(_cuda(cloud))
    with pytest.raises(TypeError, match='^convex_hull: .*cpu'):
        mb.convex_hull(torch.zeros(10, 3))


# ---------------------------------------------------------------- oriented_bounds

def _check_box(pts, to_origin, extents):
    assert to_origin.dtype == extents.dtype == np.float64 and to_origin.shape == (4, 4) and extents.shape == (3,)
    rot, shift = to_origin[:3, :3], to_origin[:3, 3]
    assert np.array_equal(to_origin[3], [0, 0, 0, 1])
    assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(rot) - 1.0) <= 1e-14
    assert extents[0] <= extents[1] <= extents[2]
    # every point inside, with no slack beyond rounding: 4 steps of the kernel's evaluation, 3 of this one, and the
    # sum, difference and halving that make the centre and the extent, each at most 2^-53 of |R_i| . |p| + |t_i|
    p = pts.astype(np.float64)
    slack = 16 * 2.0 ** -53 * (np.abs(rot) @ np.abs(p).max(axis=0) + np.abs(shift))
    q = p @ rot.T + shift
    assert (np.abs(q) <= extents / 2 + slack).all()
    # and tight: on every axis a point within the slack of each face
    assert (q.max(axis=0) >= extents / 2 - slack).all() and (q.min(axis=0) <= -extents / 2 + slack).all()


@pytest.mark.parametrize('name', ('gaussian', 'room'))
def test_oriented_bounds_equals_the_restatement(name):
    pts = _cloud(name)
    to_origin, extents = _mb().oriented_bounds(_cuda(pts))
    volume, want_extents, _ = on.oriented_bounds(pts)
    got = float(np.prod(extents))
    print(name, 'volume', got, 'restated', volume, 'relative', abs(got - volume) / volume, 'extents', extents)
    assert abs(got - volume) <= 1e-9 * volume
    assert np.allclose(extents, want_extents, rtol=1e-9, atol=0)
    _check_box(pts, to_origin, extents)
    again = _mb().oriented_bounds(_cuda(pts))
    assert np.array_equal(again[0], to_origin) and np.array_equal(again[1], extents)
    # a mesh object, a pair and a host array are the same cloud
    from monosdf_amd.utils.mesh import Mesh
    faces = np.zeros((1, 3), dtype=np.int64)
    for arg in (Mesh(pts, faces), (_cuda(pts), _cuda(faces)), pts):
        other = _mb().oriented_bounds(arg)
        assert np.array_equal(other[0], to_origin) and np.array_equal(other[1], extents)


def test_oriented_bounds_of_the_cuboid():
    """The bound: test_obb_cpu.test_restatement_on_the_cuboid derives |extent - side| < 36 sqrt(3) 2^-24."""
    pts = on.cuboid_cloud()
    to_origin, extents = _mb().oriented_bounds(_cuda(pts))
    bound = 36.0 * np.sqrt(3.0) * 2.0 ** -24
    print('cuboid: extents', extents, 'error', np.abs(extents - on.CUBOID_SIDES))
    assert (np.abs(extents - on.CUBOID_SIDES) <= bound).all()
    assert abs(np.prod(extents) - on.oriented_bounds(pts)[0]) <= 1e-9 * 6.0
    _check_box(pts, to_origin, extents)


def test_oriented_bounds_refuses():
    mb = _mb()
    with pytest.raises(ValueError, match='^oriented_bounds: .*at least 4'):
        mb.oriented_bounds(_cuda(on.tetrahedron()[:2]))
    with pytest.raises(ValueError, match='^oriented_bounds: .*one plane'):
        mb.oriented_bounds(_cuda(on.lattice()[:25]))
    with pytest.raises(TypeError, match='^oriented_bounds: .*cpu'):
        mb.oriented_bounds(torch.zeros(10, 3))


# ---------------------------------------------------------------- the crop

@functools.lru_cache(maxsize=None)
def _crop_case():
    return on.crop_case()


def test_crop_equals_the_restatement():
    mb = _mb()
    rec_v, rec_f, gt_v, gt_f = _crop_case()
    out = mb.crop_to_oriented_bounds((_cuda(rec_v), _cuda(rec_f)), (_cuda(gt_v), _cuda(gt_f)))
    to_origin = mb.oriented_bounds(_cuda(gt_v))[0]
    mask, faces, *_ = on.crop(rec_v, rec_f, gt_v, to_origin)
    assert 0 < mask.sum() < len(mask) and 0 < len(faces) < len(rec_f)
    assert np.array_equal(out.vertices, rec_v[mask].astype(np.float64))          # the original frame, the original order
    assert np.array_equal(out.faces, faces)
    # the frame found the long way gives the same crop (no vertex is within 1e-6 of a face of the scaled box)
    other = on.crop(rec_v, rec_f, gt_v, on.oriented_bounds(gt_v)[2])
    assert np.array_equal(other[0], mask) and np.array_equal(other[1], faces)
    # host arrays and Mesh objects in, vertex normals following their vertices
    from monosdf_amd.utils.mesh import Mesh
    normals = np.random.default_rng(2).normal(size=rec_v.shape)
    host = mb.crop_to_oriented_bounds(Mesh(rec_v, rec_f, normals), Mesh(gt_v, gt_f))
    assert np.array_equal(host.vertices, out.vertices) and np.array_equal(host.faces, faces)
    assert np.array_equal(host.vertex_normals, normals[mask])


def test_crop_that_keeps_everything_and_nothing():
    mb = _mb()
    rec_v, rec_f, gt_v, gt_f = _crop_case()
    gt = (_cuda(gt_v), _cuda(gt_f))
    # the ground truth itself lies strictly inside its box scaled by 1.05
    out = mb.crop_to_oriented_bounds(gt, gt)
    assert np.array_equal(out.vertices, gt_v.astype(np.float64)) and np.array_equal(out.faces, gt_f)
    far = rec_v + np.float32(100.0)
    out = mb.crop_to_oriented_bounds((_cuda(far), _cuda(rec_f)), gt)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3)
    out = mb.crop_to_oriented_bounds((_cuda(far[:0]), _cuda(rec_f[:0])), gt)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3)
    with pytest.raises(TypeError, match='^crop_to_oriented_bounds: .*cpu'):
        mb.crop_to_oriented_bounds((torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int64)), gt)


# ---------------------------------------------------------------- evaluate_replica(crop=True)

def test_evaluate_replica_with_crop():
    from monosdf_amd.utils import mesh_eval
    mb = _mb()
    rec_v, rec_f, gt_v, gt_f = _crop_case()
    rec, gt = (_cuda(rec_v), _cuda(rec_f)), (_cuda(gt_v), _cuda(gt_f))
    cropped = mb.crop_to_oriented_bounds(rec, gt)
    kw = dict(n_samples=3000, seed=4)
    with_crop = mesh_eval.evaluate_replica(rec, gt, crop=True, **kw)
    assert with_crop == mesh_eval.evaluate_replica(cropped, gt, **kw)
    plain = mesh_eval.evaluate_replica(rec, gt, **kw)
    assert plain == mesh_eval.evaluate_replica(rec, gt, crop=False, **kw)
    assert plain != with_crop
