"""GPU tests of the mesh re-fusion (csrc/refuse.hip, utils/mesh_refuse.py): the depth rasteriser against the fp64
ray-caster, the TSDF integration, the face rule and the frustum test against their fp32 restatements
(tests/refuse_numpy.py), and ``refuse`` end to end on a sphere."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import refuse_numpy as rfn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL = 1e-4                              # the project's relative tolerance
K = (50.0, 50.0, 32.0, 24.0)
H, W = 48, 64


def _mr():
    from monosdf_amd.utils import mesh_refuse
    return mesh_refuse


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _render(v, f, poses, K=K, h=H, w=W, **kw):
    return _mr().render_depth(_cuda(v), _cuda(f, np.int32), poses, K, h, w, **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene():
    """The shared scene, its fp64 depth maps and their exempt pixels: computed once, read only."""
    v, f, poses = rfn.room_scene(seed=0, n_cameras=8)
    ref, exempt, grazing = rfn.raycast(v, f, poses, K, H, W)
    for a in (v, f, poses, ref, exempt, grazing):
        a.setflags(write=False)
    return v, f, poses, ref, exempt, grazing


def _compare_depth(label, depth, ref, exempt, cap=0.005):
    """Coverage equal and |z - z_ref| <= 1e-4 z_ref on every pixel that is not exempt; at most ``cap`` exempt."""
    n_exempt = int(exempt.sum())
    print('%s: %d of %d pixels exempt' % (label, n_exempt, exempt.size))
    assert n_exempt <= cap * exempt.size
    use = ~exempt
    assert np.array_equal((depth > 0)[use], (ref > 0)[use])
    both = use & (ref > 0)
    rel = np.abs(depth[both] - ref[both]) / ref[both]
    print('%s: max |z - z_ref| / z_ref = %.3g over %d pixels' % (label, rel.max() if rel.size else 0.0, rel.size))
    assert rel.size == 0 or rel.max() <= TOL


def test_raster_equals_fp64_raycaster():
    v, f, poses, ref, exempt, grazing = _scene()
    print('grazing pixels: %d' % int(grazing.sum()))
    depth = _render(v, f, poses)
    assert depth.shape == (8, H, W) and depth.dtype == np.float32
    _compare_depth('room', depth, ref, exempt)


def test_no_cracks_inside_a_closed_box():
    v, f, poses, ref, _, _ = _scene()
    assert int((ref > 0).sum()) == 8 * H * W                 # the restatement: every ray of every camera hits
    depth = _render(v, f, poses)
    assert int((depth > 0).sum()) == 8 * H * W


def test_image_spanning_quad_has_plane_depth():
    """Two triangles larger than the view frustum at z = 2, 96 x 128 pixels: every pixel reads 2.  Their pixel boxes
    (the whole image) are far above the threshold of the cooperative path."""
    v = np.array([[-9, -9, 2], [9, -9, 2], [9, 9, 2], [-9, 9, 2]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    depth = _render(v, f, np.eye(4)[None], (50.0, 50.0, 64.0, 48.0), 96, 128)
    assert depth.shape == (1, 96, 128)
    print('quad: max |z - 2| / 2 = %.3g' % (np.abs(depth - 2.0).max() / 2.0))
    assert (np.abs(depth - 2.0) <= TOL * 2.0).all()


def test_triangles_that_cross_the_near_plane():
    """A ground-plane quad under the camera from behind it to z = 10."""
    v = np.array([[-3, 1, -2], [3, 1, -2], [3, 1, 10], [-3, 1, 10]], np.float32).astype(np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    pose = np.eye(4)[None]
    ref, exempt, _ = rfn.raycast(v, f, pose, K, H, W)
    assert (ref > 0).sum() > 500 and (ref == 0).sum() > 500
    assert ref.max() > 9.0 and 2.0 < ref[ref > 0].min() < 2.2    # from the bottom row's 1 / 0.47 to the far edge
    _compare_depth('ground', _render(v, f, pose), ref, exempt)


def test_degenerate_faces_change_nothing():
    v, f, poses, ref, exempt, _ = _scene()
    base = _render(v, f, poses)
    extra_v = np.array([[0.125] * 3, [0.25] * 3, [0.375] * 3])      # collinear, in the middle of the room, exact in fp32
    v2 = np.concatenate([v, extra_v])
    n = len(v)
    # zero area: collinear vertices, a repeated vertex, one vertex three times
    f2 = np.concatenate([f, [[n, n + 1, n + 2], [n, n, n + 1], [n + 2, n + 2, n + 2], [0, 5, 0]]])
    assert np.array_equal(_render(v2, f2, poses), base)
    # a face entirely behind the one camera
    pose = rfn.look_at((0, 0, 0), (0, 0, 1))[None]
    tri = np.array([[-1, -1, -1], [1, -1, -1], [0, 1, -1.5]], np.float64)
    assert not _render(tri, np.array([[0, 1, 2]]), pose).any()
    front = tri * [1, 1, -1]
    both = _render(np.concatenate([front, tri]), np.array([[0, 1, 2], [3, 4, 5]]), pose)
    assert np.array_equal(both, _render(front, np.array([[0, 1, 2]]), pose)) and both.any()


def test_empty_face_list_gives_zeros():
    v, _, poses, _, _, _ = _scene()
    depth = _render(v, np.zeros((0, 3), np.int64), poses)
    assert depth.shape == (8, H, W) and not depth.any()


def test_raster_is_bitwise_repeatable_and_independent_of_order_and_winding():
    v, f, poses, _, _, _ = _scene()
    base = _render(v, f, poses)
    assert np.array_equal(_render(v, f, poses), base)
    rng = np.random.default_rng(5)
    shuffled = f[rng.permutation(len(f))]
    assert np.array_equal(_render(v, shuffled, poses), base)
    flip = rng.uniform(size=len(f)) < 0.5
    rewound = np.where(flip[:, None], shuffled[:, ::-1], np.roll(shuffled, 1, axis=1))
    assert np.array_equal(_render(v, rewound, poses), base)


def test_raster_refuses_bad_meshes_on_the_host():
    v, f, poses, _, _, _ = _scene()
    bad = f.copy()
    bad[7, 2] = len(v)
    with pytest.raises(ValueError, match='face index'):
        _render(v, bad, poses)
    vn = v.copy()
    vn[3, 1] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        _render(vn, f, poses)
    with pytest.raises(TypeError, match='float32'):
        _mr().render_depth(_cuda(v, np.float64), _cuda(f, np.int32), poses, K, H, W)


# ---- TSDF


TSDF_K = (25.0, 25.0, 16.0, 12.0)
TSDF_DIMS = (24, 20, 16)
TSDF_VL, TSDF_TRUNC = 0.05, 0.15


@functools.lru_cache(maxsize=None)
def _tsdf_case():
    """The icosphere seen from 3 cameras, 24 x 32 depth maps from the fp64 ray-caster, a 24 x 20 x 16 block around it."""
    centre = np.array([0.3, -0.2, 0.8])
    v, f = rfn.icosphere(2, 0.5, centre)
    poses = np.stack([rfn.look_at(centre + p, centre) for p in ((1.6, 0.2, 0.1), (-0.3, -1.7, 0.4), (0.2, 0.5, -1.8))])
    depth = rfn.raycast(v, f, poses, TSDF_K, 24, 32)[0].astype(np.float32)
    origin = (centre - 0.5 * TSDF_VL * np.array(TSDF_DIMS)).astype(np.float32).astype(np.float64)
    for a in (depth, poses, origin):
        a.setflags(write=False)
    return depth, poses, origin


def _integrate(depth, poses, origin, **kw):
    t, w = _mr().tsdf_integrate(_cuda(depth), poses, TSDF_K, origin, TSDF_DIMS, TSDF_VL, TSDF_TRUNC, **kw)
    return t.cpu().numpy(), w.cpu().numpy()


def test_tsdf_equals_fp32_restatement():
    """weight equal exactly and |tsdf - ref| <= 1e-5 outside the exempt voxels: the fp32 error of p.z at |x| <= 2 is about
    5e-7, over a truncation of 0.15 about 3e-6, and three mean updates add under 1e-6."""
    depth, poses, origin = _tsdf_case()
    assert (depth > 0).mean() > 0.1
    ref_t, ref_w, exempt = rfn.tsdf_fp32(depth, poses, TSDF_K, origin, TSDF_DIMS, TSDF_VL, TSDF_TRUNC)
    assert (ref_w == 3).any() and (ref_w == 0).any() and (ref_t < 0).any() and (ref_t == 1).any()
    t, w = _integrate(depth, poses, origin)
    assert t.shape == TSDF_DIMS and t.dtype == np.float32 and w.dtype == np.float32
    print('tsdf: %d of %d voxels exempt' % (int(exempt.sum()), exempt.size))
    assert exempt.sum() <= 0.005 * exempt.size
    use = ~exempt
    assert np.array_equal(w[use], ref_w[use])
    err = np.abs(t[use].astype(np.float64) - ref_t[use])
    print('tsdf: max |tsdf - ref| = %.3g' % err.max())
    assert err.max() <= 1e-5
    # bitwise repeatable
    t2, w2 = _integrate(depth, poses, origin)
    assert np.array_equal(t, t2) and np.array_equal(w, w2)


def test_tsdf_view_order_trunc_and_back_side():
    depth, poses, origin = _tsdf_case()
    _, w = _integrate(depth, poses, origin)
    order = [2, 0, 1]
    _, w_perm = _integrate(depth[order], poses[order], origin)
    assert np.array_equal(w, w_perm)
    # one view, depth_trunc below its depths (the camera is 1.6 from the centre, the sphere's radius is 0.5)
    assert depth[0][depth[0] > 0].min() > 1.0
    t0, w0 = _integrate(depth[:1], poses[:1], origin, depth_trunc=1.0)
    assert not w0.any() and not t0.any()
    # a camera in the middle of the block, looking along +x with a constant depth map: the voxels behind it are untouched
    centre = np.array([0.3, -0.2, 0.8])
    pose = rfn.look_at(centre, centre + [1.0, 0, 0])[None]
    flat = np.full((1, 24, 32), 0.3, np.float32)
    t1, w1 = _integrate(flat, pose, origin)
    x = origin[0] + TSDF_VL * (np.arange(TSDF_DIMS[0]) + 0.5)
    behind = x < centre[0] - 1e-6
    assert behind.sum() >= 10 and not w1[behind].any() and not t1[behind].any()
    assert w1[~behind].any()


# ---- face rule


def test_face_rule_and_compaction():
    from monosdf_amd.utils.mesh import marching_cubes
    rng = np.random.default_rng(9)
    g = (np.arange(12) - 5.5) / 5.5
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    tsdf = (np.sqrt(x * x + y * y + z * z) - 0.7 + 0.05 * rng.normal(size=x.shape)).astype(np.float32)
    tsdf[3, 4, 5] = 0.0                                         # a value on the level: a vertex on a lattice point
    weight = (rng.uniform(size=tsdf.shape) < 0.85).astype(np.float32) * rng.integers(1, 4, tsdf.shape)
    weight = weight.astype(np.float32)
    verts, faces, _ = marching_cubes(_cuda(tsdf), 0.0, (1.0, 1.0, 1.0))
    keep = _mr().tsdf_face_keep(verts, faces, _cuda(weight)).cpu().numpy()
    vh, fh = verts.cpu().numpy(), faces.cpu().numpy()
    ref = rfn.face_keep(vh, fh, weight)
    print('face rule: %d of %d faces kept' % (int(keep.sum()), len(keep)))
    assert 0 < ref.sum() < len(ref)
    assert np.array_equal(keep, ref)
    origin, vl = (0.5, -1.0, 2.0), 0.25
    wv, wf, wn = _mr().extract_mesh(_cuda(tsdf), _cuda(weight), origin, vl)
    wv, wf, wn = wv.cpu().numpy(), wf.cpu().numpy(), wn.cpu().numpy()
    assert wv.dtype == np.float64 and wf.dtype == np.int64 and wn.shape == wv.shape
    assert len(wf) == int(ref.sum())
    assert np.array_equal(np.unique(wf), np.arange(len(wv)))                   # no vertex is unreferenced
    # the kept faces, in order, with their vertices where marching cubes put them
    assert np.array_equal(wv[wf], np.asarray(origin) + vl * (0.5 + vh.astype(np.float64)[fh[ref]]))
    # every kept face's cell has 8 observed corners
    idx = (wv[wf] - np.asarray(origin)) / vl - 0.5
    centroid = idx.mean(1)
    inner = (np.abs(centroid - np.round(centroid)) > 1e-6).all(1)             # not a face that lies in a lattice plane
    assert inner.sum() > 0.9 * len(wf)
    cell = np.floor(centroid[inner]).astype(np.int64)
    for d in range(8):
        c = cell + [(d >> 2) & 1, (d >> 1) & 1, d & 1]
        assert (weight[c[:, 0], c[:, 1], c[:, 2]] > 0).all()


# ---- refuse end to end


RF_K, RF_SIZE, RF_VL = (100.0, 100.0, 48.0, 48.0), 96, 0.02


@functools.lru_cache(maxsize=None)
def _sphere_case():
    v, f = rfn.icosphere(3, 0.5, (0, 0, 0))
    poses = np.stack([rfn.look_at(1.5 * np.eye(3)[a] * s, (0, 0, 0)) for a in range(3) for s in (1, -1)])
    for a in (v, f, poses):
        a.setflags(write=False)
    return v, f, poses


@functools.lru_cache(maxsize=None)
def _sphere_refused(block):
    from monosdf_amd.utils.mesh import Mesh
    v, f, poses = _sphere_case()
    out = _mr().refuse(Mesh(v, f), poses, RF_K, RF_SIZE, RF_SIZE, voxel_length=RF_VL, block=block)
    for a in (out.vertices, out.faces, out.vertex_normals):
        a.setflags(write=False)
    return out


def test_refuse_is_the_composition_of_its_stages():
    mr = _mr()
    v, f, poses = _sphere_case()
    whole = _sphere_refused(512)
    assert len(whole.faces) > 1000
    vc = _cuda(v)
    depth = mr.render_depth(vc, _cuda(f, np.int32), poses, RF_K, RF_SIZE, RF_SIZE)
    lo, hi = vc.min(0).values.double().cpu().numpy(), vc.max(0).values.double().cpu().numpy()
    origin, dims = mr.fusion_grid(lo, hi, RF_VL)
    origin = origin.astype(np.float32).astype(np.float64)
    tsdf, weight = mr.tsdf_integrate(depth, poses, RF_K, origin, dims, RF_VL, None)
    sv, sf, sn = mr.extract_mesh(tsdf, weight, origin, RF_VL)
    assert np.array_equal(whole.vertices, sv.cpu().numpy())
    assert np.array_equal(whole.faces, sf.cpu().numpy())
    assert np.array_equal(whole.vertex_normals, sn.cpu().numpy().astype(np.float64))
    # depth maps rendered two views at a time give the same mesh, bit for bit
    from monosdf_amd.utils.mesh import Mesh
    chunked = mr.refuse(Mesh(v, f), poses, RF_K, RF_SIZE, RF_SIZE, voxel_length=RF_VL, view_chunk=4)
    assert np.array_equal(chunked.vertices, whole.vertices) and np.array_equal(chunked.faces, whole.faces)


def _grid_keys(vertices):
    return np.unique(np.round(np.asarray(vertices) * 1e6).astype(np.int64), axis=0)


def _covered(a, b):
    """Every key of ``a`` is a key of ``b`` or a neighbour of one (one unit of the 1e-6 grid per axis)."""
    have = set(map(tuple, b))
    steps = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    return all(any((p[0] + s[0], p[1] + s[1], p[2] + s[2]) in have for s in steps) for p in map(tuple, a))


def test_refuse_in_several_blocks_gives_the_same_vertices():
    """block = 16 cuts the volume of about 58^3 voxels into 4 x 4 x 4 blocks.  The vertex sets are compared on the 1e-6
    grid after duplicates (the seam vertices of neighbouring blocks) are removed.  The TSDF values are bitwise the same
    in every blocking, but marching cubes forms index + t in fp32 with a block-local index, so a coordinate moves by up
    to an ulp of the index times the voxel (4e-8 here) and may fall on the other side of a rounding boundary of the
    grid: a vertex matches if the other set has it in the same or a neighbouring grid cell."""
    whole, blocks = _sphere_refused(512), _sphere_refused(16)
    assert len(blocks.vertices) > len(whole.vertices)             # the seams are duplicated
    assert len(blocks.faces) == len(whole.faces)                  # every cell belongs to one block
    a, b = _grid_keys(whole.vertices), _grid_keys(blocks.vertices)
    exact = len(set(map(tuple, a)) & set(map(tuple, b)))
    print('blocks: %d / %d unique vertices, %d on the same grid point' % (len(a), len(b), exact))
    assert _covered(a, b) and _covered(b, a)
    assert abs(len(a) - len(b)) <= 0.2 * len(a) and exact >= 0.7 * len(a)


def test_refuse_stays_at_the_seen_surface():
    """Every output vertex lies within sdf_trunc + sqrt(3) voxel_length of the input surface (a voxel is only updated
    when it is less than sdf_trunc behind, or anywhere in front of, the seen surface along its ray, and in front
    tau > 0: a zero crossing lies within the truncation plus one cell diagonal), tested against the sphere, whose
    icosphere lies at most 0.002 inside it; and the unseen interior gives no shell."""
    out = _sphere_refused(512)
    r = np.linalg.norm(out.vertices, axis=1)
    trunc = 3 * RF_VL
    bound = trunc + np.sqrt(3.0) * RF_VL
    print('refuse: %d vertices, %d faces, radius %.4f .. %.4f, mean | |v| - 0.5 | = %.3g' %
          (len(r), len(out.faces), r.min(), r.max(), np.abs(r - 0.5).mean()))
    assert len(r) > 1000
    assert (r >= 0.5 - 0.002 - bound).all() and (r <= 0.5 + bound).all()
    assert not (r < 0.5 - 0.002 - trunc - np.sqrt(3.0) * RF_VL).any()
    # the whole sphere is seen from the six sides: vertices in every octant
    assert len({tuple(s) for s in np.sign(out.vertices).astype(int) if 0 not in s}) == 8


# ---- frustum culling


def test_cull_to_frustums():
    from monosdf_amd.utils.mesh import Mesh
    mr = _mr()
    v, f, poses, _, _, _ = _scene()
    cams = poses[[2, 5, 7]]                                      # one of them sees most of the sphere
    seen = mr.seen_vertices(_cuda(v), cams, K, H, W).cpu().numpy()
    ref, exempt = rfn.seen_fp32(v, cams, K, H, W)
    print('cull: %d of %d vertices exempt, %d seen' % (int(exempt.sum()), len(v), int(ref.sum())))
    assert exempt.sum() <= 0.005 * len(v)
    assert 50 < ref.sum() < len(v) - 20
    assert np.array_equal(seen[~exempt], ref[~exempt])
    normals = np.random.default_rng(2).normal(size=v.shape)
    out = mr.cull_to_frustums(Mesh(v, f, normals), cams, K, H, W)
    assert np.array_equal(out.vertices, v) and np.array_equal(out.vertex_normals, normals)     # vertices are kept
    assert np.array_equal(out.faces, f[seen[f].any(1)])
    assert 0 < len(out.faces) < len(f)
    # tensors in, the same faces out
    out_t = mr.cull_to_frustums((_cuda(v), _cuda(f, np.int32)), cams, K, H, W)
    assert np.array_equal(out_t.faces, out.faces)
    # cameras that see everything: six wide-angle views from the centre of the room along the axes
    wide = (20.0, 20.0, 32.0, 24.0)
    centre_views = np.stack([rfn.look_at((0, 0, -1.0), np.array([0, 0, -1.0]) + s * np.eye(3)[a]) for a in range(3)
                             for s in (1, -1)])
    all_seen = mr.cull_to_frustums(Mesh(v, f), centre_views, wide, H, W)
    assert np.array_equal(all_seen.faces, f) and np.array_equal(all_seen.vertices, v)
    # a camera outside the room, facing away from everything
    away = rfn.look_at((0, 0, 5.0), (0, 0, 9.0))[None]
    none = mr.cull_to_frustums(Mesh(v, f), away, K, H, W)
    assert none.faces.shape == (0, 3) and np.array_equal(none.vertices, v)
