"""GPU tests of the mesh renderer (csrc/meshrender.hip, utils/mesh_render.py): visibility against the depth
rasteriser (bitwise) and the fp64 ray-caster, vertex normals, depth L1 and view rejection against their restatements
(exactly), shading against the fp64 restatement, and the depth-L1 evaluation against its stages
(tests/render_numpy.py; the scenes are certified by tests/test_meshrender_cpu.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import refuse_numpy as rfn
import render_numpy as rn
from test_gpu_refuse import _compare_depth

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monosdf_amd.utils import mesh_render as mrd                # noqa: E402
from monosdf_amd.utils import mesh_refuse as mrf                # noqa: E402

K = (50.0, 50.0, 32.0, 24.0)
H, W = 48, 64
CAP = 0.005

# max |fp32 restatement - fp64 restatement| over the non-exempt, non-background pixels of each shaded scene of this
# file, measured on the host with the restated visibility and recorded in profiles/mesh_render_errors.md; the kernel
# may differ from the fp64 restatement by 4 x this (another operation order, the hardware's pow)
SHADE_FP32_ERROR = {'back': 4.618e-07, 'none': 5.963e-07, 'none flat two_sided': 6.582e-07,
                    'front colors two_sided': 7.734e-07, 'quad': 1.899e-07}


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _vis(v, f, poses, K=K, h=H, w=W, **kw):
    d, fc = mrd.visibility(_cuda(v), _cuda(f, np.int32), poses, K, h, w, **kw)
    return d.cpu().numpy(), fc.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(h=H, w=W, cull='none'):
    """The shared scene with the fp64 restatement of one size and cull mode: computed once, read only."""
    v, f, poses = rfn.room_scene(seed=0, n_cameras=8)
    K_ = K if (h, w) == (H, W) else (70.0, 70.0, w / 2.0, h / 2.0)
    out = rn.raycast(v, f, poses, K_, h, w, cull=cull)
    for a in (v, f, poses) + out:
        a.setflags(write=False)
    return (v, f, poses, K_) + out


def _compare_faces(label, face, ref_face, exempt):
    n_exempt = int(exempt.sum())
    wrong = int((face != ref_face)[~exempt].sum())
    print('%s: %d of %d pixels exempt, %d faces differ outside them' % (label, n_exempt, exempt.size, wrong))
    assert n_exempt <= CAP * exempt.size
    assert wrong == 0


# ---- visibility


@pytest.mark.parametrize('n', [1, 3, 8])
def test_depth_is_bitwise_the_depth_rasterisers(n):
    v, f, poses = _scene()[:3]
    depth, face = mrd.visibility(_cuda(v), _cuda(f, np.int32), poses[:n], K, H, W)
    ref = mrf.render_depth(_cuda(v), _cuda(f, np.int32), poses[:n], K, H, W)
    assert depth.shape == (n, H, W) and depth.dtype == torch.float32 and face.dtype == torch.int32
    assert torch.equal(depth, ref)
    assert torch.equal(face >= 0, depth > 0) and int(face.max()) < len(f)


def test_depth_is_bitwise_the_depth_rasterisers_off_the_lane_grid():
    v, f, poses, K_ = _scene(70, 90, 'back')[:4]
    depth, _ = mrd.visibility(_cuda(v), _cuda(f, np.int32), poses, K_, 70, 90, znear=0.1, zfar=3.0, pixel_center=0.25)
    ref = mrf.render_depth(_cuda(v), _cuda(f, np.int32), poses, K_, 70, 90, znear=0.1, zfar=3.0, pixel_center=0.25)
    assert torch.equal(depth, ref) and (depth == 0).any() and (depth > 0).any()


@pytest.mark.parametrize('h,w,cull', [(H, W, 'none'), (H, W, 'back'), (H, W, 'front'), (70, 90, 'back')])
def test_face_and_depth_equal_the_fp64_raycaster(h, w, cull):
    v, f, poses, K_, ref_depth, ref_face, exempt, _ = _scene(h, w, cull)
    depth, face = _vis(v, f, poses, K_, h, w, cull=cull)
    label = 'room %dx%d cull=%s' % (h, w, cull)
    _compare_faces(label, face, ref_face, exempt)
    _compare_depth(label, depth, ref_depth, exempt)
    if cull == 'back':
        assert (face[face >= 0] >= 12).all() and (face < 0).any()       # the sphere only: the box is seen from inside
    if cull == 'front':
        assert (face >= 0).all()


def test_faces_listed_twice_report_the_first_copy():
    v, f, poses = _scene()[:3]
    base = _vis(v, f, poses)
    twice = _vis(v, np.concatenate([f, f]), poses)
    assert (twice[1] < len(f)).all()
    assert np.array_equal(twice[0], base[0]) and np.array_equal(twice[1], base[1])


def test_face_permutation_and_winding():
    v, f, poses, _, _, _, exempt, _ = _scene()
    base_d, base_f = _vis(v, f, poses)
    perm = np.random.default_rng(5).permutation(len(f))
    d, fc = _vis(v, f[perm], poses)                                     # new face k is old face perm[k]
    assert np.array_equal(d, base_d)
    assert np.array_equal(perm[fc][~exempt], base_f[~exempt])           # exact ties (exempt: on shared edges) may differ
    flipped = f[:, ::-1]
    for a, b in (('back', 'front'), ('front', 'back'), ('none', 'none')):
        da, fa = _vis(v, f, poses, cull=a)
        db, fb = _vis(v, flipped, poses, cull=b)
        assert np.array_equal(da, db) and np.array_equal(fa, fb), (a, b)
    assert not np.array_equal(_vis(v, f, poses, cull='back')[0], _vis(v, f, poses, cull='front')[0])


def test_triangle_across_the_near_plane():
    v = np.array([[-3, 1, -2], [3, 1, -2], [3, 1, 10], [-3, 1, 10]], np.float32).astype(np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    pose = np.eye(4)[None]
    for cull in ('none', 'back', 'front'):
        ref_depth, ref_face, exempt, back = rn.raycast(v, f, pose, K, H, W, cull=cull)
        depth, face = _vis(v, f, pose, cull=cull)
        _compare_faces('ground ' + cull, face, ref_face, exempt)
        _compare_depth('ground ' + cull, depth, ref_depth, exempt)
    seen = {c: int((_vis(v, f, pose, cull=c)[1] >= 0).sum()) for c in ('none', 'back', 'front')}
    assert seen['none'] > 500 and sorted((seen['back'], seen['front'])) == [0, seen['none']]


def test_degenerate_and_out_of_range_faces_change_nothing():
    v, f, poses = _scene()[:3]
    base = _vis(v, f, poses)
    extra_v = np.array([[0.125] * 3, [0.25] * 3, [0.375] * 3])
    v2, n = np.concatenate([v, extra_v]), len(v)
    f2 = np.concatenate([f, [[n, n + 1, n + 2], [n, n, n + 1], [n + 2, n + 2, n + 2], [0, 5, 0]]])
    got = _vis(v2, f2, poses)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    # an index outside [0, V) is refused by the Python layer; the kernel itself skips such a face
    with pytest.raises(ValueError, match='face index'):
        _vis(v, np.concatenate([f, [[0, 1, len(v)]]]), poses)
    f3 = np.concatenate([f, [[0, 1, len(v)], [-1, 2, 3], [2 ** 31 - 1, 1, 2]]])
    w2c = _cuda(rfn.w2c_rows(poses).reshape(-1, 12))
    raw = mrd._visibility(_cuda(v), _cuda(f3, np.int32), w2c, K, H, W, 0.05, 100.0, 0.5, 0)
    assert np.array_equal(raw[0].cpu().numpy(), base[0]) and np.array_equal(raw[1].cpu().numpy(), base[1])


def test_empty_face_list_and_repeatability():
    v, f, poses = _scene()[:3]
    depth, face = _vis(v, np.zeros((0, 3), np.int64), poses)
    assert depth.shape == (8, H, W) and not depth.any() and (face == -1).all()
    for cull in ('none', 'back'):
        a, b = _vis(v, f, poses, cull=cull), _vis(v, f, poses, cull=cull)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- vertex normals


def _fan(n):
    """n faces round vertex 0, not planar, so the order of the sum shows."""
    rng = np.random.default_rng(11)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.3 * rng.normal(size=n)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(np.float32).astype(np.float64)
    f = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)])
    return v, f


def _normal_cases():
    room = rfn.room_scene(0, 1)[:2]
    ico = rfn.icosphere(2, 0.5, (0.3, -0.2, 0.8))
    fan = _fan(70)
    v, f = rfn.icosphere(0, 1.0, (0, 0, 0))
    odd = (np.concatenate([v, [[5.0, 5.0, 5.0]], [[0.1, 0.2, 0.3]]]),            # an isolated vertex, a vertex of
           np.concatenate([f, [[0, 0, 1], [13, 13, 13], [2, 13, 2]]]))           # degenerate faces only
    return {'icosphere': ico, 'room': room, 'fan70': fan, 'isolated_and_degenerate': odd}


@pytest.mark.parametrize('case', ['icosphere', 'room', 'fan70', 'isolated_and_degenerate'])
def test_vertex_normals_equal_the_fp64_restatement(case):
    v, f = _normal_cases()[case]
    got = mrd.vertex_normals(_cuda(v), _cuda(f, np.int32)).cpu().numpy()
    ref = rn.vertex_normals(v, f)
    assert got.dtype == np.float32 and got.shape == (len(v), 3)
    assert np.array_equal(got, ref)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    if case == 'isolated_and_degenerate':
        assert got[12].tolist() == [0, 0, 1] and got[13].tolist() == [0, 0, 1]
    if case == 'fan70':
        assert (f == 0).sum() == 70


# ---- shading


def _shade_case(cull, **kw):
    v, f, poses = _scene()[:3]
    exempt = _scene(H, W, cull)[6]
    vc, fc = _cuda(v), _cuda(f, np.int32)
    depth, face = mrd.visibility(vc, fc, poses, K, H, W, cull=cull)
    opts = mrd.RenderOptions()
    normals = mrd.vertex_normals(vc, fc)
    colors = kw.pop('colors', None)
    rgb = mrd.shade(face, depth, vc, fc, poses, K, normals=normals, options=opts, base_color=opts.default_mesh_color,
                    vertex_colors=None if colors is None else _cuda(colors), **kw).cpu().numpy()
    centre, extent = rn.light_frame(v)
    args = (face.cpu().numpy(), depth.cpu().numpy(), rfn.w2c_rows(poses), K, v, f, normals.cpu().numpy(),
            opts.light_table(), centre, extent)
    ref = rn.phong(np.float64, *args, base=opts.default_mesh_color, colors=colors, **kw)
    f32 = rn.phong(np.float32, *args, base=opts.default_mesh_color, colors=colors, **kw)
    return rgb, ref, f32, face.cpu().numpy(), exempt


@pytest.mark.parametrize('cull,kw', [('back', {}), ('none', {}), ('none', dict(flat=True, two_sided=True)),
                                     ('front', dict(colors=True, two_sided=True))])
def test_shade_equals_the_fp64_restatement(cull, kw):
    kw = dict(kw)
    if kw.get('colors'):
        kw['colors'] = np.random.default_rng(4).uniform(0, 1, (len(_scene()[0]), 3)).astype(np.float32)
    rgb, ref, f32, face, exempt = _shade_case(cull, **kw)
    assert rgb.shape == (8, H, W, 3) and rgb.dtype == np.float32
    assert exempt.sum() <= CAP * exempt.size
    hit = face >= 0
    assert np.array_equal(rgb[~hit], np.ones_like(rgb[~hit]))                    # background: exactly render.json's white
    use = hit & ~exempt
    err = np.abs(rgb.astype(np.float64) - ref)[use].max()
    measured = np.abs(f32.astype(np.float64) - ref)[use].max()
    tol = 4 * SHADE_FP32_ERROR[' '.join([cull] + sorted(kw))]
    print('shade cull=%s %s: max |gpu - fp64| = %.3g, max |fp32 - fp64| = %.3g here, bound %.3g' %
          (cull, sorted(kw), err, measured, tol))
    assert ref[use].std() > 0.01
    assert err <= tol


def test_shade_of_a_fronto_parallel_quad_has_its_closed_form():
    """A quad at camera z = D seen head-on from the origin, normals toward the camera; the pixel on the optical axis has
    P = (0, 0, D), e = -N = (0, 0, 1) ... so for every light e . R = N . l = (D - L.z) / |L - P|."""
    D = 2.0
    v = np.array([[-3, -3, D], [3, -3, D], [3, 3, D], [-3, 3, D]], np.float64)
    f = np.array([[0, 2, 1], [0, 3, 2]])                                          # normal (0, 0, -1): front faces
    Kq, h, w = (50.0, 50.0, 32.5, 24.5), 49, 65
    vc, fc = _cuda(v), _cuda(f, np.int32)
    pose = np.eye(4)[None]
    depth, face = mrd.visibility(vc, fc, pose, Kq, h, w, cull='back')
    assert (face >= 0).all() and (depth == 2.0).all()
    opts = mrd.RenderOptions()
    normals = mrd.vertex_normals(vc, fc)
    assert np.array_equal(normals.cpu().numpy(), np.tile(np.float32([0, 0, -1]), (4, 1)))
    rgb = mrd.shade(face, depth, vc, fc, pose, Kq, normals=normals, options=opts, base_color=(0.7, 0.7, 0.7))
    got = rgb[0, 24, 32].cpu().numpy().astype(np.float64)
    centre, extent = np.array([0.0, 0.0, D]), 6.0
    diffuse, specular = 0.3, 0.0
    for p, kd, ks, s in zip(opts.light_position, opts.light_diffuse_power, opts.light_specular_power,
                            opts.light_specular_shininess):
        L = centre + extent * np.array([p[0], -p[1], -p[2]])                      # identity pose: right, -down, -forward
        to = L - np.array([0.0, 0.0, D])
        cos = min(max(-to[2] / np.linalg.norm(to), 0.0), 1.0)
        diffuse += kd * cos * 0.7
        specular += ks * (cos ** s if cos > 0 else 0.0) * 0.7
    expect = min(max(0.7 * diffuse + specular, 0.0), 1.0)
    print('quad: centre pixel %s, closed form %.9g' % (got.tolist(), expect))
    tol = 4 * SHADE_FP32_ERROR['quad']
    assert np.abs(got - expect).max() <= tol
    # the whole image against the restatement, and the frames as bytes
    ref = rn.phong(np.float64, face.cpu().numpy(), depth.cpu().numpy(), rfn.w2c_rows(pose), Kq, v, f,
                   normals.cpu().numpy(), opts.light_table(), (0.0, 0.0, D), 6.0, base=(0.7, 0.7, 0.7))
    err = np.abs(rgb.cpu().numpy() - ref).max()
    print('quad: max |gpu - fp64| = %.3g, bound %.3g' % (err, tol))
    assert err <= tol
    frames = mrd.render_frames((vc, fc), pose, Kq, h, w, base_color=(0.7, 0.7, 0.7), views_per_call=1)
    assert frames.dtype == torch.uint8 and frames.shape == (1, h, w, 3)
    assert torch.equal(frames, torch.floor(rgb.clamp(0, 1) * 255 + 0.5).to(torch.uint8))


# ---- depth L1 and view rejection


@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (1, 63, 65), (3, 63, 65), (3, 48, 64)])
def test_depth_l1_equals_numpy(n, h, w):
    """Values that are multiples of 2^-10 below 16: every difference and every order of the sum is exact."""
    rng = np.random.default_rng(n * 1000 + h)
    a = (rng.integers(0, 2 ** 14, (n, h, w)) / 1024.0).astype(np.float32)
    b = (rng.integers(0, 2 ** 14, (n, h, w)) / 1024.0).astype(np.float32)
    b[0, 0, 0] = a[0, 0, 0]
    got = mrd.depth_l1(_cuda(a), _cuda(b)).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (n,)
    assert np.array_equal(got, rn.depth_l1(a, b))
    assert not mrd.depth_l1(_cuda(a), _cuda(a)).cpu().numpy().any()


def _see(points, poses, K_, h, w):
    return mrd.views_see(_cuda(points), poses, K_, h, w).cpu().numpy()


@pytest.mark.parametrize('size', [1, 64, 65, 5000])
def test_views_see_equals_the_fp32_restatement(size):
    v, _, poses = _scene()[:3]
    rng = np.random.default_rng(size)
    # a cloud in a corner of the room: some cameras see it, some do not
    pts = rng.uniform((1.2, 0.9, 1.2), (1.9, 1.4, 1.9), (size, 3)).astype(np.float32)
    ref = rn.views_see(pts, poses, K, H, W)
    got = _see(pts, poses, K, H, W)
    assert got.dtype == bool and np.array_equal(got, ref)
    if size >= 64:
        assert ref.any() and not ref.all()
    # one point on a bound, at the end of a cloud of points behind the camera; fx = fy = 1, cx = cy = 0, 32 x 64:
    # q = fl(z - 1e-5); x = 64 q and y = 32 q are exact, so u == width or v == height exactly; x = 0 gives u == 0
    Kb, hb, wb = (1.0, 1.0, 0.0, 0.0), 32, 64
    z = np.float32(1.5)
    q = np.float32(z - np.float32(1e-5))
    inside = [np.float32(8) * q, np.float32(8) * q, z]
    cases = {'inside': (inside, True), 'u == 0': ([0.0, inside[1], z], False), 'v == 0': ([inside[0], 0.0, z], False),
             'u == W': ([np.float32(64) * q, inside[1], z], False), 'v == H': ([inside[0], np.float32(32) * q, z], False),
             'z == 1e-5': ([0.0, 0.0, np.float32(1e-5)], False), 'z == 1e-5, off axis': ([1e-7, 1e-7, np.float32(1e-5)], False),
             'just inside W': ([np.nextafter(np.float32(64) * q, np.float32(0)), inside[1], z], True)}
    behind = rng.uniform((-1, -1, -3), (1, 1, -1), (size - 1, 3)).astype(np.float32)
    for label, (p, expect) in cases.items():
        cloud = np.concatenate([behind, np.array([p], np.float32)])
        ref = rn.views_see(cloud, np.eye(4)[None], Kb, hb, wb)
        assert ref.tolist() == [expect], label
        assert _see(cloud, np.eye(4)[None], Kb, hb, wb).tolist() == [expect], label


def test_sample_views_reject_what_sees_the_unseen_cloud():
    rng = np.random.default_rng(2)
    unseen = rng.uniform((1.5, -1.4, -1.9), (1.9, 1.4, 1.9), (300, 3)).astype(np.float32)     # along the wall x = 2
    extents, transform = np.array([1.0, 1.0, 2.0]), np.eye(4)
    Ks, size = (30.0, 30.0, 19.5, 19.5), 40
    a = mrd.sample_views(extents, transform, 12, unseen=_cuda(unseen), seed=1, batch=7, K=Ks, height=size, width=size)
    b = mrd.sample_views(extents, transform, 12, unseen=unseen, seed=1, batch=64, K=Ks, height=size, width=size)
    assert a.shape == (12, 4, 4) and np.array_equal(a, b)
    assert not _see(unseen, a, Ks, size, size).any() and not rn.views_see(unseen, a, Ks, size, size).any()
    free = mrd.sample_views(extents, transform, 12, seed=1, batch=5)
    assert _see(unseen, free, Ks, size, size).any()                     # without the cloud some of the first 12 see it
    kept = [p for p in free if not rn.views_see(unseen, p[None], Ks, size, size)[0]]
    assert np.array_equal(np.stack(kept), a[:len(kept)])                # the accepted ones keep candidate order


def test_evaluate_depth_l1_is_the_composition_of_its_stages():
    from monosdf_amd.utils.mesh import Mesh
    v, f, _ = _scene()[:3]
    moved = v + [0.0, 0.0, 0.01]
    size, n = 40, 6
    got = mrd.evaluate_depth_l1(Mesh(moved, f), Mesh(v, f), n_imgs=n, seed=3, size=size)
    gv, gf, rv = _cuda(v), _cuda(f, np.int32), _cuda(moved)
    extents, transform = mrd.interior_view_box((gv, gf))
    Ke = (300.0, 300.0, size / 2 - 0.5, size / 2 - 0.5)
    poses = mrd.sample_views(extents, transform, n, seed=3)
    near = 0.01 * 4.0                                                   # the room is 4 x 3 x 4
    m32 = moved.astype(np.float32).astype(np.float64)                   # the moved room's own extent, as fp32 holds it
    near_moved = 0.01 * float((m32.max(0) - m32.min(0)).max())
    dg = mrf.render_depth(gv, gf, poses, Ke, size, size, znear=near, zfar=20.0)
    dr = mrf.render_depth(rv, gf, poses, Ke, size, size, znear=near_moved, zfar=20.0)
    by_hand = float(mrd.depth_l1(dg, dr).mean().item() * 100.0)
    print('depth L1 of the room moved 1 cm: %.6f cm over %d views' % (got, n))
    assert got == by_hand and 0.0 < got < 2.0
    assert np.array_equal(mrd.depth_l1(dg, dr).cpu().numpy(), rn.depth_l1(dg.cpu().numpy(), dr.cpu().numpy()))
    assert mrd.evaluate_depth_l1(Mesh(v, f), Mesh(v, f), n_imgs=n, seed=3, size=size) == 0.0
    assert mrd.evaluate_depth_l1((gv, gf), (gv, gf), n_imgs=n, seed=3, size=size, align=True) < 1e-3


def test_depth_l1_of_a_plane_moved_along_its_normal():
    """One plane z = 0 seen from a box above it; the same plane 1 cm higher.  A ray d (camera frame, d.z = 1) meets
    the plane n . x = c at depth (c - n . o) / (n_c . d) with n_c the normal in the camera frame, so moving the plane
    by delta changes every depth that is hit by delta / |n_c . d|; a ray that misses (looking up, or past zfar) reads
    0 in both.  Tolerance: the project's 1e-4 of the depths, as the mean of the hand-derived images."""
    delta, size, n, zfar, znear = 0.01, 40, 6, 20.0, 0.05
    v = np.array([[-50, -50, 0], [50, -50, 0], [50, 50, 0], [-50, 50, 0]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    box = (np.array([1.0, 1.0, 0.5]), rfn.pose_from(np.eye(3), (0.0, 0.0, 1.0)))
    got = mrd.evaluate_depth_l1((_cuda(v + [0, 0, delta]), _cuda(f, np.int32)), (_cuda(v), _cuda(f, np.int32)),
                                n_imgs=n, seed=5, size=size, zfar=zfar, znear=znear, view_box=box)
    poses = mrd.sample_views(*box, n, seed=5)
    rows = rfn.w2c_rows(poses).astype(np.float64)
    c = size / 2 - 0.5
    jj, ii = np.meshgrid(np.arange(size), np.arange(size))
    d = np.stack([(jj + 0.5 - c) / 300.0, (ii + 0.5 - c) / 300.0, np.ones((size, size))], -1)
    images = []
    for height in (0.0, delta):
        per_view = []
        for m in rows:
            n_c = m[:, 2]                                               # R (0, 0, 1)
            origin_term = height * 1.0 + (n_c @ m[:, 3])                # n_c . (R x + t) for a point of the plane
            z = origin_term / (d @ n_c)
            per_view.append(np.where((z >= znear) & (z <= zfar), z, 0.0))
        images.append(np.stack(per_view))
    assert (images[0] > 0).mean() > 0.2
    expect = np.abs(images[0] - images[1]).mean(axis=(1, 2)).mean() * 100.0
    tol = 1e-4 * 2 * images[0].mean() * 100.0
    print('plane moved 1 cm: depth L1 %.6f cm, by hand %.6f cm, tolerance %.3g' % (got, expect, tol))
    assert expect > 0.5 and abs(got - expect) <= tol
