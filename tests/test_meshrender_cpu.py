"""CPU tests of the mesh renderer (its header include/monosdf_render.h is held against its table and the Makefile by
tests/test_abi_cpu.py, as every additive header is): the host refusals of every entry point and of
utils/mesh_render.py, the readers, and certificates for the scenes of the GPU tests
(tests/test_gpu_meshrender.py): few exempt pixels, both facings present, and every mutant of the restatements
(tests/render_numpy.py) visible on them."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refuse_numpy as rfn
import render_numpy as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monosdf_amd import _lib                                    # noqa: E402
from monosdf_amd.utils import mesh_render as mrd                # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'render')
K = (50.0, 50.0, 32.0, 24.0)
H, W = 48, 64


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    return _lib.load()


BIG = 2 ** 31


def test_entries_refuse_on_the_host():
    """Every refusal and every zero-work return comes before a launch: there is no GPU here and no pointer is valid."""
    lib = _lib_or_skip()
    p = ctypes.c_void_p(64)                                     # never dereferenced on the host
    assert lib.msdf_rnd_visibility_workspace_bytes(2, 3, 4) == 8 * 24
    assert lib.msdf_rnd_visibility_workspace_bytes(0, 3, 4) == 0
    for sizes in ((-1, 3, 4), (1, BIG, 1), (1, 1, BIG), (BIG, 1, 1), (2, 2 ** 15, 2 ** 15), (1, 2 ** 16, 2 ** 15)):
        assert lib.msdf_rnd_visibility_workspace_bytes(*sizes) == -1, sizes

    def vis(nv=4, nf=1, n=1, h=4, w=4, znear=0.05, zfar=100.0, cull=0, verts=p, out=p):
        return lib.msdf_rnd_visibility(verts, nv, p, nf, p, n, 1.0, 1.0, 0.0, 0.0, h, w, znear, zfar, 0.5, cull, p,
                                       out, p, None)
    assert vis(n=0) == 0 and vis(h=0) == 0 and vis(w=0) == 0
    for kw in (dict(nv=-1), dict(nv=BIG), dict(nf=-1), dict(nf=BIG), dict(n=-1), dict(n=BIG), dict(h=BIG),
               dict(n=2, h=2 ** 15, w=2 ** 15), dict(znear=0.0), dict(znear=-1.0), dict(znear=float('nan')),
               dict(zfar=0.01), dict(cull=-1), dict(cull=3), dict(verts=None), dict(out=None)):
        assert vis(**kw) == 1, kw

    def normals(nv=4, nf=1, verts=p, out=p):
        return lib.msdf_rnd_vertex_normals(verts, nv, p, nf, p, p, out, None)
    assert normals(nv=0) == 0
    for kw in (dict(nv=-1), dict(nv=BIG), dict(nf=-1), dict(nf=BIG // 3 + 1), dict(verts=None), dict(out=None)):
        assert normals(**kw) == 1, kw

    def shade(n=1, h=4, w=4, nv=4, nf=1, face=p, lights=p, nrm=p, flat=0, rgb=p):
        return lib.msdf_rnd_shade(face, p, n, h, w, p, 1.0, 1.0, 0.0, 0.0, 0.5, p, nv, p, nf, nrm, None, 1.0, 1.0, 1.0,
                                  lights, 0.0, 0.0, 0.0, 1.0, flat, 0, rgb, None)
    assert shade(n=0) == 0 and shade(h=0) == 0
    for kw in (dict(n=-1), dict(n=BIG), dict(n=2, h=2 ** 15, w=2 ** 15), dict(nv=-1), dict(nf=BIG), dict(face=None),
               dict(lights=None), dict(nrm=None), dict(rgb=None)):
        assert shade(**kw) == 1, kw

    def l1(n=1, h=4, w=4, a=p, out=p):
        return lib.msdf_rnd_depth_l1(a, p, n, h, w, out, None)
    assert l1(n=0) == 0 and l1(w=0) == 0
    for kw in (dict(n=-1), dict(h=BIG), dict(n=2, h=2 ** 15, w=2 ** 15), dict(a=None), dict(out=None)):
        assert l1(**kw) == 1, kw

    def see(npts=4, n=1, h=4, w=4, pts=p, flags=p, fx=1.0):
        return lib.msdf_rnd_views_see(pts, npts, p, n, fx, 1.0, 0.0, 0.0, h, w, flags, None)
    assert see(n=0) == 0
    for kw in (dict(npts=-1), dict(npts=BIG), dict(n=-1), dict(n=BIG), dict(h=-1), dict(w=BIG), dict(pts=None),
               dict(flags=None), dict(fx=0.0)):
        assert see(**kw) == 1, kw


def test_python_refusals_without_a_gpu():
    v, f = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32)
    poses = np.eye(4)[None]
    with pytest.raises(TypeError, match='cpu'):
        mrd.visibility(v, f, poses, K, H, W)
    with pytest.raises(TypeError, match='cpu'):
        mrd.vertex_normals(v, f)
    with pytest.raises(TypeError, match='cpu'):
        mrd.shade(torch.zeros(1, H, W, dtype=torch.int32), torch.zeros(1, H, W), v, f, poses, K)
    with pytest.raises(TypeError, match='cpu'):
        mrd.depth_l1(torch.zeros(1, H, W), torch.zeros(1, H, W))
    with pytest.raises(TypeError, match='cpu'):
        mrd.views_see(torch.zeros(5, 3), poses, K, H, W)
    with pytest.raises(TypeError, match='cpu'):
        mrd.render_frames((v, f), poses, K, H, W)
    with pytest.raises(ValueError, match='cull'):
        mrd.visibility(v, f, poses, K, H, W, cull='sideways')
    with pytest.raises(ValueError, match='znear'):
        mrd.visibility(v, f, poses, K, H, W, znear=0.0)
    with pytest.raises(ValueError, match='2\\^31'):
        mrd.visibility(v, f, np.stack([np.eye(4)] * 3), K, 2 ** 15, 2 ** 15)
    with pytest.raises(ValueError, match='views_per_call'):
        mrd.render_frames((v, f), poses, K, H, W, views_per_call=0)
    with pytest.raises(ValueError, match='batch'):
        mrd.sample_views((1, 1, 1), np.eye(4), 3, batch=0)


# ---- readers


def test_render_options_defaults_are_the_golden_file():
    golden = mrd.RenderOptions.from_json(os.path.join(GOLDEN, 'render.json'))
    assert golden == mrd.RenderOptions()
    assert golden.cull == 'back' and not golden.mesh_show_back_face
    assert dataclass_replace(golden, mesh_show_back_face=True).cull == 'none'
    table = golden.light_table()
    assert table.dtype == np.float32 and table.shape == (42,)
    assert table[:9].tolist() == [0, 0, 2] + [np.float32(0.7)] * 3 + [np.float32(0.66), np.float32(0.2), 10]
    assert table[27 + 8] == np.float32(0.1) and table[18 + 7] == np.float32(1e-17)
    assert table[36:39].tolist() == [np.float32(0.3)] * 3 and table[39:].tolist() == [1, 1, 1]


def dataclass_replace(obj, **kw):
    import dataclasses
    return dataclasses.replace(obj, **kw)


def test_read_o3d_camera():
    pose, (fx, fy, cx, cy, h, w) = mrd.read_o3d_camera(os.path.join(GOLDEN, 'c1.json'))
    assert (fx, fy, cx, cy, h, w) == (935.30743608719376, 935.30743608719376, 959.5, 539.5, 1080, 1920)
    rot = pose[:3, :3]
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-12) and np.linalg.det(rot) > 0.999
    assert pose[3].tolist() == [0, 0, 0, 1]
    # the file stores the world-to-camera matrix column by column: its last four numbers but one are the translation
    w2c = np.linalg.inv(pose)
    assert np.allclose(w2c[:3, 3], [-0.19424164354647577, 0.21591123421766922, 1.4483504955616819], atol=1e-12)
    assert np.allclose(w2c[0, :3], [0.63562127697331727, 0.087862106970377635, -0.76698490364383032], atol=1e-12)


def test_viewmatrix_and_sample_views_without_a_cloud():
    m = mrd.viewmatrix((0.0, 2.0, 0.0), (0.0, 0.0, -1.0), (1.0, 2.0, 3.0))
    assert np.allclose(m[:3, 2], [0, 1, 0]) and np.allclose(m[:3, 3], [1, 2, 3])
    assert np.allclose(m[:3, 0], np.cross([0, 0, -1.0], [0, 1.0, 0])) and np.allclose(m[:3, 1], [0, 0, -1])
    transform = rfn.pose_from(rfn.random_rotation(np.random.default_rng(1)), (0.5, -1.0, 2.0))
    extents = np.array([1.0, 2.0, 0.5])
    a = mrd.sample_views(extents, transform, 20, seed=3, batch=7)
    b = mrd.sample_views(extents, transform, 20, seed=3, batch=64)
    assert a.shape == (20, 4, 4) and np.array_equal(a, b)
    assert not np.array_equal(a, mrd.sample_views(extents, transform, 20, seed=4))
    local = (a[:, :3, 3] - transform[:3, 3]) @ transform[:3, :3]
    assert (np.abs(local) <= extents / 2 + 1e-12).all()
    rot = a[:, :3, :3]
    assert np.allclose(rot @ rot.transpose(0, 2, 1), np.eye(3), atol=1e-9)
    # the sequence of one generator: candidate 0's six numbers
    r = np.random.default_rng(3).random(6)
    origin = transform[:3, :3] @ ((r[:3] - 0.5) * extents) + transform[:3, 3]
    target = np.round(-1e4 + 2e4 * r[3:], 2)
    assert np.allclose(a[0], mrd.viewmatrix(target - origin, (0, 0, -1.0), origin), atol=1e-12)


def test_render_mesh_help_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_mesh.py'), '--help'],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for word in ('--cameras', '--poses', '--intrinsic', '--size', '--options', '--cull', '--flat'):
        assert word in out.stdout, word


# ---- certificates for the scenes of the GPU tests


@functools.lru_cache(maxsize=None)
def _room(cull='none'):
    v, f, poses = rfn.room_scene(0, 8)
    out = rn.raycast(v, f, poses, K, H, W, cull=cull)
    for a in (v, f, poses) + out:
        a.setflags(write=False)
    return (v, f, poses) + out


def test_room_scene_has_few_exempt_pixels_and_both_facings():
    v, f, poses, depth, face, exempt, back = _room()
    ref_depth, ref_exempt, _ = rfn.raycast(v, f, poses, K, H, W)
    assert np.array_equal(depth, ref_depth)                     # the extension leaves the depth alone
    assert (exempt & ~ref_exempt).sum() == 0                    # no near ties on this scene today
    print('room: %d of %d pixels exempt' % (int(exempt.sum()), exempt.size))
    assert exempt.sum() <= 0.005 * exempt.size
    assert (face >= 0).all() and face.size == 24576
    assert int(back.sum()) == 23930 and int((~back).sum()) == 646
    assert (face[~back] >= 12).all() and (face[back] < 12).all()        # the sphere's fronts, the box's insides
    for cull in ('back', 'front'):
        _, _, _, d, fc, ex, bk = _room(cull)
        assert ex.sum() <= 0.005 * ex.size
        assert not np.array_equal(d, depth)
        assert (bk[fc >= 0] == (cull == 'front')).all()
    # culled back faces: only the sphere's near side is left; culled front faces: the box, and the sphere's far side
    # through its near one
    assert int((_room('back')[4] >= 0).sum()) == 646
    assert (_room('front')[4] >= 0).all()


@functools.lru_cache(maxsize=None)
def _shaded(dtype, **mutant):
    v, f, poses, depth, face, _, _ = _room()
    opts = mrd.RenderOptions()
    centre, extent = rn.light_frame(v)
    return rn.phong(dtype, face, depth.astype(np.float32), rfn.w2c_rows(poses), K, v, f, rn.vertex_normals(v, f),
                    opts.light_table(), centre, extent, base=opts.default_mesh_color, **mutant)


def test_every_mutant_of_the_restatements_shows_on_these_scenes():
    v, f, poses, depth, face, exempt, _ = _room()
    use = ~exempt
    # 1. tie to the larger index: the room with every face listed twice
    f2 = np.concatenate([f, f])
    small = rn.raycast(v, f2, poses[:1], K, H, W)[1]
    large = rn.raycast(v, f2, poses[:1], K, H, W, mutant_tie_largest=True)[1]
    assert (small < len(f)).all() and np.array_equal(small, face[:1]) and np.array_equal(large, small + len(f))
    # 2. cull sign flipped
    flipped = rn.raycast(v, f, poses, K, H, W, cull='back', mutant_cull_flipped=True)
    assert np.array_equal(flipped[1], _room('front')[4]) and not np.array_equal(flipped[1][use], _room('back')[4][use])
    # 3 - 5. the shading rules
    ref = _shaded(np.float64)
    assert ref.min() >= 0 and ref.max() <= 1 and ref[use].std() > 0.01
    for mutant in ('mutant_unnormalised', 'mutant_world_lights', 'mutant_unclamped_specular'):
        diff = np.abs(_shaded(np.float64, **{mutant: True}) - ref)[use].max()
        print('%s: max change %.3g' % (mutant, diff))
        assert diff > 1e-3, mutant
    # 6. > for >= in views_see cannot show on any input: the two differ only at q = z - 1e-5 == 0, where the quotient
    # is +-inf or NaN and fails the strict bounds either way.  What can be pinned is that equivalence, on the point at
    # z = 1e-5 the GPU test uses and on its neighbours, and that the bounds themselves are strict.
    eps = np.float32(1e-5)
    zs = [np.nextafter(eps, np.float32(0)), eps, np.nextafter(eps, np.float32(1))]
    for K0 in (K, (50.0, 50.0, 0.0, 0.0)):
        for xy in (0.0, 1e-7):
            for z in zs:
                pts = np.array([[xy, xy, z]], np.float32)
                got = rn.views_see(pts, np.eye(4)[None], K0, H, W)[0]
                assert got == rn.views_see(pts, np.eye(4)[None], K0, H, W, mutant_strict=True)[0]
                assert not got or z > eps, (K0, xy, z)
    # one step above 1e-5 the quotient is finite: fx x / q = 20 lies inside the frame
    q = float(zs[2] - eps)
    pts = np.array([[20.0 * q / 50.0, 20.0 * q / 50.0, zs[2]]], np.float32)
    assert rn.views_see(pts, np.eye(4)[None], (50.0, 50.0, 0.0, 0.0), H, W)[0]
