"""CPU tests of the mesh re-fusion: the ABI table, the refusals of utils/mesh_refuse.py, the numpy restatements
(tests/refuse_numpy.py) on hand-computable inputs, the pose readers and the command line."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import refuse_numpy as rfn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_ENTRIES = ('msdf_raster_depth', 'msdf_tsdf_integrate', 'msdf_tsdf_face_keep', 'msdf_cull_vertices')
K = (50.0, 50.0, 32.0, 24.0)


def test_new_entries_declared_in_header_and_table():
    from monosdf_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'monosdf_hip.h')).read()
    declared = set(re.findall(r'^(?:int|int64_t) (msdf_\w+)\(', text, flags=re.M))
    new = [n for n in _lib.exported_symbols() if n.startswith(('msdf_raster_', 'msdf_tsdf_', 'msdf_cull_'))]
    assert sorted(new) == sorted(NEW_ENTRIES)
    for name in new:
        assert name in declared, name
    assert '#define MSDF_ABI_VERSION 8' in text and _lib.ABI_VERSION == 8
    srcs = [l for l in open(os.path.join(ROOT, 'monosdf_amd', 'csrc', 'Makefile')) if l.startswith('SRCS =')]
    assert 'refuse.hip' in srcs[0].split()


def test_library_exports_the_new_entries():
    from monosdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    # argument errors are refused on the host, before any launch
    assert lib.msdf_raster_depth(None, ctypes.c_int64(0), None, ctypes.c_int64(0), None, 1, ctypes.c_float(1),
                                 ctypes.c_float(1), ctypes.c_float(0), ctypes.c_float(0), 0, 0, ctypes.c_float(0.05),
                                 ctypes.c_float(100), ctypes.c_float(0.5), None, None) == 1


def _mesh():
    from monosdf_amd.utils.mesh import Mesh
    v, f = rfn.icosphere(0, 0.5, (0, 0, 0))
    return Mesh(v, f)


def test_refusals_without_a_gpu():
    from monosdf_amd.utils import mesh_refuse as mr
    from monosdf_amd.utils.mesh import Mesh
    mesh = _mesh()
    poses = np.eye(4)[None]
    v, f = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32)
    # a CPU tensor: there is no CPU path
    with pytest.raises(TypeError, match='cpu'):
        mr.render_depth(v, f, poses, K, 48, 64)
    with pytest.raises(TypeError, match='cpu'):
        mr.tsdf_integrate(torch.zeros(1, 48, 64), poses, K, (0, 0, 0), (4, 4, 4), 0.05, 0.15)
    with pytest.raises(TypeError, match='cpu'):
        mr.tsdf_face_keep(v, f, torch.ones(4, 4, 4))
    with pytest.raises(TypeError, match='cpu'):
        mr.extract_mesh(torch.zeros(4, 4, 4), torch.ones(4, 4, 4), (0, 0, 0), 0.05)
    with pytest.raises(TypeError, match='cpu'):
        mr.seen_vertices(v, poses, K, 48, 64)
    with pytest.raises(TypeError, match='cpu'):
        mr.refuse((v, f), poses, K, 48, 64)
    with pytest.raises(TypeError, match='cpu'):
        mr.cull_to_frustums((v, f), poses, K, 48, 64)
    with pytest.raises(TypeError, match='CUDA'):
        mr.render_depth(np.zeros((4, 3), np.float32), f, poses, K, 48, 64)
    # wrong dtype or shape
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        mr.refuse((np.zeros((4, 2)), mesh.faces), poses, K, 48, 64)
    with pytest.raises(ValueError, match='integer'):
        mr.refuse((mesh.vertices, mesh.faces.astype(np.float64)), poses, K, 48, 64)
    with pytest.raises(ValueError, match='integer'):
        mr.cull_to_frustums((mesh.vertices, mesh.faces[:, :2]), poses, K, 48, 64)
    with pytest.raises(ValueError, match=r'\[n, 4, 4\]'):
        mr.refuse(mesh, np.eye(3)[None], K, 48, 64)
    with pytest.raises(ValueError, match='K must be'):
        mr.refuse(mesh, poses, (1.0, 2.0, 3.0), 48, 64)
    with pytest.raises(ValueError, match='image'):
        mr.refuse(mesh, poses, K, 0, 64)
    # faces out of range
    bad = mesh.faces.copy()
    bad[3, 1] = len(mesh.vertices)
    for faces in (bad, -mesh.faces - 1):
        with pytest.raises(ValueError, match='face index'):
            mr.refuse(Mesh(mesh.vertices, faces), poses, K, 48, 64)
        with pytest.raises(ValueError, match='face index'):
            mr.cull_to_frustums(Mesh(mesh.vertices, faces), poses, K, 48, 64)
    # a non-finite pose, an empty list of views
    for value in (np.nan, np.inf):
        p = poses.copy()
        p[0, 1, 3] = value
        with pytest.raises(ValueError, match='non-finite pose'):
            mr.refuse(mesh, p, K, 48, 64)
        with pytest.raises(ValueError, match='non-finite pose'):
            mr.cull_to_frustums(mesh, p, K, 48, 64)
    with pytest.raises(ValueError, match='empty'):
        mr.refuse(mesh, np.zeros((0, 4, 4)), K, 48, 64)
    with pytest.raises(ValueError, match='empty'):
        mr.cull_to_frustums(mesh, np.zeros((0, 4, 4)), K, 48, 64)
    # voxel_length <= 0
    for vl in (0.0, -0.01, float('nan')):
        with pytest.raises(ValueError, match='voxel_length'):
            mr.refuse(mesh, poses, K, 48, 64, voxel_length=vl)
    with pytest.raises(ValueError, match='sdf_trunc'):
        mr.refuse(mesh, poses, K, 48, 64, sdf_trunc=0.0)
    with pytest.raises(ValueError, match='block'):
        mr.refuse(mesh, poses, K, 48, 64, block=0)
    with pytest.raises(ValueError, match='view_chunk'):
        mr.refuse(mesh, poses, K, 48, 64, view_chunk=0)


def test_fusion_grid_and_blocks():
    from monosdf_amd.utils import mesh_refuse as mr
    origin, dims = mr.fusion_grid((-0.5, -0.5, -0.5), (0.5, 0.5, 0.25), 0.02)
    pad = float(np.float32(3 * np.float32(0.02))) + float(np.float32(0.02))
    assert np.allclose(origin, -0.5 - pad, atol=1e-12)
    vl = float(np.float32(0.02))
    assert dims == tuple(int(np.ceil((e + 2 * pad) / vl)) for e in (1.0, 1.0, 0.75))
    # blocks of at most `block` cells that share one layer of voxels cover every cell once
    for n, block in ((58, 16), (17, 16), (2, 512), (33, 16), (100, 7)):
        blocks = mr._block_starts(n, block)
        cells = [c for s, m in blocks for c in range(s, s + m - 1)]
        assert cells == list(range(n - 1)), (n, block)
        assert all(2 <= m <= block + 1 for _, m in blocks)
        assert all(b[0] == a[0] + a[1] - 1 for a, b in zip(blocks, blocks[1:]))


def test_raycaster_fronto_parallel_quad_has_plane_depth():
    """A quad at camera z = D seen head-on: the depth is D on every pixel it covers, not D / cos."""
    D = 2.0
    v = np.array([[-1, -0.71, D], [1, -0.71, D], [1, 0.71, D], [-1, 0.71, D]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    depth, exempt, grazing = rfn.raycast(v, f, np.eye(4)[None], K, 48, 64)
    jj, ii = np.meshgrid(np.arange(64), np.arange(48))
    x, y = (jj + 0.5 - 32.0) / 50.0 * D, (ii + 0.5 - 24.0) / 50.0 * D
    inside = (np.abs(x) < 1) & (np.abs(y) < 0.71)
    assert inside.sum() > 1000 and (~inside).sum() > 100
    assert np.array_equal(depth[0] > 0, inside)
    assert np.abs(depth[0][inside] - D).max() < 1e-12
    assert not grazing.any()
    assert not exempt.any()                    # no pixel centre lies on the outline or on the diagonal (71 (2a + 1) is odd)
    # the same quad seen from a moved and turned camera keeps its distance along the camera's axis
    pose = rfn.look_at((0.2, -0.1, -1.0), (0.2, -0.1, D))
    depth2, _, _ = rfn.raycast(v, f, pose[None], K, 48, 64)
    assert np.abs(depth2[depth2 > 0] - (D + 1.0)).max() < 1e-6          # the world-to-camera rows are fp32
    # behind the camera, beyond zfar, nearer than znear: nothing
    assert not rfn.raycast(v, f, np.eye(4)[None], K, 48, 64, zfar=1.5)[0].any()
    assert not rfn.raycast(v, f, np.eye(4)[None], K, 48, 64, znear=2.5)[0].any()
    assert not rfn.raycast(v * [1, 1, -1], f, np.eye(4)[None], K, 48, 64)[0].any()


def test_tsdf_restatement_on_a_constant_depth_map():
    """One camera at the origin looking along +z, depth 1 everywhere, 4 x 4 x 4 voxels of 0.1 around the axis from
    z = 0.7: voxel (i, j, k) has p.z = 0.75 + 0.1 k, and close to the axis s = (1 - p.z) |ray| with |ray| within 3e-5
    of 1.  Truncation 0.2: tau = (0.25 - 0.1 k) / 0.2 = 1 (clipped), 0.75, 0.25, -0.25."""
    Kc = (100.0, 100.0, 32.0, 24.0)
    depth = np.ones((1, 48, 64), np.float32)
    origin, dims = (-0.2, -0.2, 0.7), (4, 4, 4)
    tsdf, w, exempt = rfn.tsdf_fp32(depth, np.eye(4)[None], Kc, origin, dims, 0.1, 0.2)
    assert tsdf.dtype == np.float32 and w.dtype == np.float32 and tsdf.shape == dims
    assert (w == 1).all()
    # |ray|: the voxel centres are at x, y = +-0.05, +-0.15 and project to within 0.15 / 0.75 * 100 = 20 px of the centre
    expect = np.array([1.0, 0.75, 0.25, -0.25])
    for k in range(4):
        ray = np.sqrt(1 + 2 * (0.15 / (0.75 + 0.1 * k) + 0.005) ** 2)       # the longest ray of the layer (half a pixel of slack)
        lo, hi = sorted((expect[k], expect[k] * ray))
        assert (tsdf[:, :, k] >= min(lo, 1.0) - 1e-6).all() and (tsdf[:, :, k] <= min(hi, 1.0) + 1e-6).all(), k
    assert (tsdf[:, :, 0] == 1.0).all()
    # the voxel at (-0.05, -0.05, 0.85) projects to (32 - 5.88 + 0.5, 24 - 5.88 + 0.5) -> pixel (26, 18)
    s = (1 - 0.85) * np.sqrt(((26 - 32) / 100) ** 2 + ((18 - 24) / 100) ** 2 + 1)
    assert abs(tsdf[1, 1, 1] - s / 0.2) < 1e-6
    # a second, identical view: the running mean stays, the weight counts
    tsdf2, w2, _ = rfn.tsdf_fp32(np.ones((2, 48, 64), np.float32), np.stack([np.eye(4)] * 2), Kc, origin, dims, 0.1, 0.2)
    assert (w2 == 2).all() and np.abs(tsdf2 - tsdf).max() < 1e-6
    # depth beyond the cut, no depth, and a surface more than the truncation in front of the voxel: untouched
    assert (rfn.tsdf_fp32(depth, np.eye(4)[None], Kc, origin, dims, 0.1, 0.2, depth_trunc=0.9)[1] == 0).all()
    assert (rfn.tsdf_fp32(depth * 0, np.eye(4)[None], Kc, origin, dims, 0.1, 0.2)[1] == 0).all()
    t3, w3, _ = rfn.tsdf_fp32(depth * 0.7, np.eye(4)[None], Kc, origin, dims, 0.1, 0.2)
    assert (w3[:, :, 0] == 1).all() and (w3[:, :, 1] == 1).all() and (w3[:, :, 2:] == 0).all() and (t3[:, :, 2:] == 0).all()
    # behind the camera
    back = rfn.look_at((0, 0, 0), (0, 0, -1))
    assert (rfn.tsdf_fp32(depth, back[None], Kc, origin, dims, 0.1, 0.2)[1] == 0).all()


def test_face_rule_restatement():
    w = np.ones((3, 3, 3), np.float32)
    w[2, 2, 2] = 0
    v = np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5],          # inside cell (0,0,0)
                  [1.5, 2, 2], [2, 1.5, 2], [2, 2, 1.5],          # inside cell (1,1,1), whose corner (2,2,2) is unseen
                  [1, 0.5, 0], [1, 1, 0.5], [1, 0, 0.5]])         # in the lattice plane x = 1 of cell (., 0, 0)
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    assert rfn.face_keep(v, f, w).tolist() == [True, False, True]
    w[1, 1, 1] = 0
    assert rfn.face_keep(v, f, w).tolist() == [False, False, False]


def test_frustum_restatement():
    pts = np.array([[0, 0, 1], [0.63, 0, 1], [0.65, 0, 1], [0, -0.47, 1], [0, -0.49, 1], [0, 0, -1], [0, 0, 0]],
                   np.float64)
    seen, exempt = rfn.seen_fp32(pts, np.eye(4)[None], K, 48, 64)
    assert seen.tolist() == [True, True, False, True, False, False, False]
    assert not exempt[:6].any()
    away = rfn.look_at((0, 0, 0), (0, 0, -1))
    assert rfn.seen_fp32(pts, away[None], K, 48, 64)[0].tolist() == [False] * 5 + [True, False]
    assert rfn.seen_fp32(pts, np.stack([np.eye(4), away]), K, 48, 64)[0].tolist() == [True, True, False, True, False,
                                                                                     True, False]


def test_pose_readers(tmp_path):
    from monosdf_amd.utils import mesh_refuse as mr
    rng = np.random.default_rng(3)
    a, b = rfn.pose_from(rfn.random_rotation(rng), (1, 2, 3)), rfn.pose_from(rfn.random_rotation(rng), (-4, 5, 6))
    traj = tmp_path / 'traj.txt'
    traj.write_text('\n'.join(' '.join(repr(float(x)) for x in m.reshape(-1)) for m in (a, b)) + '\n')
    got = mr.read_poses(str(traj))
    assert got.shape == (2, 4, 4) and np.array_equal(got, np.stack([a, b]))
    assert np.array_equal(mr.read_poses(str(traj), every=2), a[None])
    d = tmp_path / 'pose'
    d.mkdir()
    for name, m in (('10.txt', a), ('9.txt', b)):                 # sorted by number: 9 before 10
        (d / name).write_text('\n'.join(' '.join(repr(float(x)) for x in row) for row in m) + '\n')
    (d / 'notes.md').write_text('not a pose')
    got = mr.read_poses(str(d))
    assert np.array_equal(got, np.stack([b, a]))
    lost = a.copy()
    lost[:] = -np.inf
    (d / '11.txt').write_text('\n'.join(' '.join('-inf' for _ in row) for row in lost) + '\n')
    assert mr.read_poses(str(d)).shape == (2, 4, 4)               # a lost frame is left out
    k = tmp_path / 'intrinsic_color.txt'
    k.write_text('1170.1 0 647.7 0\n0 1170.2 483.7 0\n0 0 1 0\n0 0 0 1\n')
    assert mr.read_intrinsics(str(k)) == tuple(float(np.float32(x)) for x in (1170.1, 1170.2, 647.7, 483.7))


def test_refuse_mesh_help_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'refuse_mesh.py'), '--help'],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for word in ('--poses', '--intrinsic', '--size', '--every', '--voxel', '--mode', '--scale-mat'):
        assert word in out.stdout, word
