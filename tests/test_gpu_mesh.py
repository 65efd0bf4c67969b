"""GPU tests of marching cubes (csrc/mcubes.hip) and get_surface_sliding (utils/mesh.py): the kernels against the numpy
restatement over the same generated table, mesh topology and geometry on analytic surfaces, run-to-run bit equality,
and the drop-in get_surface_sliding on the bench model."""
import os
import sys

import numpy as np
import pytest
import torch

import mc_numpy as mcn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _mc(vol, level=0.0, spacing=(1.0, 1.0, 1.0)):
    from monosdf_amd.utils.mesh import marching_cubes
    v, f, n = marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda(), level, spacing)
    return v.cpu().numpy(), f.cpu().numpy().astype(np.int64), n.cpu().numpy()


@pytest.mark.parametrize('shape', [(2, 2, 2), (37, 41, 53), (64, 64, 64), (3, 130, 65)])
def test_gpu_equals_numpy_restatement(shape):
    rng = np.random.default_rng(sum(shape))
    spacing = (0.5, 0.75, 1.25)
    for trial in range(8 if shape == (2, 2, 2) else 1):
        vol = rng.uniform(-1, 1, shape).astype(np.float32)
        level = 0.0 if trial % 2 == 0 else 0.125
        v, f, n = _mc(vol, level, spacing)
        rv, rf, rn = mcn.marching_cubes(vol, level, spacing)
        assert v.shape == rv.shape and f.shape == rf.shape
        assert np.array_equal(f, rf)
        extent = max((s - 1) * sp for s, sp in zip(shape, spacing))
        assert np.abs(v - rv).max(initial=0) <= 1e-6 * extent
        assert np.abs(n - rn).max(initial=0) <= 1e-6 * extent
    if shape == (64, 64, 64):
        below = vol < 0
        code = np.zeros((63, 63, 63), np.int64)
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            code |= below[dx:63 + dx, dy:63 + dy, dz:63 + dz].astype(np.int64) << c
        assert np.unique(code).size == 256                  # every case of the table was exercised


def test_interior_edges_shared_by_two_opposite_faces():
    vol = np.random.default_rng(7).uniform(-1, 1, (37, 41, 53)).astype(np.float32)
    v, f, _ = _mc(vol)
    use = mcn.edge_use(f)
    hi = np.array(vol.shape, np.float32) - 1
    n_border = 0
    for (a, b), cnt in use.items():
        assert cnt == 1, (a, b)                              # a directed edge in one face only
        if (b, a) not in use:                                # ... and its reverse in exactly one other, unless on the border
            pa, pb = v[a], v[b]
            assert any((pa[d] == 0 and pb[d] == 0) or (pa[d] == hi[d] and pb[d] == hi[d]) for d in range(3)), (a, b)
            n_border += 1
    assert 0 < n_border < len(use) // 10


def _grid(n):
    return np.mgrid[0:n, 0:n, 0:n].astype(np.float64)


def test_sphere_and_torus_topology_and_geometry():
    n = 128
    c = np.array([63.7, 64.2, 63.1])
    g = _grid(n) - c[:, None, None, None]
    r = 40.0
    vol = (np.sqrt((g ** 2).sum(0)) - r).astype(np.float32)
    v, f, nrm = _mc(vol)
    assert mcn.euler(v, f) == 2
    assert abs(mcn.area(v, f) / (4 * np.pi * r * r) - 1) < 0.02
    assert abs(mcn.signed_volume(v, f) / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    d = v - c
    cos = (nrm * d).sum(1) / np.linalg.norm(d, axis=1)
    assert np.median(cos) > 0.999

    R, rt = 36.0, 14.0
    x, y, z = g
    q = np.sqrt(x * x + y * y)
    vol = (np.sqrt((q - R) ** 2 + z * z) - rt).astype(np.float32)
    v, f, nrm = _mc(vol)
    assert mcn.euler(v, f) == 0
    assert abs(mcn.area(v, f) / (4 * np.pi ** 2 * R * rt) - 1) < 0.02
    assert abs(mcn.signed_volume(v, f) / (2 * np.pi ** 2 * R * rt * rt) - 1) < 0.01
    x, y, z = (v - c).T
    q = np.sqrt(x * x + y * y)
    grad = np.stack([x * (q - R) / q, y * (q - R) / q, z], 1)
    grad /= np.linalg.norm(grad, axis=1, keepdims=True)
    assert np.median((nrm * grad).sum(1)) > 0.999


def test_512_bitwise_repeatable_and_empty_volumes():
    from monosdf_amd import _lib
    from monosdf_amd.utils.mesh import marching_cubes
    n = 512
    a = torch.arange(n, device='cuda', dtype=torch.float32)
    vol = (torch.sin(a / 7.0)[:, None, None] + torch.sin(a / 9.0)[None, :, None] + torch.sin(a / 11.0)[None, None, :])
    vol = vol + 0.05 * torch.rand(n, n, n, device='cuda', generator=torch.Generator('cuda').manual_seed(0))
    first = marching_cubes(vol, 0.1, (0.01, 0.01, 0.01))
    second = marching_cubes(vol, 0.1, (0.01, 0.01, 0.01))
    assert first[0].shape[0] > 1000000 and first[1].shape[0] > 1000000
    for x, y in zip(first, second):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))            # bitwise, NaN-free or not
    assert int(first[1].min()) >= 0 and int(first[1].max()) == first[0].shape[0] - 1
    del first, second
    prof = {}
    _lib.PROFILE = prof
    try:
        for fill in (1.0, -1.0):
            v, f, nrm = marching_cubes(torch.full((70, 66, 129), fill, device='cuda'), 0.0)
            assert v.shape == (0, 3) and f.shape == (0, 3) and nrm.shape == (0, 3)
    finally:
        _lib.PROFILE = None
    assert len(prof.get('msdf_mc_count', [])) == 2
    assert 'msdf_mc_emit' not in prof


@pytest.fixture(scope='module')
def bench_model():
    import bench
    from monosdf_amd.model.network import MonoSDFNetwork
    torch.manual_seed(0)
    return MonoSDFNetwork(bench.model_conf()).cuda().eval()


@pytest.mark.parametrize('resolution', [512, 1024])
@pytest.mark.parametrize('level', [0.0, 0.001])
def test_get_surface_sliding_on_bench_model(bench_model, resolution, level, tmp_path):
    from monosdf_amd.utils import render
    from monosdf_amd.utils.mesh import Mesh, get_surface_sliding, load_ply
    sdf = lambda p: bench_model.implicit_network.raw_sdf(p)
    bound = [-1.1, 1.1]
    mesh = get_surface_sliding(None, 0, sdf, resolution=resolution, grid_boundary=bound, return_mesh=True, level=level)
    assert isinstance(mesh, Mesh)
    assert mesh.vertices.dtype == np.float64 and mesh.faces.dtype == np.int64 and len(mesh.faces) > 100000
    assert mesh.faces.min() >= 0 and mesh.faces.max() == len(mesh.vertices) - 1
    assert np.allclose(np.linalg.norm(mesh.vertex_normals, axis=1), 1, atol=1e-5)
    assert mesh.vertices.min() >= bound[0] and mesh.vertices.max() <= bound[1]
    # every vertex lies on the level set of the network within one voxel
    spacing = (bound[1] - bound[0]) / (resolution // (512 if resolution >= 512 else 128)) / 511
    with torch.no_grad():
        val = sdf(torch.from_numpy(mesh.vertices).float().cuda()).double().cpu().numpy()
    assert float((np.abs(val - level) <= spacing).mean()) >= 0.999
    # normals follow the network's field toward increasing sdf (bench model: inside_outside, so inward of its sphere):
    # central differences of the network at a sample of the vertices
    pick = np.random.default_rng(0).permutation(len(mesh.vertices))[:100000]
    x = torch.from_numpy(mesh.vertices[pick]).float().cuda()
    h = 1e-3
    with torch.no_grad():
        grad = torch.stack([sdf(x + h * e) - sdf(x - h * e) for e in torch.eye(3, device='cuda')], 1)
    grad = torch.nn.functional.normalize(grad.double(), dim=1).cpu().numpy()
    assert np.median((mesh.vertex_normals[pick] * grad).sum(1)) > 0.99
    # center / scale
    center = np.array([0.25, -0.5, 1.0])
    scaled = get_surface_sliding(None, 0, sdf, resolution=resolution, grid_boundary=bound, return_mesh=True,
                                 level=level, center=center, scale=2.0)
    assert np.array_equal(scaled.faces, mesh.faces)
    assert np.allclose(scaled.vertices, mesh.vertices / 2.0 + center, rtol=0, atol=1e-12)
    # return_mesh=False: {path}/surface_{epoch}.ply
    assert get_surface_sliding(str(tmp_path), 7, sdf, resolution=resolution, grid_boundary=bound, level=level) is None
    back = load_ply(str(tmp_path / 'surface_7.ply'))
    assert np.array_equal(back.vertices, mesh.vertices) and np.array_equal(back.faces, mesh.faces)
    assert np.array_equal(back.vertex_normals, mesh.vertex_normals)
    if resolution == 512 and level == 0.0:
        # the device volume is the host volume of sdf_volume, bit for bit
        (o1, s1, dev), = list(render.sdf_volume_device(sdf, 512, bound, shard=False))
        (o2, s2, host), = list(render.sdf_volume(sdf, 512, bound, shard=False))
        assert np.array_equal(o1, o2) and s1 == s2 and np.array_equal(dev.cpu().numpy(), host)
