"""GPU tests of the mesh evaluation (csrc/nnsearch.hip, utils/mesh_eval.py): the brute-force search, the voxel
down-sample, the surface sampler and the two metric protocols against the numpy restatements of tests/nn_numpy.py."""
import os
import sys

import numpy as np
import pytest
import torch

import nn_numpy as nnn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(1, 7), (63, 1), (1000, 1025), (20000, 20000), (70001, 333)]


def _me():
    from monosdf_amd.utils import mesh_eval
    return mesh_eval


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _shell(rng, n, radius, centre):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (radius * rng.uniform(0.99, 1.01, (n, 1))) + np.asarray(centre, np.float64)


def _cloud(kind, rng, n):
    if kind == 'cube':
        return rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    if kind == 'shell':
        return _shell(rng, n, 1.0, (0, 0, 0)).astype(np.float32)
    return _shell(rng, n, 2.5, (8, -6, 3)).astype(np.float32)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', ['cube', 'shell', 'scene_shell'])
def test_search_equals_restatement(kind, size):
    """|d_gpu - d_ref| <= 1e-6 d_ref + 1e-7 max|coordinate| (three subtractions exact to 1 ulp, three products, two
    sums and a square root bound the relative error of d near 4 * 2^-24 = 2.4e-7).  Index equal wherever the
    second-nearest point is more than 1e-5 relatively farther than the nearest; at most 0.1 % of the queries may be
    exempt from that comparison."""
    r, q = size
    rng = np.random.default_rng(1000 * SIZES.index(size) + len(kind))
    ref, qry = _cloud(kind, rng, r), _cloud(kind, rng, q)
    dist, idx = _me().nearest_neighbors(_cuda(ref), _cuda(qry))
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == (q,) and idx.shape == (q,)
    dist, idx = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    d, i, d2 = nnn.nearest(ref, qry, second=True)
    scale = max(np.abs(ref).max(), np.abs(qry).max())
    err = np.abs(dist - d) - (1e-6 * d + 1e-7 * scale)
    print('%s %dx%d: max |d_gpu - d_ref| / d_ref = %.3g' % (kind, r, q, (np.abs(dist - d) / np.maximum(d, 1e-30)).max()))
    assert err.max() <= 0
    clear = d2 > d * (1 + 1e-5)
    exempt = int((~clear).sum())
    print('%s %dx%d: %d of %d queries exempt from the index comparison' % (kind, r, q, exempt, q))
    assert exempt <= 1e-3 * q
    assert np.array_equal(idx[clear], i[clear])
    assert ((idx >= 0) & (idx < r)).all()


def test_ties_take_the_smallest_index_and_own_points_are_at_zero():
    rng = np.random.default_rng(21)
    base = _cloud('scene_shell', rng, 3000)
    ref = np.concatenate([base, base, base])[rng.permutation(9000)]
    dist, idx = _me().nearest_neighbors(_cuda(ref), _cuda(base))
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert (dist == 0.0).all()
    order = np.lexsort((np.arange(9000), ref[:, 2], ref[:, 1], ref[:, 0]))      # groups of equal points, index ascending
    first = {}
    for j in order[::-1]:
        first[ref[j].tobytes()] = j
    expect = np.array([first[p.tobytes()] for p in base])
    assert np.array_equal(idx, expect)
    for s in (1, 2, 5, 9):                                  # ties across slices of the reference cloud
        d_s, i_s = _me().nearest_neighbors(_cuda(ref), _cuda(base), n_splits=s)
        assert np.array_equal(i_s.cpu().numpy(), expect) and (d_s == 0).all()


def test_bitwise_repeatable_and_split_independent():
    from monosdf_amd import _lib
    rng = np.random.default_rng(22)
    ref, qry = _cuda(_cloud('shell', rng, 20000)), _cuda(_cloud('shell', rng, 5000))
    d0, i0 = _me().nearest_neighbors(ref, qry)
    d1, i1 = _me().nearest_neighbors(ref, qry)
    assert torch.equal(d0, d1) and torch.equal(i0, i1)
    lib = _lib.load()
    used = set()
    for s in (1, 3, 7, 20, 1000):
        used.add(lib.msdf_nn_split_count(20000, 5000, s))
        d, i = _me().nearest_neighbors(ref, qry, n_splits=s)
        assert torch.equal(d.view(torch.int32), d0.view(torch.int32)) and torch.equal(i, i0), s
    assert used == {1, 3, 7, 20}                             # 20 tiles of 1024 points: 1000 is clamped to 20


def test_raw_abi_call_and_argument_errors():
    from monosdf_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(23)
    ref_h, qry_h = _cloud('cube', rng, 5000), _cloud('cube', rng, 777)
    ref, qry = _cuda(ref_h), _cuda(qry_h)
    nbytes = lib.msdf_nn_workspace_bytes(5000, 777, 2)
    assert nbytes >= 2 * 777 * 8 and lib.msdf_nn_split_count(5000, 777, 2) == 2
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    dist = torch.full((777,), -1.0, dtype=torch.float32, device='cuda')
    idx = torch.full((777,), -1, dtype=torch.int32, device='cuda')
    st = _lib.stream_ptr()
    assert lib.msdf_nn_search(_lib.ptr(ref), 5000, _lib.ptr(qry), 777, 2, _lib.ptr(ws), _lib.ptr(dist), _lib.ptr(idx),
                              st) == 0
    torch.cuda.synchronize()
    d, i = nnn.nearest(ref_h, qry_h)
    assert np.array_equal(idx.cpu().numpy(), i) and np.abs(dist.cpu().numpy() - d).max() <= 1e-6
    # argument errors: MSDF_ERR_ARG (1) and no launch -- the outputs keep their fill
    dist.fill_(-1.0)
    idx.fill_(-1)
    a = (_lib.ptr(ref), 5000, _lib.ptr(qry), 777, 2, _lib.ptr(ws), _lib.ptr(dist), _lib.ptr(idx), st)
    for pos, bad in ((1, 0), (1, -3), (1, 2 ** 31), (3, -1), (0, None), (2, None), (5, None), (6, None), (7, None)):
        args = list(a)
        args[pos] = bad
        assert lib.msdf_nn_search(*args) == 1, (pos, bad)
    assert lib.msdf_nn_workspace_bytes(0, 10, 0) == -1 and lib.msdf_nn_split_count(0, 10, 0) == -1
    args = list(a)
    args[3] = 0                                              # no queries: success, nothing launched
    assert lib.msdf_nn_search(*args) == 0
    torch.cuda.synchronize()
    assert (dist == -1).all() and (idx == -1).all()
    keys = torch.empty(5000, dtype=torch.int64, device='cuda')
    lo = ref.min(0).values.contiguous()
    assert lib.msdf_voxel_keys(_lib.ptr(ref), 5000, _lib.ptr(lo), 0.0, _lib.ptr(keys), st) == 1
    assert lib.msdf_voxel_keys(None, 5000, _lib.ptr(lo), 0.1, _lib.ptr(keys), st) == 1
    assert lib.msdf_voxel_keys(_lib.ptr(ref), 5000, _lib.ptr(lo), 0.1, _lib.ptr(keys), st) == 0
    order = torch.argsort(keys, stable=True)
    out = torch.empty(5000, 3, dtype=torch.float32, device='cuda')
    assert lib.msdf_voxel_mean(_lib.ptr(ref), _lib.ptr(order), None, 5000, 10, _lib.ptr(out), st) == 1
    assert lib.msdf_voxel_mean(_lib.ptr(ref), _lib.ptr(order), _lib.ptr(order), 5000, 5001, _lib.ptr(out), st) == 1
    torch.cuda.synchronize()


def _ulp_distance(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_voxel_down_sample_equals_restatement():
    rng = np.random.default_rng(24)
    big = rng.uniform(-1, 1, (200000, 3)).astype(np.float32)
    one = (np.float32(3.0) + rng.uniform(0, 0.009, (37, 3))).astype(np.float32)
    for pts, n_expect in ((big, None), (one, 1)):
        out = _me().voxel_down_sample(_cuda(pts), 0.02)
        again = _me().voxel_down_sample(_cuda(pts), 0.02)
        assert torch.equal(out, again)
        out = out.cpu().numpy()
        ref = nnn.voxel_down_sample(pts, 0.02)
        assert out.shape == ref.shape and out.dtype == np.float32
        if n_expect is not None:
            assert len(out) == n_expect
        ulps = _ulp_distance(out, ref)
        print('voxel_down_sample %d -> %d points: %d coordinates differ, max %d ulp' % (
            len(pts), len(out), int((ulps > 0).sum()), int(ulps.max())))
        assert ulps.max() <= 1


def _two_triangles():
    # areas 1 and 3, and a zero-area face between them
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [5, 0, 1], [7, 0, 1], [5, 3, 1], [1, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 6, 1], [3, 4, 5]], np.int64)
    return v, f


def _check_on_faces(v, f, pts, fi):
    v = v.astype(np.float64)
    o, e1, e2 = v[f[fi, 0]], v[f[fi, 1]] - v[f[fi, 0]], v[f[fi, 2]] - v[f[fi, 0]]
    rel = pts.astype(np.float64) - o
    a = np.stack([e1, e2], 2)                                # [n, 3, 2]
    ata = np.einsum('nij,nik->njk', a, a)
    atb = np.einsum('nij,ni->nj', a, rel)
    uv = np.linalg.solve(ata, atb[:, :, None])[:, :, 0]
    assert uv.min() >= -1e-5 and uv.max() <= 1 + 1e-5 and (uv.sum(1) <= 1 + 1e-5).all()
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    extent = (v.max(0) - v.min(0)).max()
    assert np.abs((rel * n).sum(1)).max() <= 1e-6 * extent


def test_sample_surface():
    me = _me()
    v, f = _two_triangles()
    n = 100000
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    pts, fi = me.sample_surface(_cuda(v), _cuda(f, np.int64), n, gen)
    assert pts.shape == (n, 3) and pts.dtype == torch.float32 and fi.shape == (n,) and fi.dtype == torch.int64
    gen.manual_seed(5)
    pts2, fi2 = me.sample_surface(_cuda(v), _cuda(f, np.int64), n, gen)
    assert torch.equal(pts, pts2) and torch.equal(fi, fi2)
    pts, fi = pts.cpu().numpy(), fi.cpu().numpy()
    assert (fi == 1).sum() == 0                               # the zero-area face gets none
    sigma = np.sqrt(n * 0.75 * 0.25)
    assert abs((fi == 2).sum() - 0.75 * n) <= 6 * sigma
    _check_on_faces(v, f, pts, fi)
    # a closed mesh with edges of order 1: an octahedron
    ov = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    of = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    pts, fi = me.sample_surface(_cuda(ov), _cuda(of, np.int64), 40000, gen)
    _check_on_faces(ov, of, pts.cpu().numpy(), fi.cpu().numpy())
    assert np.bincount(fi.cpu().numpy(), minlength=8).min() > 40000 / 8 - 6 * np.sqrt(40000 * 0.125 * 0.875)
    nrm = me.face_normals(_cuda(v), _cuda(f, np.int64)).cpu().numpy()
    assert np.allclose(nrm, nnn.face_normals(v, f), atol=1e-6) and (nrm[1] == 0).all()


def _sphere_mesh(radius, spacing=0.02, half=1.1):
    from monosdf_amd.utils.mesh import marching_cubes
    n = int(round(2 * half / spacing)) + 1
    g = torch.linspace(-half, half, n, device='cuda', dtype=torch.float64)
    x, y, z = torch.meshgrid(g, g, g, indexing='ij')
    vol = ((x * x + y * y + z * z).sqrt() - radius).float()
    step = float(g[1] - g[0])
    verts, faces, _ = marching_cubes(vol, 0.0, (step, step, step))
    return (verts - half).contiguous(), faces


def test_evaluate_scannet_on_concentric_spheres():
    me = _me()
    (pv, _), (gv, _) = _sphere_mesh(1.03), _sphere_mesh(1.00)
    got = me.evaluate_scannet(pv, gv, threshold=0.05, down_sample=0.02)
    assert list(got) == ['Acc', 'Comp', 'Prec', 'Recal', 'F-score'] and all(type(x) is float for x in got.values())
    pd, gd = me.voxel_down_sample(pv, 0.02).cpu().numpy(), me.voxel_down_sample(gv, 0.02).cpu().numpy()
    want = nnn.scannet_metrics(pd, gd, 0.05)
    for k in want:
        print('scannet %s: gpu %.9g restatement %.9g' % (k, got[k], want[k]))
        assert got[k] == pytest.approx(want[k], rel=1e-5), k
    assert abs(got['Acc'] - 0.03) <= 0.02 and abs(got['Comp'] - 0.03) <= 0.02
    # thresholds on either side of the radius difference; both ratios zero gives 0.0, not a division by zero
    far = me.evaluate_scannet(pv, gv, threshold=0.001, down_sample=0.02)
    assert far['Prec'] == 0.0 and far['Recal'] == 0.0 and far['F-score'] == 0.0


def test_evaluate_replica_on_concentric_spheres():
    from monosdf_amd.utils.mesh import Mesh
    me = _me()
    (pv, pf), (gv, gf) = _sphere_mesh(1.03), _sphere_mesh(1.00)
    got, s = me.evaluate_replica((pv, pf), (gv, gf), n_samples=50000, dist_th=0.05, seed=3, return_samples=True)
    assert s['rec_points'].shape == (50000, 3) and s['gt_points'].shape == (50000, 3)
    want = nnn.replica_metrics(s['rec_points'].cpu().numpy(), s['rec_normals'].cpu().numpy(),
                               s['gt_points'].cpu().numpy(), s['gt_normals'].cpu().numpy(), 0.05)
    assert set(got) == set(want)
    for k in want:
        print('replica %s: gpu %.9g restatement %.9g' % (k, got[k], want[k]))
        assert got[k] == pytest.approx(want[k], rel=1e-5), k
    assert got['normal_avg'] > 99.0
    assert got['chamfer'] == pytest.approx((got['accuracy'] + got['completion']) / 2)
    assert abs(got['accuracy'] - 3.0) <= 2.0 and abs(got['completion'] - 3.0) <= 2.0
    # the sampled normals are the face normals of the faces the samples came from
    fn = nnn.face_normals(pv.cpu().numpy(), pf.cpu().numpy())[s['rec_faces'].cpu().numpy()]
    assert np.abs(s['rec_normals'].cpu().numpy() - fn).max() <= 1e-6
    # same seed, same numbers; Mesh objects are accepted
    again = me.evaluate_replica(Mesh(pv.cpu().numpy(), pf.cpu().numpy()), Mesh(gv.cpu().numpy(), gf.cpu().numpy()),
                                n_samples=50000, dist_th=0.05, seed=3)
    assert again == got
    none = me.evaluate_replica((pv, pf), (gv, gf), n_samples=2000, dist_th=0.001)
    assert none['precision'] == 0.0 and none['completion_ratio'] == 0.0 and none['fscore'] == 0.0


def test_refusals():
    me = _me()
    good = torch.zeros(8, 3, device='cuda')
    with pytest.raises(TypeError, match='cpu'):
        me.nearest_neighbors(good.cpu(), good)
    with pytest.raises(TypeError, match='cpu'):
        me.nearest_neighbors(good, good.cpu())
    with pytest.raises(TypeError, match='float32'):
        me.nearest_neighbors(good.double(), good)
    with pytest.raises(TypeError, match='float32'):
        me.voxel_down_sample(good.double(), 0.02)
    bad = good.clone()
    bad[3, 1] = float('nan')
    with pytest.raises(ValueError, match='finite'):
        me.nearest_neighbors(bad, good)
    with pytest.raises(ValueError, match='finite'):
        me.nearest_neighbors(good, bad)
    with pytest.raises(ValueError, match='empty'):
        me.nearest_neighbors(good[:0], good)
    with pytest.raises(ValueError):
        me.nearest_neighbors(good[:, :2], good)
    with pytest.raises(ValueError, match='positive'):
        me.voxel_down_sample(good, 0.0)
    d, i = me.nearest_neighbors(good, good[:0])              # no queries: empty outputs
    assert d.shape == (0,) and i.shape == (0,)
