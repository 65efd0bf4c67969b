"""CPU tests of the mesh evaluation: the numpy restatements (tests/nn_numpy.py) against the libraries the reference's
scripts call and on hand-computable inputs, the PLY reader, the ABI table, and the refusals of utils/mesh_eval.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import nn_numpy as nnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_ENTRIES = ('msdf_nn_split_count', 'msdf_nn_workspace_bytes', 'msdf_nn_search', 'msdf_voxel_keys',
               'msdf_voxel_mean')


def _clouds(seed, r, q):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (r, 3)), rng.uniform(-1, 1, (q, 3))


def _check_against_library(query_fn):
    for seed, (r, q) in enumerate([(1, 5), (50, 300), (3000, 2000)]):
        ref, qry = _clouds(seed, r, q)
        d, i, d2 = nnn.nearest(ref, qry, second=True)
        ld, li = query_fn(ref, qry)
        assert np.abs(d - ld).max() <= 1e-12 * np.abs(ld).max()
        clear = d2 > d * (1 + 1e-9)
        assert clear.mean() > 0.99
        assert np.array_equal(i[clear], li[clear])


def test_restatement_search_equals_scipy_ckdtree():
    spatial = pytest.importorskip('scipy.spatial')
    _check_against_library(lambda ref, qry: spatial.cKDTree(ref).query(qry))


def test_restatement_search_equals_sklearn_kdtree():
    neighbors = pytest.importorskip('sklearn.neighbors')

    def query(ref, qry):
        d, i = neighbors.KDTree(ref).query(qry)
        return d.reshape(-1), i.reshape(-1)
    _check_against_library(query)


def test_restatement_search_smallest_index_on_ties():
    base = np.random.default_rng(3).uniform(-1, 1, (40, 3))
    ref = np.concatenate([base, base, base])
    perm = np.random.default_rng(4).permutation(len(ref))
    ref = ref[perm]
    d, i = nnn.nearest(ref, base)
    assert (d == 0).all()
    for k in range(len(base)):
        assert i[k] == np.flatnonzero((ref == base[k]).all(1)).min()
    d1, i1 = nnn.nearest(ref, base, chunk=7)
    assert np.array_equal(i, i1) and np.array_equal(d, d1)


def _lattice(z):
    g = np.linspace(0, 1, 11)
    x, y = np.meshgrid(g, g, indexing='ij')
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1)


@pytest.mark.parametrize('offset,inside', [(0.03, 1.0), (0.07, 0.0)])
def test_scannet_metrics_on_offset_lattices(offset, inside):
    m = nnn.scannet_metrics(_lattice(offset), _lattice(0.0), threshold=0.05)
    assert set(m) == {'Acc', 'Comp', 'Prec', 'Recal', 'F-score'}
    assert m['Acc'] == pytest.approx(offset, rel=1e-12) and m['Comp'] == pytest.approx(offset, rel=1e-12)
    assert m['Prec'] == inside and m['Recal'] == inside
    assert m['F-score'] == inside and not np.isnan(m['F-score'])


def test_scannet_metrics_directions():
    """Acc is measured from the predicted points, Comp from the target's: a prediction that covers half the target."""
    gt = _lattice(0.0)
    pred = gt[gt[:, 0] <= 0.5 + 1e-9]
    m = nnn.scannet_metrics(pred, gt, threshold=0.05)
    assert m['Acc'] == 0.0 and m['Prec'] == 1.0
    assert m['Comp'] > 0.1 and m['Recal'] == pytest.approx(len(pred) / len(gt))


@pytest.mark.parametrize('offset,inside', [(0.03, 100.0), (0.07, 0.0)])
def test_replica_metrics_on_offset_lattices(offset, inside):
    a, b = _lattice(offset), _lattice(0.0)
    up = np.tile([0.0, 0.0, 1.0], (len(a), 1))
    tilt = np.tile([0.0, 0.6, -0.8], (len(a), 1))
    m = nnn.replica_metrics(a, tilt, b, up, dist_th=0.05)
    assert m['accuracy'] == pytest.approx(100 * offset, rel=1e-12)
    assert m['completion'] == pytest.approx(100 * offset, rel=1e-12)
    assert m['chamfer'] == pytest.approx(100 * offset, rel=1e-12)
    assert m['precision'] == inside and m['completion_ratio'] == inside and m['fscore'] == inside
    assert m['normal_acc'] == pytest.approx(80.0) and m['normal_comp'] == pytest.approx(80.0)
    assert m['normal_avg'] == pytest.approx(80.0)


def test_voxel_restatement_means_are_centres():
    v = 0.25                                               # exact in fp32, as are the centres and offsets below
    rng = np.random.default_rng(5)
    # the cloud's minimum is the centre of voxel (0, 0, 0), a single point, so the bins are centred on the lattice;
    # every other occupied voxel has indices >= 1 and holds pairs of points symmetric about its centre
    cells = np.concatenate([[[0, 0, 0]], np.unique(rng.integers(1, 12, (60, 3)), axis=0)])
    centres = (cells * v).astype(np.float32)
    pts = [centres[:1]]
    for c in centres[1:]:
        off = (rng.integers(-31, 32, (int(rng.integers(1, 4)), 3)) / 256.0).astype(np.float32)   # |offset| < v / 2
        pts += [c + off, c - off]
    pts = np.concatenate(pts).astype(np.float32)
    assert np.array_equal(pts.min(0), centres[0])
    perm = rng.permutation(len(pts))
    out = nnn.voxel_down_sample(pts[perm], v)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    assert out.dtype == np.float32 and out.shape == (len(cells), 3)
    assert np.array_equal(out, centres[order])


def test_voxel_restatement_single_voxel_and_order():
    pts = np.array([[0.0, 0.0, 0.0], [0.004, 0.002, 0.006], [0.1, 0.0, 0.0], [0.0, 0.0, 0.1]], np.float32)
    out = nnn.voxel_down_sample(pts, 0.02)
    assert out.shape == (3, 3)
    assert np.array_equal(out[0], ((pts[0].astype(np.float64) + pts[1]) / 2).astype(np.float32))
    assert np.array_equal(out[1], pts[3]) and np.array_equal(out[2], pts[2])    # (0,0,5) before (5,0,0)


def test_face_normals_and_areas():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [0, 0, 1], [1, 0, 0]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3], [0, 4, 1]])
    assert np.allclose(nnn.face_areas(v, f), [3, 3, 1, 0])
    assert np.allclose(nnn.face_normals(v, f), [[0, 0, 1], [0, 0, -1], [0, -1, 0], [0, 0, 0]])


def _write_ply(path, fmt, rng):
    """A PLY as another program might write it: extra vertex properties, float x / double y / float z in an unusual
    order, uint8 colours, faces with a ushort count type, uint indices and a trailing flag."""
    n, m = 17, 9
    v = rng.normal(size=(n, 3)).astype(np.float32).astype(np.float64)
    f = rng.integers(0, n, (m, 3))
    q = rng.uniform(size=n).astype(np.float32)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    head = ('ply\nformat %s 1.0\ncomment made by a test\nelement vertex %d\n'
            'property float quality\nproperty float x\nproperty double y\nproperty uchar red\nproperty uchar green\n'
            'property uchar blue\nproperty float z\nelement face %d\nproperty list ushort uint vertex_indices\n'
            'property uchar flags\nend_header\n' % (fmt, n, m))
    with open(path, 'wb') as fh:
        fh.write(head.encode('ascii'))
        if fmt == 'ascii':
            for k in range(n):
                fh.write(('%r %r %r %d %d %d %r\n' % (float(q[k]), float(v[k, 0]), float(v[k, 1]), col[k, 0],
                                                        col[k, 1], col[k, 2], float(v[k, 2]))).encode())
            for k in range(m):
                fh.write(('3 %d %d %d 7\n' % tuple(f[k])).encode())
        else:
            vd = np.dtype([('q', '<f4'), ('x', '<f4'), ('y', '<f8'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'),
                           ('z', '<f4')])
            rec = np.empty(n, vd)
            rec['q'], rec['x'], rec['y'], rec['z'] = q, v[:, 0], v[:, 1], v[:, 2]
            rec['r'], rec['g'], rec['b'] = col[:, 0], col[:, 1], col[:, 2]
            fd = np.dtype([('n', '<u2'), ('v', '<u4', (3,)), ('flags', 'u1')])
            frec = np.empty(m, fd)
            frec['n'], frec['v'], frec['flags'] = 3, f, 7
            fh.write(rec.tobytes() + frec.tobytes())
    return v, f


@pytest.mark.parametrize('fmt', ['ascii', 'binary_little_endian'])
def test_read_ply_foreign_files(fmt, tmp_path):
    from monosdf_amd.utils.mesh_eval import read_ply
    p = str(tmp_path / 'm.ply')
    v, f = _write_ply(p, fmt, np.random.default_rng(11))
    m = read_ply(p)
    assert m.vertices.dtype == np.float64 and m.faces.dtype == np.int64
    assert np.array_equal(m.vertices, v) and np.array_equal(m.faces, f)


def test_read_ply_reads_mesh_export_and_refuses_others(tmp_path):
    from monosdf_amd.utils.mesh import Mesh
    from monosdf_amd.utils.mesh_eval import read_ply
    rng = np.random.default_rng(0)
    src = Mesh(rng.normal(size=(50, 3)), rng.integers(0, 50, (70, 3)), rng.normal(size=(50, 3)))
    p = str(tmp_path / 'own.ply')
    src.export(p, 'ply')
    back = read_ply(p)
    assert np.array_equal(back.vertices, src.vertices) and np.array_equal(back.faces, src.faces)
    assert np.array_equal(back.vertex_normals, src.vertex_normals)
    quad = tmp_path / 'quad.ply'
    quad.write_bytes(b'ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
                     b'element face 1\nproperty list uchar int vertex_indices\nend_header\n'
                     b'0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n')
    with pytest.raises(ValueError, match='triangle'):
        read_ply(str(quad))
    big = tmp_path / 'big.ply'
    big.write_bytes(b'ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n')
    with pytest.raises(ValueError, match='binary_big_endian'):
        read_ply(str(big))


def test_new_entries_declared_in_header_and_table():
    from monosdf_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'monosdf_hip.h')).read()
    declared = set(re.findall(r'^(?:int|int64_t) (msdf_\w+)\(', text, flags=re.M))
    new = [n for n in _lib.exported_symbols() if n.startswith(('msdf_nn_', 'msdf_voxel_'))]
    assert sorted(new) == sorted(NEW_ENTRIES)
    for name in new:
        assert name in declared, name
    assert '#define MSDF_ABI_VERSION 8' in text and _lib.ABI_VERSION == 8


def test_refusals_without_a_gpu():
    from monosdf_amd.utils import mesh_eval as me
    pts = torch.zeros(4, 3)
    with pytest.raises(TypeError, match='cpu'):
        me.nearest_neighbors(pts, pts)
    with pytest.raises(TypeError, match='cpu'):
        me.voxel_down_sample(pts, 0.02)
    with pytest.raises(TypeError, match='cpu'):
        me.sample_surface(pts, torch.zeros(1, 3, dtype=torch.int64), 10)
    with pytest.raises(TypeError, match='cpu'):
        me.face_normals(pts, torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(TypeError, match='cpu'):
        me.evaluate_scannet(pts, pts)
    with pytest.raises(TypeError, match='CUDA'):
        me.nearest_neighbors(np.zeros((4, 3), np.float32), pts)
