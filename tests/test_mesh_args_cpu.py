"""CPU tests of utils/mesh_args.py, the argument handling the mesh tools share: every entry point that takes a mesh
refuses a bad one on the host before anything is uploaded (so these pass where there is no GPU: a premature upload
would raise something else), the vertex compaction against a loop in numpy, the one PLY reader under both of its
names, and the workspace helper's refusal of the -1 the ABI returns."""
import os
import sys

import numpy as np
import pytest
import torch

import refuse_numpy as rfn
from test_mesh_eval_cpu import _write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = (50.0, 50.0, 32.0, 24.0)
POSES = np.eye(4)[None]
TETRAHEDRON = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64),
               np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64))


def _icosphere():
    v, f = rfn.icosphere(0, 0.5, (0, 0, 0))
    assert v.shape == (12, 3) and f.shape == (20, 3)
    return v, f


def _entry_points():
    from monosdf_amd.utils import mesh_dtu as md, mesh_eval as me, mesh_refuse as mr
    good = _icosphere()
    dtu = (np.zeros((4, 3), np.float32), np.ones((2, 2, 2)), np.zeros((2, 3)), 1.0, [0, 0, 1, 0])
    return {'refuse': lambda m: mr.refuse(m, POSES, K, 48, 64),
            'cull_to_frustums': lambda m: mr.cull_to_frustums(m, POSES, K, 48, 64),
            'cull_to_masks': lambda m: md.cull_to_masks(m, np.zeros((1, 3, 4)), np.zeros((1, 8, 8), np.uint8)),
            'evaluate_replica': lambda m: me.evaluate_replica(m, good, n_samples=10),
            'evaluate_dtu': lambda m: md.evaluate_dtu(m, *dtu)}


def _bad_meshes():
    v, f = _icosphere()

    def changed(array, index, value):
        out = array.copy()
        out[index] = value
        return out
    return {'index_V': (v, changed(f, (3, 1), len(v)), 'face index'),
            'index_minus_1': (v, changed(f, (19, 2), -1), 'face index'),
            'nan': (changed(v, (5, 0), np.nan), f, 'non-finite'),
            'inf': (changed(v, (11, 2), np.inf), f, 'non-finite'),
            'vertices_V2': (v[:, :2], f, r'\[V, 3\]'),
            'float_faces': (v, f.astype(np.float64), 'integer')}


@pytest.mark.parametrize('form', ['Mesh', 'pair'])
@pytest.mark.parametrize('case', sorted(_bad_meshes()))
@pytest.mark.parametrize('entry', sorted(_entry_points()))
def test_bad_mesh_is_refused_on_the_host(entry, case, form):
    from monosdf_amd.utils.mesh import Mesh
    v, f, fragment = _bad_meshes()[case]
    if form == 'Mesh':
        mesh = Mesh(*_icosphere())
        mesh.vertices, mesh.faces = v, f           # the constructor would reshape [V, 2] and cast float faces
    else:
        mesh = (v, f)
    with pytest.raises(ValueError, match=fragment) as err:
        _entry_points()[entry](mesh)
    assert str(err.value).startswith(entry + ':')


def _compact_loop(keep, faces):
    """Faces with all three vertices kept, renumbered by counting the kept vertices before each: one at a time."""
    new_index, n = {}, 0
    for i, k in enumerate(keep):
        if k:
            new_index[i] = n
            n += 1
    out = [[new_index[i] for i in face] for face in faces.tolist() if all(keep[i] for i in face)]
    return np.array(out, np.int64).reshape(-1, 3)


@pytest.mark.parametrize('mesh', ['tetrahedron', 'icosphere'])
def test_compact_faces_equals_the_loop(mesh):
    from monosdf_amd.utils.mesh_args import compact_faces
    v, f = TETRAHEDRON if mesh == 'tetrahedron' else _icosphere()
    n = len(v)
    some = f[:len(f) // 4]                         # extract_mesh's mask: the vertices that the kept faces use
    used = np.zeros(n, bool)
    used[some.reshape(-1)] = True
    masks = {'all': np.ones(n, bool), 'none': np.zeros(n, bool), 'one_dropped': np.arange(n) != 2, 'used': used}
    assert 0 < used.sum() < n
    for name, keep in masks.items():
        for dtype in (torch.int32, torch.int64):
            got = compact_faces(torch.from_numpy(keep), torch.from_numpy(f).to(dtype))
            assert got.dtype == torch.int64 and got.dim() == 2 and got.shape[1] == 3, name
            assert np.array_equal(got.numpy(), _compact_loop(keep, f)), name
    assert np.array_equal(compact_faces(torch.from_numpy(masks['all']), torch.from_numpy(f)).numpy(), f)
    assert compact_faces(torch.from_numpy(masks['none']), torch.from_numpy(f)).shape == (0, 3)
    assert len(_compact_loop(masks['one_dropped'], f)) == (1 if mesh == 'tetrahedron' else 15)
    for all_kept in (False, True):                 # the selection may be left out where it would keep every face
        assert np.array_equal(compact_faces(torch.from_numpy(used), torch.from_numpy(some), all_kept).numpy(),
                              _compact_loop(used, some))
    assert len(_compact_loop(used, some)) == len(some)             # the faces that formed the mask all survive
    assert compact_faces(torch.zeros(0, dtype=torch.bool), torch.zeros(0, 3, dtype=torch.int64)).shape == (0, 3)


def test_one_ply_reader_under_both_names(tmp_path):
    from monosdf_amd.utils import mesh, mesh_eval
    assert mesh.load_ply is mesh.read_ply and mesh_eval.read_ply is mesh.read_ply
    for fmt in ('ascii', 'binary_little_endian'):
        p = str(tmp_path / (fmt + '.ply'))
        v, f = _write_ply(p, fmt, np.random.default_rng(11))
        m = mesh.load_ply(p)
        assert m.vertices.dtype == np.float64 and m.faces.dtype == np.int64
        assert np.array_equal(m.vertices, v) and np.array_equal(m.faces, f)
    rng = np.random.default_rng(1)
    src = mesh.Mesh(rng.normal(size=(31, 3)), rng.integers(0, 31, (40, 3)), rng.normal(size=(31, 3)))
    p = str(tmp_path / 'own.ply')
    src.export(p, 'ply')
    back = mesh_eval.read_ply(p)
    for got, want in ((back.vertices, src.vertices), (back.vertex_normals, src.vertex_normals),
                      (back.faces, src.faces)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert back.vertices.dtype == np.float64 and back.faces.dtype == np.int64
    bad = tmp_path / 'bad.ply'
    bad.write_bytes(b'ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
                    b'element face 1\nproperty list uchar int vertex_indices\nend_header\n'
                    b'0 0 0\n1 0 0\n1 1 0\n3 0 1 3\n')
    with pytest.raises(ValueError, match='face index'):
        mesh.load_ply(str(bad))


def test_workspace_refuses_sizes_out_of_range():
    from monosdf_amd import _lib
    from monosdf_amd.utils.mesh_args import workspace
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    assert _lib.load().msdf_mc_workspace_bytes(1, 1, 1) == -1
    with pytest.raises(ValueError, match='marching_cubes: msdf_mc_workspace_bytes'):
        workspace('marching_cubes', 'msdf_mc_workspace_bytes', 1, 1, 1, device='cpu')
    assert workspace('marching_cubes', 'msdf_mc_workspace_bytes', 4, 4, 4, device='cpu').dtype == torch.uint8


def test_tensor_checks_without_a_gpu():
    from monosdf_amd.utils import mesh_args as ma
    with pytest.raises(TypeError, match=r'f: x must be a CUDA tensor \(there is no CPU path\), got cpu'):
        ma.check_tensor('f', 'x', torch.zeros(4, 3))
    with pytest.raises(TypeError, match='got ndarray'):
        ma.check_tensor('f', 'x', np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError, match='cpu'):
        ma.mesh_tensors('f', (torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32)))
    with pytest.raises(TypeError, match='CUDA'):
        ma.mesh_tensors('f', (np.zeros((4, 3)), torch.zeros(1, 3, dtype=torch.int32)))
    a, b = torch.zeros(1), torch.zeros(1, device='meta')
    assert ma.same_device('f', a=a, b=a) == a.device
    with pytest.raises(ValueError, match='f: a on cpu, b on meta'):
        ma.same_device('f', a=a, b=b)
    assert ma.device_of(np.zeros(3), a, None) is None


def test_positive_number_takes_what_float_takes_and_refuses_the_rest():
    from monosdf_amd.utils import mesh_args as ma
    refused = [(bad, 'positive and finite') for bad in (0, -1.0, float('nan'), float('inf'))]
    for bad, fragment in refused + [('wide', 'a number'), (None, 'a number')]:
        for arg in ('cell', 'radius'):
            with pytest.raises(ValueError, match=r'^radius_thin: %s must be %s, got ' % (arg, fragment)):
                ma.positive_number('radius_thin', arg, bad)
    for value, want in ((1, 1.0), (np.float32(2), 2.0), ('3', 3.0)):
        got = ma.positive_number('f', 'x', value)
        assert type(got) is float and got == want
    assert ma.search_distance('f', 20) == 20.0 and type(ma.search_distance('f', 20)) is float
    with pytest.raises(ValueError, match='^f: max_dist must be finite as a float32'):
        ma.search_distance('f', 1e39)
    with pytest.raises(ValueError, match='^f: max_dist must be positive and finite'):
        ma.search_distance('f', 0)


@pytest.mark.parametrize('form', ['host', 'tensor'])
@pytest.mark.parametrize('with_normals', [False, True])
def test_kept_mesh_equals_indexing_by_hand(form, with_normals):
    from monosdf_amd.utils import mesh_args as ma
    from monosdf_amd.utils.mesh import Mesh
    rng = np.random.default_rng(5)
    v = rng.normal(size=(5, 3)).astype(np.float32)
    n = rng.normal(size=(5, 3))
    f = np.array([[0, 1, 2], [1, 2, 4], [2, 3, 4]], np.int64)
    keep = np.array([True, True, True, False, True])
    faces = ma.compact_faces(torch.from_numpy(keep), torch.from_numpy(f))
    assert faces.tolist() == [[0, 1, 2], [1, 2, 3]]
    wrap = torch.from_numpy if form == 'tensor' else (lambda a: a)
    got = ma.kept_mesh(wrap(v), wrap(n) if with_normals else None, torch.from_numpy(keep), faces)
    assert isinstance(got, Mesh)
    for array, dtype in ((got.vertices, np.float64), (got.vertex_normals, np.float64), (got.faces, np.int64)):
        assert array.dtype == dtype
    assert np.array_equal(got.vertices, v[[0, 1, 2, 4]].astype(np.float64))
    assert np.array_equal(got.faces, np.array([[0, 1, 2], [1, 2, 3]]))
    assert np.array_equal(got.vertex_normals, n[[0, 1, 2, 4]] if with_normals else np.zeros((4, 3)))
    assert isinstance(ma.host_array(torch.zeros(2)), np.ndarray) and ma.host_array(v) is v
