"""GPU test of the mesh intake of utils/mesh_args.py: CUDA tensors are checked in one device reduction, and a mesh
gives the same results whether it arrives as numpy arrays or as the tensors they upload to.  No function that indexes
device memory with the faces is handed a bad mesh here: that they all go through the intake is checked by reading."""
import os
import sys

import numpy as np
import pytest
import torch

import dtu_numpy as dn
import refuse_numpy as rfn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TETRAHEDRON = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64),
               np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64))


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def test_intake_of_cuda_tensors_and_of_numpy_arrays_agree():
    from monosdf_amd.utils import mesh_args as ma, mesh_dtu as md, mesh_eval as me
    for v, f in (TETRAHEDRON, rfn.icosphere(0, 0.5, (0, 0, 0))):
        for index_type in (np.int32, np.int64):
            tv, tf = _cuda(v, np.float32), _cuda(f, index_type)
            gv, gf, normals = ma.mesh_tensors('test', (tv, tf))
            assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and normals is None
            assert gv.is_contiguous() and gf.is_contiguous() and gv.device == tv.device and gf.device == tv.device
            assert torch.equal(gv, tv) and torch.equal(gf.long(), tf.long())
        hv, hf, _ = ma.mesh_tensors('test', (v, f), tv.device)           # the host form uploads to the same tensors
        assert hv.dtype == torch.float32 and hf.dtype == torch.int32 and torch.equal(hv, gv) and torch.equal(hf, gf)
        sliced = torch.stack([tv, tv], 1)[:, 0]                          # not contiguous
        assert not sliced.is_contiguous() and ma.mesh_tensors('test', (sliced, tf))[0].is_contiguous()
        for bad_index in (len(v), -1):
            bad = tf.clone()
            bad[-1, 1] = bad_index
            with pytest.raises(ValueError, match=r'test: face index outside \[0, %d\)' % len(v)):
                ma.mesh_tensors('test', (tv, bad))
        for value in (float('nan'), float('inf')):
            bad = tv.clone()
            bad[1, 2] = value
            with pytest.raises(ValueError, match='test: non-finite'):
                ma.mesh_tensors('test', (bad, tf))
        assert ma.mesh_tensors('test', (tv, tf[:0]))[1].shape == (0, 3)

    inner, outer = rfn.icosphere(2, 0.5, (0, 0, 0)), rfn.icosphere(2, 0.52, (0, 0, 0))
    as_tensors = [(_cuda(v, np.float32), _cuda(f, np.int64)) for v, f in (inner, outer)]
    from_numpy = me.evaluate_replica(inner, outer, n_samples=2000, seed=3)
    from_tensors = me.evaluate_replica(*as_tensors, n_samples=2000, seed=3)
    assert from_numpy == from_tensors
    # in cm: the shells are 2 cm apart (their facets a little less), and 2000 samples on 3 m^2 lie about 4 cm apart
    assert 1.5 < from_numpy['accuracy'] < 10 and 1.5 < from_numpy['completion'] < 10 and from_numpy['normal_avg'] > 90

    proj, masks, verts = dn.ring_scene(seed=6, n_vertices=300)
    rng = np.random.default_rng(2)
    faces = rng.integers(0, len(verts), (500, 3))
    faces[:150] = np.argsort(np.abs(verts).max(1))[rng.integers(0, 60, (150, 3))]
    a = md.cull_to_masks((verts, faces), proj, masks, radius=3)
    b = md.cull_to_masks((_cuda(verts, np.float32), _cuda(faces, np.int64)), proj, torch.from_numpy(masks).cuda(),
                         radius=3)
    assert 0 < len(a.vertices) < len(verts) and 0 < len(a.faces) < len(faces)
    assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces)
