"""CPU tests of the DTU protocol: the numpy restatements (tests/dtu_numpy.py) against the libraries the reference's
scripts call (sklearn's KD-tree radius query, scipy's binary dilation, torch's grid_sample), the ABI table, and the
refusals of utils/mesh_dtu.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import dtu_numpy as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTU_ENTRIES = ('msdf_dtu_dilate_workspace_bytes', 'msdf_dtu_dilate', 'msdf_dtu_mask_vertices',
               'msdf_dtu_lattice_count', 'msdf_dtu_lattice_emit', 'msdf_dtu_thin_workspace_bytes',
               'msdf_dtu_thin_keys', 'msdf_dtu_thin_prepare', 'msdf_dtu_thin_round', 'msdf_dtu_thin_finish')
CASES = dn.thin_cases()
EXPECTED_ROUNDS = {'sorted_chain': 400, 'duplicates': 2}


def _reference_thin(points, radius, order):
    """eval.py:82-94 as written: the cloud in visiting order, sklearn's radius query, the loop over every point."""
    neighbors = pytest.importorskip('sklearn.neighbors')
    order = np.arange(len(points)) if order is None else order
    data = points[order].astype(np.float64)
    engine = neighbors.NearestNeighbors(n_neighbors=1, radius=radius, algorithm='kd_tree')
    engine.fit(data)
    idxs = engine.radius_neighbors(data, radius=radius, return_distance=False)
    mask = np.ones(len(data), bool)
    for curr, near in enumerate(idxs):
        if mask[curr]:
            mask[near] = 0
            mask[curr] = 1
    out = np.zeros(len(points), bool)
    out[order] = mask
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_thinning_restatement_equals_the_reference_code_path(name):
    points, radius, order = CASES[name]
    got = dn.radius_thin(points, radius, order)
    assert np.array_equal(got, _reference_thin(points, radius, order))
    assert 0 < got.sum() < len(points)


@pytest.mark.parametrize('name', sorted(CASES))
def test_round_iteration_equals_the_sequential_greedy(name):
    points, radius, order = CASES[name]
    kept, rounds = dn.thin_rounds(points, radius, order)
    assert np.array_equal(kept, dn.radius_thin(points, radius, order))
    print('%s: %d points, %d kept, %d rounds' % (name, len(points), kept.sum(), rounds))
    if name in EXPECTED_ROUNDS:
        assert rounds == EXPECTED_ROUNDS[name]
    else:
        assert rounds <= 16                                   # logarithmic depth on an unsorted order


def test_thinning_counts_pairs_at_exactly_r():
    pts = np.array([[0, 0, 0], [1.5, 2.0, 0], [1.5, 2.0, 2.5], [4.0, 2.0, 2.5000005]], np.float32)
    assert dn.radius_thin(pts, 2.5).tolist() == [True, False, True, True]         # the last is 5e-7 beyond r
    assert dn.radius_thin(pts, np.nextafter(2.5, 0)).tolist() == [True, True, True, True]


@pytest.mark.parametrize('radius', [1, 5, 12])
def test_dilation_restatement_equals_scipy(radius):
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(radius)
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    disk = (xx * xx + yy * yy) <= radius * radius             # skimage.morphology.disk
    assert [int(r.sum()) for r in disk] == [2 * w + 1 for w in dn.disk_halfwidths(radius).values()]
    corners = np.zeros((37, 70), bool)
    for y in (0, 18, 36):
        for x in (0, 35, 69):
            corners[y, x] = True
    for m in (rng.uniform(size=(37, 70)) < 0.01, corners, np.ones((37, 70), bool), np.zeros((37, 70), bool),
              rng.uniform(size=(9, 100)) < 0.02):
        assert np.array_equal(dn.dilate(m, radius), ndimage.binary_dilation(m, structure=disk))
    stack = rng.uniform(size=(3, 37, 70)) < 0.01
    assert np.array_equal(dn.dilate(stack, radius), np.stack([dn.dilate(m, radius) for m in stack]))


def test_vertex_rule_equals_grid_sample():
    """The restatement against the reference's own lines (evaluate_single_scene.py:71-93) on the CPU.  Vertices whose
    px or py lies within 1e-3 of a half-integer or of 0 / W-1 / H-1 in some view (and within a pixel of that view's
    image) are exempt: there the reference's renormalisation through [-1, 1] may round to the other side.  At most
    1 % may be exempt."""
    # expected share: 2e-3 per axis and view that sees the vertex, about 1 % here; the seed is one that stays below
    proj, masks, verts = dn.ring_scene(seed=5)
    n, h, w = masks.shape
    dilated = dn.dilate(masks, 3)
    kept = dn.mask_vertices(verts, proj, dilated)
    px, py = dn.project(verts, proj)
    P = torch.from_numpy(proj.astype(np.float32))
    hom = torch.cat([torch.from_numpy(verts), torch.ones(len(verts), 1)], 1).permute(1, 0)
    sampled = []
    for i in range(n):
        cam = P[i] @ hom
        pix = (cam[:2] / (cam[2].unsqueeze(0) + 1e-6)).permute(1, 0).contiguous()
        pix[..., 0] /= w - 1
        pix[..., 1] /= h - 1
        pix = (pix - 0.5) * 2
        valid = ((pix > -1.) & (pix < 1.)).all(dim=-1).float()
        maski = torch.from_numpy(dilated[i]).float()[None, None]
        s = torch.nn.functional.grid_sample(maski, pix[None, None], mode='nearest', padding_mode='zeros',
                                            align_corners=True)[0, -1, 0]
        sampled.append(s + (1. - valid))
    ref = (torch.stack(sampled, -1) > 0.).all(dim=-1).numpy()

    def near(p, size):
        with np.errstate(invalid='ignore'):
            return (np.abs(p - np.floor(p) - 0.5) < 1e-3) | (np.abs(p) < 1e-3) | (np.abs(p - (size - 1)) < 1e-3)
    px64, py64 = px.astype(np.float64), py.astype(np.float64)
    with np.errstate(invalid='ignore'):
        around = (px64 > -1) & (px64 < w) & (py64 > -1) & (py64 < h)      # elsewhere both sides call it not valid
    exempt = ((near(px64, w) | near(py64, h)) & around).any(0)
    print('%d of %d vertices exempt; %d kept' % (exempt.sum(), len(verts), kept.sum()))
    assert exempt.mean() <= 0.01
    assert np.array_equal(kept[~exempt], ref[~exempt])
    assert 0.05 < kept.mean() < 0.95


def test_sampler_restatement_on_hand_computable_faces():
    v = np.array([[0, 0, 0], [0.9, 0, 0], [0, 0.9, 0], [0.15, 0, 0], [0, 1, 0], [2, 0, 0]], np.float32)
    # right triangle, n1 = n2 = 4: a + b = (i + j + 1) / 4 reaches 1 exactly at i + j = 3, which the strict < drops
    pts = dn.sample_lattice(v, [[0, 1, 2]], 0.2)
    assert len(pts) == 6
    ij = [(i, j) for i in range(5) for j in range(5) if i + j < 3]
    expect = np.array([[np.float64(np.float32(0.9)) * (i + 0.5) / 4, np.float64(np.float32(0.9)) * (j + 0.5) / 4, 0]
                       for i, j in ij]).astype(np.float32)
    assert np.array_equal(pts, expect)
    assert len(dn.sample_lattice(v, [[0, 3, 4]], 0.2)) == 0          # n1 = 0, n2 = 5: every a is 0.5 / 1e-7
    assert len(dn.sample_lattice(v, [[0, 1, 5]], 0.2)) == 0          # zero area


def test_cull_mesh_reindexes():
    v = np.arange(15, dtype=np.float64).reshape(5, 3)
    f = np.array([[0, 1, 2], [2, 3, 4], [0, 2, 4]])
    kept = np.array([True, False, True, True, True])
    nv, nf = dn.cull_mesh(v, f, kept)
    assert np.array_equal(nv, v[[0, 2, 3, 4]]) and np.array_equal(nf, [[1, 2, 3], [0, 1, 3]])


def test_projections_from_cameras():
    from monosdf_amd.utils.mesh_dtu import dtu_projections
    proj, _, _ = dn.ring_scene(seed=0, n_views=3)
    cams = {}
    for i, P in enumerate(proj):
        scale = np.diag([2.0, 2.0, 2.0, 1.0])
        scale[:3, 3] = [0.1, -0.2, 0.3]
        world = np.concatenate([P * (-3.0 if i == 1 else 5.0), [[0, 0, 0, 1]]]) @ np.linalg.inv(scale)
        cams['world_mat_%d' % i], cams['scale_mat_%d' % i] = world, scale
    got = dtu_projections(cams, 3)
    assert got.shape == (3, 3, 4) and np.abs(got - proj).max() < 1e-4
    assert np.allclose(np.linalg.norm(got[:, 2, :3], axis=1), 1.0)
    with pytest.raises(ValueError, match='world_mat_3'):
        dtu_projections(cams, 4)


def test_dtu_entries_declared_in_header_and_table():
    from monosdf_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'monosdf_hip.h')).read()
    declared = set(re.findall(r'^(?:int|int64_t) (msdf_\w+)\(', text, flags=re.M))
    new = [n for n in _lib.exported_symbols() if n.startswith('msdf_dtu_')]
    assert sorted(new) == sorted(DTU_ENTRIES)
    for name in new:
        assert name in declared, name
        assert len(_lib.signatures('monosdf_hip.h')[name]) > 0
    assert '#define MSDF_ABI_VERSION 8' in text and _lib.ABI_VERSION == 8


def test_refusals_without_a_gpu():
    from monosdf_amd.utils import mesh_dtu as md
    pts = torch.zeros(4, 3)
    faces = torch.zeros(1, 3, dtype=torch.int64)
    img = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match='cpu'):
        md.dilate_masks(img)
    with pytest.raises(TypeError, match='cpu'):
        md.mask_vertices(pts, np.zeros((1, 3, 4)), img)
    with pytest.raises(TypeError, match='cpu'):
        md.sample_lattice(pts, faces)
    with pytest.raises(TypeError, match='cpu'):
        md.radius_thin(pts, 0.2)
    with pytest.raises(TypeError, match='cpu'):
        md.cull_to_masks((pts, faces), np.zeros((1, 3, 4)), img)
    with pytest.raises(TypeError, match='cpu'):
        md.evaluate_dtu(pts, pts, np.ones((2, 2, 2)), np.zeros((2, 3)), 1.0, [0, 0, 1, 0])
    for radius in (0, -1.0, float('nan'), float('inf'), 'wide'):
        with pytest.raises(ValueError, match='radius'):
            md.radius_thin(pts, radius)
    for order in (torch.arange(3), torch.arange(4, dtype=torch.int32), torch.zeros(4, 1, dtype=torch.int64),
                  [0, 1, 2, 3]):
        with pytest.raises(ValueError, match='order'):
            md.radius_thin(pts, 0.2, order)
    for radius in (-1, 33, 2.5):
        with pytest.raises(ValueError, match='radius'):
            md.dilate_masks(img, radius)
    with pytest.raises(ValueError, match='density'):
        md.sample_lattice(pts, faces, 0.0)


def test_read_dtu_scene_and_masks(tmp_path):
    sio = pytest.importorskip('scipy.io')
    from monosdf_amd.utils.mesh import Mesh
    from monosdf_amd.utils.mesh_dtu import read_dtu_scene, read_masks
    rng = np.random.default_rng(0)
    os.makedirs(tmp_path / 'ObsMask')
    os.makedirs(tmp_path / 'Points' / 'stl')
    obs = rng.integers(0, 2, (5, 6, 7)).astype(np.uint8)
    bb = np.array([[-1.5, -2.0, -3.0], [4.0, 5.0, 6.0]])
    sio.savemat(str(tmp_path / 'ObsMask' / 'ObsMask24_10.mat'), {'ObsMask': obs, 'BB': bb, 'Res': 10.0})
    sio.savemat(str(tmp_path / 'ObsMask' / 'Plane24.mat'), {'P': np.array([[0.1], [0.2], [0.9], [-3.0]])})
    stl = rng.normal(size=(30, 3)).astype(np.float32)
    Mesh(stl, np.zeros((0, 3), np.int64)).export(str(tmp_path / 'Points' / 'stl' / 'stl024_total.ply'))
    scene = read_dtu_scene(str(tmp_path), 24)
    assert np.array_equal(scene['obs_mask'], obs) and scene['res'] == 10.0
    assert scene['bb'].dtype == np.float32 and np.array_equal(scene['bb'], bb.astype(np.float32))
    assert np.array_equal(scene['plane'], [0.1, 0.2, 0.9, -3.0])
    assert np.array_equal(scene['stl_points'], stl.astype(np.float64))
    stack = (rng.uniform(size=(3, 8, 9)) < 0.5)
    np.save(str(tmp_path / 'masks.npy'), stack.astype(np.uint8) * 255)
    assert np.array_equal(read_masks(str(tmp_path / 'masks.npy')), stack.astype(np.uint8))
    image = pytest.importorskip('PIL.Image')
    os.makedirs(tmp_path / 'mask')
    for k in (2, 0, 1):
        rgb = np.repeat((stack[k].astype(np.uint8) * 255)[..., None], 3, axis=2)
        image.fromarray(rgb).save(str(tmp_path / 'mask' / ('%03d.png' % k)))
    assert np.array_equal(read_masks(str(tmp_path / 'mask')), stack.astype(np.uint8))
