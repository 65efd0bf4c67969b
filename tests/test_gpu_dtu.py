"""GPU tests of the DTU protocol (csrc/dtueval.hip, utils/mesh_dtu.py) against the numpy restatements of
tests/dtu_numpy.py.  Every comparison is exact unless a tolerance is stated."""
import os
import sys

import numpy as np
import pytest
import torch

import dtu_numpy as dn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

THIN_CASES = dn.thin_cases()


def _md():
    from monosdf_amd.utils import mesh_dtu
    return mesh_dtu


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---------------------------------------------------------------- dilation

def _small_masks():
    """name -> [3, 37, 70] uint8: 70 is no multiple of the 32-bit word and more than one word; 37 is under 2 r + 1
    for r = 12 x 2 and over it for r = 1, 5 and 12."""
    rng = np.random.default_rng(0)
    h, w = 37, 70
    out = {'empty': np.zeros((3, h, w), np.uint8), 'full': np.full((3, h, w), 255, np.uint8),
           'random': (rng.uniform(size=(3, h, w)) < 0.01).astype(np.uint8) * 200}
    single = np.zeros((9, h, w), np.uint8)
    for k, (y, x) in enumerate([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2),
                                (h // 2, 0), (h // 2, w - 1), (h // 2, w // 2)]):
        single[k, y, x] = 1
    for k in range(3):
        out['single_%d' % k] = single[3 * k:3 * k + 3]
    return out


@pytest.mark.parametrize('radius', [1, 5, 12])
def test_dilation_equals_restatement(radius):
    for name, m in _small_masks().items():
        got = _md().dilate_masks(torch.from_numpy(m).cuda(), radius)
        assert got.dtype == torch.uint8 and got.shape == m.shape
        assert np.array_equal(got.cpu().numpy(), dn.dilate(m, radius).astype(np.uint8)), name
    m = _small_masks()['random']
    as_bool = _md().dilate_masks(torch.from_numpy(m != 0).cuda(), radius)
    assert np.array_equal(as_bool.cpu().numpy(), dn.dilate(m, radius).astype(np.uint8))


def test_dilation_at_the_protocol_size():
    m = (np.random.default_rng(1).uniform(size=(1, 1200, 1600)) < 0.001).astype(np.uint8)
    got = _md().dilate_masks(torch.from_numpy(m).cuda(), 12)
    assert np.array_equal(got.cpu().numpy(), dn.dilate(m, 12).astype(np.uint8))
    assert torch.equal(got, _md().dilate_masks(torch.from_numpy(m).cuda(), 12))
    none = _md().dilate_masks(torch.zeros(0, 5, 5, dtype=torch.uint8, device='cuda'))
    assert none.shape == (0, 5, 5)


# ---------------------------------------------------------------- vertex rule, cull

def test_vertex_rule_equals_restatement():
    proj, masks, verts = dn.ring_scene(seed=5)
    dilated = dn.dilate(masks, 3)
    kept, seen = dn.mask_vertices(verts, proj, dilated, reasons=True)
    shares = {'culled': (~kept).mean(), 'kept, valid in no view': (kept & ~seen).mean(),
              'kept by the masks': (kept & seen).mean()}
    print(shares)
    assert min(shares.values()) >= 0.05
    d_gpu = _md().dilate_masks(torch.from_numpy(masks).cuda(), 3)
    got = _md().mask_vertices(_cuda(verts), proj, d_gpu)
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), kept)
    assert np.array_equal(_md().mask_vertices(_cuda(verts), torch.from_numpy(proj), d_gpu.bool()).cpu().numpy(), kept)
    assert _md().mask_vertices(_cuda(verts[:0]), proj, d_gpu).shape == (0,)


def test_cull_to_masks_drops_vertices_and_reindexes():
    from monosdf_amd.utils.mesh import Mesh
    proj, masks, verts = dn.ring_scene(seed=6, n_vertices=300)
    rng = np.random.default_rng(2)
    faces = rng.integers(0, len(verts), (500, 3))
    faces[:150] = np.argsort(np.abs(verts).max(1))[rng.integers(0, 60, (150, 3))]     # faces near the ball survive
    normals = rng.normal(size=(len(verts), 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    kept = dn.mask_vertices(verts, proj, dn.dilate(masks, 3))
    ev, ef = dn.cull_mesh(verts.astype(np.float64), faces, kept)
    assert 0 < len(ev) < len(verts) and 0 < len(ef) < len(faces)
    out = _md().cull_to_masks(Mesh(verts, faces, normals), proj, masks, radius=3)
    assert np.array_equal(out.vertices, ev) and np.array_equal(out.faces, ef)
    assert np.array_equal(out.vertex_normals, normals[kept])
    assert out.faces.min() >= 0 and out.faces.max() < len(out.vertices)
    pair = _md().cull_to_masks((_cuda(verts), _cuda(faces, np.int64)), proj, torch.from_numpy(masks).cuda(), radius=3)
    assert np.array_equal(pair.vertices, ev) and np.array_equal(pair.faces, ef)


# ---------------------------------------------------------------- lattice sampler

def _sampler_meshes():
    rng = np.random.default_rng(3)
    v = np.array([[0, 0, 0], [0.9, 0, 0], [0, 0.9, 0], [0.15, 0, 0], [0, 1, 0], [2, 0, 0],
                  [0.1, 0.2, 0.3], [8.2, 0.5, 0.1], [0.7, 8.4, 1.0]], np.float32)
    rv = rng.uniform(0, 0.6, (1500, 3)).astype(np.float32)
    rf = rng.integers(0, 1500, (3000, 3))
    rf[::97] = rf[::97, [0, 0, 2]]                                      # some faces with a repeated vertex
    return {
        'zero_area': (v, [[0, 1, 5]], 0.2),
        'n1_zero': (v, [[0, 3, 4]], 0.2),
        'strict_less': (v, [[0, 1, 2]], 0.2),
        'n40': (v, [[6, 7, 8]], 0.2),
        'n160': (v, [[6, 7, 8]], 0.05),
        'mixed': (v, [[0, 1, 5], [6, 7, 8], [0, 3, 4], [0, 1, 2], [8, 6, 7], [2, 1, 0]], 0.2),
        'random_3000': (rv, rf, 0.2),
        'all_degenerate': (v, [[0, 1, 5], [0, 0, 1], [3, 3, 3]], 0.2),
    }


@pytest.mark.parametrize('name', sorted(_sampler_meshes()))
def test_sampler_equals_restatement(name):
    v, f, density = _sampler_meshes()[name]
    expect = dn.sample_lattice(v, f, density)
    got = _md().sample_lattice(_cuda(v), _cuda(f, np.int64), density)
    print('%s: %d points from %d faces' % (name, len(expect), len(f)))
    assert got.dtype == torch.float32 and got.shape == expect.shape
    assert np.array_equal(got.cpu().numpy(), expect)
    assert {'zero_area': 0, 'n1_zero': 0, 'strict_less': 6, 'all_degenerate': 0}.get(name, len(expect)) == len(expect)
    if name == 'n40':
        assert 500 < len(expect) < 1500
    if name == 'random_3000':
        again = _md().sample_lattice(_cuda(v), _cuda(f, np.int32), density)
        assert torch.equal(got, again)


def test_sampler_refuses_bad_faces_and_too_many_points():
    v = _cuda([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    with pytest.raises(ValueError, match='face index'):
        _md().sample_lattice(v, _cuda([[0, 1, 3]], np.int64))
    with pytest.raises(ValueError, match='2\\^31'):
        _md().sample_lattice(v * 1000, _cuda([[0, 1, 2]], np.int64), 0.001)
    assert _md().sample_lattice(v, _cuda(np.zeros((0, 3)), np.int64)).shape == (0, 3)


# ---------------------------------------------------------------- thinning

def _thin_gpu(points, radius, order=None):
    o = None if order is None else torch.from_numpy(np.asarray(order, np.int64)).cuda()
    return _md().radius_thin(_cuda(points), radius, o, return_rounds=True)


@pytest.mark.parametrize('name', sorted(THIN_CASES))
def test_thinning_equals_sequential_greedy(name):
    points, radius, order = THIN_CASES[name]
    expect = dn.radius_thin(points, radius, order)
    keep, rounds = _thin_gpu(points, radius, order)
    print('%s: %d points, %d kept, %d rounds' % (name, len(points), expect.sum(), rounds))
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), expect)
    again, _ = _thin_gpu(points, radius, order)
    assert torch.equal(keep, again)
    assert rounds <= (400 if name == 'sorted_chain' else 16)


@pytest.mark.parametrize('n', [0, 1, 257, 1025])
def test_thinning_sizes_and_orders(n):
    rng = np.random.default_rng(n)
    points = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    radius = 0.12
    for order in (None, np.arange(n)[::-1].copy(), rng.permutation(n)):
        keep, _ = _thin_gpu(points, radius, order)
        assert keep.shape == (n,)
        assert np.array_equal(keep.cpu().numpy(), dn.radius_thin(points, radius, order))


def test_thinning_negative_coordinates_straddling_cell_faces():
    """Points a few ulps either side of the faces of the cell grid (whose origin is the cloud's minimum), at negative
    coordinates: neighbours within r then lie in different cells."""
    rng = np.random.default_rng(11)
    radius = 0.25
    cell = radius * (1 + 2.0 ** -10)
    k = rng.integers(0, 8, (1500, 3))
    jitter = rng.choice([-3e-7, -1e-7, 0.0, 1e-7, 3e-7, 0.05, -0.05, 0.12], (1500, 3))
    points = np.concatenate([[[-2.0, -2.0, -2.0]], -2.0 + k * cell + jitter]).astype(np.float32)
    points = np.maximum(points, np.float32(-2.0))
    order = rng.permutation(len(points))
    expect = dn.radius_thin(points, radius, order)
    keep, rounds = _thin_gpu(points, radius, order)
    assert np.array_equal(keep.cpu().numpy(), expect) and 0 < expect.sum() < len(points)
    assert np.array_equal(_thin_gpu(points, radius)[0].cpu().numpy(), dn.radius_thin(points, radius))


def test_thinning_refuses_a_bad_order():
    pts = _cuda(np.zeros((4, 3)))
    for bad in ([0, 1, 2, 2], [0, 1, 2, 4], [-1, 0, 1, 2]):
        with pytest.raises(ValueError, match='permutation'):
            _md().radius_thin(pts, 0.2, torch.tensor(bad, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError, match='order on'):
        _md().radius_thin(pts, 0.2, torch.arange(4))


# ---------------------------------------------------------------- protocol

def _icosphere(radius, subdivisions):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int64)


@pytest.fixture(scope='module')
def protocol():
    """An icosphere of radius 30 against an stl cloud on radius 30.5; the box of ``bb`` and ``patch`` cuts the sphere,
    the observation mask covers half the grid, the plane passes through the centre and ``max_dist`` drops the stl
    points over the part that the box cut away."""
    from monosdf_amd.utils.mesh import Mesh
    rng = np.random.default_rng(5)
    verts, faces = _icosphere(30.0, 2)
    d = rng.normal(size=(4000, 3))
    stl = (30.5 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    obs = np.zeros((21, 21, 21), np.uint8)
    obs[:11] = 1
    args = dict(obs_mask=obs, bb=np.array([[-20, -20, -20], [20, 20, 20]], np.float32), res=2.0,
                plane=np.array([0.0, 0.0, 1.0, 0.0]), density=2.0, patch=5, max_dist=3)
    metrics, clouds = _md().evaluate_dtu(Mesh(verts, faces), stl, seed=3, return_clouds=True, **args)
    cloud = np.concatenate([verts, dn.sample_lattice(verts, faces, 2.0)])
    order = clouds['order'].cpu().numpy()
    expect = dn.evaluate(cloud, order, stl, **{k: v for k, v in args.items()})
    return dict(verts=verts, faces=faces, stl=stl, args=args, metrics=metrics, clouds=clouds, cloud=cloud,
                order=order, expect=expect)


def _close(got, want, scale):
    return abs(got - want) <= 1e-6 * want + 1e-7 * scale


def test_protocol_stages_equal_restatement(protocol):
    p = protocol
    clouds, (want, stages) = p['clouds'], p['expect']
    assert np.array_equal(clouds['data_pcd'].cpu().numpy(), p['cloud'])
    assert sorted(p['order'].tolist()) == list(range(len(p['cloud'])))
    assert np.array_equal(clouds['keep'].cpu().numpy(), stages['keep'])
    for k in ('data_in', 'data_in_obs', 'stl_above'):
        assert np.array_equal(clouds[k].cpu().numpy(), stages[k]), k
    n = [len(p['cloud']), int(stages['keep'].sum()), len(stages['data_in']), len(stages['data_in_obs']),
         len(stages['stl_above'])]
    print('cloud %d, thinned %d, inbound %d, observed %d, stl above %d' % tuple(n))
    assert n[0] > n[1] > n[2] > n[3] > 0 and 0 < n[4] < len(p['stl'])
    assert (stages['dist_s2d'] >= 3).any() and (stages['dist_s2d'] < 3).any()
    scale = 31.0
    print(p['metrics'], want)
    assert set(p['metrics']) == {'d2s', 's2d', 'overall'}
    for k in ('d2s', 's2d', 'overall'):
        assert isinstance(p['metrics'][k], float) and _close(p['metrics'][k], want[k], scale), k


def test_protocol_is_repeatable_and_takes_an_order(protocol):
    from monosdf_amd.utils.mesh import Mesh
    p = protocol
    again = _md().evaluate_dtu((_cuda(p['verts']), _cuda(p['faces'], np.int64)), _cuda(p['stl']), seed=3, **p['args'])
    assert again == p['metrics']
    given = _md().evaluate_dtu(Mesh(p['verts'], p['faces']), p['stl'], order=p['clouds']['order'], **p['args'])
    assert given == p['metrics']
    other = _md().evaluate_dtu(Mesh(p['verts'], p['faces']), p['stl'], seed=4, return_clouds=True, **p['args'])[1]
    assert not torch.equal(other['order'], p['clouds']['order'])


def test_protocol_pcd_mode(protocol):
    p = protocol
    got, clouds = _md().evaluate_dtu(_cuda(p['cloud']), p['stl'], order=p['clouds']['order'], return_clouds=True,
                                     **p['args'])
    assert got == p['metrics']
    assert torch.equal(clouds['keep'], p['clouds']['keep'])
    from_numpy = _md().evaluate_dtu(p['cloud'], p['stl'], order=p['clouds']['order'], **p['args'])
    assert from_numpy == p['metrics']
