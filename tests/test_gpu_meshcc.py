"""GPU tests of the mesh connected components (csrc/meshcc.hip, utils/mesh_clean.py) and of the aligned high-res
export (utils/mesh.get_surface_high_res_mesh).  The labels are unique, so every comparison with the restatement
(tests/meshcc_numpy.py) on the constructed inputs (tests/meshcc_cases.py) is ``torch.equal``."""
import os
import sys

import numpy as np
import pytest
import torch

import meshcc_cases as cases
import meshcc_numpy as cc

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_CACHE = {}


def _mc():
    from monosdf_amd.utils import mesh_clean
    return mesh_clean


def _mesh():
    from monosdf_amd.utils import mesh
    return mesh


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _gpu_marching_cubes(vol, level, spacing):
    v, f, n = _mesh().marching_cubes(torch.from_numpy(vol).cuda(), level, spacing)
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def _cases():
    """Every constructed case, the marching-cubes one from the project's own marching_cubes; built once."""
    if not _CACHE:
        mc_case, normals = cases.mc_case(_gpu_marching_cubes)
        for c in cases.tiny_cases() + cases.strip_cases() + [cases.tetrahedra_case(), cases.soup_case(),
                                                             cases.vertex_soup_case(), mc_case]:
            _CACHE[c.name] = c
        _CACHE['#normals'] = normals
    return _CACHE


CASE_NAMES = sorted(c.name for c in cases.all_cases())


def _pair(case):
    return _cuda(case.vertices, np.float32), _cuda(case.faces, np.int64)


def _want(case, rule):
    key = ('#labels', case.name, rule)
    if key not in _CACHE:
        _CACHE[key] = cc.face_components(case.faces, len(case.vertices), rule)
    return _CACHE[key]


# ---------------------------------------------------------------- labels

@pytest.mark.parametrize('rule', cc.RULES)
@pytest.mark.parametrize('name', CASE_NAMES)
def test_labels_equal_the_restatement(name, rule):
    case = _cases()[name]
    case.structure(case)
    want, want_count = _want(case, rule)
    mesh = _pair(case)
    labels, count = _mc().face_components(mesh, rule)
    assert labels.dtype == torch.int64 and labels.is_cuda and labels.shape == (len(case.faces),)
    assert isinstance(count, int) and count == want_count
    assert torch.equal(labels.cpu(), torch.from_numpy(want))
    again, count2 = _mc().face_components(mesh, rule)
    assert count2 == count and torch.equal(again, labels)
    if name.startswith('strip'):
        assert count == 1 and int(labels.max()) == 0


def test_int32_faces_and_host_meshes_give_the_same_labels():
    case = _cases()['soup']
    want = torch.from_numpy(_want(case, 'edge')[0])
    v, f = _pair(case)
    assert torch.equal(_mc().face_components((v, f.int()), 'edge')[0].cpu(), want)
    assert torch.equal(_mc().face_components((case.vertices, case.faces), 'edge')[0].cpu(), want)
    host = _mesh().Mesh(case.vertices, case.faces)
    assert torch.equal(_mc().face_components(host, 'edge')[0].cpu(), want)


# ---------------------------------------------------------------- sizes

@pytest.mark.parametrize('rule', cc.RULES)
@pytest.mark.parametrize('name', ['empty', 'one face', 'strip bit-reversed', 'tetrahedra', 'soup',
                                  'interleaved soups', 'marching cubes'])
def test_component_sizes(name, rule):
    """Face counts equal; areas within (n_s - 1) 2^-53 relative of the fsum of the per-face areas -- the bound of an
    fp64 sum of n_s non-negative terms in any order.  The per-face areas are the device's (0.5 |e1 x e2| in fp64),
    which the integer-coordinate cases pin bitwise to numpy's and the marching-cubes case to rounding."""
    case = _cases()[name]
    want_labels, n = _want(case, rule)
    mesh = _pair(case)
    labels, count = _mc().face_components(mesh, rule)
    faces, area = _mc().component_sizes(mesh, labels, count)
    assert faces.dtype == torch.int64 and area.dtype == torch.float64 and faces.shape == area.shape == (n,)
    per_face = _mc().face_areas(mesh).cpu().numpy()
    restated = cc.face_areas(case.vertices, case.faces)
    if name == 'marching cubes':
        # every product of the cross product is at most |e1| |e2| <= 3 h^2 and is rounded to 2^-53 of that, fused or
        # not (a sliver's area is a difference of such products: no relative bound holds); 2^-48 leaves 10x room
        assert np.abs(per_face - restated).max() <= 2.0 ** -48 * 3 * cases.mc_volume()[1] ** 2
    else:
        assert np.array_equal(per_face, restated)                 # small integers: every operation is exact or sqrt
    want_faces, want_area = cc.component_sizes(per_face, want_labels, n)
    assert torch.equal(faces.cpu(), torch.from_numpy(want_faces))
    got = area.cpu().numpy()
    bound = (want_faces - 1) * 2.0 ** -53 * want_area
    worst = float(np.max(np.abs(got - want_area) / np.maximum(want_area, 1e-300))) if n else 0.0
    print('%s / %s: %d components, largest %d faces, worst relative area error %.3g' %
          (name, rule, n, int(want_faces.max()) if n else 0, worst))
    assert (np.abs(got - want_area) <= bound).all()
    faces2, area2 = _mc().component_sizes(mesh, labels, count)
    assert torch.equal(faces2, faces) and torch.equal(area2.view(torch.int64), area.view(torch.int64))


def test_segment_sum_is_a_fixed_tree_on_a_long_segment():
    """One segment of 100 003 terms between two short ones and an empty one: more than one pass of the workgroup's
    512 lanes, a tail, and the same bits on every call."""
    from monosdf_amd.utils import mesh_args as ma
    rng = np.random.default_rng(9)
    sizes = [3, 100003, 0, 700]
    values = rng.uniform(0.0, 1.0, sum(sizes)) * 10.0 ** rng.integers(-6, 3, sum(sizes))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    v, s = _cuda(values, np.float64), _cuda(start, np.int64)
    outs = []
    for _ in range(2):
        out = torch.full((len(sizes),), -1.0, dtype=torch.float64, device='cuda')
        ma.call('msdf_mcc_segment_sum', v, s, len(sizes), out)
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))
    import math
    want = np.array([math.fsum(values[a:b].tolist()) for a, b in zip(start[:-1], start[1:])])
    bound = np.maximum(np.array(sizes) - 1, 0) * 2.0 ** -53 * want
    assert (np.abs(outs[0].cpu().numpy() - want) <= bound).all() and outs[0][2].item() == 0.0


# ---------------------------------------------------------------- largest_component, remove_small_components

def _marked_mesh(case):
    """A Mesh whose normal of vertex i is (i, 2 i, 3 i): a normal that follows its vertex names it."""
    marks = np.arange(len(case.vertices), dtype=np.float64)[:, None] * np.array([[1.0, 2.0, 3.0]])
    return _mesh().Mesh(case.vertices.astype(np.float64), case.faces, marks), marks


@pytest.mark.parametrize('by', ['area', 'faces'])
def test_largest_component_of_the_marching_cubes_scene(by):
    case = _cases()['marching cubes']
    labels, n = _want(case, 'edge')
    count, area = cc.component_sizes(cc.face_areas(case.vertices, case.faces), labels, n)
    best = cc.largest(area if by == 'area' else count)
    used, faces = cc.select(case.vertices, case.faces, labels == best)
    assert abs(area[best] - cases.MC_AREAS['torus']) <= cases.MC_AREA_RTOL * cases.MC_AREAS['torus']
    mesh, marks = _marked_mesh(case)
    out = _mc().largest_component(mesh, 'edge', by)
    assert isinstance(out, _mesh().Mesh)
    assert np.array_equal(out.faces, faces) and out.faces.dtype == np.int64            # original order, re-indexed
    assert np.array_equal(out.vertices, case.vertices[used].astype(np.float64))         # compacted
    assert np.array_equal(out.vertex_normals, marks[used])                              # normals follow
    assert len(np.unique(out.faces)) == len(out.vertices) < len(case.vertices)
    pair = _mc().largest_component(_pair(case), 'edge', by)
    assert np.array_equal(pair.faces, faces) and np.array_equal(pair.vertices, out.vertices)


def test_remove_small_components():
    case = _cases()['marching cubes']
    labels, n = _want(case, 'edge')
    count, area = cc.component_sizes(cc.face_areas(case.vertices, case.faces), labels, n)
    mesh, marks = _marked_mesh(case)
    order = np.argsort(area)
    cut_area = 0.5 * (area[order[0]] + area[order[1]])                # drops the smallest component only
    cut_faces = int(np.sort(count)[1]) + 1                            # keeps the component with most faces only
    for kwargs, keep in (({'min_area': cut_area}, area >= cut_area), ({'min_faces': cut_faces}, count >= cut_faces),
                         ({'min_area': cut_area, 'min_faces': cut_faces}, (area >= cut_area) & (count >= cut_faces)),
                         ({'min_faces': 1}, count >= 1), ({'min_area': 1e9}, area >= 1e9)):
        used, faces = cc.select(case.vertices, case.faces, keep[labels])
        out = _mc().remove_small_components(mesh, connectivity='edge', **kwargs)
        assert np.array_equal(out.faces, faces.reshape(-1, 3)), kwargs
        assert np.array_equal(out.vertices, case.vertices[used].astype(np.float64)), kwargs
        assert np.array_equal(out.vertex_normals, marks[used]), kwargs
    assert len(_mc().remove_small_components(mesh, min_area=1e9).vertices) == 0


def test_a_tie_goes_to_the_lower_index():
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    local = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    verts = np.concatenate([corner + 4, corner])                       # the first component uses the later vertices
    faces = np.stack([local, local + 4], 1).reshape(-1, 3)[[1, 0, 2, 3, 4, 5, 6, 7]]
    labels, n = cc.face_components(faces, 8, 'edge')
    assert n == 2 and labels[0] == 0 and faces[0].min() >= 4
    for by in ('area', 'faces'):
        out = _mc().largest_component((_cuda(verts, np.float32), _cuda(faces, np.int64)), 'edge', by)
        assert np.array_equal(out.faces, cc.select(verts, faces, labels == 0)[1])
        assert np.array_equal(out.vertices, verts[4:].astype(np.float64))
    mesh = (_cuda(verts, np.float32), _cuda(faces, np.int64))
    got = _mc().component_sizes(mesh, *_mc().face_components(mesh))
    assert got[0].tolist() == [4, 4] and got[1][0].item() == got[1][1].item()


def test_empty_mesh_comes_back_empty():
    v = torch.zeros(3, 3, device='cuda')
    f = torch.zeros(0, 3, dtype=torch.int64, device='cuda')
    labels, n = _mc().face_components((v, f))
    assert n == 0 and labels.shape == (0,) and labels.dtype == torch.int64
    out = _mc().largest_component((v, f))
    assert len(out.faces) == 0 and len(out.vertices) == 0
    count, area = _mc().component_sizes((v, f), labels, 0)
    assert count.shape == area.shape == (0,)


# ---------------------------------------------------------------- merge_vertices

def _patches(shift):
    """Two unit-square patches of 4 x 4 cells meeting along x = 1, each with its own vertices; the second patch's seam
    vertices are displaced by ``shift`` along x.  fp64."""
    n = 4
    g = np.arange(n + 1) / n
    x, y = np.meshgrid(g, g, indexing='ij')
    a = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1)
    b = a + np.array([[1.0, 0.0, 0.0]])
    b[: n + 1, 0] += shift                                            # x index 0 of the second patch: the seam
    cell = np.array([[i * (n + 1) + j for j in range(n)] for i in range(n)]).ravel()
    quads = np.stack([cell, cell + n + 1, cell + n + 2, cell, cell + n + 2, cell + 1], 1).reshape(-1, 3)
    return np.concatenate([a, b]), np.concatenate([quads, quads + len(a)])


def test_merge_vertices_closes_a_seam():
    verts, faces = _patches(3e-7)
    normals = np.arange(len(verts), dtype=np.float64)[:, None] * np.ones((1, 3))
    mesh = _mesh().Mesh(verts, faces, normals)
    assert _mc().face_components(mesh, 'edge')[1] == 2
    for digits, n_components, n_merged in ((8, 2, 0), (5, 1, 5)):
        kept, want_faces = cc.merge_vertices(verts, faces, digits)
        assert len(kept) == len(verts) - n_merged
        out = _mc().merge_vertices(mesh, digits)
        assert np.array_equal(out.vertices, verts[kept])               # the first of each group, in ascending order
        assert np.array_equal(out.vertex_normals, normals[kept])
        assert np.array_equal(out.faces, want_faces) and len(out.faces) == len(faces)
        assert _mc().face_components(out, 'edge')[1] == n_components
    # CUDA fp32 vertices are keyed by their exact values
    v32 = verts.astype(np.float32)
    kept, want_faces = cc.merge_vertices(v32.astype(np.float64), faces, 5)
    out = _mc().merge_vertices((_cuda(v32, np.float32), _cuda(faces, np.int64)), 5)
    assert len(kept) == len(verts) - 5 and np.array_equal(out.vertices, v32[kept].astype(np.float64))
    assert np.array_equal(out.faces, want_faces)


# ---------------------------------------------------------------- get_surface_high_res_mesh

CAP_C = np.array([0.1, -0.05, 0.0])
CAP_U = np.array([1.0, 0.6, 0.4]) / np.linalg.norm([1.0, 0.6, 0.4])
CAP_R, CAP_HALF = 0.3, 0.8
_PERP = np.cross(CAP_U, [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(CAP_U, [0.0, 0.0, 1.0]))
SPH_C, SPH_R = CAP_C + 0.8 * _PERP, 0.1                # 0.8 from the axis: see test_high_res_mesh_scene
RESOLUTION = 64


def _capsule_np(p):
    d = p - CAP_C
    t = np.clip(d @ CAP_U, -CAP_HALF, CAP_HALF)
    return np.linalg.norm(d - t[:, None] * CAP_U, axis=1) - CAP_R


def _sphere_np(p):
    return np.linalg.norm(p - SPH_C, axis=1) - SPH_R


class _Scene:
    """min(capsule, sphere), both exact distances, on CUDA tensors; counts the points it is asked for."""

    def __init__(self):
        self.c, self.u, self.s = (torch.tensor(a, dtype=torch.float32, device='cuda') for a in (CAP_C, CAP_U, SPH_C))
        self.points = 0

    def __call__(self, p):
        assert p.is_cuda and p.dtype == torch.float32 and p.dim() == 2 and p.shape[1] == 3
        self.points += p.shape[0]
        d = p - self.c
        t = (d @ self.u).clamp(-CAP_HALF, CAP_HALF)
        capsule = (d - t[:, None] * self.u).norm(dim=1) - CAP_R
        return torch.minimum(capsule, (p - self.s).norm(dim=1) - SPH_R)


def _high_res(take_components):
    key = ('#high res', take_components)
    if key not in _CACHE:
        scene = _Scene()
        frame = _mesh().high_res_grid(scene, RESOLUTION, take_components=take_components, seed=0)
        coarse = scene.points
        mesh = _mesh().get_surface_high_res_mesh(scene, RESOLUTION, take_components=take_components, seed=0)
        _CACHE[key] = (frame, mesh, coarse, scene.points - 2 * coarse)
    return _CACHE[key]


def test_high_res_mesh_scene():
    """The sphere lies outside the capsule's aligned box plus eps plus one step whatever the two short axes of the
    frame are: the box reaches at most sqrt(2) (0.3 + 0.1 + h) + slack from the capsule's axis, the sphere starts at
    0.8 - 0.1 from it."""
    (mean, rot, axes), mesh, coarse, fine = _high_res(True)
    h = axes[0][1] - axes[0][0]
    assert 2 ** 0.5 * (CAP_R + 0.1 + 2 * h) < 0.8 - SPH_R - h
    assert coarse == 100 ** 3 and fine == len(axes[0]) * len(axes[1]) * len(axes[2])
    # the frame: a rotation, one row along the capsule; the mean near its centre
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-12) and np.linalg.det(rot) > 0
    along = np.abs(rot @ CAP_U)
    assert along.max() > 0.999 and np.linalg.norm(mean - CAP_C) < 0.05
    lengths = sorted(len(a) for a in axes)
    assert lengths[0] == RESOLUTION and lengths[1] >= RESOLUTION and lengths[2] > 2 * RESOLUTION
    assert len(axes[int(along.argmax())]) == lengths[2]


def test_high_res_mesh_keeps_the_capsule_only():
    (_, _, axes), mesh, _, _ = _high_res(True)
    h = axes[0][1] - axes[0][0]
    assert mesh is not None and len(mesh.faces) > 10000 and mesh.vertices.dtype == np.float64
    cap, sph = np.abs(_capsule_np(mesh.vertices)), np.abs(_sphere_np(mesh.vertices))
    print('h = %.5f, max |capsule sdf| = %.3g h, min |sphere sdf| = %.3g h' % (h, cap.max() / h, sph.min() / h))
    assert (cap <= h).all()
    assert not (sph <= h).any()
    # unit normals, rotated into the world with the vertices: they point along the capsule's gradient
    d = mesh.vertices - CAP_C
    t = np.clip(d @ CAP_U, -CAP_HALF, CAP_HALF)
    grad = d - t[:, None] * CAP_U
    grad /= np.linalg.norm(grad, axis=1, keepdims=True)
    assert ((mesh.vertex_normals * grad).sum(1) > 0.9).all()


def test_high_res_mesh_without_the_filter_reaches_the_sphere():
    (_, _, axes), mesh, _, _ = _high_res(False)
    h = axes[0][1] - axes[0][0]
    sdf = np.minimum(_capsule_np(mesh.vertices), _sphere_np(mesh.vertices))
    assert (np.abs(sdf) <= h).all()
    assert (np.abs(_sphere_np(mesh.vertices)) <= h).any()
    assert min(len(a) for a in axes) == RESOLUTION


def test_high_res_mesh_is_reproducible():
    _, mesh, _, _ = _high_res(True)
    again = _mesh().get_surface_high_res_mesh(_Scene(), RESOLUTION, take_components=True, seed=0)
    assert np.array_equal(again.vertices, mesh.vertices) and np.array_equal(again.faces, mesh.faces)
    assert np.array_equal(again.vertex_normals, mesh.vertex_normals)


def test_high_res_mesh_of_an_all_positive_sdf_is_none():
    assert _mesh().get_surface_high_res_mesh(lambda p: p.norm(dim=1) + 0.5, 16) is None


# ---------------------------------------------------------------- argument errors

def test_argument_errors_name_the_function():
    mc = _mc()
    v = torch.zeros(4, 3, device='cuda')
    f = torch.tensor([[0, 1, 2], [1, 2, 3]], device='cuda')
    bad_index = torch.tensor([[0, 1, 4]], device='cuda')
    bad_vertex = v.clone()
    bad_vertex[2, 1] = float('nan')
    calls = {'face_components': lambda m: mc.face_components(m), 'largest_component': lambda m: mc.largest_component(m),
             'remove_small_components': lambda m: mc.remove_small_components(m, min_faces=1),
             'merge_vertices': lambda m: mc.merge_vertices(m), 'face_areas': lambda m: mc.face_areas(m),
             'component_sizes': lambda m: mc.component_sizes(m, torch.zeros(m[1].shape[0], dtype=torch.int64,
                                                                            device='cuda'), 1)}
    for name, fn in calls.items():
        with pytest.raises(TypeError, match='^%s: vertices must be a CUDA tensor' % name):
            fn((v.cpu(), f))
        with pytest.raises(ValueError, match='^%s: face index outside' % name):
            fn((v, bad_index))
        with pytest.raises(ValueError, match='^%s: ' % name):
            fn((bad_vertex, f))
    with pytest.raises(TypeError, match='^component_sizes: labels must be a CUDA tensor'):
        mc.component_sizes((v, f), torch.zeros(2, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match='^component_sizes: 3 labels'):
        mc.component_sizes((v, f), torch.zeros(3, dtype=torch.int64, device='cuda'), 1)
    with pytest.raises(ValueError, match='^component_sizes: a label outside'):
        mc.component_sizes((v, f), torch.tensor([0, 5], device='cuda'), 2)
    with pytest.raises(ValueError, match='^face_components: connectivity'):
        mc.face_components((v, f), 'face')
