"""Constructed inputs of the mesh connected-components tests (CPU and GPU).  A case is a Case(name, vertices fp32
[V,3], faces int64 [F,3], structure), where ``structure(case)`` asserts, from the restatement (tests/meshcc_numpy.py),
that the case exercises what it is named for.  Everything is built once, on import, from fixed seeds."""
import math
from collections import namedtuple

import numpy as np

import mc_numpy
import meshcc_numpy as cc

Case = namedtuple('Case', 'name vertices faces structure')


def _counts(case):
    return {r: cc.face_components(case.faces, len(case.vertices), r)[1] for r in cc.RULES}


def _expect(**want):
    def structure(case):
        got = _counts(case)
        assert got == want, (case.name, got)
    return structure


def _grid_vertices(n, seed):
    """n distinct vertices with small integer coordinates (exact cross products in any arithmetic)."""
    rng = np.random.default_rng(seed)
    v = np.stack([np.arange(n) % 64, (np.arange(n) // 64) % 64, np.arange(n) // 4096], 1)
    return (v + rng.integers(0, 2, (n, 1)) * np.array([[0, 0, 64]])).astype(np.float32)


def _faces(rows):
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def tiny_cases():
    v = _grid_vertices(8, 0)
    return [
        Case('empty', v, _faces([]), _expect(edge=0, edge_any=0, vertex=0)),
        Case('one face', v, _faces([[0, 1, 2]]), _expect(edge=1, edge_any=1, vertex=1)),
        Case('shared edge', v, _faces([[0, 1, 2], [2, 1, 3]]), _expect(edge=1, edge_any=1, vertex=1)),
        Case('shared vertex', v, _faces([[0, 1, 2], [2, 3, 4]]), _expect(edge=2, edge_any=2, vertex=1)),
        Case('three on an edge', v, _faces([[0, 1, 2], [1, 0, 3], [0, 1, 4]]), _expect(edge=3, edge_any=1, vertex=1)),
        Case('duplicated face', v, _faces([[0, 1, 2], [0, 1, 2], [5, 6, 7]]), _expect(edge=2, edge_any=2, vertex=2)),
        # (a, a, b): its edge (a, b) is listed twice, so a neighbour across it makes a run of three
        Case('degenerate face', v, _faces([[3, 3, 4], [3, 4, 5], [5, 4, 6]]), _expect(edge=2, edge_any=1, vertex=1)),
    ]


STRIP_FACES = 4097


def _bit_reverse(n_bits):
    idx = np.arange(1 << n_bits)
    out = np.zeros_like(idx)
    for b in range(n_bits):
        out |= ((idx >> b) & 1) << (n_bits - 1 - b)
    return out


def strip_cases():
    """A triangle strip of 4 097 faces, listed forward, reversed and bit-reversed: one component; long chains, failed
    hooks, and runs of equal keys that cross every workgroup boundary of the link launch."""
    n = STRIP_FACES
    verts = np.stack([np.arange(n + 2) // 2, np.arange(n + 2) % 2, np.zeros(n + 2)], 1).astype(np.float32)
    faces = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1)
    faces[1::2] = faces[1::2][:, [1, 0, 2]]                              # consistent winding
    rev = _bit_reverse(13)
    orders = {'forward': np.arange(n), 'reversed': np.arange(n)[::-1], 'bit-reversed': rev[rev < n]}

    def structure(case):
        assert len(case.faces) == n and sorted(map(tuple, np.sort(case.faces, 1).tolist())) == \
            sorted(map(tuple, np.sort(faces, 1).tolist()))
        assert _counts(case) == {'edge': 1, 'edge_any': 1, 'vertex': 1}
        # every inner edge is a run of exactly two keys, and 3 n keys span more than 48 workgroups of 256
        keys = np.sort(cc.edge_keys(case.faces))
        assert (np.unique(keys, return_counts=True)[1] == 2).sum() == n - 1 and len(keys) > 48 * 256

    return [Case('strip ' + k, verts, faces[o], structure) for k, o in orders.items()]


def tetrahedra_case():
    """1 000 disjoint tetrahedra, face order and vertex ids shuffled: 1 000 components under every rule, numbered by
    first face -- which is neither the order of the roots' vertex ids nor that of the tetrahedra."""
    rng = np.random.default_rng(11)
    n = 1000
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    verts = (corner[None] + 2 * np.stack([np.arange(n) % 10, (np.arange(n) // 10) % 10, np.arange(n) // 100], 1)[:, None])
    verts = verts.reshape(-1, 3).astype(np.float32)
    local = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    faces = (local[None] + 4 * np.arange(n)[:, None, None]).reshape(-1, 3)
    new_id = rng.permutation(4 * n)                                      # vertex old -> new
    shuffled = np.empty_like(verts)
    shuffled[new_id] = verts
    faces = new_id[faces][rng.permutation(4 * n)]

    def structure(case):
        assert _counts(case) == {'edge': n, 'edge_any': n, 'vertex': n}
        labels, _ = cc.face_components(case.faces, len(case.vertices), 'vertex')
        other, _ = cc.face_components(case.faces, len(case.vertices), 'vertex', mistake='root order')
        assert not np.array_equal(labels, other)
        assert (np.bincount(labels) == 4).all()

    return Case('tetrahedra', shuffled, faces, structure)


def soup_case():
    """rng.integers(0, 150, (3000, 3)): the three rules give three different component counts, and both edge rules
    many components of two or more faces."""
    rng = np.random.default_rng(5)
    faces = rng.integers(0, 150, (3000, 3))

    def structure(case):
        got = _counts(case)
        assert len(set(got.values())) == 3, got
        for rule in ('edge', 'edge_any'):
            labels, _ = cc.face_components(case.faces, len(case.vertices), rule)
            assert (np.bincount(labels) >= 2).sum() >= 100, rule
        with_three = cc.face_components(case.faces, len(case.vertices), 'edge', mistake='runs of 3')[0]
        assert not np.array_equal(with_three, cc.face_components(case.faces, len(case.vertices), 'edge')[0])

    return Case('soup', _grid_vertices(150, 1), faces, structure)


def vertex_soup_case():
    """Four soups on disjoint vertex ranges, interleaved face by face: 'vertex' gives more than one component."""
    rng = np.random.default_rng(6)
    parts = [rng.integers(0, 150, (3000, 3)) + 150 * k for k in range(4)]
    faces = np.stack(parts, 1).reshape(-1, 3)

    def structure(case):
        got = _counts(case)
        assert got['vertex'] == 4 and len(set(got.values())) == 3, got
        assert cc.face_components(case.faces, len(case.vertices), 'vertex')[0][:8].tolist() == [0, 1, 2, 3] * 2

    return Case('interleaved soups', _grid_vertices(600, 2), faces, structure)


# two spheres and a torus in [-1, 1]^3: (centre, radius) and (centre, major, minor; axis z)
MC_SPHERES = (((-0.5, -0.5, -0.5), 0.3), ((0.5, 0.5, -0.45), 0.25))
MC_TORUS = ((0.0, 0.0, 0.4), 0.4, 0.12)
MC_N = 48
MC_AREAS = {'torus': 4 * math.pi ** 2 * MC_TORUS[1] * MC_TORUS[2],
            'sphere 0': 4 * math.pi * MC_SPHERES[0][1] ** 2, 'sphere 1': 4 * math.pi * MC_SPHERES[1][1] ** 2}
# an inscribed triangulation with edges e <= sqrt(3) h of a surface of curvature k loses about (e k)^2 / 8 of its
# area: 5 % at h = 2 / 47 and k = 1 / 0.12; the interpolated crossings of an exact distance add far less
MC_AREA_RTOL = 0.05


def mc_volume():
    """The SDF (exact distances, their minimum) on the 48^3 grid, fp32, and the grid spacing."""
    g = np.linspace(-1.0, 1.0, MC_N)
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    d = []
    for c, r in MC_SPHERES:
        d.append(np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r)
    c, major, minor = MC_TORUS
    ring = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - major
    d.append(np.sqrt(ring ** 2 + (z - c[2]) ** 2) - minor)
    return np.minimum.reduce(d).astype(np.float32), g[1] - g[0]


def mc_case(marching_cubes=mc_numpy.marching_cubes):
    """The marching-cubes mesh of the scene (``marching_cubes(volume, level, spacing) -> verts, faces, normals`` as
    numpy arrays; default: the numpy restatement of the project's own) -> Case, with the normals as a fifth value."""
    vol, h = mc_volume()
    verts, faces, normals = marching_cubes(vol, 0.0, (h, h, h))

    def structure(case):
        assert _counts(case) == {'edge': 3, 'edge_any': 3, 'vertex': 3}
        labels, n = cc.face_components(case.faces, len(case.vertices), 'edge')
        _, area = cc.component_sizes(cc.face_areas(case.vertices, case.faces), labels, n)
        assert np.allclose(np.sort(area), np.sort(list(MC_AREAS.values())), rtol=MC_AREA_RTOL, atol=0), area

    return Case('marching cubes', np.asarray(verts, np.float32), np.asarray(faces, np.int64), structure), normals


def all_cases():
    """Every case that needs no GPU to build (the marching-cubes one from the numpy marching cubes)."""
    return tiny_cases() + strip_cases() + [tetrahedra_case(), soup_case(), vertex_soup_case(), mc_case()[0]]
