"""Numpy / plain-Python restatement of the mesh connected-components method (csrc/meshcc.hip, utils/mesh_clean.py),
for the tests: the edge keys, the walk over the runs of equal keys under both rules, a sequential union-find whose
roots are the smallest ids, the numbering by first face, fp64 areas summed with math.fsum, the key rule of
merge_vertices and the axes of aligned_grid.  Nothing here is imported by the package."""
import math

import numpy as np

RULES = ('edge', 'edge_any', 'vertex')


def edge_keys(faces):
    """keys[3f + e] = (min << 32) | max of edge e of face f; edges (v0,v1), (v1,v2), (v2,v0)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b = f, np.roll(f, -1, axis=1)
    return ((np.minimum(a, b) << 32) | np.maximum(a, b)).reshape(-1)


def face_pairs(faces, rule, mistake=None):
    """The pairs of face ids that the edge rules unite, from the stably sorted keys.  'edge': the two faces of every
    run of exactly two equal keys; 'edge_any': neighbours within every run.  mistake 'runs of 3': 'edge' also takes
    the runs of three."""
    keys = edge_keys(faces)
    order = np.argsort(keys, kind='stable')
    keys = keys[order]
    pairs, i, n = [], 0, len(keys)
    while i < n:
        j = i
        while j + 1 < n and keys[j + 1] == keys[i]:
            j += 1
        run = j - i + 1
        if rule == 'edge_any' or run == 2 or (mistake == 'runs of 3' and run == 3):
            pairs += [(order[k] // 3, order[k + 1] // 3) for k in range(i, j)]
        i = j + 1
    return pairs


def vertex_pairs(faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return [(r[0], r[1]) for r in f] + [(r[0], r[2]) for r in f]


def min_roots(n, pairs):
    """Sequential union-find, larger root under smaller -> root[i] = the smallest id of i's component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def number_by_first(group):
    """group [F]: any id per face, equal within a component -> (labels, count) numbered by first face index."""
    labels, seen = np.empty(len(group), dtype=np.int64), {}
    for i, g in enumerate(np.asarray(group).tolist()):
        labels[i] = seen.setdefault(g, len(seen))
    return labels, len(seen)


def face_components(faces, n_vertices, rule, mistake=None):
    """(labels int64 [F], count): the components of the faces under ``rule``, numbered in ascending order of their
    first face.  mistake 'root order' (rule 'vertex'): numbered in ascending order of the vertex root instead."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros(0, dtype=np.int64), 0
    if rule == 'vertex':
        root = min_roots(n_vertices, vertex_pairs(f))[f[:, 0]]
        if mistake == 'root order':
            ids = np.unique(root)
            return np.searchsorted(ids, root), len(ids)
        return number_by_first(root)
    return number_by_first(min_roots(len(f), face_pairs(f, rule, mistake)))


def graph(faces, n_vertices, rule):
    """The face graph as (rows, cols) of its edges, for scipy's connected_components."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if rule != 'vertex':
        pairs = face_pairs(f, rule)
    else:                                              # faces that share a vertex: a chain through each vertex's faces
        pairs = []
        flat, face = f.reshape(-1), np.repeat(np.arange(len(f)), 3)
        order = np.argsort(flat, kind='stable')
        flat, face = flat[order], face[order]
        same = flat[1:] == flat[:-1]
        pairs = list(zip(face[:-1][same], face[1:][same]))
    rows = np.array([p[0] for p in pairs], dtype=np.int64)
    cols = np.array([p[1] for p in pairs], dtype=np.int64)
    return rows, cols


def face_areas(vertices, faces):
    """0.5 |e1 x e2| in fp64 on the fp32 vertices."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt((c * c).sum(axis=1))


def component_sizes(areas, labels, count):
    """(face counts, fsum of the areas) per component."""
    faces = np.bincount(labels, minlength=count)
    return faces, np.array([math.fsum(np.asarray(areas)[labels == s].tolist()) for s in range(count)])


def largest(sizes):
    return int(np.argmax(sizes))                       # the first of equal maxima


def select(vertices, faces, keep_faces):
    """(kept vertex indices ascending, re-indexed faces) of a face selection."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[keep_faces]
    used = np.unique(f)
    return used, np.searchsorted(used, f)


def merge_keys(vertices, digits):
    return np.rint(np.asarray(vertices, dtype=np.float64) * 10.0 ** digits).astype(np.int64)


def merge_vertices(vertices, faces, digits):
    """(kept vertex indices ascending, re-indexed faces): equal key triples merge into the lowest index."""
    first, target = {}, []
    for i, k in enumerate(map(tuple, merge_keys(vertices, digits).tolist())):
        target.append(first.setdefault(k, i))
    target = np.array(target, dtype=np.int64)
    kept = np.unique(target)
    return kept, np.searchsorted(kept, target[np.asarray(faces, dtype=np.int64).reshape(-1, 3)])


def aligned_grid(lo, hi, resolution, eps=0.1):
    """plots.get_grid's three axes, written on its own."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    side = hi - lo
    s = [a for a in range(3) if side[a] == side.min()][0]
    short = np.linspace(lo[s] - eps, hi[s] + eps, resolution)
    step = (short[-1] - short[0]) / (resolution - 1)
    return tuple(short if a == s else np.arange(lo[a] - eps, hi[a] + step + eps, step) for a in range(3))
