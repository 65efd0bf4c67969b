"""Mesh clean-up on the GPU: connected components, the largest-component filter and the vertex merge that the
reference does on the CPU with trimesh.

* ``face_components``: the components of the face graph, trimesh's ``Trimesh.split(only_watertight=False)`` rule
  (``'edge'``: two faces are adjacent when they are the only two on an edge) and two looser ones, by a lock-free
  union-find over the sorted edge keys (csrc/meshcc.hip, ABI msdf_mcc_* of include/monosdf_meshcc.h).
* ``component_sizes``: face count and fp64 area per component.
* ``largest_component``: ``components[areas.argmax()]`` of plots.get_surface_high_res_mesh / get_surface_by_grid
  (plots.py:334-337) and the commented-out step of evaluation/eval.py:87-90.  ``remove_small_components``: the
  same selection by bounds.
* ``merge_vertices``: the position rule of trimesh's ``merge_vertices``, which ``trimesh.load`` applies before any
  evaluation script sees a mesh.

Everything runs on CUDA tensors; there is no CPU path.  Arguments are checked by utils/mesh_args.py.  The labels are
unique -- the smallest face index of a component names it -- so the same mesh gives the same labels every call,
whatever order the atomics of the union-find land in.
"""
import numpy as np
import torch

from . import mesh_args as ma
from .mesh import Mesh
from .mesh_eval import _face_cross

CONNECTIVITY = ('edge', 'edge_any', 'vertex')
_MAX_FACES = (2 ** 31 - 1) // 3          # 3 F edge keys are indexed in int32


def _connectivity(name, connectivity):
    if connectivity not in CONNECTIVITY:
        raise ValueError("%s: connectivity must be 'edge', 'edge_any' or 'vertex', got %r" % (name, connectivity))
    return connectivity


def _by(name, by):
    if by not in ('area', 'faces'):
        raise ValueError("%s: by must be 'area' or 'faces', got %r" % (name, by))
    return by


def _first_index_labels(first):
    """first [F] int64: for every face the smallest face index of its component -> (labels [F], count): components
    numbered in ascending order of that index.  One host read."""
    head = first == torch.arange(first.shape[0], device=first.device)
    rank = torch.cumsum(head, 0) - 1
    return rank[first], int(rank[-1]) + 1


def _face_components(name, v, f, connectivity):
    dev, F, V = f.device, f.shape[0], v.shape[0]
    if F == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), 0
    if F > _MAX_FACES:
        raise ValueError('%s: %d faces: the 3 F edge keys are indexed in int32' % (name, F))
    with torch.cuda.device(dev):
        if connectivity == 'vertex':
            parent = torch.empty(V, dtype=torch.int32, device=dev)
            ma.call('msdf_mcc_init', parent, V)
            ma.call('msdf_mcc_link_vertices', f, F, parent)
            ma.call('msdf_mcc_flatten', parent, V)
            root = parent[f[:, 0].long()].long()                    # the vertex root of a face: that of its v0
            face = torch.arange(F, device=dev)
            first = torch.full((V,), F, dtype=torch.int64, device=dev).scatter_reduce(0, root, face, 'amin')
            return _first_index_labels(first[root])
        keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        ma.call('msdf_mcc_edge_keys', f, F, keys)
        sorted_keys, order = torch.sort(keys, stable=True)
        parent = torch.empty(F, dtype=torch.int32, device=dev)
        ma.call('msdf_mcc_init', parent, F)
        ma.call('msdf_mcc_link_edges', sorted_keys, order, 3 * F, 0 if connectivity == 'edge' else 1, parent)
        ma.call('msdf_mcc_flatten', parent, F)
    return _first_index_labels(parent.long())                       # the root is the smallest face of its component


def face_components(mesh, connectivity='edge'):
    """The connected components of the faces -> (labels [F] int64 CUDA, n_components int).  ``mesh``: a Mesh or a
    (vertices, faces) pair (CUDA tensors, or numpy arrays, which are uploaded).

    ``connectivity``: ``'edge'``: two faces are adjacent when they are the only two faces on an edge -- trimesh's
    ``face_adjacency``, the rule of ``Trimesh.split``: an edge with three or more faces connects none of them;
    ``'edge_any'``: all faces on an edge are adjacent; ``'vertex'``: faces that share a vertex are adjacent.
    Vertices are compared by index, not by position: see ``merge_vertices``.

    Components are numbered in ascending order of their first face index, the numbering of
    ``scipy.sparse.csgraph.connected_components`` on the face graph.  The same mesh gives the same labels every call.
    One host read (the count)."""
    name = 'face_components'
    _connectivity(name, connectivity)
    v, f, _ = ma.mesh_tensors(name, mesh)
    return _face_components(name, v, f, connectivity)


def _face_areas(v, f):
    """0.5 |e1 x e2| in fp64 on the fp32 vertices, [F]."""
    return 0.5 * _face_cross(v, f)[3].norm(dim=1)


def face_areas(mesh):
    """The area of every face, [F] float64 CUDA: 0.5 |e1 x e2| in fp64 on the fp32 vertices."""
    v, f, _ = ma.mesh_tensors('face_areas', mesh)
    return _face_areas(v, f)


def _component_sizes(name, v, f, labels, n):
    dev = f.device
    count = torch.bincount(labels, minlength=n)
    area = torch.zeros(n, dtype=torch.float64, device=dev)
    if n > 0:
        if count.shape[0] != n:
            raise ValueError('%s: a label outside [0, %d)' % (name, n))
        order = torch.sort(labels, stable=True)[1]
        values = _face_areas(v, f)[order].contiguous()
        seg_start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        seg_start[1:] = torch.cumsum(count, 0)
        with torch.cuda.device(dev):
            ma.call('msdf_mcc_segment_sum', values, seg_start, n, area)
    return count, area


def component_sizes(mesh, labels, n_components):
    """(face_count [n] int64, area [n] float64) of the components that ``face_components`` found.  Face area is
    0.5 |e1 x e2| in fp64 on the fp32 vertices; the faces are sorted stably by label and each component is summed in
    a fixed order (no atomics): the same input gives bitwise the same areas every call."""
    name = 'component_sizes'
    v, f, _ = ma.mesh_tensors(name, mesh)
    ma.check_tensor(name, 'labels', labels, (torch.int64,), '[F]')
    ma.same_device(name, faces=f, labels=labels)
    n = int(n_components)
    if labels.shape[0] != f.shape[0] or n < 0 or (n == 0) != (f.shape[0] == 0):
        raise ValueError('%s: %d labels, %d components for %d faces' % (name, labels.shape[0], n, f.shape[0]))
    return _component_sizes(name, v, f, labels, n)


def _select(name, mesh, v, f, normals, keep_faces):
    """The mesh of the faces ``keep_faces`` (bool [F]), in their order, with the unreferenced vertices dropped."""
    kept = f[keep_faces]
    keep = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    keep[kept.long().reshape(-1)] = True
    faces = ma.compact_faces(keep, kept, all_kept=True)
    # a (vertices, faces) pair comes back as what was searched, a mesh object with its own vertices and normals
    return ma.kept_mesh(v if normals is None else ma.mesh_parts(mesh)[0], normals, keep, faces)


def largest_component(mesh, connectivity='edge', by='area'):
    """The largest connected component as a Mesh: ``components[areas.argmax()]`` of plots.py:334-337.  ``by``:
    ``'area'`` or ``'faces'``; of equal maxima the component of lowest index (the one whose first face comes first)
    wins, as with ``argmax``.  Faces keep their original order, unreferenced vertices are dropped and the faces
    re-indexed; vertex normals follow their vertices when a mesh object came in.  A mesh without faces comes back
    empty."""
    name = 'largest_component'
    _connectivity(name, connectivity)
    _by(name, by)
    v, f, normals = ma.mesh_tensors(name, mesh)
    return _select(name, mesh, v, f, normals, _largest_mask(name, v, f, connectivity, by))


def _largest_mask(name, v, f, connectivity, by):
    """bool [F]: the faces of the largest component of a mesh that ``mesh_tensors`` has passed."""
    labels, n = _face_components(name, v, f, connectivity)
    if n == 0:
        return torch.zeros(0, dtype=torch.bool, device=f.device)
    count, area = _component_sizes(name, v, f, labels, n)
    size = area if by == 'area' else count
    return labels == (size == size.max()).nonzero()[0, 0]           # the first of equal maxima


def remove_small_components(mesh, min_faces=None, min_area=None, connectivity='edge'):
    """The mesh without the components that have fewer than ``min_faces`` faces or less than ``min_area`` area (a
    component stays when it meets every bound given).  Compaction as in ``largest_component``.  ValueError when
    neither bound is given."""
    name = 'remove_small_components'
    _connectivity(name, connectivity)
    if min_faces is None and min_area is None:
        raise ValueError('%s: give min_faces, min_area or both' % name)
    v, f, normals = ma.mesh_tensors(name, mesh)
    labels, n = _face_components(name, v, f, connectivity)
    if n == 0:
        return _select(name, mesh, v, f, normals, torch.zeros(0, dtype=torch.bool, device=f.device))
    count, area = _component_sizes(name, v, f, labels, n)
    ok = torch.ones(n, dtype=torch.bool, device=f.device)
    if min_faces is not None:
        ok &= count >= int(min_faces)
    if min_area is not None:
        ok &= area >= float(min_area)
    return _select(name, mesh, v, f, normals, ok[labels])


def merge_keys(vertices, digits=8, name='merge_vertices'):
    """The per-axis integer keys of ``merge_vertices``: rint(v * 10**digits) in fp64 as int64, [V, 3]; a CUDA tensor
    or a host array in, the same kind out.  ValueError if |v| * 10**digits >= 2^53 (the product would not be an
    exact integer's neighbour any more) or a coordinate is not finite."""
    scale = 10.0 ** int(digits)
    if isinstance(vertices, torch.Tensor):
        scaled = vertices.double() * scale
        top = float(scaled.abs().max()) if scaled.numel() else 0.0
    else:
        scaled = np.asarray(vertices, dtype=np.float64) * scale
        top = float(np.abs(scaled).max()) if scaled.size else 0.0
    if not top < 2.0 ** 53:                            # also refuses NaN and inf
        raise ValueError('%s: |v| * 10**%d reaches 2^53 (or a coordinate is not finite): use fewer digits' %
                         (name, int(digits)))
    if isinstance(vertices, torch.Tensor):
        return torch.round(scaled).long()
    return np.rint(scaled).astype(np.int64)


def merge_vertices(mesh, digits=8):
    """Vertices at one position become one vertex -> Mesh.  The position rule of trimesh's ``merge_vertices``: the key
    of a vertex is rint(v * 10**digits) per axis, computed in fp64, and vertices with equal key triples merge into
    the one of lowest index, which keeps its coordinates and its normal.  The output vertices stay in ascending order
    of that first index; the faces are re-indexed and none is dropped (a face may become degenerate).  Host fp64
    vertices are keyed in fp64, CUDA fp32 vertices by their exact fp64 values.  ValueError if
    |v| * 10**digits >= 2^53.

    A ``get_surface_sliding`` mesh is concatenated from blocks: every block runs marching cubes on its own and the
    vertices on a seam exist once per block, computed from different block origins, so the copies differ in their
    last bits.  Such a mesh falls apart at the seams under ``face_components`` until its seam vertices are merged,
    and that needs a coarser ``digits`` than 8 (well below the voxel size, well above fp32 rounding at the scene's
    scale: 5 for a scene of unit size) before a component split.

    trimesh additionally compares vertex normals by default when a mesh has them (``merge_norm=False``); this
    function compares positions only."""
    name = 'merge_vertices'
    hv, hf, normals = ma.mesh_parts(mesh)
    if isinstance(hv, torch.Tensor):
        v, f, _ = ma.mesh_tensors(name, mesh)
        dev = v.device
        keys = merge_keys(v, digits, name)
    else:
        dev = ma.device_of(hf)
        hv = np.asarray(hv, dtype=np.float64)
        if hv.ndim == 2 and hv.shape[1] == 3:
            host_keys = merge_keys(hv, digits, name)                # before anything is uploaded
        v, f, _ = ma.mesh_tensors(name, (hv, hf), dev)
        dev = v.device
        keys = ma.upload(host_keys, dev)
    V = v.shape[0]
    if V == 0:
        return Mesh(np.zeros((0, 3)), ma.host_array(f))
    distinct, inverse = torch.unique(keys, dim=0, return_inverse=True)
    index = torch.arange(V, device=dev)
    first = torch.full((distinct.shape[0],), V, dtype=torch.int64, device=dev)
    first = first.scatter_reduce(0, inverse, index, 'amin')[inverse]           # per vertex: the one it merges into
    keep = first == index
    return ma.kept_mesh(hv, normals, keep, (torch.cumsum(keep, 0) - 1)[first[f.long()]].reshape(-1, 3))
