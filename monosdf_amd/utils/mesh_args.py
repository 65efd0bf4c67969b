"""Argument handling of the mesh tools (utils/mesh.py, mesh_eval.py, mesh_refuse.py, mesh_dtu.py, mesh_clean.py,
mesh_bounds.py, mesh_align.py, point_grid.py): each rule their entry points apply before a kernel sees a pointer, and
the one way a culled mesh goes back to the caller, stated once.

* ``check_tensor``, ``same_device``: the CUDA tensor an entry point accepts (there is no CPU path).
* ``mesh_tensors``: a mesh object or a (vertices, faces) pair -> float32 / int32 device tensors, its contents checked
  exactly once: host arrays on the host before anything is uploaded, CUDA tensors in one device reduction and one
  host read.  ``cloud_tensor``: the same for a point cloud.  A mesh object is anything with ``.vertices``, ``.faces``
  and ``.vertex_normals`` (utils/mesh.py's Mesh, a trimesh.Trimesh).
* ``workspace``, ``call``: the scratch buffer an ABI entry asks for, and the call itself.
* ``compact_faces``, ``finite_bounds``: dropping vertices with their faces; the bounding box of a cloud.
* ``positive_number``, ``search_distance``: a cell side, a radius, a density, a search bound.
* ``host_array``, ``kept_mesh``: the kept vertices, their normals and the re-indexed faces as a Mesh on the host.

Every error begins with the public function's name, which the caller passes as ``name``.
"""
import numpy as np
import torch

from .. import _lib


def check_tensor(name, arg, t, dtypes=(torch.float32,), shape='[N, 3]'):
    """TypeError unless ``t`` is a CUDA tensor of one of ``dtypes``; ValueError unless its shape fits ``shape``
    ('[N, 3]', '[n, H, W]', '[nx, ny, nz]': as many dims, a last dim of 3 where it says so) with fewer than 2^31
    rows."""
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise TypeError('%s: %s must be a CUDA tensor (there is no CPU path), got %s' %
                        (name, arg, t.device if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dtype not in dtypes:
        raise TypeError('%s: %s must be %s, got %s' % (name, arg, ' or '.join(str(d) for d in dtypes), t.dtype))
    if t.dim() != shape.count(',') + 1 or (shape.endswith(', 3]') and t.shape[-1] != 3):
        raise ValueError('%s: %s must be %s, got %s' % (name, arg, shape, tuple(t.shape)))
    if max(t.shape) >= 2 ** 31:
        raise ValueError('%s: %s of shape %s: int32 indices hold fewer than 2^31' % (name, arg, tuple(t.shape)))


def same_device(name, **tensors):
    """ValueError unless the named tensors are on one device -> that device."""
    (first, t0), *rest = tensors.items()
    for arg, t in rest:
        if t.device != t0.device:
            raise ValueError('%s: %s on %s, %s on %s' % (name, first, t0.device, arg, t.device))
    return t0.device


def device_of(*args):
    """The device of the first CUDA tensor among ``args``, where the host data of the same call goes; else None."""
    for a in args:
        if isinstance(a, torch.Tensor) and a.device.type == 'cuda':
            return a.device
    return None


def upload(array, device=None, dtype=None):
    """A host array as a contiguous tensor on ``device`` (None: the current CUDA device)."""
    return torch.from_numpy(np.ascontiguousarray(array, dtype)).to('cuda' if device is None else device)


def mesh_parts(mesh):
    """(vertices, faces, vertex normals or None) of a mesh object or a (vertices, faces) pair, as they came."""
    if all(hasattr(mesh, a) for a in ('vertices', 'faces', 'vertex_normals')):
        return mesh.vertices, mesh.faces, mesh.vertex_normals
    vertices, faces = mesh
    return vertices, faces, None


def refuse_contents(name, finite, in_range, n_vertices):
    if not finite:
        raise ValueError('%s: non-finite vertex coordinates' % name)
    if not in_range:
        raise ValueError('%s: face index outside [0, %d)' % (name, n_vertices))


def mesh_tensors(name, mesh, device=None):
    """A mesh object or a (vertices, faces) pair -> (vertices float32 [V,3], faces int32 [F,3], host normals or None):
    contiguous tensors on one device.  ValueError for a non-finite coordinate and for a face index outside [0, V).
    Host arrays: checked on the host, then uploaded to ``device`` (None: the current CUDA device).  CUDA tensors
    (float32; int32 / int64): type, dtype and shape on the host, the contents in one device reduction and one host
    read.  The functions that receive the result index device memory with it and check nothing again."""
    v, f, normals = mesh_parts(mesh)
    if isinstance(v, torch.Tensor) or isinstance(f, torch.Tensor):
        check_tensor(name, 'vertices', v, shape='[V, 3]')
        check_tensor(name, 'faces', f, (torch.int32, torch.int64), '[F, 3]')
        same_device(name, vertices=v, faces=f)
        v = v.contiguous()
        flags = [torch.isfinite(v).all()]
        if f.shape[0] > 0:
            lo, hi = torch.aminmax(f)
            flags.append((lo >= 0) & (hi < v.shape[0]))
        finite, *in_range = torch.stack(flags).tolist()
        refuse_contents(name, finite, all(in_range), v.shape[0])
        return v, f.to(torch.int32).contiguous(), normals
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError('%s: vertices must be [V, 3], got %s' % (name, v.shape))
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError('%s: faces must be an integer [F, 3] array, got %s %s' % (name, f.dtype, f.shape))
    if max(len(v), len(f)) >= 2 ** 31:
        raise ValueError('%s: %d vertices, %d faces: int32 indices hold fewer than 2^31' % (name, len(v), len(f)))
    refuse_contents(name, np.isfinite(v).all(), not f.size or (f.min() >= 0 and f.max() < len(v)), len(v))
    return upload(v, device, np.float32), upload(f, device, np.int32), normals


def cloud_tensor(name, arg, cloud, device=None):
    """A mesh object (its vertices), a numpy array (its first three columns, uploaded to ``device``) or a CUDA tensor
    -> float32 CUDA [N,3]."""
    if hasattr(cloud, 'vertices'):
        cloud = cloud.vertices
    if isinstance(cloud, np.ndarray):
        cloud = upload(cloud[:, :3], device, np.float32)
    check_tensor(name, arg, cloud)
    return cloud


def workspace(name, entry, *sizes, device):
    """The uint8 scratch tensor that the ABI's ``entry`` (a ``msdf_*_workspace_bytes``) asks for at ``sizes``."""
    n = int(getattr(_lib.load(), entry)(*sizes))
    if n < 0:
        raise ValueError('%s: %s%s: sizes out of range' % (name, entry, sizes))
    return torch.empty(n, dtype=torch.uint8, device=device)


def call(entry, *args):
    """One call of the ABI's ``entry`` on the current stream of the current device, which the caller has made the
    tensors' own (``with torch.cuda.device(...)``); the tensors among ``args`` go as their device pointers."""
    _lib.call(entry, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _lib.stream_ptr())


def compact_faces(keep, faces, all_kept=False):
    """keep: bool [V]; faces: integer [F,3] -> int64 [F',3]: the faces with all three vertices kept, in their order,
    re-indexed to the rows of ``vertices[keep]``.  ``all_kept``: the caller formed ``keep`` from these faces, so none
    is dropped and the selection (a gather, a reduction and a host read) is left out.  Any device."""
    f = faces.long()
    if not all_kept:
        f = f[keep[f].all(dim=1)]
    return (torch.cumsum(keep, 0) - 1)[f].reshape(-1, 3)


def host_array(a):
    """A tensor (any device) or a host array as a numpy array."""
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def kept_mesh(vertices, normals, keep, faces):
    """The Mesh of the rows ``keep`` (bool [V], a tensor on any device) of ``vertices`` and, unless None, ``normals``
    (each a tensor or a host array), with ``faces`` as they are: already re-indexed to those rows (``compact_faces``).
    Mesh converts to fp64 / int64 itself."""
    from .mesh import Mesh                                     # at call time: utils/mesh.py imports this module
    keep_h = host_array(keep)
    return Mesh(host_array(vertices)[keep_h], host_array(faces),
                None if normals is None else host_array(normals)[keep_h])


def positive_number(name, arg, value):
    """``value`` as a Python float; ValueError unless it is a number, positive and finite."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s: %s must be a number, got %r' % (name, arg, value))
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError('%s: %s must be positive and finite, got %r' % (name, arg, value))
    return v


def search_distance(name, max_dist):
    """``max_dist`` of a bounded search as a Python float: positive and finite, as a float32 too."""
    md = positive_number(name, 'max_dist', max_dist)
    if md > float(np.finfo(np.float32).max):
        raise ValueError('%s: max_dist must be finite as a float32, got %r' % (name, max_dist))
    return md


def finite_bounds(name, points):
    """Per-axis bounds of a non-empty cloud [N,3] -> (min on the device, min, max as fp64 host tensors [3]); one
    reduction and one host copy.  ValueError for non-finite coordinates."""
    lo, hi = torch.aminmax(points, dim=0)
    lo_h, hi_h = torch.stack([lo, hi]).double().cpu()
    if not bool(torch.isfinite(lo_h).all() and torch.isfinite(hi_h).all()):
        raise ValueError('%s: non-finite coordinates' % name)
    return lo, lo_h, hi_h
