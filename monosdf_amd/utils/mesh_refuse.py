"""Mesh re-fusion and view culling on the GPU: what the reference's evaluation does to an exported mesh before it
scores it (csrc/refuse.hip, ABI msdf_raster_* / msdf_tsdf_* / msdf_cull_*).

* ``render_depth``: a depth map of the mesh from every pose, in place of pyrender's offscreen renderer
  (scannet_eval/evaluate.py:76-109).
* ``tsdf_integrate``: the depth maps fused into a dense block of voxels by the rule of open3d's TSDF volumes
  (evaluate.py:114-135; ``ScalableTSDFVolume.integrate``).
* ``extract_mesh``: marching cubes on that block, with open3d's rule that a cell gives triangles only if all its eight
  corners were observed (``extract_triangle_mesh``).
* ``refuse``: the three together, ``refuse(mesh, poses, K)`` of evaluate.py:111-137 and postprocess/refuse.py: the
  result has no surface that no camera saw (back sides of walls, the inside of closed furniture).
* ``cull_to_frustums``: the cheaper variant of the Replica protocol (replica_eval/cull_mesh.py:58-87): faces whose
  vertices lie in no camera frustum are dropped.
* ``read_poses``, ``read_intrinsics``: ScanNet ``pose/N.txt`` directories, Replica ``traj.txt``, ``intrinsic_*.txt``.

All cameras are OpenCV-style: x right, y down, z forward, ``pose`` a 4x4 camera-to-world matrix (the frame the
reference reaches after ``fix_pose`` and after cull_mesh.py's axis flips); ``K`` is (fx, fy, cx, cy) or a matrix with
them at [0,0], [1,1], [0,2], [1,2].  Every pose is inverted on the host in fp64 and used in fp32.  Everything runs on
CUDA tensors; there is no CPU path.  Arguments are checked by utils/mesh_args.py: every function that takes a mesh
validates it once (``mesh_tensors``) and hands it on to the unchecked ``_raster`` / ``_seen``.  The same inputs give
bitwise the same outputs every call (no floating-point atomics).  Not built: colour fusion (the reference fuses a
constant white).

Parity with pyrender's rasteriser and with open3d's integration is UNVERIFIED: neither library is available where this
is built and the reference holds no recorded output of them.  The pixel rule (a pixel's ray goes through its centre,
``pixel_center`` = 0.5) is OpenGL's; the TSDF rule is open3d's ``UniformTSDFVolume`` written down from its source.  Both
are pinned by the numpy restatements of the tests (tests/refuse_numpy.py) only.
"""
import os
import re

import numpy as np
import torch

from . import mesh_args as ma
from .mesh import Mesh, concatenate, marching_cubes


def _intrinsics(name, K):
    k = np.asarray(K, dtype=np.float64)
    if k.ndim == 2 and k.shape[0] >= 3 and k.shape[1] >= 3:
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape != (4,):
        raise ValueError('%s: K must be (fx, fy, cx, cy) or a 3x3 / 4x4 matrix, got shape %s' % (name, k.shape))
    if not np.isfinite(k).all() or not (k[0] > 0 and k[1] > 0):
        raise ValueError('%s: intrinsics must be finite with fx, fy > 0, got %s' % (name, k.tolist()))
    return tuple(float(np.float32(x)) for x in k)


def _world_to_camera(name, poses):
    """[n,4,4] camera-to-world (numpy or tensor) -> [n,12] float32 host array of world-to-camera rows."""
    if isinstance(poses, torch.Tensor):
        poses = poses.detach().cpu().numpy()
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1:] != (4, 4):
        raise ValueError('%s: poses must be [n, 4, 4] camera-to-world matrices, got %s' % (name, p.shape))
    if p.shape[0] == 0:
        raise ValueError('%s: the list of views is empty' % name)
    if p.shape[0] > 65535:
        raise ValueError('%s: %d views: at most 65535 in one call' % (name, p.shape[0]))
    if not np.isfinite(p).all():
        raise ValueError('%s: non-finite pose' % name)
    try:
        inv = np.linalg.inv(p)
    except np.linalg.LinAlgError:
        raise ValueError('%s: a pose is not invertible' % name)
    return np.ascontiguousarray(inv[:, :3, :].reshape(-1, 12), dtype=np.float32)


def _image_size(name, height, width):
    h, w = int(height), int(width)
    if h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError('%s: image of %d x %d pixels' % (name, h, w))
    return h, w


def _raster(v, f, w2c, intr, h, w, znear, zfar, pixel_center):
    n = w2c.shape[0]
    depth = torch.empty(n, h, w, dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        ma.call('msdf_raster_depth', v, v.shape[0], f, f.shape[0], w2c, n, *intr, h, w, float(znear), float(zfar),
                float(pixel_center), depth)
    return depth


def render_depth(vertices, faces, poses, K, height, width, znear=0.05, zfar=100.0, pixel_center=0.5):
    """Depth maps of a mesh from ``n`` poses in one call: ``depth [n, height, width]`` float32 on the mesh's device.

    vertices [V,3] float32 (world), faces [F,3] int32 (int64 is converted): CUDA tensors.  Pixel (row i, column j) is
    the camera-frame z of the nearest intersection of the ray through ((j + pixel_center - cx) / fx,
    (i + pixel_center - cy) / fy, 1) with any face, whatever its winding, among intersections with
    znear <= z <= zfar; 0 where there is none (pyrender's defaults, and what its depth buffer reads for background).
    A face that crosses the near plane covers what its visible part covers.  Two faces that share an edge leave no
    crack: a ray between them hits at least one.  Faces without area touch nothing; ``F = 0`` gives zeros.  The image
    is bitwise the same every call and for every order and winding of the faces (a minimum over the faces).
    Parity with pyrender's rasteriser is UNVERIFIED (see the module's docstring): the half-pixel rule is OpenGL's.
    ValueError for a face index outside [0, V) and for non-finite coordinates or poses."""
    name = 'render_depth'
    w2c = _world_to_camera(name, poses)
    intr = _intrinsics(name, K)
    h, w = _image_size(name, height, width)
    if not (float(znear) > 0.0 and float(zfar) >= float(znear) and np.isfinite(pixel_center)):
        raise ValueError('%s: 0 < znear <= zfar needed, got %r, %r' % (name, znear, zfar))
    v, f, _ = ma.mesh_tensors(name, (vertices, faces))
    return _raster(v, f, ma.upload(w2c, v.device), intr, h, w, znear, zfar, pixel_center)


def _fusion_params(name, voxel_length, sdf_trunc, depth_trunc):
    vl = float(np.float32(voxel_length))
    if not (vl > 0.0 and np.isfinite(vl)):
        raise ValueError('%s: voxel_length must be positive, got %r' % (name, voxel_length))
    trunc = 3.0 * vl if sdf_trunc is None else float(np.float32(sdf_trunc))
    trunc = float(np.float32(trunc))
    if not (trunc > 0.0 and np.isfinite(trunc)):
        raise ValueError('%s: sdf_trunc must be positive, got %r' % (name, sdf_trunc))
    if np.isnan(depth_trunc):
        raise ValueError('%s: depth_trunc is not a number' % name)
    return vl, trunc, float(np.float32(depth_trunc))


def _integrate(depth, w2c, intr, origin, offset, dims, vl, trunc, dtrunc, state=None):
    nx, ny, nz = dims
    dev = depth.device
    if state is None:
        tsdf = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
        weight = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    else:
        tsdf, weight = state
    with torch.cuda.device(dev):
        ma.call('msdf_tsdf_integrate', depth, w2c, depth.shape[0], *intr, depth.shape[1], depth.shape[2], *origin,
                *offset, nx, ny, nz, vl, trunc, dtrunc, 0 if state is None else 1, tsdf, weight)
    return tsdf, weight


def _grid_args(name, origin, dims, offset):
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError('%s: origin must be 3 finite numbers' % name)
    d = tuple(int(x) for x in dims)
    off = tuple(int(x) for x in offset)
    if len(d) != 3 or min(d) < 1 or d[0] * d[1] * d[2] >= 2 ** 31:
        raise ValueError('%s: dims must be 3 positive counts with fewer than 2^31 voxels, got %s' % (name, d))
    if len(off) != 3 or min(off) < 0 or max(a + b for a, b in zip(off, d)) > 2 ** 24:
        raise ValueError('%s: offset must be >= 0 and offset + dims <= 2^24, got %s' % (name, off))
    return tuple(float(np.float32(x)) for x in o), d, off


def tsdf_integrate(depth, poses, K, origin, dims, voxel_length, sdf_trunc, depth_trunc=5.0, offset=(0, 0, 0)):
    """Depth maps fused into a dense block of voxels: ``(tsdf [nx,ny,nz] float32, weight [nx,ny,nz] float32)``.

    depth [n, H, W] float32 CUDA (0 = nothing seen), poses [n,4,4].  Voxel (i, j, k) has its centre at
    origin + voxel_length (i + 0.5, j + 0.5, k + 0.5) (open3d's ``UniformTSDFVolume``; with ``offset`` the block starts
    at voxel ``offset`` of a larger volume with that origin: i + offset[0] and so on).  For each view, in the order
    given, in fp32 with separately rounded operations:
      p = R x + t with [R|t] = pose^-1; skip the view if p.z <= 0
      u = int(fx p.x / p.z + cx + 0.5), v = int(fy p.y / p.z + cy + 0.5); skip if negative or outside the image
      d = depth[v, u]; skip if d <= 0 or d > depth_trunc
      s = (d - p.z) |((u - cx) / fx, (v - cy) / fy, 1)|; skip if s <= -sdf_trunc
      tsdf = (tsdf w + min(1, s / sdf_trunc)) / (w + 1); w += 1          (from tsdf = 0, w = 0)
    ``sdf_trunc`` None: 3 voxel_length.    One lane owns one voxel and applies the views in order: no atomics, bitwise reproducible.  The rule is written
    down from open3d's source; parity with open3d is UNVERIFIED (see the module's docstring)."""
    name = 'tsdf_integrate'
    ma.check_tensor(name, 'depth', depth, shape='[n, H, W]')
    w2c = _world_to_camera(name, poses)
    if w2c.shape[0] != depth.shape[0]:
        raise ValueError('%s: %d depth maps, %d poses' % (name, depth.shape[0], w2c.shape[0]))
    intr = _intrinsics(name, K)
    _image_size(name, depth.shape[1], depth.shape[2])
    vl, trunc, dtrunc = _fusion_params(name, voxel_length, sdf_trunc, depth_trunc)
    o, d, off = _grid_args(name, origin, dims, offset)
    return _integrate(depth.contiguous(), ma.upload(w2c, depth.device), intr, o, off, d, vl, trunc, dtrunc)


def tsdf_face_keep(vertices, faces, weight):
    """open3d's validity rule for the faces of ``marching_cubes(tsdf, 0.0)`` (vertices in index units): a bool mask
    [F], true iff every lattice point in [floor(min), ceil(max)] per axis of the face's three vertices has
    ``weight > 0``.  For a face with area those are the 8 corners of its cell (open3d emits a cell's triangles only if
    all 8 corners were observed); for a face that lies in a cell face, that face's 4 corners."""
    name = 'tsdf_face_keep'
    ma.check_tensor(name, 'vertices', vertices, shape='[V, 3]')
    ma.check_tensor(name, 'faces', faces, (torch.int32,), '[F, 3]')
    ma.check_tensor(name, 'weight', weight, shape='[nx, ny, nz]')
    if weight.numel() == 0 or weight.numel() >= 2 ** 31:
        raise ValueError('%s: weight must be [nx, ny, nz], got %s' % (name, tuple(weight.shape)))
    dev = ma.same_device(name, vertices=vertices, faces=faces, weight=weight)
    v, f, wt = vertices.contiguous(), faces.contiguous(), weight.contiguous()
    keep = torch.zeros(f.shape[0], dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ma.call('msdf_tsdf_face_keep', v, v.shape[0], f, f.shape[0], wt, *wt.shape, keep)
    return keep.bool()


def extract_mesh(tsdf, weight, origin, voxel_length, offset=(0, 0, 0)):
    """The zero level set of a fused block, observed cells only: ``marching_cubes(tsdf, 0.0)`` in index units, the
    faces ``tsdf_face_keep`` keeps, vertices no kept face refers to dropped and the faces re-indexed.
    -> (vertices [V,3] float64 world = origin + voxel_length (0.5 + offset + v) (voxel_length as fp32), faces [F,3] int64, normals [V,3]
    float32), CUDA tensors.  Normals and winding point toward increasing tsdf: the free space in front of the surface."""
    name = 'extract_mesh'
    ma.check_tensor(name, 'weight', weight, shape='[nx, ny, nz]')
    if not isinstance(tsdf, torch.Tensor) or tsdf.shape != weight.shape or tsdf.device != weight.device:
        raise ValueError('%s: tsdf and weight must have one shape and device' % name)
    o = torch.tensor([float(x) for x in np.asarray(origin, np.float64).reshape(3)], dtype=torch.float64)
    off = torch.tensor([float(int(x)) for x in offset], dtype=torch.float64)
    vl = _fusion_params(name, voxel_length, None, 0.0)[0]
    v, f, nrm = marching_cubes(tsdf, 0.0, (1.0, 1.0, 1.0))
    if f.shape[0] > 0:
        f = f[tsdf_face_keep(v, f, weight)].long()
        used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
        used[f.reshape(-1)] = True
        v, nrm, f = v[used], nrm[used], ma.compact_faces(used, f, all_kept=True)
    else:
        f = f.long()
    world = (o + vl * (0.5 + off)).to(v.device) + vl * v.double()
    return world, f, nrm


def fusion_grid(vmin, vmax, voxel_length, sdf_trunc=None):
    """The volume ``refuse`` fuses into: the bounding box [vmin, vmax] padded by sdf_trunc + voxel_length on every
    side -> (origin [3] float64, dims (nx, ny, nz) voxels, each >= 2)."""
    vl, trunc, _ = _fusion_params('fusion_grid', voxel_length, sdf_trunc, 0.0)
    lo = np.asarray(vmin, np.float64).reshape(3) - (trunc + vl)
    hi = np.asarray(vmax, np.float64).reshape(3) + (trunc + vl)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError('fusion_grid: bounds %s .. %s' % (lo.tolist(), hi.tolist()))
    dims = np.maximum(np.ceil((hi - lo) / vl).astype(np.int64), 2)
    if dims.max() > 2 ** 24:
        raise ValueError('fusion_grid: %d voxels along an axis (extent %g, voxel %g): at most 2^24' %
                         (dims.max(), float((hi - lo).max()), vl))
    return lo, tuple(int(d) for d in dims)


def _block_starts(n_voxels, block):
    """Blocks of at most ``block`` cells (block + 1 voxels) that share one layer of voxels: [(start, voxels)]."""
    return [(s, min(block, n_voxels - 1 - s) + 1) for s in range(0, n_voxels - 1, block)]


@torch.no_grad()
def refuse(mesh, poses, K, height, width, voxel_length=0.01, sdf_trunc=None, depth_trunc=5.0, block=512,
           view_chunk=None):
    """``refuse(mesh, poses, K)`` of scannet_eval/evaluate.py:111-137 (postprocess/refuse.py is the same at 1 mm): the
    mesh is rendered to a depth map from every pose, the depth maps are fused into a TSDF volume (``voxel_length``,
    ``sdf_trunc`` = 3 voxel_length by default, depths beyond ``depth_trunc`` ignored) and a new mesh is extracted,
    which holds only surface some camera saw.  -> Mesh.

    ``mesh``: a Mesh or a (vertices, faces) pair (numpy arrays are uploaded; CUDA tensors: float32 / int32).  The
    volume is the mesh's bounding box padded by sdf_trunc + voxel_length, cut into blocks of at most ``block`` cells
    per axis (< 1290: marching cubes takes fewer than 2^31 voxels) that share one layer of voxels, as
    get_surface_sliding's do: memory is bounded by one block, every voxel has the same value in every block that holds
    it, and the seam vertices of neighbouring blocks stay separate.  Each block is integrated over all views, extracted
    and joined with ``mesh.concatenate``; only the final mesh crosses to the host.  The depth maps (n H W 4 bytes) are
    rendered once; with ``view_chunk`` they are rendered ``view_chunk`` views at a time instead, again for every block,
    and held one chunk at a time.  Parity with pyrender and open3d is UNVERIFIED (see the module's docstring)."""
    name = 'refuse'
    w2c_h = _world_to_camera(name, poses)
    intr = _intrinsics(name, K)
    h, w = _image_size(name, height, width)
    vl, trunc, dtrunc = _fusion_params(name, voxel_length, sdf_trunc, depth_trunc)
    block = int(block)
    if block < 1 or (block + 1) ** 3 >= 2 ** 31:
        raise ValueError('%s: block must be in [1, 1289], got %d' % (name, block))
    n = w2c_h.shape[0]
    chunk = n if view_chunk is None else int(view_chunk)
    if chunk < 1:
        raise ValueError('%s: view_chunk must be positive, got %r' % (name, view_chunk))
    v, f, _ = ma.mesh_tensors(name, mesh)
    if v.shape[0] == 0 or f.shape[0] == 0:
        return concatenate([])
    w2c = ma.upload(w2c_h, v.device)
    lo, hi = torch.aminmax(v, dim=0)
    origin, dims = fusion_grid(lo.double().cpu().numpy(), hi.double().cpu().numpy(), vl, trunc)
    origin32 = tuple(float(np.float32(x)) for x in origin)
    chunks = [(a, min(a + chunk, n)) for a in range(0, n, chunk)]
    depth = _raster(v, f, w2c, intr, h, w, 0.05, 100.0, 0.5) if len(chunks) == 1 else None
    parts = []
    for si, mi in _block_starts(dims[0], block):
        for sj, mj in _block_starts(dims[1], block):
            for sk, mk in _block_starts(dims[2], block):
                state = None
                for a, b in chunks:
                    d = depth if depth is not None else _raster(v, f, w2c[a:b].contiguous(), intr, h, w, 0.05,
                                                                100.0, 0.5)
                    state = _integrate(d, w2c[a:b].contiguous(), intr, origin32, (si, sj, sk), (mi, mj, mk), vl, trunc,
                                       dtrunc, state)
                bv, bf, bn = extract_mesh(state[0], state[1], origin32, vl, (si, sj, sk))
                del state
                if bf.shape[0] > 0:
                    parts.append(Mesh(bv.cpu().numpy(), bf.cpu().numpy(), bn.cpu().numpy()))
    return concatenate(parts)


def seen_vertices(vertices, poses, K, height, width):
    """For every vertex whether some camera sees it: bool [V] on the vertices' device.  vertices [V,3] float32 CUDA.
    With p = pose^-1 x, in fp32: seen iff p.z >= 1e-5 and 0 < fx p.x / (p.z - 1e-5) + cx < width and
    0 < fy p.y / (p.z - 1e-5) + cy < height (the test of replica_eval/cull_mesh.py:66-81 in the OpenCV frame; the
    1e-5 is the reference's).  One lane per vertex loops over the views and stops at the first that sees it."""
    name = 'seen_vertices'
    ma.check_tensor(name, 'vertices', vertices, shape='[V, 3]')
    return _seen(vertices.contiguous(), _world_to_camera(name, poses), _intrinsics(name, K),
                 *_image_size(name, height, width))


def _seen(v, w2c, intr, h, w):
    seen = torch.zeros(v.shape[0], dtype=torch.uint8, device=v.device)
    with torch.cuda.device(v.device):
        ma.call('msdf_cull_vertices', v, v.shape[0], ma.upload(w2c, v.device), w2c.shape[0], *intr, h, w, seen)
    return seen.bool()


@torch.no_grad()
def cull_to_frustums(mesh, poses, K, height, width):
    """replica_eval/cull_mesh.py:58-87: the faces none of whose three vertices lies in any camera frustum
    (``seen_vertices``) are dropped; the vertices all stay, as trimesh's ``update_faces`` leaves them.  ``mesh``: a Mesh
    or a (vertices, faces) pair (numpy arrays are uploaded; CUDA tensors: float32 / int32).  -> Mesh."""
    name = 'cull_to_frustums'
    w2c, intr, size = _world_to_camera(name, poses), _intrinsics(name, K), _image_size(name, height, width)
    v, f, nrm = ma.mesh_tensors(name, mesh)
    seen = _seen(v, w2c, intr, *size)
    keep = seen[f.long()].any(dim=1) if f.shape[0] > 0 else torch.zeros(0, dtype=torch.bool, device=v.device)
    hv = ma.mesh_parts(mesh)[0]                        # the vertices all stay, host ones as they came (fp64)
    return Mesh(v.cpu().numpy() if isinstance(hv, torch.Tensor) else hv, f[keep].cpu().numpy(), nrm)


def read_poses(path, every=1):
    """Camera-to-world matrices [n,4,4] float64 from a ScanNet ``pose`` directory (files ``N.txt`` holding a 4x4
    matrix, taken in ascending N; scannet_eval/evaluate.py:62-73) or a Replica ``traj.txt`` (16 numbers per line, row
    major; cull_mesh.py:14-24, whose two axis flips and the later sign changes cancel: the file's matrices are
    OpenCV-style as they stand).  ``every``: keep every ``every``-th view.  Views with a non-finite entry (ScanNet
    marks lost tracking with -inf) are left out."""
    if os.path.isdir(path):
        names = [n for n in os.listdir(path) if re.fullmatch(r'\d+\.txt', n)]
        names.sort(key=lambda n: int(n[:-4]))
        mats = [np.loadtxt(os.path.join(path, n), dtype=np.float64).reshape(-1) for n in names[::every]]
    else:
        with open(path) as fh:
            rows = [line.split() for line in fh if line.strip()]
        mats = [np.array([float(x) for x in r], dtype=np.float64) for r in rows[::every]]
    for m in mats:
        if m.shape != (16,):
            raise ValueError('read_poses: %s: a pose of %d numbers (16 needed)' % (path, m.size))
    mats = [m.reshape(4, 4) for m in mats if np.isfinite(m).all()]
    return np.stack(mats) if mats else np.zeros((0, 4, 4))


def read_intrinsics(path):
    """(fx, fy, cx, cy) from a text file holding a 3x3 or 4x4 intrinsic matrix (ScanNet's ``intrinsic_color.txt``) or
    the four numbers themselves."""
    k = np.loadtxt(path, dtype=np.float64)
    if k.size == 4:
        return tuple(float(x) for x in k.reshape(-1))
    return _intrinsics('read_intrinsics', k)
