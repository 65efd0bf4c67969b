"""Mesh evaluation on the GPU: what the reference's scripts compute after the mesh export.

* ``nearest_neighbors``: exact brute-force 1-nearest-neighbour search (csrc/nnsearch.hip, ABI msdf_nn_*), in place of
  sklearn's ``KDTree(...).query`` (scannet_eval/evaluate.py:16-26) and scipy's ``cKDTree(...).query``
  (replica_eval/eval_recon.py:25-43, 96-106).
* ``voxel_down_sample``: the rule of open3d's ``PointCloud.voxel_down_sample`` (evaluate.py:36-38; ABI msdf_voxel_*).
* ``sample_surface``, ``face_normals``: trimesh.sample.sample_surface and Trimesh.face_normals (eval_recon.py:138-158).
* ``evaluate_scannet``: ``evaluate`` (evaluate.py:29-56).  ``evaluate_replica``: the metrics of ``calc_3d_metric``
  (eval_recon.py:138-177).
* ``read_ply``: ASCII / binary little-endian PLY meshes written by other programs.

Everything runs on CUDA tensors; there is no CPU path.  Out of scope: ICP alignment (``get_align_transformation``),
the oriented-bounding-box crop of ``calc_3d_metric`` (eval_recon.py:121-136), and any grid- or tree-accelerated search:
brute force is the exact baseline a later one is checked against.  View culling and TSDF re-fusion (``refuse``), which
the reference applies to the predicted mesh before it calls these metrics, are in utils/mesh_refuse.py; the DTU protocol
and its mask culling are in utils/mesh_dtu.py.
"""
import numpy as np
import torch

from .. import _lib
from .mesh import Mesh


def _check_cloud(name, arg, t):
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise TypeError('%s: %s must be a CUDA tensor (there is no CPU path), got %s' %
                        (name, arg, t.device if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dtype != torch.float32:
        raise TypeError('%s: %s must be float32, got %s' % (name, arg, t.dtype))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError('%s: %s must be [N, 3], got %s' % (name, arg, tuple(t.shape)))
    if t.shape[0] >= 2 ** 31:
        raise ValueError('%s: %s has %d points: int32 indices hold fewer than 2^31' % (name, arg, t.shape[0]))


def nearest_neighbors(reference, query, n_splits=0):
    """For every ``query[i]`` the closest point of ``reference``: ``(dist [Q] float32, idx [Q] int64)``, exact, by
    brute force on the GPU.  reference [R,3], query [Q,3]: float32 CUDA tensors on one device.

    The squared distance is dx^2 + dy^2 + dz^2 of the three fp32 differences (relative error of ``dist`` about 2.4e-7
    wherever the clouds lie).  Of several reference points at the same fp32 squared distance the smallest index wins.
    The same inputs give bitwise the same outputs every call and for every ``n_splits`` (over how many slices of the
    reference cloud the work is spread; 0 = chosen from the sizes).  ValueError for an empty reference cloud and for
    non-finite coordinates (one device reduction and one host read)."""
    _check_cloud('nearest_neighbors', 'reference', reference)
    _check_cloud('nearest_neighbors', 'query', query)
    if reference.device != query.device:
        raise ValueError('nearest_neighbors: reference on %s, query on %s' % (reference.device, query.device))
    R, Q = reference.shape[0], query.shape[0]
    if R == 0:
        raise ValueError('nearest_neighbors: the reference cloud is empty')
    dev = query.device
    ref, qry = reference.contiguous(), query.contiguous()
    if not bool((torch.isfinite(ref).all() & torch.isfinite(qry).all()).item()):
        raise ValueError('nearest_neighbors: non-finite coordinates')
    dist = torch.empty(Q, dtype=torch.float32, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q > 0:
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = torch.empty(int(lib.msdf_nn_workspace_bytes(R, Q, int(n_splits))), dtype=torch.uint8, device=dev)
            _lib.call('msdf_nn_search', _lib.ptr(ref), R, _lib.ptr(qry), Q, int(n_splits), _lib.ptr(ws),
                      _lib.ptr(dist), _lib.ptr(idx), _lib.stream_ptr())
    return dist, idx.long()


_VOXEL_AXIS_MAX = 2 ** 21            # cells per axis the 63-bit voxel key holds


def voxel_down_sample(points, voxel_size):
    """One point per occupied voxel, the mean of the points in it: points [N,3] float32 CUDA -> [M,3].

    The rule of open3d's ``PointCloud.voxel_down_sample``: voxel of a point = floor((p - (min_bound - v/2)) / v) per
    axis with min_bound the per-axis minimum of the cloud.  Arithmetic: the voxel coordinate in fp32 with separately
    rounded operations, the sum of a voxel in fp64 in ascending original point index, rounded once to fp32.  Output
    order: ascending (ix, iy, iz).  No floating-point atomics: the same cloud gives bitwise the same output every call.
    Parity with open3d's own binning is UNVERIFIED: open3d is not available where this is built and the reference
    holds no recorded output of it, so the rule is pinned by the numpy restatement of the tests only (a point within
    rounding of a voxel face may fall on the other side there, and open3d's output order is its hash map's)."""
    _check_cloud('voxel_down_sample', 'points', points)
    v = float(np.float32(voxel_size))
    if not v > 0.0:
        raise ValueError('voxel_down_sample: voxel_size must be positive, got %r' % (voxel_size,))
    n = points.shape[0]
    dev = points.device
    if n == 0:
        return points.new_empty(0, 3)
    pts = points.contiguous()
    lo, hi = torch.aminmax(pts, dim=0)
    lo_h, hi_h = lo.double().cpu(), hi.double().cpu()
    if not bool(torch.isfinite(lo_h).all() and torch.isfinite(hi_h).all()):
        raise ValueError('voxel_down_sample: non-finite coordinates')
    if float(((hi_h - lo_h) / v).max()) + 2.0 >= _VOXEL_AXIS_MAX:
        raise ValueError('voxel_down_sample: more than 2^21 voxels along an axis (extent %g, voxel %g)' %
                         (float((hi_h - lo_h).max()), v))
    with torch.cuda.device(dev):
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.call('msdf_voxel_keys', _lib.ptr(pts), n, _lib.ptr(lo.contiguous()), v, _lib.ptr(keys),
                  _lib.stream_ptr())
        sorted_keys, order = torch.sort(keys, stable=True)
        head = torch.ones(n, dtype=torch.bool, device=dev)
        head[1:] = sorted_keys[1:] != sorted_keys[:-1]
        seg_start = head.nonzero().squeeze(1).contiguous()
        m = seg_start.shape[0]
        out = torch.empty(m, 3, dtype=torch.float32, device=dev)
        _lib.call('msdf_voxel_mean', _lib.ptr(pts), _lib.ptr(order), _lib.ptr(seg_start), n, m, _lib.ptr(out),
                  _lib.stream_ptr())
    return out


def _check_mesh(name, vertices, faces):
    _check_cloud(name, 'vertices', vertices)
    if not isinstance(faces, torch.Tensor) or faces.device != vertices.device:
        raise TypeError('%s: faces must be a tensor on %s' % (name, vertices.device))
    if faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('%s: faces must be an integer [F, 3] tensor' % name)


def _face_cross(vertices, faces):
    """origin, the two edge vectors and their cross product per face, in fp64."""
    tri = vertices.double()[faces.long()]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    return tri[:, 0], e1, e2, torch.linalg.cross(e1, e2)


def face_normals(vertices, faces):
    """Unit normals by the right-hand rule, [F,3] float32; zero for degenerate (zero-area) faces."""
    _check_mesh('face_normals', vertices, faces)
    c = _face_cross(vertices, faces)[3]
    norm = c.norm(dim=1, keepdim=True)
    return torch.where(norm > 0, c / torch.where(norm > 0, norm, torch.ones_like(norm)),
                       torch.zeros_like(c)).float()


def sample_surface(vertices, faces, count, generator=None):
    """``count`` points uniform on the surface, as trimesh.sample.sample_surface: a face drawn with probability
    proportional to its area, a uniform point in it (the unit square folded onto the triangle).
    -> (points [count,3] float32, face_index [count] int64).  Degenerate (zero-area) faces are never drawn.
    ``generator``: a torch.Generator on the vertices' device; the same seed gives the same samples."""
    _check_mesh('sample_surface', vertices, faces)
    dev = vertices.device
    origin, e1, e2, c = _face_cross(vertices, faces)
    cum = torch.cumsum(0.5 * c.norm(dim=1), 0)
    if faces.shape[0] == 0 or not float(cum[-1]) > 0.0:
        raise ValueError('sample_surface: the mesh has no area')
    u = torch.rand(count, 3, dtype=torch.float64, device=dev, generator=generator)
    # pick in [0, total): face i is drawn for cum[i-1] <= pick < cum[i], an empty interval for a zero-area face
    pick = torch.minimum(u[:, 0] * cum[-1], torch.nextafter(cum[-1], torch.zeros_like(cum[-1])))
    face_index = torch.searchsorted(cum, pick, right=True)
    a, b = u[:, 1], u[:, 2]
    fold = a + b > 1.0
    a, b = torch.where(fold, 1.0 - a, a), torch.where(fold, 1.0 - b, b)
    pts = origin[face_index] + a[:, None] * e1[face_index] + b[:, None] * e2[face_index]
    return pts.float(), face_index


def _cloud(x, dev=None):
    """A Mesh, a numpy array or a CUDA tensor -> float32 CUDA [N,3] (host data is uploaded; a CPU tensor is refused
    by the functions that receive it)."""
    if isinstance(x, Mesh):
        x = x.vertices
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x[:, :3], np.float32)).to(dev or 'cuda')
    return x


def _fscore(p, r):
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def evaluate_scannet(pred_vertices, gt_vertices, threshold=0.05, down_sample=0.02):
    """``evaluate`` of scannet_eval/evaluate.py:29-56 on two vertex clouds (float32 CUDA tensors [N,3]; numpy arrays
    and Mesh objects are uploaded): both voxel-down-sampled (``down_sample`` = 0 / None: not), nearest neighbours both
    ways, then with the reference's keys, as Python floats:
      'Acc'   mean distance from the predicted points to the target cloud      'Prec'  share of them < threshold
      'Comp'  mean distance from the target points to the predicted cloud      'Recal' share of them < threshold
      'F-score' 2 Prec Recal / (Prec + Recal), 0.0 when both are zero.
    The down-sample follows open3d's rule but its parity with open3d is unverified (see voxel_down_sample)."""
    pred, gt = _cloud(pred_vertices), _cloud(gt_vertices)
    if down_sample:
        pred, gt = voxel_down_sample(pred, down_sample), voxel_down_sample(gt, down_sample)
    else:
        _check_cloud('evaluate_scannet', 'pred_vertices', pred)
        _check_cloud('evaluate_scannet', 'gt_vertices', gt)
    if pred.shape[0] == 0 or gt.shape[0] == 0:
        raise ValueError('evaluate_scannet: an empty cloud')
    dist1, _ = nearest_neighbors(pred, gt)              # target -> predicted
    dist2, _ = nearest_neighbors(gt, pred)              # predicted -> target
    vals = torch.stack([dist2.double().mean(), dist1.double().mean(), (dist2 < threshold).double().mean(),
                        (dist1 < threshold).double().mean()]).tolist()
    acc, comp, prec, recal = vals
    return {'Acc': acc, 'Comp': comp, 'Prec': prec, 'Recal': recal, 'F-score': _fscore(prec, recal)}


def _mesh_tensors(m, name):
    if isinstance(m, Mesh):
        v, f = m.vertices, m.faces
    else:
        v, f = m
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    if isinstance(f, np.ndarray):
        f = torch.from_numpy(np.ascontiguousarray(f, np.int64)).to(v.device)
    _check_mesh(name, v, f)
    return v, f


def evaluate_replica(rec, gt, n_samples=200000, dist_th=0.05, seed=0, return_samples=False):
    """The metrics of ``calc_3d_metric`` (replica_eval/eval_recon.py:138-177).  ``rec``, ``gt``: Mesh objects or
    (vertices [V,3], faces [F,3]) pairs (CUDA tensors, or numpy arrays, which are uploaded).  ``n_samples``
    area-weighted surface samples of each mesh (``seed`` fixes them), nearest neighbours both ways, then:
      'accuracy'  mean distance rec -> gt, cm            'precision'         share of rec samples within dist_th, %
      'completion' mean distance gt -> rec, cm           'completion_ratio'  share of gt samples within dist_th, %
      'fscore'    2 P R / (P + R) of those two, %, 0.0 when both are zero
      'chamfer'   (accuracy + completion) / 2, cm
      'normal_acc' / 'normal_comp'  mean |cos| between the face normal of a rec / gt sample and the face normal of its
                  nearest neighbour in the other cloud, %;  'normal_avg' their mean.
    The reference draws a second set of samples for the normals; here one set serves both.  Not done here: the ICP
    alignment and the oriented-bounding-box crop that ``calc_3d_metric`` applies first (pass meshes already aligned
    and cropped).  ``return_samples``: also a dict with 'rec_points', 'rec_faces', 'gt_points', 'gt_faces' (the samples
    and the face each came from), 'rec_normals', 'gt_normals' (per sample)."""
    rv, rf = _mesh_tensors(rec, 'evaluate_replica')
    gv, gf = _mesh_tensors(gt, 'evaluate_replica')
    gen = torch.Generator(device=rv.device)
    gen.manual_seed(int(seed))
    rp, rfi = sample_surface(rv, rf, n_samples, gen)
    gp, gfi = sample_surface(gv, gf, n_samples, gen)
    rn, gn = face_normals(rv, rf)[rfi], face_normals(gv, gf)[gfi]
    d_acc, i_gt = nearest_neighbors(gp, rp)             # rec -> gt
    d_comp, i_rec = nearest_neighbors(rp, gp)           # gt -> rec
    n_acc = (rn.double() * gn.double()[i_gt]).sum(1).abs().mean()
    n_comp = (gn.double() * rn.double()[i_rec]).sum(1).abs().mean()
    vals = torch.stack([d_acc.double().mean(), d_comp.double().mean(), (d_acc < dist_th).double().mean(),
                        (d_comp < dist_th).double().mean(), n_acc, n_comp]).tolist()
    acc, comp, prec, ratio, n_acc, n_comp = vals
    out = {'accuracy': acc * 100, 'completion': comp * 100, 'precision': prec * 100, 'completion_ratio': ratio * 100,
           'fscore': _fscore(prec, ratio) * 100, 'chamfer': (acc * 100 + comp * 100) / 2,
           'normal_acc': n_acc * 100, 'normal_comp': n_comp * 100, 'normal_avg': (n_acc + n_comp) * 0.5 * 100}
    if return_samples:
        return out, {'rec_points': rp, 'rec_faces': rfi, 'rec_normals': rn,
                     'gt_points': gp, 'gt_faces': gfi, 'gt_normals': gn}
    return out


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2',
              'ushort': 'u2', 'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4',
              'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _ply_header(data):
    if data[:4] not in (b'ply\n', b'ply\r'):
        raise ValueError('read_ply: not a PLY file')
    end = data.find(b'end_header')
    if end < 0:
        raise ValueError('read_ply: no end_header')
    body = data.index(b'\n', end) + 1
    fmt, elements = None, []
    for line in data[:end].decode('ascii').splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ('comment', 'obj_info'):
            continue
        if w[0] == 'format':
            fmt = w[1]
        elif w[0] == 'element':
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property':
            if not elements:
                raise ValueError('read_ply: property before element')
            try:
                if w[1] == 'list':
                    elements[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
                else:
                    elements[-1][2].append((w[2], _PLY_TYPES[w[1]], None))
            except KeyError as e:
                raise ValueError('read_ply: unknown property type %s' % e)
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError('read_ply: format %r is not read (ascii and binary_little_endian are)' % fmt)
    return fmt, elements, body


def read_ply(path):
    """A triangle mesh from an ASCII or binary little-endian PLY written by any program -> Mesh.  Vertex properties:
    x, y, z found by name (float or double; nx, ny, nz too if present), every other scalar property skipped.  Faces:
    the list property ``vertex_indices`` / ``vertex_index`` of any integer count and index type, triangles only; other
    scalar face properties skipped.  A file without a face element gives a mesh without faces (a point cloud)."""
    with open(path, 'rb') as fh:
        data = fh.read()
    fmt, elements, pos = _ply_header(data)
    names = [e[0] for e in elements]
    if 'vertex' not in names:
        raise ValueError('read_ply: no vertex element')
    wanted = names.index('face') if 'face' in names else names.index('vertex')
    tokens = data[pos:].split() if fmt == 'ascii' else None
    tpos = 0
    verts = normals = None
    faces = np.zeros((0, 3), np.int64)
    for k, (name, count, props) in enumerate(elements[:wanted + 1]):
        lists = [p for p in props if p[2] is not None]
        if name == 'face':
            if len(lists) != 1 or lists[0][0] not in ('vertex_indices', 'vertex_index'):
                raise ValueError('read_ply: face element needs one list property vertex_indices')
        elif lists:
            raise ValueError('read_ply: list property in element %r' % name)
        # the record of one row, lists taken as triangles (checked below)
        fields = []
        for pname, a, b in props:
            if b is None:
                fields.append((pname, '<' + a))
            else:
                fields += [(pname + '#n', '<' + a), (pname, '<' + b, (3,))]
        dt = np.dtype(fields)
        width = sum(3 if len(f) == 3 else 1 for f in fields)
        if fmt == 'ascii':
            flat = np.array(tokens[tpos:tpos + count * width], dtype=np.float64)
            if flat.size != count * width:
                raise ValueError('read_ply: file ends inside element %r (only triangle faces are read)' % name)
            flat = flat.reshape(count, width)
            tpos += count * width
            rows, c = {}, 0
            for f in fields:
                w = 3 if len(f) == 3 else 1
                rows[f[0]] = flat[:, c] if w == 1 else flat[:, c:c + 3]
                c += w
        else:
            if pos + count * dt.itemsize > len(data):
                raise ValueError('read_ply: file ends inside element %r (only triangle faces are read)' % name)
            rows = np.frombuffer(data, dt, count, pos)
            pos += count * dt.itemsize
        if name == 'vertex':
            for axis in 'xyz':
                if axis not in dt.names:
                    raise ValueError('read_ply: vertex property %r missing' % axis)
            verts = np.stack([np.asarray(rows[a], np.float64) for a in 'xyz'], 1).reshape(-1, 3)
            if all(a in dt.names for a in ('nx', 'ny', 'nz')):
                normals = np.stack([np.asarray(rows[a], np.float64) for a in ('nx', 'ny', 'nz')], 1).reshape(-1, 3)
        elif name == 'face':
            lname = lists[0][0]
            if count and not (np.asarray(rows[lname + '#n']) == 3).all():
                raise ValueError('read_ply: only triangles are read')
            faces = np.asarray(rows[lname]).astype(np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError('read_ply: face index out of range')
    return Mesh(verts, faces, normals)
