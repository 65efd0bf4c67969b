"""Mesh rendering on the GPU: which face every pixel shows, shaded frames and the depth L1 of two meshes
(csrc/meshrender.hip, ABI include/monosdf_render.h, which states every rule operation by operation).

* ``visibility``: depth and face index per pixel from every pose, with back- or front-face culling; with
  ``cull='none'`` the depth is bit for bit ``mesh_refuse.render_depth``'s (one rasteriser, csrc/raster_core.h).
* ``vertex_normals``: area-weighted smooth normals (what open3d's ``compute_vertex_normals`` does, as far as its
  source was recalled when this was written).
* ``RenderOptions``, ``shade``, ``render_frames``: the frames of render/render_trajectory_open3d.py and
  render_tntvideos_open3d.py: Phong shading with the four lights of render/render.json, which move with the camera.
* ``read_o3d_camera``: open3d's ``PinholeCameraParameters`` JSON, the files those scripts are steered with.
* ``depth_l1``, ``views_see``, ``interior_view_box``, ``sample_views``, ``evaluate_depth_l1``: ``calc_2d_metric`` of
  replica_eval/eval_recon.py:196-285: the mean depth difference of two meshes over random views from inside the room
  that see none of the points the ground truth never observed.

Cameras are OpenCV-style as in utils/mesh_refuse.py (``pose`` a 4x4 camera-to-world matrix, ``K`` = (fx, fy, cx, cy) or
a matrix); everything runs on CUDA tensors, arguments are checked by utils/mesh_args.py, and the same inputs give
bitwise the same outputs every call (no floating-point atomics).

Parity with open3d is UNVERIFIED throughout: there is no open3d and no OpenGL context where this is built and the
reference holds no recorded frame.  The shading follows open3d's Phong shader as far as render.json determines it;
vertex normals, the light rig (positions relative to the bounding box, in the camera's axes) and the near plane of
``evaluate_depth_l1`` (0.01 of the largest extent) are written down from memory of its source.  They are pinned by the
numpy restatements of the tests (tests/render_numpy.py) only.  Not built: wireframe and point rendering,
anti-aliasing, textures, the coloured error clouds.
"""
import dataclasses
import json

import numpy as np
import torch

from . import mesh_args as ma
from .mesh_refuse import _image_size, _intrinsics, _raster, _world_to_camera

CULL = {'none': 0, 'back': 1, 'front': 2}
LIGHT_TABLE_FLOATS = 42


def _planes(name, znear, zfar, pixel_center):
    if not (float(znear) > 0.0 and float(zfar) >= float(znear) and np.isfinite(pixel_center)):
        raise ValueError('%s: 0 < znear <= zfar needed, got %r, %r' % (name, znear, zfar))
    return float(znear), float(zfar), float(pixel_center)


def _cull_mode(name, cull):
    if cull not in CULL:
        raise ValueError("%s: cull must be 'none', 'back' or 'front', got %r" % (name, cull))
    return CULL[cull]


def _visibility(v, f, w2c, intr, h, w, znear, zfar, pixel_center, cull):
    n = w2c.shape[0]
    depth = torch.empty(n, h, w, dtype=torch.float32, device=v.device)
    face = torch.empty(n, h, w, dtype=torch.int32, device=v.device)
    ws = ma.workspace('visibility', 'msdf_rnd_visibility_workspace_bytes', n, h, w, device=v.device)
    with torch.cuda.device(v.device):
        ma.call('msdf_rnd_visibility', v, v.shape[0], f, f.shape[0], w2c, n, *intr, h, w, znear, zfar, pixel_center,
                cull, ws, depth, face)
    return depth, face


def visibility(vertices, faces, poses, K, height, width, znear=0.05, zfar=100.0, pixel_center=0.5, cull='none'):
    """What every pixel of ``n`` views shows: ``(depth [n, H, W] float32, face [n, H, W] int32)`` on the mesh's device.

    Arguments as ``mesh_refuse.render_depth``.  depth is the camera-frame z of the nearest accepted intersection (0:
    none), face the index of the face that gives it (-1: none): of several faces that reach exactly the same bits of
    depth, the smallest index.  ``cull``: 'none' takes every face and then depth is bit for bit ``render_depth``'s;
    'back' drops a face where it is seen from behind (its normal (b - a) x (c - a) points away from the camera), 'front'
    where it is seen from the front.  Marching-cubes meshes of this package wind their faces so that the normal points
    toward growing SDF, the free space a camera stands in: 'back' is the natural choice for them.  Bitwise repeatable;
    the face order matters only through the index that is reported."""
    name = 'visibility'
    w2c = _world_to_camera(name, poses)
    intr = _intrinsics(name, K)
    h, w = _image_size(name, height, width)
    if w2c.shape[0] * h * w >= 2 ** 31:
        raise ValueError('%s: %d views of %d x %d pixels: fewer than 2^31 pixels in one call' % (name, w2c.shape[0], h, w))
    znear, zfar, pc = _planes(name, znear, zfar, pixel_center)
    mode = _cull_mode(name, cull)
    v, f, _ = ma.mesh_tensors(name, (vertices, faces))
    return _visibility(v, f, ma.upload(w2c, v.device), intr, h, w, znear, zfar, pc, mode)


def _vertex_normals(v, f):
    n_v, n_f = v.shape[0], f.shape[0]
    normals = torch.empty(n_v, 3, dtype=torch.float32, device=v.device)
    if n_v == 0:
        return normals
    if 3 * n_f >= 2 ** 31:
        raise ValueError('vertex_normals: %d faces: 3 F must stay below 2^31' % n_f)
    flat = f.reshape(-1).long()
    # the (vertex, face) pairs in face order, sorted by vertex: stable, so each vertex keeps its faces ascending
    order = torch.sort(flat, stable=True).indices
    inc_face = torch.div(order, 3, rounding_mode='floor').to(torch.int32).contiguous()
    counts = torch.bincount(flat, minlength=n_v)
    inc_start = torch.zeros(n_v + 1, dtype=torch.int32, device=v.device)
    inc_start[1:] = torch.cumsum(counts, 0).to(torch.int32)
    with torch.cuda.device(v.device):
        ma.call('msdf_rnd_vertex_normals', v, n_v, f, n_f, inc_start, inc_face, normals)
    return normals


def vertex_normals(vertices, faces):
    """Smooth vertex normals [V, 3] float32: per vertex the sum of (b - a) x (c - a) over its faces (so weighted by
    area), in fp64 in ascending face index, normalised in fp64 and rounded once; (0, 0, 1) for a vertex without a face
    with area.  Faces with a repeated index add nothing.  Parity with open3d's ``compute_vertex_normals`` is
    UNVERIFIED (see the module's docstring)."""
    v, f, _ = ma.mesh_tensors('vertex_normals', (vertices, faces))
    return _vertex_normals(v, f)


_LIGHT_FIELDS = ('position', 'color', 'diffuse_power', 'specular_power', 'specular_shininess')


@dataclasses.dataclass(frozen=True)
class RenderOptions:
    """The fields of open3d's ``RenderOption`` JSON that the shading uses; the defaults are render/render.json's."""
    background_color: tuple = (1.0, 1.0, 1.0)
    default_mesh_color: tuple = (0.7, 0.7, 0.7)
    light_ambient_color: tuple = (0.3, 0.3, 0.3)
    light_position: tuple = ((0.0, 0.0, 2.0), (0.0, 0.0, -2.0), (2.0, 2.0, 0.0), (-2.0, -2.0, 0.0))
    light_color: tuple = ((0.7, 0.7, 0.7),) * 4
    light_diffuse_power: tuple = (0.66000000000000014, 0.66000000000000014, 0.36000000000000015, 0.10000000000000014)
    light_specular_power: tuple = (0.2, 0.2, 1.0000000000000001e-17, 9.9999999999999998e-17)
    light_specular_shininess: tuple = (10.0, 10.0, 10.0, 0.1)
    light_on: bool = True
    mesh_show_back_face: bool = False

    @property
    def cull(self):
        """'none' when the file shows back faces, else 'back'."""
        return 'none' if self.mesh_show_back_face else 'back'

    @classmethod
    def from_json(cls, path):
        with open(path) as fh:
            d = json.load(fh)
        if d.get('class_name', 'RenderOption') != 'RenderOption':
            raise ValueError('RenderOptions.from_json: %s holds a %r' % (path, d.get('class_name')))

        def triple(key):
            return tuple(float(x) for x in d[key])
        lights = {f: tuple(triple('light%d_%s' % (i, f)) if f in ('position', 'color') else float(d['light%d_%s' % (i, f)])
                           for i in range(4)) for f in _LIGHT_FIELDS}
        return cls(background_color=triple('background_color'), default_mesh_color=triple('default_mesh_color'),
                   light_ambient_color=triple('light_ambient_color'), light_position=lights['position'],
                   light_color=lights['color'], light_diffuse_power=lights['diffuse_power'],
                   light_specular_power=lights['specular_power'],
                   light_specular_shininess=lights['specular_shininess'], light_on=bool(d.get('light_on', True)),
                   mesh_show_back_face=bool(d.get('mesh_show_back_face', False)))

    def light_table(self):
        """The 42 floats msdf_rnd_shade reads: per light position, colour, kd, ks, shininess; ambient; background.
        ``light_on`` false: no light has power and the ambient colour is white, so a pixel shows its base colour."""
        rows = []
        for i in range(4):
            kd, ks = (self.light_diffuse_power[i], self.light_specular_power[i]) if self.light_on else (0.0, 0.0)
            rows += [*self.light_position[i], *self.light_color[i], kd, ks, self.light_specular_shininess[i]]
        rows += list(self.light_ambient_color if self.light_on else (1.0, 1.0, 1.0)) + list(self.background_color)
        table = np.asarray(rows, np.float32)
        if table.shape != (LIGHT_TABLE_FLOATS,) or not np.isfinite(table).all():
            raise ValueError('RenderOptions: every light needs 3 + 3 + 3 finite numbers')
        return table


def _colour(name, arg, c):
    c = np.asarray(c, np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError('%s: %s must be 3 finite numbers' % (name, arg))
    return tuple(float(np.float32(x)) for x in c)


def _light_frame(v):
    """Centre and largest extent of the finite bounding box of the vertices, as the fp32 numbers the kernel gets."""
    if v.shape[0] == 0:
        return (0.0, 0.0, 0.0), 0.0
    _, lo, hi = ma.finite_bounds('shade', v)
    centre = ((lo + hi) / 2).numpy()
    return tuple(float(np.float32(x)) for x in centre), float(np.float32((hi - lo).max().item()))


def _shade(face, depth, w2c, intr, pc, v, f, normals, colors, base, table, centre, extent, flat, two_sided):
    n, h, w = face.shape
    rgb = torch.empty(n, h, w, 3, dtype=torch.float32, device=face.device)
    with torch.cuda.device(face.device):
        ma.call('msdf_rnd_shade', face, depth, n, h, w, w2c, *intr, pc, v, v.shape[0], f, f.shape[0], normals, colors,
                *base, table, *centre, extent, 1 if flat else 0, 1 if two_sided else 0, rgb)
    return rgb


def shade(face, depth, vertices, faces, poses, K, normals=None, options=RenderOptions(), base_color=(1.0, 1.0, 1.0),
          vertex_colors=None, flat=False, two_sided=False, pixel_center=0.5):
    """Phong-shaded frames ``rgb [n, H, W, 3]`` float32 in [0, 1] from the ``(depth, face)`` of ``visibility`` for the
    same mesh, poses and intrinsics.

    Per pixel, in the camera frame: the hit point is depth times the pixel's ray; the barycentric weights are the ray's
    own edge terms; the normal is the interpolated vertex normal (``normals`` [V, 3] float32, default
    ``vertex_normals``), normalised, or with ``flat`` the face's own; ``two_sided`` turns it toward the camera.  Four
    point lights at centre + extent (p.x right + p.y up + p.z toward the viewer) of the mesh's bounding box, in the
    camera's axes: the rig moves with the camera.  colour = base (ambient + sum kd cos_theta c) + sum ks cos_alpha^s c,
    clamped to [0, 1]; ``base_color`` is one colour, ``vertex_colors`` [V, 3] float32 are interpolated instead.
    Background pixels get ``options.background_color`` exactly.  include/monosdf_render.h states every operation."""
    name = 'shade'
    ma.check_tensor(name, 'face', face, (torch.int32,), '[n, H, W]')
    ma.check_tensor(name, 'depth', depth, shape='[n, H, W]')
    if face.shape != depth.shape:
        raise ValueError('%s: face %s, depth %s' % (name, tuple(face.shape), tuple(depth.shape)))
    w2c = _world_to_camera(name, poses)
    if w2c.shape[0] != face.shape[0]:
        raise ValueError('%s: %d images, %d poses' % (name, face.shape[0], w2c.shape[0]))
    intr = _intrinsics(name, K)
    _image_size(name, face.shape[1], face.shape[2])
    if face.numel() >= 2 ** 31 or not np.isfinite(pixel_center):
        raise ValueError('%s: fewer than 2^31 pixels and a finite pixel_center needed' % name)
    v, f, _ = ma.mesh_tensors(name, (vertices, faces))
    dev = ma.same_device(name, face=face, depth=depth, vertices=v)
    if normals is None:
        normals = None if flat else _vertex_normals(v, f)
    else:
        ma.check_tensor(name, 'normals', normals, shape='[V, 3]')
        if normals.shape[0] != v.shape[0] or normals.device != dev:
            raise ValueError('%s: normals must be [%d, 3] on %s' % (name, v.shape[0], dev))
        normals = normals.contiguous()
    if vertex_colors is not None:
        ma.check_tensor(name, 'vertex_colors', vertex_colors, shape='[V, 3]')
        if vertex_colors.shape[0] != v.shape[0] or vertex_colors.device != dev:
            raise ValueError('%s: vertex_colors must be [%d, 3] on %s' % (name, v.shape[0], dev))
        vertex_colors = vertex_colors.contiguous()
    centre, extent = _light_frame(v)
    return _shade(face.contiguous(), depth.contiguous(), ma.upload(w2c, dev), intr, float(pixel_center), v, f, normals,
                  vertex_colors, _colour(name, 'base_color', base_color), ma.upload(options.light_table(), dev), centre,
                  extent, flat, two_sided)


def to_uint8(rgb):
    """floor(clamp(c, 0, 1) * 255 + 0.5) as uint8."""
    return torch.floor(rgb.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)


@torch.no_grad()
def render_frames(mesh, poses, K, height, width, options=RenderOptions(), base_color=(1.0, 1.0, 1.0), flat=False,
                  views_per_call=8, cull=None):
    """The shaded frames of a mesh along a trajectory: uint8 ``[n, height, width, 3]`` on the mesh's device, by
    ``to_uint8``.  ``mesh``: a Mesh or a (vertices, faces) pair.  Faces are culled as ``options.cull`` says (render.json
    hides back faces) unless ``cull`` names a mode; normals are ``vertex_normals`` of the mesh (a mesh object's own
    are not used: they need not be area-weighted).  ``views_per_call`` views are rendered at a time, so that the
    64-bit workspace of ``visibility`` stays at 8 bytes x views_per_call x height x width."""
    name = 'render_frames'
    w2c_h = _world_to_camera(name, poses)
    intr = _intrinsics(name, K)
    h, w = _image_size(name, height, width)
    chunk = int(views_per_call)
    if chunk < 1 or chunk * h * w >= 2 ** 31:
        raise ValueError('%s: views_per_call must be positive with fewer than 2^31 pixels a call, got %r' %
                         (name, views_per_call))
    mode = _cull_mode(name, options.cull if cull is None else cull)
    base = _colour(name, 'base_color', base_color)
    v, f, _ = ma.mesh_tensors(name, mesh)
    normals = None if flat else _vertex_normals(v, f)
    table = ma.upload(options.light_table(), v.device)
    centre, extent = _light_frame(v)
    w2c = ma.upload(w2c_h, v.device)
    out = torch.empty(w2c.shape[0], h, w, 3, dtype=torch.uint8, device=v.device)
    for a in range(0, w2c.shape[0], chunk):
        rows = w2c[a:a + chunk].contiguous()
        depth, face = _visibility(v, f, rows, intr, h, w, 0.05, 100.0, 0.5, mode)
        out[a:a + chunk] = to_uint8(_shade(face, depth, rows, intr, 0.5, v, f, normals, None, base, table, centre,
                                           extent, flat, False))
    return out


def read_o3d_camera(path):
    """open3d's ``PinholeCameraParameters`` JSON (the ``tmpN.json`` / ``c1.json`` the rendering scripts are steered
    with) -> ``(pose [4,4] float64 camera-to-world, (fx, fy, cx, cy, height, width))``.  ``extrinsic`` is the
    world-to-camera matrix and ``intrinsic_matrix`` the 3 x 3, both stored column by column."""
    with open(path) as fh:
        d = json.load(fh)
    if d.get('class_name') != 'PinholeCameraParameters':
        raise ValueError('read_o3d_camera: %s holds a %r' % (path, d.get('class_name')))
    ext = np.asarray(d['extrinsic'], np.float64)
    k = np.asarray(d['intrinsic']['intrinsic_matrix'], np.float64)
    if ext.shape != (16,) or k.shape != (9,):
        raise ValueError('read_o3d_camera: %s: extrinsic of %d and intrinsic_matrix of %d numbers' %
                         (path, ext.size, k.size))
    k = k.reshape(3, 3).T
    pose = np.linalg.inv(ext.reshape(4, 4).T)
    return pose, (float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2]), int(d['intrinsic']['height']),
                  int(d['intrinsic']['width']))


def depth_l1(a, b):
    """Per view the mean of |a - b| over all pixels: [n] float64.  a, b: [n, H, W] float32 CUDA.  The difference is
    taken in fp32 (as numpy does on two float32 images), the sum in fp64 in a fixed order."""
    name = 'depth_l1'
    ma.check_tensor(name, 'a', a, shape='[n, H, W]')
    ma.check_tensor(name, 'b', b, shape='[n, H, W]')
    if a.shape != b.shape:
        raise ValueError('%s: a %s, b %s' % (name, tuple(a.shape), tuple(b.shape)))
    dev = ma.same_device(name, a=a, b=b)
    if a.numel() == 0 or a.numel() >= 2 ** 31:
        raise ValueError('%s: images of shape %s' % (name, tuple(a.shape)))
    out = torch.empty(a.shape[0], dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ma.call('msdf_rnd_depth_l1', a.contiguous(), b.contiguous(), *a.shape, out)
    return out


def views_see(points, poses, K, height, width):
    """For each of ``n`` views whether any point of the cloud projects into its frame: bool [n] on the cloud's device.
    ``check_proj`` of eval_recon.py:68-94 in the OpenCV frame, fp32: with (x, y, z) the point in the camera frame and
    q = z - 1e-5: q >= 0 and 0 < (fx x + cx z) / q < width and 0 < (fy y + cy z) / q < height."""
    name = 'views_see'
    pts = ma.cloud_tensor(name, 'points', points).contiguous()
    w2c = _world_to_camera(name, poses)
    intr = _intrinsics(name, K)
    h, w = _image_size(name, height, width)
    flags = torch.empty(w2c.shape[0], dtype=torch.int32, device=pts.device)
    with torch.cuda.device(pts.device):
        ma.call('msdf_rnd_views_see', pts, pts.shape[0], ma.upload(w2c, pts.device), w2c.shape[0], *intr, h, w, flags)
    return flags.bool()


def interior_view_box(gt):
    """``get_cam_position`` (eval_recon.py:196-204): the box inside a room that views are sampled from ->
    ``(extents [3], transform [4,4])``: the oriented bounding box of ``gt`` (``mesh_bounds.oriented_bounds``) with its
    extents times (0.3, 0.7, 0.7), and the inverse of its ``to_origin`` with 0.4 added to entry [2, 3]."""
    from .mesh_bounds import oriented_bounds
    to_origin, extents = oriented_bounds(gt)
    extents = np.asarray(extents, np.float64) * np.array([0.3, 0.7, 0.7])
    transform = np.linalg.inv(np.asarray(to_origin, np.float64))
    transform[2, 3] += 0.4
    return extents, transform


def viewmatrix(z, up, pos):
    """eval_recon.py:16-22 as a 4 x 4: columns unit(up x z), unit(z x that), unit(z), pos."""
    def unit(x):
        return x / np.linalg.norm(x)
    vec2 = unit(np.asarray(z, np.float64))
    vec0 = unit(np.cross(np.asarray(up, np.float64), vec2))
    vec1 = unit(np.cross(vec2, vec0))
    m = np.eye(4)
    m[:3, :] = np.stack([vec0, vec1, vec2, np.asarray(pos, np.float64)], 1)
    return m


def sample_views(extents, transform, n, unseen=None, seed=0, batch=256, K=(300.0, 300.0, 249.5, 249.5), height=500,
                 width=500):
    """``n`` random views from inside a room, as the loop of ``calc_2d_metric`` draws them -> poses [n, 4, 4] float64.

    Candidate k takes six numbers, in sequence, from one ``numpy.random.default_rng(seed)``: u in [0, 1)^3 gives the
    origin transform ((u - 0.5) extents) (``trimesh.sample.volume_rectangular``), then per axis a target
    round(uniform(-1e4, 1e4), 2); its frame is ``viewmatrix(target - origin, (0, 0, -1), origin)``.  With ``unseen``
    (a cloud [N, 3]) a candidate is rejected when ``views_see`` finds a point of it in the frame of ``K``, ``height``,
    ``width``.  Candidates are tested ``batch`` at a time; the accepted ones keep candidate order and the first ``n``
    are returned, so the result does not depend on ``batch``.  (The reference draws from Python's and numpy's global
    generators: its views cannot be reproduced, only their distribution.)"""
    name = 'sample_views'
    n, batch = int(n), int(batch)
    if n < 0 or batch < 1:
        raise ValueError('%s: n >= 0 and batch >= 1 needed, got %r, %r' % (name, n, batch))
    extents = np.asarray(extents, np.float64).reshape(3)
    transform = np.asarray(transform, np.float64).reshape(4, 4)
    rng = np.random.default_rng(seed)
    cloud = None if unseen is None else ma.cloud_tensor(name, 'unseen', unseen)
    kept, drawn = [], 0
    while len(kept) < n:
        if drawn > 1000 * n + 10000:
            raise RuntimeError('%s: %d candidates gave %d of %d views: the unseen points are in every frame' %
                               (name, drawn, len(kept), n))
        r = rng.random((batch, 6))
        drawn += batch
        origins = ((r[:, :3] - 0.5) * extents) @ transform[:3, :3].T + transform[:3, 3]
        targets = np.round(-1e4 + 2e4 * r[:, 3:], 2)
        poses = np.stack([viewmatrix(t - o, (0.0, 0.0, -1.0), o) for o, t in zip(origins, targets)])
        if cloud is not None and cloud.shape[0] > 0:
            poses = poses[~views_see(cloud, poses, K, height, width).cpu().numpy()]
        kept.extend(poses)
    return np.stack(kept[:n]) if n else np.zeros((0, 4, 4))


def _near_plane(v):
    """0.01 of the largest extent of the bounding box of the mesh being rendered."""
    _, lo, hi = ma.finite_bounds('evaluate_depth_l1', v)
    return 0.01 * float((hi - lo).max().item())


@torch.no_grad()
def evaluate_depth_l1(rec, gt, n_imgs=1000, unseen=None, align=False, seed=0, size=500, focal=300.0, zfar=20.0,
                      znear=None, views_per_call=64, view_box=None):
    """``calc_2d_metric`` (eval_recon.py:196-285): the depth L1 of ``rec`` against ``gt`` in centimetres: both meshes
    are rendered (every face, as ``mesh_show_back_face = True`` there) from ``n_imgs`` views of ``sample_views`` inside
    ``interior_view_box(gt)``, ``size`` x ``size`` pixels, fx = fy = ``focal``, cx = cy = size / 2 - 0.5, depth 0 where
    nothing is hit within [znear, zfar]; the result is 100 x the mean over the views of ``depth_l1``.

    ``znear`` None: 0.01 x the largest bounding-box extent of the mesh being rendered, for each of the two (open3d's rule
    for an eye inside the box as far as it was recalled: UNVERIFIED).  ``unseen``: the cloud the ground truth never
    observed (``*_pc_unseen.npy``); views that see a point of it are redrawn.  ``align``: ``rec`` first goes through
    ``mesh_align.align_mesh``.  ``view_box``: ``(extents, transform)`` to sample the views from, in place of
    ``interior_view_box(gt)``.  ``rec``, ``gt``: Mesh objects or (vertices, faces) pairs."""
    name = 'evaluate_depth_l1'
    size = int(size)
    h, w = _image_size(name, size, size)
    K = (float(focal), float(focal), size / 2.0 - 0.5, size / 2.0 - 0.5)
    intr = _intrinsics(name, K)
    gv, gf, _ = ma.mesh_tensors(name, gt, ma.device_of(*ma.mesh_parts(rec)))
    if align:
        from .mesh_align import align_mesh
        rv, rf = align_mesh(rec, (gv, gf))[0]
    else:
        rv, rf, _ = ma.mesh_tensors(name, rec, gv.device)
    if gv.shape[0] == 0 or rv.shape[0] == 0:
        raise ValueError('%s: a mesh without vertices' % name)
    extents, transform = interior_view_box((gv, gf)) if view_box is None else view_box
    poses = sample_views(extents, transform, n_imgs, unseen=unseen, seed=seed, K=K, height=h, width=w)
    if len(poses) == 0:
        raise ValueError('%s: n_imgs must be positive' % name)
    near_g = _near_plane(gv) if znear is None else float(znear)
    near_r = _near_plane(rv) if znear is None else float(znear)
    _planes(name, near_g, zfar, 0.5), _planes(name, near_r, zfar, 0.5)
    w2c = ma.upload(_world_to_camera(name, poses), gv.device)
    errors = []
    for a in range(0, len(poses), int(views_per_call)):
        rows = w2c[a:a + int(views_per_call)].contiguous()
        dg = _raster(gv, gf, rows, intr, h, w, near_g, float(zfar), 0.5)
        dr = _raster(rv, rf, rows, intr, h, w, near_r, float(zfar), 0.5)
        errors.append(depth_l1(dg, dr))
    return float(torch.cat(errors).mean().item() * 100.0)
