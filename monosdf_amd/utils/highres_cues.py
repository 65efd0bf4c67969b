"""High-resolution monocular cues on the GPU: the patch merge of ``preprocess/generate_high_res_map.py --mode
merge_patches``.

The monocular networks take 384 x 384 input, so a high-resolution training image gets a grid of overlapping depth and
normal predictions (stride 128: a 7 x 14 grid for 1152 x 2048).  The merge stitches them in chains: every row left to
right, then the row strips top to bottom, then a fit to a separately predicted centre patch.

* ``merge_depth``: each patch is fitted to the running mosaic by a least-squares scale and shift over the overlap and
  cross-faded in; the mosaic is fitted to the centre patch and normalised to [0, 1] (reference lines 44-64, 93-130,
  297-338).
* ``merge_normals``: each patch is fitted by the best rotation over the overlap (a 3 x 3 SVD), cross-faded in and
  renormalised; the mosaic is rotated onto the centre patch (lines 67-87, 133-174, 340-383).
* ``decode_normals``: the stored ``v in [0, 1]`` -> unit normals, in fp32 as numpy does it.
* ``merge_scan``: a directory of patch files in the reference's layout -> the per-image cue files and previews.

The sums, the solves (the SVD included) and the blends run in csrc/highres.hip (ABI msdf_hrc_* of
include/monosdf_highres.h, which states the arithmetic): sums and solves in fp64 in a fixed order, every stored value
formed in fp64 and rounded once, no atomics.  A merge is a sequence of launches on the current stream with nothing
read back in between; all images of a batch advance together and no image's result depends on another's.  Inputs are
CUDA tensors, there is no CPU path (``decode_normals`` alone is plain elementwise torch and works anywhere).

Not built: ``--mode create_patches`` (cropping, and the RGB resize to 2048 x 1152 by cv2.resize, whose parity could not
be checked without cv2), the rewriting of ``cameras.npz``, and ``extract_monocular_cues.py`` (the Omnidata networks
themselves).
"""
import os

import numpy as np
import torch

from . import mesh_args as ma


def mosaic_size(rows, cols, patch, stride):
    """(H, W) of the mosaic of a ``rows`` x ``cols`` grid of ``patch``-sized patches ``stride`` apart.  ValueError
    unless 1 <= stride < patch with an overlap patch - stride of at least 2 (a cross-fade needs two lines)."""
    rows, cols, patch, stride = int(rows), int(cols), int(patch), int(stride)
    if rows < 1 or cols < 1:
        raise ValueError('mosaic_size: a grid of %d x %d patches' % (rows, cols))
    if not 1 <= stride < patch or patch - stride < 2:
        raise ValueError('mosaic_size: patch %d, stride %d: need 1 <= stride < patch and an overlap of at least 2'
                         % (patch, stride))
    return patch + stride * (rows - 1), patch + stride * (cols - 1)


def step_count(rows, cols, mid=False):
    """The steps of one image's chain: rows (cols - 1) row steps, rows - 1 column steps, the centre fit."""
    return rows * (cols - 1) + (rows - 1) + (1 if mid else 0)


def decode_normals(v):
    """The normals stored as ``v in [0, 1]`` -> unit vectors: n = 2 v - 1, then n / (|n| + 1e-15) over dim -3, with
    |n| = sqrt((x x + y y) + z z).  Elementwise in the tensor's own dtype and numpy's order of operations (for fp32
    input bitwise what ``n = v * 2. - 1.; n / (np.linalg.norm(n, axis=0) + 1e-15)`` gives).  Any device."""
    if not isinstance(v, torch.Tensor) or not v.dtype.is_floating_point:
        raise TypeError('decode_normals: a floating-point tensor, got %s' % (v.dtype if isinstance(v, torch.Tensor) else
                                                                             type(v).__name__))
    if v.dim() < 3 or v.shape[-3] != 3:
        raise ValueError('decode_normals: the shape must end in [3, h, w], got %s' % (tuple(v.shape),))
    n = v * 2.0 - 1.0
    sq = n * n
    x, y, z = sq.unbind(-3)
    # the sum rounds to the tensor's dtype before 1e-15 is added, as numpy's fp32 norm does
    length = torch.sqrt((x + y) + z) + 1e-15
    return n / length.unsqueeze(-3)


def _merge(name, patches, stride, mid, channels, dtype, normalize):
    """The checked launch.  patches [N, R, C, (3,) P, P] of ``dtype`` -> (out, steps)."""
    N, R, C, P = patches.shape[0], patches.shape[1], patches.shape[2], patches.shape[-1]
    H, W = mosaic_size(R, C, P, stride)
    dev = patches.device
    if N == 0:
        raise ValueError('%s: no images' % name)
    if mid is not None:
        if P % 2:
            raise ValueError('%s: the centre fit needs an even patch side (the reference crops H//2 - P//2 : '
                             'H//2 + P//2), got %d' % (name, P))
        if tuple(mid.shape) != (N,) + tuple(patches.shape[3:]):
            raise ValueError('%s: mid must be %s, got %s' % (name, (N,) + tuple(patches.shape[3:]), tuple(mid.shape)))
        ma.same_device(name, patches=patches, mid=mid)
        mid = mid.to(dtype).contiguous()
    patches = patches.contiguous()
    n_steps = step_count(R, C, mid is not None)
    k = 2 if channels == 1 else 9
    with torch.cuda.device(dev):
        ws = ma.workspace(name, 'msdf_hrc_workspace_bytes', N, R, C, P, int(stride), channels, device=dev)
        out = torch.empty((N, H, W) if channels == 1 else (N, 3, H, W), dtype=dtype, device=dev)
        steps = torch.empty((N, n_steps, k), dtype=torch.float64, device=dev)
        if channels == 1:
            ma.call('msdf_hrc_merge_depth', patches, mid, N, R, C, P, int(stride), 1 if normalize else 0, ws, out,
                    steps if n_steps else None)
        else:
            ma.call('msdf_hrc_merge_normals', patches, mid, N, R, C, P, int(stride), ws, out,
                    steps if n_steps else None)
    return out, steps


def _batched(name, arg, t, dtypes, shape):
    """A CUDA tensor of the dimensions of ``shape``, or of one fewer (a single image), checked by
    ``mesh_args.check_tensor`` -> (the batched tensor, whether it came batched)."""
    single = isinstance(t, torch.Tensor) and t.dim() == shape.count(',')
    if single:
        t = t.unsqueeze(0)
    ma.check_tensor(name, arg, t, dtypes, shape)
    return t, not single


def merge_depth(patches, stride, mid=None, normalize=True, return_steps=False):
    """Merge depth patches.  patches: float32 CUDA [N, R, C, P, P] (or [R, C, P, P]: one image); mid: the centre
    patches [N, P, P] (or [P, P]) or None -> the mosaic float32 [N, H, W] (or [H, W]), normalised to [0, 1] per image
    unless ``normalize`` is false.  ``return_steps``: also the (scale, shift) of every step as float64
    [N, n_steps, 2], rows first (row by row, left to right), then the column steps, then the centre fit.  An all-zero
    patch has a singular fit and contributes zeros.  Bitwise the same every call, and per image whatever the batch."""
    name = 'merge_depth'
    patches, batched = _batched(name, 'patches', patches, (torch.float32,), '[N, R, C, P, P]')
    if patches.shape[-1] != patches.shape[-2]:
        raise ValueError('%s: patches must be square, got %s' % (name, tuple(patches.shape)))
    if mid is not None:
        mid = _batched(name, 'mid', mid, (torch.float32,), '[N, P, P]')[0]
    out, steps = _merge(name, patches, stride, mid, 1, torch.float32, normalize)
    if not batched:
        out, steps = out[0], steps[0]
    return (out, steps) if return_steps else out


def merge_normals(patches, stride, mid=None, encoded=True, return_steps=False):
    """Merge normal patches.  patches: CUDA [N, R, C, 3, P, P] (or [R, C, 3, P, P]); ``encoded``: they and ``mid``
    ([N, 3, P, P]) hold v in [0, 1] as the files do (float32, decoded here by ``decode_normals``), otherwise unit
    normals (float32 or float64) -> the mosaic encoded as (n + 1) / 2, float64 [N, 3, H, W].  ``return_steps``: also the
    rotation of every step as float64 [N, n_steps, 3, 3], in the order of ``merge_depth``.  A rotation is only defined
    where the overlap's correlation matrix has rank two or more."""
    name = 'merge_normals'
    dtypes = (torch.float32,) if encoded else (torch.float32, torch.float64)
    patches, batched = _batched(name, 'patches', patches, dtypes, '[N, R, C, 3, P, P]')
    if patches.shape[-1] != patches.shape[-2] or patches.shape[-3] != 3:
        raise ValueError('%s: patches must be [.., 3, P, P], got %s' % (name, tuple(patches.shape)))
    if mid is not None:
        mid = _batched(name, 'mid', mid, dtypes, '[N, 3, P, P]')[0]
    if encoded:
        patches = decode_normals(patches)
        mid = None if mid is None else decode_normals(mid)
    out, steps = _merge(name, patches.double(), stride, mid, 3, torch.float64, False)
    steps = steps.reshape(steps.shape[0], steps.shape[1], 3, 3)
    if not batched:
        out, steps = out[0], steps[0]
    return (out, steps) if return_steps else out


# ---------------------------------------------------------------- files

def _load_grid(patch_dir, index, rows, cols, kind, patch):
    grid = []
    for j in range(rows):
        for i in range(cols):
            a = np.load(os.path.join(patch_dir, '%06d_%02d_%02d_%s.npy' % (index, j, i, kind)))
            grid.append(np.asarray(a, dtype=np.float32))
    a = np.stack(grid)
    want = (rows * cols,) + ((patch, patch) if kind == 'depth' else (3, patch, patch))
    if a.shape != want:
        raise ValueError('merge_scan: image %d: %s patches of shape %s, expected %s' % (index, kind, a.shape[1:], want[1:]))
    return a.reshape((rows, cols) + want[1:])


def scan_indices(patch_dir):
    """The image numbers that have a ``%06d_00_00_depth.npy`` in ``patch_dir``, ascending."""
    found = []
    for f in os.listdir(patch_dir):
        if f.endswith('_00_00_depth.npy') and f[:6].isdigit() and len(f) == len('000000_00_00_depth.npy'):
            found.append(int(f[:6]))
    return sorted(found)


def merge_scan(patch_dir, out_dir, rows=7, cols=14, patch=384, stride=128, batch=4, device=None, previews=True):
    """Merge every image of a directory in the reference's layout: ``%06d_%02d_%02d_depth.npy`` [P, P] and
    ``..._normal.npy`` [3, P, P] (row, column), ``%06d_mid_depth.npy`` and ``%06d_mid_normal.npy`` -> in ``out_dir``
    ``%06d_depth.npy`` (float32 [H, W]), ``%06d_normal.npy`` (float64 [3, H, W], encoded) and, with ``previews``,
    ``%06d_depth.png`` (viridis) and ``%06d_normal.png`` by matplotlib.  ``batch`` images go through each launch.
    Returns the image numbers written."""
    if not torch.cuda.is_available():
        raise RuntimeError('merge_scan: needs a GPU (there is no CPU path)')
    mosaic_size(rows, cols, patch, stride)
    if int(batch) < 1:
        raise ValueError('merge_scan: batch must be at least 1, got %s' % (batch,))
    device = torch.device('cuda' if device is None else device)
    indices = scan_indices(patch_dir)
    if not indices:
        raise ValueError('merge_scan: no %%06d_00_00_depth.npy in %s' % patch_dir)
    os.makedirs(out_dir, exist_ok=True)
    if previews:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    for a in range(0, len(indices), int(batch)):
        group = indices[a:a + int(batch)]
        depth = np.stack([_load_grid(patch_dir, i, rows, cols, 'depth', patch) for i in group])
        normal = np.stack([_load_grid(patch_dir, i, rows, cols, 'normal', patch) for i in group])
        mid_d = np.stack([np.load(os.path.join(patch_dir, '%06d_mid_depth.npy' % i)).astype(np.float32) for i in group])
        mid_n = np.stack([np.load(os.path.join(patch_dir, '%06d_mid_normal.npy' % i)).astype(np.float32) for i in group])
        d = merge_depth(ma.upload(depth, device), stride, ma.upload(mid_d, device)).cpu().numpy()
        n = merge_normals(ma.upload(normal, device), stride, ma.upload(mid_n, device)).cpu().numpy()
        for k, i in enumerate(group):
            np.save(os.path.join(out_dir, '%06d_depth.npy' % i), d[k])
            np.save(os.path.join(out_dir, '%06d_normal.npy' % i), n[k])
            if previews:
                plt.imsave(os.path.join(out_dir, '%06d_depth.png' % i), d[k], cmap='viridis')
                plt.imsave(os.path.join(out_dir, '%06d_normal.png' % i), np.clip(np.moveaxis(n[k], 0, 2), 0.0, 1.0))
    return indices
