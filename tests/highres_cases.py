"""The inputs of the high-resolution cue tests (test_highres_cpu.py, test_gpu_highres.py), regenerated from seeds.

A depth patch is a * g + b + noise of one smooth scene field g sampled where the patch lies in the mosaic, with a per
patch a in [0.5, 2] and b in [-1, 1]; a normal patch is a per-patch proper rotation of one broad scene normal field,
plus noise, renormalised and stored as the files store it: v = (n + 1) / 2 in fp32.  The scene fields are anisotropic
on purpose: the normals spread more along x than along y, so that the two smaller singular values of an overlap's
correlation matrix stay apart (the conditioning that test_highres_cpu.py asserts).

``scripts/make_golden_highres.py`` records, per case, a SHA-256 of these arrays and what the reference's own functions
make of them (tests/golden/highres/<case>.npz).
"""
import hashlib

import numpy as np

# name -> geometry and construction.  `images`: the seeds of the images of the batch; `zero`, `negative`, `improper`:
# (row, column) of the patch that is all zeros / has a negative scale / is rotated by an improper matrix.
CASES = {
    'c1': dict(P=12, S=4, R=3, C=4, mid=True, images=(101,)),                # overlap 96: less than one pass of 256
    'c2': dict(P=30, S=10, R=2, C=5, mid=False, images=(102,)),              # overlap 600: off the 64-lane grid
    'c3': dict(P=96, S=32, R=3, C=3, mid=False, images=(103,)),              # several trips of every strided loop
    'c4': dict(P=20, S=8, R=2, C=3, mid=False, images=(104,)),               # P != 3 S
    'c5_row': dict(P=12, S=4, R=1, C=4, mid=False, images=(105,)),           # no column phase
    'c5_col': dict(P=12, S=4, R=3, C=1, mid=False, images=(106,)),           # no row phase
    'c5_one': dict(P=12, S=4, R=1, C=1, mid=False, images=(107,)),           # no step at all
    'c6': dict(P=12, S=4, R=3, C=4, mid=True, images=(108, 101, 109)),       # image 1 is case c1
    'c7': dict(P=12, S=4, R=2, C=4, mid=False, images=(110,), zero=(1, 1), cues=('depth',)),
    'c8': dict(P=12, S=4, R=2, C=4, mid=False, images=(111,), negative=(0, 2), cues=('depth',)),
    'c9': dict(P=12, S=4, R=2, C=4, mid=False, images=(112,), improper=(1, 2), cues=('normal',)),
    'c10_depth': dict(P=384, S=128, R=7, C=14, mid=True, images=(113,), cues=('depth',)),
    'c10_normal': dict(P=384, S=128, R=2, C=3, mid=True, images=(114,), cues=('normal',)),
}
DEPTH_NOISE = 0.05         # large enough that fitting the mosaic to the patch (regression dilution) shows
RECORDED_OUTPUTS = ('c1', 'c2', 'c4')        # the cases whose reference outputs are stored, not only their gaps


def cues(name):
    return CASES[name].get('cues', ('depth', 'normal'))


def mosaic_size(case):
    return case['P'] + case['S'] * (case['R'] - 1), case['P'] + case['S'] * (case['C'] - 1)


def step_count(case):
    return case['R'] * (case['C'] - 1) + case['R'] - 1 + (1 if case['mid'] else 0)


def row_step(case, r, c):
    """The index of the step that merges patch (r, c), c >= 1, into its row."""
    return r * (case['C'] - 1) + c - 1


def _scene_depth(rng, H, W):
    y, x = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing='ij')
    f = rng.uniform(0.5, 2.0, 4)
    ph = rng.uniform(0.0, 2 * np.pi, 4)
    return (2.0 + 0.6 * np.sin(2 * np.pi * f[0] * x + ph[0]) * np.cos(2 * np.pi * f[1] * y + ph[1])
            + 0.4 * np.sin(2 * np.pi * f[2] * (x + y) + ph[2]) + 0.5 * x - 0.3 * y * np.cos(2 * np.pi * f[3] * x + ph[3]))


def _scene_normals(rng, H, W):
    y, x = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing='ij')
    f = rng.uniform(0.7, 1.6, 4)
    ph = rng.uniform(0.0, 2 * np.pi, 4)
    gx = 1.1 * np.sin(2 * np.pi * f[0] * x + ph[0]) + 0.5 * np.cos(2 * np.pi * f[1] * y + ph[1])
    gy = 0.35 * np.sin(2 * np.pi * f[2] * y + ph[2]) + 0.2 * np.cos(2 * np.pi * f[3] * x + ph[3]) + 0.15
    n = np.stack([gx, gy, np.ones_like(gx)])
    return n / np.linalg.norm(n, axis=0)[None]


def _rotation(rng, max_angle=0.6):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(-max_angle, max_angle)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def _depth_image(case, seed):
    P, S, R, C = case['P'], case['S'], case['R'], case['C']
    H, W = mosaic_size(case)
    rng = np.random.default_rng(seed)
    g = _scene_depth(rng, H, W)
    patches = np.empty((R, C, P, P), dtype=np.float32)
    for r in range(R):
        for c in range(C):
            a, b = rng.uniform(0.5, 2.0), rng.uniform(-1.0, 1.0)
            if case.get('negative') == (r, c):
                a = -a
            q = a * g[r * S:r * S + P, c * S:c * S + P] + b + rng.normal(0.0, DEPTH_NOISE, (P, P))
            if case.get('zero') == (r, c):
                q = np.zeros((P, P))
            patches[r, c] = q
    a, b = rng.uniform(0.5, 2.0), rng.uniform(-1.0, 1.0)
    y0, x0 = H // 2 - P // 2, W // 2 - P // 2
    mid = (a * g[y0:y0 + P, x0:x0 + P] + b + rng.normal(0.0, DEPTH_NOISE, (P, P))).astype(np.float32)
    return patches, mid


def _normal_image(case, seed):
    P, S, R, C = case['P'], case['S'], case['R'], case['C']
    H, W = mosaic_size(case)
    rng = np.random.default_rng(seed + 5000)
    field = _scene_normals(rng, H, W)

    def encode(n, rot):
        n = np.einsum('ab,bhw->ahw', rot, n) + rng.normal(0.0, 0.01, n.shape)
        n = n / np.linalg.norm(n, axis=0)[None]
        return ((n + 1.0) / 2.0).astype(np.float32)

    patches = np.empty((R, C, 3, P, P), dtype=np.float32)
    for r in range(R):
        for c in range(C):
            rot = _rotation(rng)
            if case.get('improper') == (r, c):
                rot = rot @ np.diag([1.0, -1.0, 1.0])
            patches[r, c] = encode(field[:, r * S:r * S + P, c * S:c * S + P], rot)
    y0, x0 = H // 2 - P // 2, W // 2 - P // 2
    mid = encode(field[:, y0:y0 + P, x0:x0 + P], _rotation(rng))
    return patches, mid


def _stack(case, make):
    images = [make(case, seed) for seed in case['images']]
    return np.stack([i[0] for i in images]), (np.stack([i[1] for i in images]) if case['mid'] else None)


def depth_inputs(name):
    """(patches float32 [N, R, C, P, P], mid float32 [N, P, P] or None)."""
    return _stack(CASES[name], _depth_image)


def normal_inputs(name):
    """(patches float32 [N, R, C, 3, P, P], mid float32 [N, 3, P, P] or None), encoded as the files are."""
    return _stack(CASES[name], _normal_image)


def decode(v):
    """numpy's decode of the reference (lines 348-349), in the array's own dtype."""
    n = v * 2. - 1.
    axis = n.ndim - 3
    return n / np.expand_dims(np.linalg.norm(n, axis=axis) + 1e-15, axis)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(str((a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
    return h.hexdigest()
