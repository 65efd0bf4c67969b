"""Records what the reference's own merge functions make of the cases of tests/highres_cases.py.

    python scripts/make_golden_highres.py [--reference DIR] [--cases c1 c2 ..]

Runs only where the reference is present (like oracle/make_golden*.py).  ``preprocess/generate_high_res_map.py`` parses
its command line and walks a data folder when imported, so only its function definitions are taken: the FunctionDef
nodes of its syntax tree are compiled and executed at record time, with torch and numpy in their namespace.  Nothing of
its text is written anywhere.  Its ``align_x``, ``align_y``, ``align_normal_x``, ``align_normal_y``,
``compute_scale_and_shift`` and ``best_fit_transform`` are driven through the chains of its lines 297-383 with the
case's patch side and stride in place of 384 and 128.

Writes tests/golden/highres/<case>.npz (a folder of its own: tests/helpers.py takes every .npz directly under
tests/golden for a recorded forward pass of the network):
  * sha256: of the regenerated inputs (depth patches, depth mid, normal patches, normal mid of the case);
  * depth_gap_raw, depth_gap_out: max |reference - float64 restatement| / max |restatement's mosaic|, before and after
    the final normalisation; normal_gap, normal_gap_steps: max |reference - restatement| of the saved normals and of
    the rotations (absolute);
    (the normals are decoded in fp32 and handed to the reference's functions as float64, see normal_chain);
  * for the cases of highres_cases.RECORDED_OUTPUTS also the reference's outputs themselves: depth_raw, depth_out,
    depth_steps [n_steps, 2], normal_out (as saved: (n + 1) / 2), normal_steps [n_steps, 3, 3].
A case with several images records image by image, stacked.
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import highres_cases as hc      # noqa: E402
import highres_numpy as hn      # noqa: E402
from oracle import ref_loader   # noqa: E402


def reference_functions(reference):
    path = os.path.join(reference, 'preprocess', 'generate_high_res_map.py')
    tree = ast.parse(open(path).read(), path)
    module = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef)], type_ignores=[])
    space = {'torch': torch, 'np': np}
    exec(compile(module, path, 'exec'), space)
    return space


def depth_chain(fn, patches, mid, S):
    """Lines 297-335 with P, S for 384, 128 -> (raw, out, steps)."""
    R, C, P = patches.shape[:3]
    O = P - S
    steps, rows = [], []

    def fit(p, t):
        scale, shift = fn['compute_scale_and_shift'](p, t, torch.ones_like(t))
        steps.append((float(scale[0]), float(shift[0])))

    for j in range(R):
        depths = [torch.from_numpy(patches[j, i])[None] for i in range(C)]
        left, s1 = depths[0], S
        for right in depths[1:]:
            fit(right[:, :, 0:O], left[:, :, s1:left.shape[2]])
            left = fn['align_x'](left, right, s1, left.shape[2], 0, O)
            s1 += S
        rows.append(left)
    top, s1 = rows[0], S
    for bottom in rows[1:]:
        fit(bottom[:, 0:O, :], top[:, s1:top.shape[1], :])
        top = fn['align_y'](top, bottom, s1, top.shape[1], 0, O)
        s1 += S
    if mid is not None:
        H, W = top.shape[1:]
        mid_depth = torch.from_numpy(mid)[None]
        crop = top[:, H // 2 - P // 2:H // 2 + P // 2, W // 2 - P // 2:W // 2 + P // 2]
        fit(crop, mid_depth)
        scale, shift = fn['compute_scale_and_shift'](crop, mid_depth, torch.ones_like(mid_depth))
        top = scale * top + shift
    out = (top - top.min()) / (top.max() - top.min())
    return top[0].numpy(), out[0].numpy(), np.array(steps, dtype=np.float64).reshape(-1, 2)


def normal_chain(fn, patches, mid, S):
    """Lines 340-383 -> (what is saved: (n + 1) / 2, steps).  patches, mid: as stored, v in [0, 1]; decoded in fp32 as
    the reference does, then handed over as float64, which is what the device kernels receive.  (Left in fp32, the
    first step of every row would multiply two fp32 arrays and run its SVD in fp32, an accident of dtype promotion
    that moves the result by 1e-7 and that this project does not restate.)"""
    R, C, _, P = patches.shape[:4]
    O = P - S
    steps, rows = [], []

    def decode(v):
        n = v * 2. - 1.
        return (n / (np.linalg.norm(n, axis=0) + 1e-15)[None]).astype(np.float64)

    def fit(a, b):
        steps.append(fn['best_fit_transform'](a.reshape(3, -1).T, b.reshape(3, -1).T))

    for j in range(R):
        normals = [decode(patches[j, i]) for i in range(C)]
        left, s1 = normals[0], S
        for right in normals[1:]:
            fit(right[:, :, 0:O], left[:, :, s1:left.shape[2]])
            left = fn['align_normal_x'](left, right, s1, left.shape[2], 0, O)
            s1 += S
        rows.append(left)
    top, s1 = rows[0], S
    for bottom in rows[1:]:
        fit(bottom[:, 0:O, :], top[:, s1:top.shape[1], :])
        top = fn['align_normal_y'](top, bottom, s1, top.shape[1], 0, O)
        s1 += S
    if mid is not None:
        H, W = top.shape[1:]
        mid_normal = decode(mid)
        crop = top[:, H // 2 - P // 2:H // 2 + P // 2, W // 2 - P // 2:W // 2 + P // 2]
        rot = fn['best_fit_transform'](crop.reshape(3, -1).T, mid_normal.reshape(3, -1).T)
        steps.append(rot)
        top = (rot @ top.reshape(3, -1)).reshape(top.shape)
    return (top + 1.) / 2., np.array(steps, dtype=np.float64).reshape(-1, 3, 3)


def record(fn, name):
    case = hc.CASES[name]
    S = case['S']
    doc, hashed = {}, []
    if 'depth' in hc.cues(name):
        patches, mid = hc.depth_inputs(name)
        hashed += [patches, mid]
        raw, out, steps, gap_raw, gap_out = [], [], [], 0.0, 0.0
        for n in range(len(patches)):
            m = None if mid is None else mid[n]
            ref = depth_chain(fn, patches[n], m, S)
            res = hn.merge_depth(patches[n], S, m)
            gap_raw = max(gap_raw, hn.relative_gap(ref[0], res['raw'], res['raw']))
            gap_out = max(gap_out, hn.relative_gap(ref[1], res['out'], res['out']))
            raw.append(ref[0]), out.append(ref[1]), steps.append(ref[2])
        doc.update(depth_gap_raw=gap_raw, depth_gap_out=gap_out)
        if name in hc.RECORDED_OUTPUTS:
            doc.update(depth_raw=np.stack(raw), depth_out=np.stack(out), depth_steps=np.stack(steps))
    if 'normal' in hc.cues(name):
        patches, mid = hc.normal_inputs(name)
        hashed += [patches, mid]
        out, steps, gap, gap_steps = [], [], 0.0, 0.0
        for n in range(len(patches)):
            m = None if mid is None else mid[n]
            ref = normal_chain(fn, patches[n], m, S)
            res = hn.merge_normals(hc.decode(patches[n]), S, None if m is None else hc.decode(m))
            gap = max(gap, float(np.abs(ref[0] - res['out']).max()))
            if len(ref[1]):
                gap_steps = max(gap_steps, float(np.abs(ref[1] - res['steps']).max()))
            out.append(ref[0]), steps.append(ref[1])
        doc.update(normal_gap=gap, normal_gap_steps=gap_steps)
        if name in hc.RECORDED_OUTPUTS:
            doc.update(normal_out=np.stack(out), normal_steps=np.stack(steps))
    doc['sha256'] = hc.sha256(*hashed)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.path.dirname(ref_loader.REF_ROOT))
    ap.add_argument('--cases', nargs='*', default=sorted(hc.CASES))
    args = ap.parse_args()
    if not os.path.isdir(args.reference):
        raise SystemExit('make_golden_highres.py: the reference is not present at %s' % args.reference)
    fn = reference_functions(args.reference)
    for name in args.cases:
        doc = record(fn, name)
        os.makedirs(os.path.join(ROOT, 'tests', 'golden', 'highres'), exist_ok=True)
        path = os.path.join(ROOT, 'tests', 'golden', 'highres', '%s.npz' % name)
        np.savez_compressed(path, **doc)
        print(name, {k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in doc.items()},
              '%d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
