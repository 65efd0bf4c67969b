"""Times of the high-resolution cue merge on one MI355X at the reference's geometry.

    python scripts/bench_highres.py [--images 8] [--repeats 5] [--no-host] [--out profiles/highres_bench.json]

Grid 7 x 14, patches of 384 at stride 128 (a 1152 x 2048 mosaic), --images images per call, inputs drawn on the device
(a smooth field with a per-patch scale and shift for depth; rotated copies of one normal field, stored as
v = (n + 1) / 2 in fp32): the times do not depend on the values.  After one warm-up call each:
  * msdf_hrc_merge_depth and msdf_hrc_merge_normals alone by HIP events (median of --repeats), buffers allocated once;
    the launches of a call are counted from the geometry;
  * against the bound the kernels are held to: every patch pixel read once for its sums and once for its
    blend, every mosaic pixel written once -> bytes, the time they take at the HBM peak, and the achieved share of it;
    beside it the bytes the kernels move as written (overlap reads of the mosaic, the row strips written and read
    again), counted from the shapes;
  * ``merge_depth`` and ``merge_normals`` end to end by a host clock around a synchronise (allocation, the fp32 decode
    of the normals and their conversion to fp64 included);
  * unless --no-host: the float64 restatement (tests/highres_numpy.py) of ONE image on the host, once, for scale, and
    the distance of the device's first image from it.
No time or ratio here is a pass condition.  Writes one JSON document.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0                   # MI355X specification
ROWS, COLS, PATCH, STRIDE = 7, 14, 384, 128


def _events(fn, repeats):
    samples = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b))
    return float(np.median(samples)), [round(s, 4) for s in samples]


def _wall(fn, repeats):
    samples = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(samples)), [round(s, 3) for s in samples]


def make_inputs(n, seed=0):
    """Depth patches [n, R, C, P, P] fp32 and mid [n, P, P]; encoded normal patches [n, R, C, 3, P, P] fp32 and mid."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    H, W = PATCH + STRIDE * (ROWS - 1), PATCH + STRIDE * (COLS - 1)
    y = torch.linspace(0, 1, H, device='cuda')[:, None]
    x = torch.linspace(0, 1, W, device='cuda')[None, :]
    field = 2.0 + 0.6 * torch.sin(7.0 * x + 1.0) * torch.cos(5.0 * y) + 0.4 * torch.sin(9.0 * (x + y)) + 0.5 * x
    nx = 1.1 * torch.sin(6.0 * x + 0.3) + 0.5 * torch.cos(7.0 * y)
    ny = 0.35 * torch.sin(8.0 * y + 1.0) + 0.2 * torch.cos(5.0 * x) + 0.15
    normal = torch.stack([nx.expand(H, W), ny.expand(H, W), torch.ones(H, W, device='cuda')])
    normal = normal / normal.norm(dim=0, keepdim=True)
    depth = torch.empty(n, ROWS, COLS, PATCH, PATCH, device='cuda')
    enc = torch.empty(n, ROWS, COLS, 3, PATCH, PATCH, device='cuda')
    for r in range(ROWS):
        for c in range(COLS):
            ys, xs = slice(r * STRIDE, r * STRIDE + PATCH), slice(c * STRIDE, c * STRIDE + PATCH)
            a = torch.rand(n, 1, 1, device='cuda', generator=g) * 1.5 + 0.5
            b = torch.rand(n, 1, 1, device='cuda', generator=g) * 2.0 - 1.0
            depth[:, r, c] = a * field[ys, xs] + b + 0.05 * torch.randn(n, PATCH, PATCH, device='cuda', generator=g)
            q, _ = torch.linalg.qr(torch.eye(3, device='cuda') + 0.2 * torch.randn(n, 3, 3, device='cuda', generator=g))
            q = q * torch.sign(torch.linalg.det(q))[:, None, None]
            v = torch.einsum('nab,bhw->nahw', q, normal[:, ys, xs])
            v = v + 0.01 * torch.randn(v.shape, device='cuda', generator=g)
            enc[:, r, c] = (v / v.norm(dim=1, keepdim=True) + 1.0) / 2.0
    y0, x0 = H // 2 - PATCH // 2, W // 2 - PATCH // 2
    mid_d = (1.3 * field[y0:y0 + PATCH, x0:x0 + PATCH] - 0.2).expand(n, PATCH, PATCH).contiguous()
    mid_n = ((normal[:, y0:y0 + PATCH, x0:x0 + PATCH] + 1.0) / 2.0).expand(n, 3, PATCH, PATCH).contiguous()
    return depth, mid_d, enc, mid_n


def traffic(n, channels, elem):
    """Bytes of one call: the bound of DESIGN 4.15 and what the kernels move as written, from the shapes."""
    R, C, P, S = ROWS, COLS, PATCH, STRIDE
    O, H, W = P - S, P + S * (R - 1), P + S * (C - 1)
    px = channels * elem
    bound = (2 * n * R * C * P * P + n * H * W) * px
    rows = n * R * (P * P * 2 + (C - 1) * (2 * O * P + P * P + O * P + P * P))      # copy; reduce, apply read + write
    cols = n * (R - 1) * (2 * O * W + P * W + O * W + P * W)
    mid = n * 2 * P * P
    if channels == 1:
        end = n * H * W * (2 + 2)                                                    # centre fit + min/max, normalise
    else:
        end = n * H * W * 2 + n * R * 2 * S * P                                      # rotate + encode; first heads
    return int(bound), int((rows + cols + mid + end) * px)


def launches(channels):
    R, C = ROWS, COLS
    steps = 3 * (C - 1) + 3 * (R - 1) + 1 + 2                                        # copy launch, centre reduce + solve
    return steps + (3 if channels == 1 else 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'highres_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_highres.py needs a GPU')
    from monosdf_amd.utils import highres_cues as hr, mesh_args as ma
    n = args.images
    H, W = hr.mosaic_size(ROWS, COLS, PATCH, STRIDE)
    depth, mid_d, enc, mid_n = make_inputs(n)
    n_steps = hr.step_count(ROWS, COLS, True)
    doc = {'what': 'merge of %d images per call, grid %d x %d, patch %d, stride %d -> %d x %d; entry points by HIP '
                   'events, wrappers by a host clock around a synchronise; medians of %d after a warm-up call'
                   % (n, ROWS, COLS, PATCH, STRIDE, H, W, args.repeats),
           'device': torch.cuda.get_device_name(0), 'images': n, 'steps_per_image': n_steps,
           'hbm_peak_tbs': HBM_PEAK_TBS, 'hbm_peak_source': 'specification; not measured'}

    def entry(name, channels, patches, mid, out_shape, dtype, elem):
        ws = ma.workspace('bench', 'msdf_hrc_workspace_bytes', n, ROWS, COLS, PATCH, STRIDE, channels, device='cuda')
        out = torch.empty(out_shape, dtype=dtype, device='cuda')
        steps = torch.empty(n, n_steps, 2 if channels == 1 else 9, dtype=torch.float64, device='cuda')
        tail = (1,) if channels == 1 else ()

        def run():
            ma.call(name, patches, mid, n, ROWS, COLS, PATCH, STRIDE, *tail, ws, out, steps)

        run()
        ms, every = _events(run, args.repeats)
        bound, moved = traffic(n, channels, elem)
        at_peak_ms = bound / (HBM_PEAK_TBS * 1e12) * 1e3
        return {'ms': round(ms, 4), 'ms_all': every, 'ms_per_image': round(ms / n, 4), 'launches': launches(channels),
                'bound_bytes': bound, 'bound_ms_at_hbm_peak': round(at_peak_ms, 4),
                'share_of_hbm_peak': round(at_peak_ms / ms, 4), 'bytes_as_written': moved,
                'tbs_as_written': round(moved / (ms * 1e-3) / 1e12, 3), 'workspace_bytes': int(ws.numel())}, out

    doc['depth_entry'], d_out = entry('msdf_hrc_merge_depth', 1, depth, mid_d, (n, H, W), torch.float32, 4)
    decoded = hr.decode_normals(enc).double()
    decoded_mid = hr.decode_normals(mid_n).double()
    doc['normals_entry'], n_out = entry('msdf_hrc_merge_normals', 3, decoded, decoded_mid, (n, 3, H, W), torch.float64, 8)
    first_depth, first_normals = d_out[0].cpu().numpy(), n_out[0].cpu().numpy()
    del decoded, decoded_mid, d_out, n_out
    torch.cuda.empty_cache()

    hr.merge_depth(depth, STRIDE, mid_d)
    ms, every = _wall(lambda: hr.merge_depth(depth, STRIDE, mid_d), args.repeats)
    doc['merge_depth_ms'], doc['merge_depth_ms_all'] = round(ms, 3), every
    hr.merge_normals(enc, STRIDE, mid_n)
    ms, every = _wall(lambda: hr.merge_normals(enc, STRIDE, mid_n), args.repeats)
    doc['merge_normals_ms'], doc['merge_normals_ms_all'] = round(ms, 3), every

    if args.no_host:
        doc['host_restatement'] = None
    else:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import highres_cases as hc
        import highres_numpy as hn
        p, m = depth[0].cpu().numpy(), mid_d[0].cpu().numpy()
        t0 = time.perf_counter()
        res_d = hn.merge_depth(p, STRIDE, m)
        t1 = time.perf_counter()
        pn, mn = hc.decode(enc[0].cpu().numpy()), hc.decode(mid_n[0].cpu().numpy())
        t2 = time.perf_counter()
        res_n = hn.merge_normals(pn, STRIDE, mn)
        t3 = time.perf_counter()
        doc['host_restatement'] = {
            'what': 'tests/highres_numpy.py, float64, one image, one run',
            'depth_ms': round((t1 - t0) * 1e3, 1), 'normals_ms': round((t3 - t2) * 1e3, 1),
            'depth_gap_to_device': hn.relative_gap(first_depth, res_d['out'], res_d['out']),
            'normals_gap_to_device': float(np.abs(first_normals - res_n['out']).max()),
            'normals_gap_note': 'the device decodes in fp32 itself; a last-place difference of its division or square '
                                'root from numpy enters here'}
    text = json.dumps(doc, indent=1)
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
