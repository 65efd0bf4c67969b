"""Times of the mesh component split on one MI355X, on marching-cubes meshes of an analytic scene with floaters.

    python scripts/bench_mesh_clean.py [--resolutions 128 256 512] [--repeats 5] [--out profiles/mesh_clean_bench.json]

Scene: a blob (a sphere with a sinusoidal bump field) in [-1, 1]^3 plus a lattice of small noise floaters around it,
meshed by the project's marching_cubes at each resolution.  Timed per resolution, with HIP events around each stage
after one warm-up pass over every stage (median of --repeats): the edge keys, the stable sort, the link launch (with
the init launch before it), the flatten launch, the component sizes (areas, sort by label, segment sums) and the
compaction of the kept component;
and ``largest_component`` end to end with a host clock around a device synchronise (it ends in host copies).  Where
scipy imports, scipy.sparse.csgraph.connected_components on the same face graph is timed on the CPU (host clock,
graph construction not included) and its labels are compared with the GPU's.  No time or ratio here is a pass
condition.  Writes one JSON document.
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


def scene_volume(n, device):
    """min(blob, floaters) on the n^3 grid over [-1, 1]^3, float32, and the grid spacing."""
    g = torch.linspace(-1.0, 1.0, n, device=device, dtype=torch.float64)
    x, y, z = torch.meshgrid(g, g, g, indexing='ij')
    blob = torch.sqrt(x * x + y * y + z * z) - 0.55 - 0.05 * torch.sin(9 * x) * torch.sin(7 * y) * torch.sin(8 * z)
    # floaters: one small sphere per cell of a 12^3 lattice, its radius drawn per cell, present in about a third
    cells = 12
    gen = torch.Generator(device='cpu').manual_seed(0)
    radius = torch.rand(cells, cells, cells, generator=gen, dtype=torch.float64) * 0.05 - 0.03     # <= 0.02
    radius = radius.to(device)
    pitch = 2.0 / cells

    def local(c):
        return (c + 1.0) / pitch

    ix, iy, iz = (local(c).floor().clamp(0, cells - 1).long() for c in (x, y, z))
    fx, fy, fz = ((local(c) - i - 0.5) * pitch for c, i in ((x, ix), (y, iy), (z, iz)))
    floaters = torch.sqrt(fx * fx + fy * fy + fz * fz) - radius[ix, iy, iz]
    return torch.minimum(blob, floaters).float().contiguous(), float(g[1] - g[0])


def _events(fn, repeats):
    """Median device time of fn() in milliseconds (HIP events on the current stream), and every sample."""
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
    return float(np.median(samples)), [round(s, 4) for s in samples]


def bench_resolution(n, repeats):
    from monosdf_amd.utils import mesh_args as ma, mesh_clean
    from monosdf_amd.utils.mesh import marching_cubes
    dev = torch.device('cuda')
    vol, h = scene_volume(n, dev)
    v, f, _ = marching_cubes(vol, 0.0, (h, h, h))
    del vol
    F = f.shape[0]
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    parent = torch.empty(F, dtype=torch.int32, device=dev)
    state = {}

    def stage_keys():
        ma.call('msdf_mcc_edge_keys', f, F, keys)

    def stage_sort():
        state['sorted'], state['order'] = torch.sort(keys, stable=True)

    def stage_link():
        ma.call('msdf_mcc_init', parent, F)
        ma.call('msdf_mcc_link_edges', state['sorted'], state['order'], 3 * F, 0, parent)

    def stage_flatten():
        ma.call('msdf_mcc_flatten', parent, F)

    def stage_sizes():
        state['sizes'] = mesh_clean._component_sizes('bench', v, f, state['labels'], state['n'])

    def stage_compact():
        keep_faces = state['labels'] == state['best']
        kept = f[keep_faces]
        keep = torch.zeros(v.shape[0], dtype=torch.bool, device=dev)
        keep[kept.long().reshape(-1)] = True
        state['out'] = (v[keep], ma.compact_faces(keep, kept, all_kept=True))

    def prepare():                                       # one pass over every stage: warm-up, and the stages' inputs
        stage_keys()
        stage_sort()
        stage_link()
        stage_flatten()
        state['labels'], state['n'] = mesh_clean._first_index_labels(parent.long())
        stage_sizes()
        state['best'] = int(state['sizes'][1].argmax())
        stage_compact()

    prepare()
    out = {'resolution': n, 'vertices': int(v.shape[0]), 'faces': int(F), 'components': state['n'],
           'largest_component_faces': int(state['sizes'][0][state['best']]), 'stages_ms': {}, 'stages_ms_all': {}}
    for name, fn in (('keys', stage_keys), ('sort', stage_sort), ('link', stage_link), ('flatten', stage_flatten),
                     ('sizes', stage_sizes), ('compaction', stage_compact)):
        if name == 'flatten':
            # flatten of an already flat forest is not the work: link again before each timed flatten
            samples = []
            for _ in range(repeats):
                stage_link()
                samples.append(_events(stage_flatten, 1)[0])
            med, every = float(np.median(samples)), [round(s, 4) for s in samples]
        else:
            med, every = _events(fn, repeats)
        out['stages_ms'][name], out['stages_ms_all'][name] = round(med, 4), every
    mesh_clean.largest_component((v, f), 'edge', 'area')
    med, every = _wall(lambda: mesh_clean.largest_component((v, f), 'edge', 'area'), repeats)
    out['largest_component_ms'], out['largest_component_ms_all'] = round(med, 3), every
    # estimated traffic of the four graph stages but the sort: bytes that must cross HBM per face
    out['graph_bytes_per_face_estimate'] = 12 + 24 + 48 + 4 + 8
    try:
        from scipy import sparse
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        out['scipy_connected_components_ms'] = None
        return out
    sk, order = state['sorted'].cpu().numpy(), state['order'].cpu().numpy()
    same = sk[1:] == sk[:-1]
    two = same.copy()
    two[1:] &= ~same[:-1]
    two[:-1] &= ~same[1:]
    rows, cols = order[:-1][two] // 3, order[1:][two] // 3
    adjacency = sparse.coo_matrix((np.ones(len(rows), bool), (rows, cols)), shape=(F, F)).tocsr()
    samples = []
    for _ in range(max(1, min(repeats, 3))):
        t0 = time.perf_counter()
        n_cpu, labels_cpu = connected_components(adjacency, directed=False)
        samples.append((time.perf_counter() - t0) * 1e3)
    out['scipy_connected_components_ms'] = round(float(np.median(samples)), 3)
    out['scipy_labels_equal'] = bool(n_cpu == state['n'] and np.array_equal(labels_cpu, state['labels'].cpu().numpy()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolutions', type=int, nargs='+', default=[128, 256, 512])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_clean_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_clean.py needs a GPU')
    doc = {'what': 'component split of marching-cubes meshes of a blob with floaters; stage times by HIP events, '
                   'largest_component by a host clock around a synchronise; medians of %d after a warm-up pass'
                   % args.repeats,
           'device': torch.cuda.get_device_name(0), 'connectivity': 'edge',
           'runs': [bench_resolution(n, args.repeats) for n in args.resolutions]}
    text = json.dumps(doc, indent=1)
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
