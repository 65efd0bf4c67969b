"""Numpy restatement of the grid-bounded nearest-neighbour search (csrc/gridnn.hip, mesh_eval.nearest_neighbors_within)
and of the fp32 brute force it must equal bit for bit (csrc/nnsearch.hip), with the constructed inputs that the CPU and
the GPU tests share.

``d2_fp32`` repeats the kernels' rounding: the three differences in fp32, dx*dx rounded to fp32, then two fused steps
fmaf(dy, dy, .) and fmaf(dz, dz, .), each rounded once.  ``brute`` is the reference: the minimum over
(bits of d2, index).  ``grid_search`` follows the kernel: fp64 cells clamped to the grid, records in cell order, a
start table, cubes of Chebyshev radius k = 1, 2, 4, ... scanned whole, the stop rule and the reporting rule.  Its
``mistake`` argument swaps in one of five plausible errors, which the tests show the cases catch."""
import numpy as np

SLACK = 1.0 + 2.0 ** -10
NONE = np.uint64(0x7f800000ffffffff)               # d2 = +inf, index -1
MISTAKES = ('first_nonempty', 'bound_k_plus_1', 'kmax_floor', 'cell_order_ties', 'no_max_dist_test')
CELL_FRACTION = 16                                 # default cell side: max_dist over this
MAX_CELLS = 2 ** 25


def _fma32(a, b, c):
    """float32(a * b + c) rounded ONCE, for float32 arrays.  The product is exact in fp64; the fp64 sum is rounded to
    odd (the error of the sum from TwoSum; an inexact even result moves to its odd neighbour on the side of the error),
    which the final rounding to fp32 then rounds as if from the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def d2_fp32(q, r):
    """fp32 squared distances as the kernels form them; q, r: float32 [..., 3], broadcast against each other."""
    dx, dy, dz = (q[..., k] - r[..., k] for k in range(3))
    return _fma32(dz, dz, _fma32(dy, dy, dx * dx))


def _keys(d2, idx):
    return (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def _unpack(keys):
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return d2, (keys & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).astype(np.int64)


def brute(reference, query, pairs=4000000):
    """(dist float32 [Q], idx int64 [Q]): sqrt of the smallest ``d2_fp32`` over all reference points, the smallest
    index among equal d2.  Every pair is looked at; to keep that quick the fused expression is evaluated only for the
    points of a query whose separately rounded fp32 d2 is within 1e-5 relative (plus 1e-30) of the query's smallest:
    either form is within 3e-7 relative of the true value, so the fused minimum and all its ties are among them."""
    ref, qry = np.ascontiguousarray(reference, np.float32), np.ascontiguousarray(query, np.float32)
    best = np.empty(len(qry), np.uint64)
    chunk = max(1, pairs // len(ref))
    for a in range(0, len(qry), chunk):
        q = qry[a:a + chunk]
        rough = np.zeros((len(q), len(ref)), np.float32)
        for k in range(3):
            d = q[:, k, None] - ref[None, :, k]
            rough += d * d
        near = rough <= rough.min(axis=1, keepdims=True) * np.float32(1 + 1e-5) + np.float32(1e-30)
        qi, ri = np.nonzero(near)                              # rows ascending: each query's pairs are contiguous
        keys = _keys(d2_fp32(q[qi], ref[ri]), ri)
        first = np.flatnonzero(np.concatenate([[True], qi[1:] != qi[:-1]]))
        best[a:a + chunk] = np.minimum.reduceat(keys, first)
    d2, idx = _unpack(best)
    return np.sqrt(d2), idx


def within(dist, idx, max_dist):
    """What the bounded search must return, from the brute-force answer: (d, i) kept where d <= float32(max_dist),
    (+inf, -1) elsewhere."""
    keep = dist <= np.float32(max_dist)
    return np.where(keep, dist, np.float32(np.inf)), np.where(keep, idx, -1)


def grid_dims(lo, hi, h, max_cells):
    """(h, [nx, ny, nz]): the cell side enlarged by quarters until floor((hi - lo) / h) + 1 per axis fits max_cells."""
    while True:
        n = [float(np.floor((float(b) - float(a)) / h)) + 1.0 for a, b in zip(lo, hi)]
        if n[0] * n[1] * n[2] <= max_cells:
            return h, [int(c) for c in n]
        h *= 1.25


def cell_coords(points, lo, h, n):
    """int64 [N, 3]: floor((p - lo) / h) in fp64 on the fp32 coordinates, clamped to the grid while still fp64."""
    c = np.floor((points.astype(np.float64) - lo) / h)
    return np.clip(c, 0.0, np.asarray(n, np.float64) - 1.0).astype(np.int64)


def grid_search(reference, query, max_dist, cell=None, max_cells=None, mistake=None):
    """The kernel's method, all queries of one ring at a time.  -> (dist float32 [Q], idx int64 [Q])."""
    assert mistake is None or mistake in MISTAKES
    ref, qry = np.ascontiguousarray(reference, np.float32), np.ascontiguousarray(query, np.float32)
    md = float(max_dist)
    lo, hi = ref.min(axis=0).astype(np.float64), ref.max(axis=0).astype(np.float64)
    h, n = grid_dims(lo, hi, md / CELL_FRACTION if cell is None else float(cell),
                     MAX_CELLS if max_cells is None else max_cells)
    nx, ny, nz = n
    rc = cell_coords(ref, lo, h, n)
    linear = (rc[:, 0] * ny + rc[:, 1]) * nz + rc[:, 2]
    order = np.argsort(linear, kind='stable')                  # records: cell order, ascending index inside a cell
    rec = ref[order]
    starts = np.searchsorted(linear[order], np.arange(nx * ny * nz + 1))
    # what breaks a tie of d2: the point's index -- or, as the mistake, its place in the scan (cell) order
    tag = np.arange(len(ref)) if mistake == 'cell_order_ties' else order
    kmax = int(np.floor(md / h)) if mistake == 'kmax_floor' else int(np.ceil(md * SLACK / h))
    kmax = max(1, min(kmax, max(n)))
    qc = cell_coords(qry, lo, h, n)
    best = np.full(len(qry), NONE, np.uint64)
    active = np.arange(len(qry))
    k = 1
    while len(active):
        c = qc[active]
        x0, x1 = np.maximum(c[:, 0] - k, 0), np.minimum(c[:, 0] + k, nx - 1)
        y0, y1 = np.maximum(c[:, 1] - k, 0), np.minimum(c[:, 1] + k, ny - 1)
        z0, z1 = np.maximum(c[:, 2] - k, 0), np.minimum(c[:, 2] + k, nz - 1)
        for ox in range(-k, k + 1):
            for oy in range(-k, k + 1):
                x, y = c[:, 0] + ox, c[:, 1] + oy
                inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
                col = (x[inside] * ny + y[inside]) * nz
                a, b = starts[col + z0[inside]], starts[col + z1[inside] + 1]      # the column's z-run: one range
                count = b - a
                if not count.sum():
                    continue
                owner = np.repeat(np.flatnonzero(inside), count)                  # position in `active`, ascending
                r = np.repeat(a - np.cumsum(count) + count, count) + np.arange(count.sum())
                keys = _keys(d2_fp32(qry[active[owner]], rec[r]), tag[r])
                first = np.flatnonzero(np.concatenate([[True], owner[1:] != owner[:-1]]))
                got = active[owner[first]]
                best[got] = np.minimum(best[got], np.minimum.reduceat(keys, first))
        d2 = _unpack(best[active])[0].astype(np.float64)
        bound = ((k + 1) * h if mistake == 'bound_k_plus_1' else k * h / SLACK) ** 2
        done = d2 <= bound
        if mistake == 'first_nonempty':
            done = best[active] != NONE
        if k >= kmax:
            break
        active = active[~done]
        k = min(2 * k, kmax)
    d2, idx = _unpack(best)
    if mistake == 'cell_order_ties':
        idx = np.where(idx >= 0, order[np.maximum(idx, 0)], -1)
    dist = np.sqrt(d2)
    if mistake == 'no_max_dist_test':
        return np.where(idx >= 0, dist, np.float32(np.inf)), idx
    return within(dist, idx, md)


# ---------------------------------------------------------------- the constructed inputs

def _f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def lattice(rng):
    """The 7^3 integer lattice in shuffled index order."""
    g = np.arange(7, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    return pts[rng.permutation(len(pts))]


def shell(rng, count, radius):
    d = rng.normal(size=(count, 3))
    return (radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def small_cases():
    """name -> (reference, query, max_dist, cells): the inputs of a few points each, every one with every cell side
    it is meant for (None: the default)."""
    rng = np.random.default_rng(11)
    lat = lattice(rng)
    # every third point a second time, under a second index
    dup = np.concatenate([lat, lat[::3]])[rng.permutation(len(lat) + len(lat[::3]))]
    return {
        'ring order': (_f32([(0.6, 0.9, 0.9), (3.05, 1.5, 1.5), (0, 0, 0), (6, 6, 6)]), _f32([(1.95, 1.5, 1.5)]), 4.0,
                       (1.0,)),
        'last ring': (_f32([(0, 0, 0), (9.99, 0, 0)]), _f32([(5, 0, 0)]), 5.0, (0.3,)),
        '3-4-5': (_f32([(0, 0, 0), (100, 100, 100)]),
                  _f32([(3, 4, 0), (-3, -4, 0), (0, 0, 5), (103, 104, 100), (0, 0, 5.000001), (4, 4, 0), (50, 50, 50)]),
                  5.0, (None, 0.3, 1.0, 7.0)),
        'lattice ties': (lat, lat + np.float32(0.5), 2.0, (0.25, 0.7, 1.0, 2.5)),
        'lattice ties, duplicates': (dup, lat + np.float32(0.5), 2.0, (0.25, 0.7, 1.0, 2.5)),
        'outside the box': (lat, _f32([(-10, 0, 0), (8, 8, 8), (3.5, 0, 0), (0, -4.9, 0), (0, 0, 1e4)]), 5.0,
                            (None, 1.0)),
    }


THREE_FOUR_FIVE_REPORTED = [True, True, True, True, False, False, False]


def crowded_cell():
    """5000 points inside one cell of side 1 and one isolated point; queries in the cluster, near the isolated point
    and between them with no neighbour within max_dist = 2."""
    rng = np.random.default_rng(12)
    ref = np.concatenate([rng.uniform(0.05, 0.95, (5000, 3)), [[20.5, 0.5, 0.5]]]).astype(np.float32)
    qry = np.concatenate([rng.uniform(0.0, 1.0, (300, 3)), [20.5, 0.5, 0.5] + rng.uniform(-1.2, 1.2, (200, 3)),
                          [10.0, 0.5, 0.5] + rng.uniform(-2.0, 2.0, (100, 3))]).astype(np.float32)
    return ref, qry, 2.0, (1.0,)


def off_lane_sizes():
    """(R, Q) -> (reference, query): uniform clouds of sizes off the 64-lane and 256-lane grids; max_dist = 0.3."""
    rng = np.random.default_rng(13)
    return {(R, Q): (rng.uniform(0, 1, (R, 3)).astype(np.float32), rng.uniform(-0.1, 1.1, (Q, 3)).astype(np.float32))
            for R in (1, 2, 1000) for Q in (1, 63, 65, 257, 1027)}


def sphere_shells(shift=0.0):
    """Radius 30.0 (10^4 points) against radius 30.5 (2 10^4 points), the outer shell cut by the half-space x < 12 so
    that the inner points over the cut have no neighbour within max_dist = 3; both shifted by ``shift``."""
    rng = np.random.default_rng(14)
    inner, outer = shell(rng, 10000, 30.0), shell(rng, 20000, 30.5)
    outer = outer[outer[:, 0] < 12.0]
    return inner + np.float32(shift), outer + np.float32(shift), 3.0
