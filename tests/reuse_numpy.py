"""Numpy restatement of the SDF node's evaluation order (msdf_sampler_finish's row_map, ops.SdfReuse): what
tests/test_sdf_reuse_cpu.py checks on the CPU and tests/test_gpu_sdf_reuse.py compares the kernel's map with."""
import numpy as np


def merged_positions(v):
    """v [N, S]: a ray's final candidates in the finish kernel's order.  Returns the position of every candidate in the
    ray's sorted set: the number of candidates that are smaller, ties broken by index (a stable sort)."""
    order = np.argsort(v, axis=1, kind='stable')
    pos = np.empty_like(order)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(v.shape[1]), v.shape), axis=1)
    return pos


def row_map(pos, n_extra, n_eik):
    """pos [N, S]: merged position of candidate j of every ray; the last n_extra candidates are the dense-set columns
    (in extra_idx order).  Returns row_map [N S + n_eik]: the output row (ray * S + position) of every evaluation row.
    Evaluation rows: [0, n_extra N) row ray * n_extra + e; then ray by ray the other S - n_extra samples in sorted
    order; then the n_eik eikonal rows, unchanged."""
    N, S = pos.shape
    n_other = S - n_extra
    out = np.full(N * S + n_eik, -1, dtype=np.int64)
    for ray in range(N):
        for e in range(n_extra):
            out[ray * n_extra + e] = ray * S + pos[ray, n_other + e]
        others = np.sort(pos[ray, :n_other])
        out[N * n_extra + ray * n_other:N * n_extra + (ray + 1) * n_other] = ray * S + others
    out[N * S:] = np.arange(N * S, N * S + n_eik)
    return out


def column_slots(row0, n_eval):
    """Inverse of extra_idx[0]: entry c = position of column c in row0, -1 if it is not in it."""
    slots = np.full(n_eval, -1, dtype=np.int64)
    slots[np.asarray(row0)] = np.arange(len(row0))
    return slots
