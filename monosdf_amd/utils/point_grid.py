"""The uniform grid of the bounded nearest-neighbour search (csrc/gridnn.hip, ABI msdf_gnn_* of
include/monosdf_gridnn.h) as an object: a reference cloud is put into its cells once and searched as often as wanted.

``mesh_eval.nearest_neighbors_within`` builds one per call; ``mesh_align`` builds the target's once per alignment and
queries it every iteration.  Arguments are the callers' business: they check with utils/mesh_args.py and make the
clouds' device the current one.
"""
import numpy as np
import torch

from . import mesh_args as ma

GRID_CELL_FRACTION = 16              # default cell side: max_dist over this (the best of the sweep of DESIGN 4.12)
GRID_MAX_CELLS = 2 ** 25             # default cap of the cell count: a start table of 128 MiB (unmeasured)
_GRID_CELLS_LIMIT = 2 ** 31 - 2      # the start table is indexed in int32


def grid_dims(lo, hi, h, max_cells):
    """The grid of ``nearest_neighbors_within`` over the box lo..hi (three Python floats each): the cell side, ``h``
    enlarged by steps of a quarter until the cell count fits ``max_cells``, and the cells per axis,
    floor((hi - lo) / h) + 1 in fp64, the expression that gives a point its cell.  -> (h, (nx, ny, nz))"""
    while True:
        n = [np.floor((b - a) / h) + 1.0 for a, b in zip(lo, hi)]
        if n[0] * n[1] * n[2] <= max_cells:
            return h, tuple(int(c) for c in n)
        h *= 1.25


class PointGrid:
    """A reference cloud in the cells of a uniform grid over its bounding box.

    ``reference``: float32 [R,3], checked, contiguous, R >= 1, on the current device; ``lo_h``, ``hi_h``: its bounds
    (fp64 host tensors [3], ``mesh_args.finite_bounds``); ``cell``: the cell side asked for; ``max_cells``: the cap of
    the cell count, to which the cell side is enlarged (``grid_dims``).  The points are binned (msdf_gnn_cells),
    sorted by cell with a stable ``torch.sort`` and gathered into records in that order (msdf_gnn_records); a dense
    table holds every cell's first record.

    ``grid``: (lo_x, lo_y, lo_z, h, nx, ny, nz), the arguments that msdf_gnn_cells and msdf_gnn_query share;
    ``n_ref``, ``records``, ``starts``: the other arguments of msdf_gnn_query."""

    def __init__(self, reference, lo_h, hi_h, cell, max_cells=GRID_MAX_CELLS):
        lo = lo_h.tolist()
        h, dims = grid_dims(lo, hi_h.tolist(), cell, max(1, int(min(max_cells, _GRID_CELLS_LIMIT))))
        self.grid = (*lo, h, *dims)
        self.n_ref = R = reference.shape[0]
        dev = reference.device
        cells = torch.empty(R, dtype=torch.int32, device=dev)
        ma.call('msdf_gnn_cells', reference, R, *self.grid, cells)
        sorted_cells, order = torch.sort(cells, stable=True)
        self.records = ma.workspace('nearest_neighbors_within', 'msdf_gnn_workspace_bytes', R, device=dev)
        ma.call('msdf_gnn_records', reference, order, R, self.records)
        every_cell = torch.arange(dims[0] * dims[1] * dims[2] + 1, dtype=torch.int32, device=dev)
        self.starts = torch.searchsorted(sorted_cells, every_cell, out_int32=True)

    def query(self, points, max_dist, int32=False):
        """For every point (float32 [Q,3], checked, contiguous, Q >= 1, on the grid's device) its nearest reference
        point if that is within ``max_dist`` (a float that ``mesh_args.search_distance`` has passed):
        -> (dist [Q] float32, idx [Q] int64), (+inf, -1) where there is none.  ``int32``: the indices as msdf_gnn_query
        wrote them, which the ICP kernels read."""
        Q, dev = points.shape[0], points.device
        cells = torch.empty(Q, dtype=torch.int32, device=dev)
        ma.call('msdf_gnn_cells', points, Q, *self.grid, cells)
        order = torch.sort(cells, stable=True)[1]
        dist = torch.empty(Q, dtype=torch.float32, device=dev)
        idx = torch.empty(Q, dtype=torch.int32, device=dev)
        ma.call('msdf_gnn_query', points, order, Q, self.records, self.n_ref, self.starts, *self.grid, max_dist, dist,
                idx)
        return dist, idx if int32 else idx.long()
