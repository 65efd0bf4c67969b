"""The SDF node's evaluation order (dense-set columns first) and the column -> slot table of the sampler's saving
forward kernel, restated in numpy (tests/reuse_numpy.py).  No GPU."""
import numpy as np
import pytest
import torch

import reuse_numpy as rn

N_FINAL, N_EXTRA, N_EVAL = 64, 32, 128
S = N_FINAL + N_EXTRA + 2


def _candidates(N, seed, ties=False):
    """What the finish kernel sorts per ray: 64 importance samples, near, far, 32 columns of the 128 first-round
    samples (the same columns for every ray)."""
    rng = np.random.default_rng(seed)
    dense = np.sort(rng.uniform(0.05, 3.0, size=(N, N_EVAL)), axis=1).astype(np.float32)
    final = rng.uniform(0.05, 3.0, size=(N, N_FINAL)).astype(np.float32)
    extra = rng.permutation(N_EVAL)[:N_EXTRA]
    if ties:
        final[:, :4] = dense[:, extra[:4]]        # importance samples that coincide with dense-set columns
        dense[:, extra[5]] = 0.0                  # ... and a column at `near`
    near, far = np.zeros((N, 1), np.float32), np.full((N, 1), 3.85, np.float32)
    return np.concatenate([final, near, far, dense[:, extra]], axis=1), extra


@pytest.mark.parametrize('N,n_eik,ties', [(1, 0, False), (2, 8, False), (3, 12, True), (5, 20, False), (16, 64, True)])
def test_row_map_is_the_stated_permutation(N, n_eik, ties):
    v, _ = _candidates(N, seed=N, ties=ties)
    pos = rn.merged_positions(v)
    rm = rn.row_map(pos, N_EXTRA, n_eik)
    P = N * S + n_eik
    assert rm.shape == (P,) and sorted(rm.tolist()) == list(range(P))         # a permutation
    assert (rm[N * S:] == np.arange(N * S, P)).all()                         # the eikonal block maps to itself
    z_sorted = np.sort(v, axis=1, kind='stable').reshape(-1)
    for ray in range(N):
        ext = rm[ray * N_EXTRA:(ray + 1) * N_EXTRA]
        assert (ext // S == ray).all()
        # an extra row holds the z of its column, in extra_idx order
        assert (z_sorted[ext] == v[ray, N_FINAL + 2:]).all()
        oth = rm[N * N_EXTRA + ray * (S - N_EXTRA):N * N_EXTRA + (ray + 1) * (S - N_EXTRA)]
        assert (oth // S == ray).all() and (np.diff(oth) > 0).all()          # the ray's other rows, sorted
        assert (np.diff(z_sorted[oth]) >= 0).all()
        assert sorted(ext.tolist() + oth.tolist()) == list(range(ray * S, (ray + 1) * S))


def test_merged_positions_break_ties_by_index():
    v = np.array([[2.0, 1.0, 2.0, 1.0, 0.5]], np.float32)
    assert rn.merged_positions(v).tolist() == [[3, 1, 4, 2, 0]]


def test_col_slot_inverts_the_first_row_of_extra_idx():
    from monosdf_amd.model.ray_sampler import ErrorBoundSampler
    for seed in range(4):
        row0 = np.random.default_rng(seed).permutation(N_EVAL)[:N_EXTRA]
        slots = ErrorBoundSampler.column_slots(torch.from_numpy(row0), N_EVAL)
        assert slots.dtype == torch.int32 and slots.tolist() == rn.column_slots(row0, N_EVAL).tolist()
        assert slots[torch.from_numpy(row0)].tolist() == list(range(N_EXTRA))
        assert int((slots >= 0).sum()) == N_EXTRA and int(slots.min()) == -1
    # not a set of distinct first-round columns: no table, nothing is saved
    assert ErrorBoundSampler.column_slots(torch.tensor([3, 5, 3]), N_EVAL) is None
    assert ErrorBoundSampler.column_slots(torch.tensor([3, N_EVAL]), N_EVAL) is None
    assert ErrorBoundSampler.column_slots(torch.tensor([-1, 2]), N_EVAL) is None


def test_reusable_rows_are_whole_workgroups():
    """n_reuse = the 64-row workgroups that lie entirely inside the 32 N extra rows."""
    for N, want in [(1, 0), (2, 64), (3, 64), (5, 128), (16, 512), (1024, 32768)]:
        assert (N * N_EXTRA) // 64 * 64 == want
