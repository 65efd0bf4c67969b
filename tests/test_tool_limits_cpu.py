"""The largest count every size query of the mesh tools accepts, pinned at 2^31 - 2, 2^31 - 1 and 2^31.  The tools share
one limit, MSDF_COUNT_MAX = 2^31 - 1 (csrc/tool_common.h), under two predicates: a count stored in int32 is accepted
through the limit itself, a count that must stay below it only through 2^31 - 2.  Which entry uses which is part of its
behaviour, so it is written down here, entry by entry and argument by argument.  Nothing here launches: a `*_bytes`
entry point returns a size or -1 on the host."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX = 2 ** 31 - 1
SLICE = 2048                                          # points of one workgroup of obb_support_k and icp_accumulate_k


def slices(n):
    return (n + SLICE - 1) // SLICE


# (entry, the arguments with the count n in place, the last accepted count, the size in bytes where n is accepted)
CASES = {
    'nn n_ref': ('msdf_nn_workspace_bytes', lambda n: (n, 1, 1), MAX, lambda n: 256),           # 1 split x 1 query x 8
    'nn n_query': ('msdf_nn_workspace_bytes', lambda n: (1, n, 1), MAX, lambda n: 8 * n),
    'gnn n_ref': ('msdf_gnn_workspace_bytes', lambda n: (n,), MAX, lambda n: 16 * n),
    'dtu_thin n': ('msdf_dtu_thin_workspace_bytes', lambda n: (n,), MAX, lambda n: 89 * n),
    'rnd n_views': ('msdf_rnd_visibility_workspace_bytes', lambda n: (n, 1, 1), MAX, lambda n: 8 * n),
    'rnd height': ('msdf_rnd_visibility_workspace_bytes', lambda n: (1, n, 1), MAX, lambda n: 8 * n),
    'rnd width': ('msdf_rnd_visibility_workspace_bytes', lambda n: (1, 1, n), MAX, lambda n: 8 * n),
    'obb n_points': ('msdf_obb_support_workspace_bytes', lambda n: (n, 1), MAX - 1, lambda n: slices(n) * 12),
    'obb n_planes': ('msdf_obb_support_workspace_bytes', lambda n: (1, n), MAX - 1, lambda n: 12 * n),
    'icp n': ('msdf_icp_workspace_bytes', lambda n: (n,), MAX - 1, lambda n: slices(n) * 17 * 8),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_size_query_at_the_int32_limit(case):
    from monosdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    entry, arguments, last, size = CASES[case]
    query = getattr(_lib.load(), entry)
    for n in (MAX - 1, MAX, MAX + 1):
        assert query(*arguments(n)) == (size(n) if n <= last else -1), (entry, arguments(n))
    assert query(*arguments(-1)) == -1
