"""Every header of the C ABI against its table in monosdf_amd/_lib.py, the Makefile and the built library, by one rule
(tests/abi_cases.py).  What is specific to a feature -- workspace sizes, the refusals of its entry points -- stays in
that feature's own CPU tests."""
import ctypes
import os
import re

import pytest

import abi_cases as abi
from monosdf_amd import _lib

HEADERS = _lib.headers()
CSRC = os.path.join(abi.ROOT, 'monosdf_amd', 'csrc')
MAKEFILE = open(os.path.join(CSRC, 'Makefile')).read()


def prerequisites(obj):
    """What the Makefile's dependency lines (`targets: prerequisites`, no variable assignment) give the object."""
    lines = [re.match(r'^([\w.% ]+): (?!EXTRA)(.*)$', l) for l in MAKEFILE.splitlines()]
    return {word for m in lines if m and obj in m.group(1).split() for word in m.group(2).split()}


def test_every_header_with_entry_points_has_a_table():
    declaring = sorted(h for h in os.listdir(abi.INCLUDE) if h.endswith('.h') and abi.prototypes(h))
    assert sorted(HEADERS) == declaring
    assert HEADERS[0] == abi.VERSIONED and set(HEADERS[1:]) == set(abi.ADDITIVE)
    assert _lib.exported_symbols() == sorted(_lib.signatures(abi.VERSIONED))
    assert '#define MSDF_ABI_VERSION 8' in abi.header_text(abi.VERSIONED) and _lib.ABI_VERSION == 8


def test_an_entry_under_two_headers_is_refused_at_import():
    """The binding's own source with one ICP entry named under the grid header as well."""
    source = open(_lib.__file__).read()
    twice = source.replace("}, 'monosdf_meshcc.h': {", "    'msdf_icp_solve': [],\n}, 'monosdf_meshcc.h': {", 1)
    assert twice != source
    with pytest.raises(ImportError, match='two headers.*msdf_icp_solve'):
        exec(compile(twice, _lib.__file__, 'exec'), {'__name__': 'abi_twice', '__file__': _lib.__file__})


@pytest.mark.parametrize('header', HEADERS)
def test_header_and_table_agree(header):
    """The names, the number of arguments, the ctypes type of each and the rule by which load() chooses the return
    type."""
    assert ctypes.c_int is ctypes.c_int32
    protos, table = abi.prototypes(header), _lib.signatures(header)
    assert sorted(p[1] for p in protos) == sorted(table) and len(protos) == len(table)
    if header == abi.VERSIONED:
        assert len(protos) == abi.VERSIONED_COUNT
    else:
        assert sorted(table) == sorted(abi.ADDITIVE[header]['entries'])
    tables = set()
    for ret, name, params in protos:
        accepted = abi.accepted_argtypes(name, params)
        assert len(table[name]) == len(accepted), (name, len(table[name]), len(accepted))
        for i, (have, want) in enumerate(zip(table[name], accepted)):
            assert have in want, (name, i, have, want)
            assert header == abi.VERSIONED or len(want) == 1, (name, i, want)    # additive headers pass no struct
            if have is ctypes.c_void_p and len(want) == 2:
                tables.add(name)
        assert (ret == 'int64_t') == name.endswith('_bytes'), name
    assert tables == (abi.DEVICE_TABLES if header == abi.VERSIONED else set())


@pytest.mark.parametrize('header', HEADERS)
def test_loaded_library_is_bound_as_the_header_says(header):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run python __graft_entry__.py)')
    lib, table = _lib.load(), _lib.signatures(header)
    protos = abi.prototypes(header)
    assert len(protos) == len(table)
    for ret, name, _ in protos:
        assert getattr(lib, name).restype is (ctypes.c_int64 if ret == 'int64_t' else ctypes.c_int), name
        assert getattr(lib, name).argtypes == table[name], name
    assert lib.msdf_abi_version() == _lib.ABI_VERSION == 8


@pytest.mark.parametrize('header', sorted(abi.ADDITIVE))
def test_additive_header_keeps_to_itself(header):
    """An additive header's names carry its prefix and end in a stream unless they size a workspace; no other table
    holds them and no other header's text names them, but for the headers the case lists; it leaves the ABI version to
    the versioned header; its source is built, depends on the header, and is compiled without contraction where its
    arithmetic is pinned operation by operation; a further header its source shares with other sources is a
    prerequisite of every object whose source includes it."""
    case = abi.ADDITIVE[header]
    prefix, source = case['prefix'], case['source']
    for ret, name, params in abi.prototypes(header):
        assert name.startswith(prefix), name
        assert (abi.parameters(params)[-1][-1] == 'stream') != name.endswith('_bytes'), name
    for other in HEADERS:
        if other != header:
            assert not [n for n in _lib.signatures(other) if n.startswith(prefix)], other
            declared = [p[1] for p in abi.prototypes(other)]
            assert not [n for n in declared if n.startswith(prefix)], other
            assert prefix not in abi.header_text(other) or other in case.get('named_in', ()), other
    assert 'MSDF_ABI_VERSION' not in abi.header_text(header).replace('MSDF_ABI_VERSION are unchanged', '')
    srcs = [l for l in MAKEFILE.splitlines() if l.startswith('SRCS =')]
    assert len(srcs) == 1 and source + '.hip' in srcs[0].split()
    assert re.search(r'^%s\.o: .*include/%s' % (source, re.escape(header)), MAKEFILE, flags=re.M)
    contraction_off = re.search(r'^%s\.o: EXTRA \+= .*-ffp-contract=off' % source, MAKEFILE, flags=re.M)
    assert bool(contraction_off) == case['no_contraction']
    for shared in case.get('depends', ()):
        users = [s[:-4] for s in srcs[0].split()
                 if s.endswith('.hip') and '#include "%s"' % shared in open(os.path.join(CSRC, s)).read()]
        assert source in users and len(users) > 1, (shared, users)
        for user in users:
            assert shared in prerequisites(user + '.o'), (shared, user)


def test_icp_header_leaves_the_grid_header_alone():
    assert 'msdf_icp_' not in abi.header_text('monosdf_gridnn.h')
