"""Generates monosdf_amd/csrc/mc_tables.h, the 256-case marching-cubes table, from a rule (no copied table).

    python scripts/gen_mc_tables.py            # rewrite the header
    python scripts/gen_mc_tables.py --check    # exit 1 if the committed header differs from what the rule gives

Conventions (shared with csrc/mcubes.hip and tests/mc_numpy.py):
* corner c = dx | dy << 1 | dz << 2 of a cell; the cube code has bit c set when corner c is BELOW the level (v < level).
* edge e = 4 * axis + m runs along `axis` from corner EDGE_C0[e] (axis bit 0) to EDGE_C0[e] | 1 << axis; m counts the
  other two corner bits in ascending order.  The edge belongs to the grid node at EDGE_C0[e]'s offset (its owner).
* every face of the cube puts segments between its crossing edges.  A face with 4 crossing edges (diagonal corners of
  one class) keeps its below corners separated: each below corner is cut off by the segment joining its two face edges.
  The rule depends on that face's 4 corner classes alone, so two cells sharing a face put the same segments on it.
* a segment on face f (outward normal n_f) is directed d so that n_f x d points into the face's above part; the
  directed segments then chain into closed loops whose right-hand normal points from below toward above.
* each loop is fan-triangulated from one of its vertices: the first (in loop order from its smallest edge) from which
  no fan diagonal joins two edges of one cube face, so that a diagonal is never also used by the neighbouring cell.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'monosdf_amd', 'csrc', 'mc_tables.h')


def _edges():
    c0 = []
    for axis in range(3):
        others = [b for b in range(3) if b != axis]
        for m in range(4):
            c0.append(((m & 1) << others[0]) | ((m >> 1) << others[1]))
    return c0


EDGE_AXIS = [e // 4 for e in range(12)]
EDGE_C0 = _edges()


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def edge_mid(e):
    p = corner_pos(EDGE_C0[e])
    p[EDGE_AXIS[e]] = 0.5
    return p


def edge_corners(e):
    return EDGE_C0[e], EDGE_C0[e] | (1 << EDGE_AXIS[e])


def face_corners(axis, side):
    """The 4 corners of face (axis, side) in cyclic order."""
    b, d = [x for x in range(3) if x != axis]
    base = side << axis
    return [base, base | 1 << b, base | 1 << b | 1 << d, base | 1 << d]


def _edge_between(c0, c1):
    for e in range(12):
        if set(edge_corners(e)) == {c0, c1}:
            return e
    raise AssertionError((c0, c1))


FACES = [(axis, side) for axis in range(3) for side in range(2)]


def face_segments(axis, side, below):
    """Directed segments (edge_from, edge_to) the rule puts on face (axis, side); below[c]: class of corner c."""
    cyc = face_corners(axis, side)
    fedges = [_edge_between(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]
    crossing = [fedges[i] for i in range(4) if below[cyc[i]] != below[cyc[(i + 1) % 4]]]
    pairs = []
    if len(crossing) == 2:
        pairs.append((crossing[0], crossing[1]))
    elif len(crossing) == 4:
        for i in range(4):               # cut off each below corner: its two face edges
            if below[cyc[i]]:
                pairs.append((fedges[(i - 1) % 4], fedges[i]))
    n_f = np.zeros(3)
    n_f[axis] = 1.0 if side else -1.0
    segs = []
    for a, b in pairs:
        pa, pb = edge_mid(a), edge_mid(b)
        w = np.cross(n_f, pb - pa)
        shared = set(edge_corners(a)) & set(edge_corners(b))
        # a corner that lies alone on one side of the segment (adjacent edges), else any corner (parallel edges:
        # both sides are pure)
        c = shared.pop() if shared else cyc[0]
        s = float(np.dot(w, corner_pos(c) - 0.5 * (pa + pb)))
        assert s != 0.0
        toward_c_is_above = not below[c]
        segs.append((a, b) if (s > 0) == toward_c_is_above else (b, a))
    return segs


def _face_of_edge_pair(a, b):
    """True when edges a and b lie on a common cube face."""
    for axis, side in FACES:
        on = [e for e in (a, b) if all(((c >> axis) & 1) == side for c in edge_corners(e))]
        if len(on) == 2:
            return True
    return False


def case_loops(code):
    below = [(code >> c) & 1 == 1 for c in range(8)]
    nxt = {}
    for axis, side in FACES:
        for a, b in face_segments(axis, side, below):
            assert a not in nxt, (code, a)
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (code, loop)
        loops.append(loop)
    return loops


def fan(loop):
    n = len(loop)
    for r in range(n):
        rot = loop[r:] + loop[:r]
        if all(not _face_of_edge_pair(rot[0], rot[i]) for i in range(2, n - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, n - 1)]
    raise AssertionError('no fan apex without a face diagonal: %r' % loop)


def build_tables():
    """-> list of 256 triangle lists [(e0, e1, e2), ...]."""
    return [[t for loop in case_loops(code) for t in fan(loop)] for code in range(256)]


def render_header(tables):
    max_t = max(len(t) for t in tables)
    out = ['// GENERATED by scripts/gen_mc_tables.py -- do not edit; rerun the script instead.',
           '// Marching-cubes case table: corner c = dx | dy << 1 | dz << 2, code bit c = (v[c] < level);',
           '// edge e = 4 * axis + m from corner MC_EDGE_C0[e] along axis; triangles point from below toward above.',
           '#pragma once',
           '#include <stdint.h>',
           '',
           '#ifndef MC_TABLE',
           '#define MC_TABLE static const      // mcubes.hip puts the tables in device constant memory',
           '#endif',
           '',
           '#define MC_MAX_TRIS %d' % max_t,
           '',
           'MC_TABLE int8_t MC_EDGE_C0[12] = {%s};' % ', '.join(str(c) for c in EDGE_C0),
           '',
           'MC_TABLE uint8_t MC_TRI_COUNT[256] = {']
    for r in range(0, 256, 32):
        out.append('  ' + ', '.join(str(len(tables[c])) for c in range(r, r + 32)) + ',')
    out.append('};')
    out.append('')
    out.append('// triangle t of case c: edges MC_TRIS[c][3 t .. 3 t + 2]; unused entries -1')
    out.append('MC_TABLE int8_t MC_TRIS[256][3 * MC_MAX_TRIS] = {')
    for c in range(256):
        flat = [e for t in tables[c] for e in t]
        flat += [-1] * (3 * max_t - len(flat))
        out.append('  {%s},' % ', '.join(str(e) for e in flat))
    out.append('};')
    return '\n'.join(out) + '\n'


def main(argv):
    text = render_header(build_tables())
    if '--check' in argv:
        ok = os.path.exists(HEADER) and open(HEADER).read() == text
        print('mc_tables.h %s' % ('matches the rule' if ok else 'DIFFERS from the rule'))
        return 0 if ok else 1
    with open(HEADER, 'w') as f:
        f.write(text)
    print('wrote %s' % os.path.relpath(HEADER, ROOT))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
