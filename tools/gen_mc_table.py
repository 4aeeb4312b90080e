"""Generates the marching-cubes triangle table of ibgs_amd/csrc/tsdf.hip (`TSDF_MC_TRI`) and prints it as C.

The table is this project's own; it is derived here from two rules instead of being copied from a published one:

  corners   c = dx | dy << 1 | dz << 2 (x fastest); case bit c is set when corner c is negative (tsdf < 0)
  edges     e = 4 a + (ob | oc << 1): the edge along axis a whose owner corner has offset ob / oc on the other two axes (b < c) and 0 on a;
            it joins the owner to owner + e_a

  1. On every cube face the crossing edges are joined by segments that SEPARATE the negative corners: a face with two crossings gets one
     segment, a face whose negative corners sit on a diagonal gets two, each cutting one negative corner off.  The choice depends on the
     face's four signs alone, so two cells that share a face draw the same segments on it (no cracks).
  2. Each segment is directed so that the negative corners lie on its left seen from outside the cube.  Every crossing edge then has one
     incoming and one outgoing segment, and the segments form closed directed loops.  Each loop is fanned from the vertex whose worst
     triangle is best oriented (edge midpoints as vertices), the fan reversed so that every triangle's normal (v1 - v0) x (v2 - v0) points
     towards the non-negative corners (free space).

Rows are 16 entries: up to five triangles of three edge indices, -1 after the last.  Run `python tools/gen_mc_table.py` to print the rows."""
import itertools

import numpy as np

CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)


def edge_corners(e):
    """(owner corner, other corner) of edge e."""
    a, k = divmod(e, 4)
    b, c = [x for x in range(3) if x != a]
    off = [0, 0, 0]
    off[b] = k & 1
    off[c] = k >> 1
    c0 = off[0] | off[1] << 1 | off[2] << 2
    return c0, c0 | (1 << a)


def edge_mid(e):
    c0, c1 = edge_corners(e)
    return 0.5 * (CORNERS[c0] + CORNERS[c1])


def face_edges(axis, side):
    """The four cube edges lying on face (axis, side)."""
    out = []
    for e in range(12):
        c0, c1 = edge_corners(e)
        if CORNERS[c0][axis] == side and CORNERS[c1][axis] == side:
            out.append(e)
    return out


def face_segments(case, axis, side):
    """Directed segments (e_from, e_to) of one face, negative corners on the left seen from outside."""
    neg = lambda c: (case >> c) & 1
    crossing = [e for e in face_edges(axis, side) if neg(edge_corners(e)[0]) != neg(edge_corners(e)[1])]
    if not crossing:
        return []
    fc = [c for c in range(8) if CORNERS[c][axis] == side]
    normal = np.zeros(3); normal[axis] = 2 * side - 1
    if len(crossing) == 2:
        groups = [(crossing, [c for c in fc if neg(c)])]
    else:
        # diagonal pattern: one segment around each negative corner, joining the two crossing edges that touch it
        groups = []
        for c in fc:
            if neg(c):
                groups.append(([e for e in crossing if c in edge_corners(e)], [c]))
    segs = []
    for (ea, eb), negs in groups:
        pa, pb = edge_mid(ea), edge_mid(eb)
        side_of = np.dot(np.cross(pb - pa, CORNERS[negs[0]] - pa), normal)
        segs.append((ea, eb) if side_of > 0 else (eb, ea))
    return segs


def case_triangles(case):
    nxt = {}
    for axis, side in itertools.product(range(3), range(2)):
        for a, b in face_segments(case, axis, side):
            assert a not in nxt
            nxt[a] = b
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop = [start]
        seen.add(start)
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        tris += best_fan(case, loop)
    return tris


def orientation_score(case, tri):
    """sum over the triangle's three edges of n . (non-negative corner - negative corner), n its normal at edge midpoints"""
    p = [edge_mid(e) for e in tri]
    n = np.cross(p[1] - p[0], p[2] - p[0])
    s = 0.0
    for e in tri:
        c0, c1 = edge_corners(e)
        s += np.dot(n, CORNERS[c0] - CORNERS[c1]) * (1 if (case >> c1) & 1 else -1)
    return s


def best_fan(case, loop):
    """The reversed fan (normals towards the non-negative corners) of the loop from the start vertex whose worst triangle is best oriented
    (ties: the first such start)."""
    best = None
    for r in range(len(loop)):
        lp = loop[r:] + loop[:r]
        fan = [(lp[0], lp[i + 1], lp[i]) for i in range(1, len(lp) - 1)]
        score = min(orientation_score(case, t) for t in fan)
        if best is None or score > best[0] + 1e-12:
            best = (score, fan)
    return best[1]


def table():
    rows = []
    for case in range(256):
        tris = case_triangles(case)
        assert len(tris) <= 5, (case, tris)
        row = [e for t in tris for e in t]
        rows.append(row + [-1] * (16 - len(row)))
    return rows


if __name__ == "__main__":
    rows = table()
    print("__constant__ int8_t TSDF_MC_TRI[256][16] = {")
    for case, row in enumerate(rows):
        print("    {%s},%s" % (", ".join("%2d" % x for x in row), "  // %3d" % case))
    print("};")
