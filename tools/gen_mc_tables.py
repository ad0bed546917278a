"""Generates make-it-3d_amd/csrc/mi3d_mc_tables.h: the 256-case marching-cubes triangle table of Part 8 of mi3d.h.

    python tools/gen_mc_tables.py [--check]      (--check: regenerate in memory and compare with the committed header)

The table is CONSTRUCTED, not transcribed: the classic explicit table (Bourke, "Polygonising a scalar field") is on no
machine this project builds on and cannot be quoted reliably from memory, and what the mesh needs from it is a set of
properties, not a provenance (tests/test_mc_tables_cpu.py checks them through mi3d_mc_case, independently of this file):

  * cube corners and edges are numbered as in Bourke's note (CORNERS / EDGES below); bit c of the case index is set iff
    corner c is INSIDE (value >= iso);
  * on every cube face the surface leaves directed segments that depend on the four corner states of that face alone:
    one corner cut off, two adjacent corners cut off, or - on an ambiguous face (two diagonal corners inside) - the rule
    RULE[axis][which diagonal is inside] says whether the two INSIDE corners are cut off separately or the two OUTSIDE
    ones.  A neighbouring cube sees the same face, hence the same segments reversed: no cracks;
  * inside the cube the segments chain into closed loops, and every loop is filled with a disc of triangles whose
    diagonals never lie in a cube face (a diagonal in a face would be a segment the neighbour does not have);
  * triangles are wound so that the normal points from inside to outside.

The rule that comes out separates the two INSIDE corners on every ambiguous face of every axis (the first candidate of
the search below, which would fall back to mixed per-axis / per-diagonal rules if some case did not fit five triangles
or had no admissible triangulation; none does).
"""
import itertools
import os
import sys

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
EDGE_OF = {frozenset(e): i for i, e in enumerate(EDGES)}


def _faces():
    """(axis, side, corners in cyclic order, counter-clockwise seen from outside the cube)."""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            cyc = []
            for (cu, cv) in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, cu, cv
                cyc.append(CORNERS.index(tuple(p)))
            # (u, v, axis) is a cyclic shift of (x, y, z) for axis 0 and 2, an odd permutation for axis 1
            ccw_from_plus = axis != 1
            if ccw_from_plus != (side == 1):
                cyc.reverse()
            out.append((axis, side, cyc))
    return out


FACES = _faces()
FACE_EDGE_SETS = [frozenset(EDGE_OF[frozenset((c[i], c[(i + 1) % 4]))] for i in range(4)) for _, _, c in FACES]


def _diag_id(axis, side, cyc, inside):
    """Which diagonal of the face is inside, named by in-face coordinates so that both sides of an axis agree:
    0 = the corners (0,0),(1,1) of the two other axes, 1 = (1,0),(0,1)."""
    u, v = [a for a in range(3) if a != axis]
    c = CORNERS[[k for k in cyc if inside[k]][0]]
    return 0 if c[u] == c[v] else 1


def face_segments(case, rule):
    """Directed segments (edge_from, edge_to) of `case`: walking along a segment on the face, seen from outside the
    cube, a cut-off INSIDE corner lies to the right (an OUTSIDE corner that is cut off: to the left)."""
    inside = [(case >> c) & 1 for c in range(8)]
    segs = []
    for axis, side, cyc in FACES:
        s = [inside[c] for c in cyc]
        n = sum(s)

        def e(i, j):
            return EDGE_OF[frozenset((cyc[i % 4], cyc[j % 4]))]

        def cut(i, want_inside):
            # corner i of the (counter-clockwise) cycle cut off from its two neighbours: from the edge towards the
            # previous corner to the edge towards the next one the corner is on the right
            a, b = e(i - 1, i), e(i, i + 1)
            return (a, b) if want_inside else (b, a)

        if n in (0, 4):
            continue
        if n == 1:
            segs.append(cut(s.index(1), True))
        elif n == 3:
            segs.append(cut(s.index(0), False))
        elif s[0] == s[2]:  # ambiguous: a diagonal inside
            sep_inside = rule[axis][_diag_id(axis, side, cyc, inside)]
            for i in range(4):
                if s[i] == (1 if sep_inside else 0):
                    segs.append(cut(i, bool(sep_inside)))
        else:  # two adjacent corners inside: i, i+1
            i = [k for k in range(4) if s[k] and s[(k + 1) % 4]][0]
            a, b = e(i - 1, i), e(i + 1, i + 2)
            segs.append((a, b))
    return segs


def loops_of(segs):
    nxt = dict(segs)
    assert len(nxt) == len(segs) and set(nxt) == set(nxt.values()), segs
    seen, loops = set(), []
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        loops.append(loop)
    return loops


def _in_face(a, b):
    return any(a in f and b in f for f in FACE_EDGE_SETS)


def triangulate(loop):
    """First triangulation of the polygon (lexicographic over the recursion) none of whose diagonals lies in a face."""
    n = len(loop)

    def rec(i, j):  # triangulations of the sub-polygon loop[i..j], given that chord (i, j) is allowed
        if j - i < 2:
            return [[]]
        res = []
        for k in range(i + 1, j):
            if k - i >= 2 and _in_face(loop[i], loop[k]):
                continue
            if j - k >= 2 and _in_face(loop[k], loop[j]):
                continue
            for left in rec(i, k):
                for right in rec(k, j):
                    res.append(left + [(loop[i], loop[k], loop[j])] + right)
                    if res:
                        return res
        return res

    res = rec(0, n - 1)
    return res[0] if res else None


def build(rule):
    rows = []
    for case in range(256):
        tris = []
        for loop in loops_of(face_segments(case, rule)):
            t = triangulate(loop)
            if t is None:
                return None
            tris += t
        if len(tris) > 5:
            return None
        rows.append(tris)
    return rows


def anchor_ok(rows):
    import numpy as np
    mid = [(np.array(CORNERS[a], float) + np.array(CORNERS[b], float)) / 2 for a, b in EDGES]
    for c in range(8):
        (t,) = rows[1 << c]
        n = np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]])
        out = np.mean([CORNERS[k] for k in range(8) if k != c], 0) - np.array(CORNERS[c], float)
        if not n @ out > 0:
            return False
    return True


def search():
    # prefer rules that separate the inside corners (1) on as many (axis, diagonal) pairs as possible
    order = sorted(itertools.product((1, 0), repeat=6), key=lambda r: -sum(r))
    for r in order:
        rule = [r[0:2], r[2:4], r[4:6]]
        rows = build(rule)
        if rows is not None:
            return rule, rows
    raise SystemExit("no face rule fits five triangles per cube")


def render(rule, rows):
    def row(tris):
        flat = [e for t in tris for e in t]
        return "{" + ", ".join(f"{e:2d}" for e in flat + [-1] * (16 - len(flat))) + "}"

    lines = [
        "// mi3d_mc_tables.h - the 256-case marching-cubes tables of include/mi3d.h Part 8, shared by host and device code.",
        "// GENERATED by tools/gen_mc_tables.py (which states the construction); tests/test_mc_tables_cpu.py checks the",
        "// properties the mesh relies on.  Do not edit by hand.",
        "//",
        "// Corner c of a cube with min corner (i, j, k) is (i, j, k) + MI3D_MC_CORNERS[c]; edge e joins the corners",
        "// MI3D_MC_EDGES[e]; bit c of the case index is set iff corner c is inside (value >= iso).  A row lists the cube",
        "// edges of up to five triangles, -1 terminated.  Ambiguous faces, by (axis of the face normal, inside diagonal",
        "// 0 = in-face corners (0,0),(1,1) / 1 = (1,0),(0,1)): 1 = the inside corners are separated, 0 = the outside ones:",
        "//   " + ", ".join(f"{'xyz'[a]}: {tuple(rule[a])}" for a in range(3)),
        "#ifndef MI3D_MC_TABLES_H",
        "#define MI3D_MC_TABLES_H",
        "",
        "#define MI3D_MC_CORNERS_INIT {" + ", ".join("{%d, %d, %d}" % c for c in CORNERS) + "}",
        "#define MI3D_MC_EDGES_INIT {" + ", ".join("{%d, %d}" % e for e in EDGES) + "}",
        "",
        "/* triangles per case */",
        "#define MI3D_MC_NTRI_INIT { \\",
    ]
    for i in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(rows[c])) for c in range(i, i + 32)) + (", \\" if i < 224 else " \\"))
    lines += ["}", "", "/* cube edges of the triangles of each case */", "#define MI3D_MC_TRI_INIT { \\"]
    for c in range(256):
        lines.append(f"    /* {c:3d} */ " + row(rows[c]) + ("," if c < 255 else "") + " \\")
    lines += ["}", "", "#endif /* MI3D_MC_TABLES_H */", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    rule, rows = search()
    assert anchor_ok(rows), "winding anchor failed"
    text = render(rule, rows)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "make-it-3d_amd", "csrc",
                        "mi3d_mc_tables.h")
    if "--check" in sys.argv:
        sys.exit(0 if open(path).read() == text else "mi3d_mc_tables.h differs from what this script generates")
    open(path, "w").write(text)
    print(f"wrote {path}: rule {rule}, {sum(len(r) for r in rows)} triangles over 256 cases, "
          f"max {max(len(r) for r in rows)}")
