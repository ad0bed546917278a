"""CPU: the marching-cubes case table of include/mi3d.h Part 8, read through mi3d_mc_case, has the properties that make
a mesh watertight and consistently oriented - and a NumPy restatement of the whole extraction (`marching_cubes_ref`),
the expected value of tests/test_mesh_gpu.py, exercised here on a sphere so that a broken restatement is found without
a GPU.

The table's provenance is not tested (it is constructed by tools/gen_mc_tables.py); these properties are:
  * a triangle only uses cube edges that join an inside and an outside corner, and every such edge is used;
  * the patch in a cube is an oriented surface whose boundary lies in the cube's faces;
  * FACE CONSISTENCY: what a case leaves on a cube face is a function of that face's four corner states, and the
    neighbouring cube leaves the same segments reversed (12 288 pairs of cubes) - no cracks, whatever the volume;
  * the winding anchor: normals point away from an inside corner;
  * cases 0 and 255 are empty, the count table matches the rows, no row has more than 5 triangles.
"""
import ctypes
import itertools

import numpy as np
import pytest

# the numbering include/mi3d.h documents
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def load_table():
    """rows[case] = [(e0, e1, e2), ...] and counts[case], both as mi3d_mc_case reports them."""
    from mi3d import _lib
    fn = _lib.lib().mi3d_mc_case
    rows, counts = [], []
    for case in range(256):
        buf = (ctypes.c_int8 * 16)(*([77] * 16))
        counts.append(fn(case, buf))
        r = list(buf)
        assert -1 in r, (case, r)
        r = r[:r.index(-1)]
        assert len(r) % 3 == 0 and all(0 <= e < 12 for e in r), (case, r)
        rows.append([tuple(r[i:i + 3]) for i in range(0, len(r), 3)])
    return rows, counts


@pytest.fixture(scope="module")
def table():
    return load_table()


def _inside(case):
    return [(case >> c) & 1 for c in range(8)]


def _face_edges(axis, side):
    return frozenset(e for e, (a, b) in enumerate(EDGES) if CORNERS[a][axis] == side and CORNERS[b][axis] == side)


FACES = [(axis, side, _face_edges(axis, side)) for axis in range(3) for side in (0, 1)]


def _directed(tris):
    return [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]


def test_mc_case_rejects_bad_arguments():
    from mi3d import _lib
    fn = _lib.lib().mi3d_mc_case
    buf = (ctypes.c_int8 * 16)()
    assert fn(256, buf) == -1 and fn(0, None) == -1


def test_triangles_use_exactly_the_crossing_edges(table):
    rows, _ = table
    for case in range(256):
        ins = _inside(case)
        crossing = {e for e, (a, b) in enumerate(EDGES) if ins[a] != ins[b]}
        used = {e for t in rows[case] for e in t}
        assert used == crossing, (case, used, crossing)
        assert all(len(set(t)) == 3 for t in rows[case]), case


def test_patch_is_an_oriented_surface_with_its_boundary_in_the_faces(table):
    rows, _ = table
    for case in range(256):
        uses = {}
        for a, b in _directed(rows[case]):
            uses[(a, b)] = uses.get((a, b), 0) + 1
        for (a, b), n in uses.items():
            in_face = any(a in f and b in f for _, _, f in FACES)
            back = uses.get((b, a), 0)
            if in_face:
                assert n == 1 and back == 0, (case, a, b)
            else:
                assert n == 1 and back == 1, (case, a, b)


def _face_segments(rows, case, axis, side):
    """Directed segments the case leaves on a face, each end named by the in-face coordinates of its edge's corners."""
    f = _face_edges(axis, side)
    u, v = [a for a in range(3) if a != axis]

    def key(e):
        return frozenset((CORNERS[c][u], CORNERS[c][v]) for c in EDGES[e])
    return frozenset((key(a), key(b)) for a, b in _directed(rows[case]) if a in f and b in f)


def test_face_consistency_over_all_pairs_of_neighbouring_cubes(table):
    rows, _ = table
    pairs = 0
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        seg = {(case, side): _face_segments(rows, case, axis, side) for case in range(256) for side in (0, 1)}

        def cases_with(side, state):
            """The 16 cases whose corners on `side` of the axis have the in-face states `state[(u, v)]`."""
            out = []
            for rest in itertools.product((0, 1), repeat=4):
                case, it = 0, iter(rest)
                for c, xyz in enumerate(CORNERS):
                    bit = state[(xyz[u], xyz[v])] if xyz[axis] == side else next(it)
                    case |= bit << c
                out.append(case)
            return out

        for bits in itertools.product((0, 1), repeat=4):
            state = dict(zip(((0, 0), (1, 0), (1, 1), (0, 1)), bits))
            for a in cases_with(1, state):       # the cube below the face: the face is its side 1
                for b in cases_with(0, state):   # the cube above it
                    sa, sb = seg[(a, 1)], seg[(b, 0)]
                    assert sb == frozenset((y, x) for x, y in sa), (axis, bits, a, b)
                    pairs += 1
    assert pairs == 12288


def test_winding_anchor_on_the_one_corner_cases(table):
    rows, _ = table
    mid = [(np.array(CORNERS[a], float) + np.array(CORNERS[b], float)) / 2 for a, b in EDGES]
    for c in range(8):
        (t,) = rows[1 << c]
        n = np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]])
        outward = np.mean([CORNERS[k] for k in range(8) if k != c], 0) - np.array(CORNERS[c], float)
        assert n @ outward > 0, c


def test_counts_and_empty_cases(table):
    rows, counts = table
    assert rows[0] == [] and rows[255] == []
    for case in range(256):
        assert counts[case] == len(rows[case]) <= 5, case


# ------------------------------------------------------------------------------------------------ the restatement

def marching_cubes_ref(vol, iso, origin=(0, 0, 0), spacing=(1, 1, 1), rows=None):
    """include/mi3d.h Part 8 in NumPy float32: vertices float32 [nv, 3], triangles int32 [nt, 3], in the contract's order.
    vol [Rx, Ry, Rz] float32 (x slowest)."""
    vol = np.ascontiguousarray(vol, np.float32)
    Rx, Ry, Rz = vol.shape
    iso = np.float32(iso)
    origin = np.asarray(origin, np.float32)
    spacing = np.asarray(spacing, np.float32)
    if rows is None:
        rows, _ = load_table()
    ins = vol >= iso                                   # NaN: outside
    lin = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)

    # vertices: one per crossing grid edge, owned by the edge's lower point; order (owner, axis)
    owners, axes, coords = [], [], []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = ins[lo] != ins[hi]
        va, vb = vol[lo][cross], vol[hi][cross]
        with np.errstate(all="ignore"):
            t = (iso - va) / (vb - va)                 # float32, each operation rounded once
        t = np.where((t >= 0) & (t <= 1), t, np.float32(0.5)).astype(np.float32)
        own = lin[lo][cross]
        ijk = np.stack(np.unravel_index(own, vol.shape), -1).astype(np.float32)
        ijk[:, axis] = ijk[:, axis] + t
        zero = np.float32(0.0)
        for c in range(3):
            if c != axis:
                ijk[:, c] = ijk[:, c] + zero
        coords.append(origin[None, :] + spacing[None, :] * ijk)
        owners.append(own)
        axes.append(np.full(own.shape, axis, np.int64))
    owners, axes, coords = np.concatenate(owners), np.concatenate(axes), np.concatenate(coords).astype(np.float32)
    order = np.lexsort((axes, owners))
    owners, axes, vertices = owners[order], axes[order], coords[order]
    vid = {(int(o), int(a)): n for n, (o, a) in enumerate(zip(owners, axes))}   # the weld: (owner point, axis) -> id

    # triangles: by cell (linear index of the min corner), then table order
    case = np.zeros((Rx - 1, Ry - 1, Rz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= ins[dx:Rx - 1 + dx, dy:Ry - 1 + dy, dz:Rz - 1 + dz].astype(np.int64) << c
    edge_owner = []
    for a, b in EDGES:
        pa, pb = np.array(CORNERS[a]), np.array(CORNERS[b])
        edge_owner.append((np.minimum(pa, pb), int(np.nonzero(pa != pb)[0][0])))
    tris = []
    for i, j, k in zip(*np.nonzero((case != 0) & (case != 255))):   # C order = increasing linear index
        for t in rows[int(case[i, j, k])]:
            tri = []
            for e in t:
                off, axis = edge_owner[e]
                o = ((int(i) + off[0]) * Ry + int(j) + off[1]) * Rz + int(k) + off[2]
                tri.append(vid[(int(o), axis)])
            tris.append(tri)
    triangles = np.array(tris, np.int32).reshape(-1, 3)
    return vertices, triangles


def edge_uses(triangles):
    """{(a, b): times the directed edge a -> b occurs}."""
    uses = {}
    t = np.asarray(triangles, np.int64)
    for a, b in np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]):
        uses[(int(a), int(b))] = uses.get((int(a), int(b)), 0) + 1
    return uses


def assert_closed_and_oriented(triangles):
    """Every undirected edge belongs to exactly two triangles, once in each direction; returns the number of edges."""
    uses = edge_uses(triangles)
    for (a, b), n in uses.items():
        assert a != b and n == 1 and uses.get((b, a), 0) == 1, (a, b, n)
    return len(uses) // 2


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def sphere_volume(R, r0=0.6, centre=(0.0, 0.0, 0.0)):
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (r0 - d).astype(np.float32)


def test_restatement_on_a_sphere(table):
    rows, _ = table
    R, r0 = 16, 0.6
    h = np.float32(2.0 / (R - 1))
    v, t = marching_cubes_ref(sphere_volume(R, r0), 0.0, (-1, -1, -1), (h, h, h), rows)
    assert v.dtype == np.float32 and t.dtype == np.int32 and len(v) > 100 and len(t) > 200
    E = assert_closed_and_oriented(t)
    assert len(v) - E + len(t) == 2                          # a sphere
    assert t.min() == 0 and t.max() == len(v) - 1            # every vertex is used, every index valid
    assert len(np.unique(v, axis=0)) == len(v)               # welded: no position twice
    vol = signed_volume(v, t)
    assert 0.7 * 4 / 3 * np.pi * r0 ** 3 < vol < 4 / 3 * np.pi * r0 ** 3   # outward normals; inscribed polyhedron
    assert np.all(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - r0) <= float(h))
    # the order of the contract: owners ascend, triangles follow their cells
    v2, t2 = marching_cubes_ref(sphere_volume(R, r0), 0.0, (-1, -1, -1), (h, h, h), rows)
    assert v.tobytes() == v2.tobytes() and t.tobytes() == t2.tobytes()


def test_restatement_t_rule_and_non_finite_values(table):
    """t = 0.5 where (iso - va) / (vb - va) is not within [0, 1] - only reachable through non-finite values - and NaN
    counts as outside."""
    rows, _ = table
    vol = np.full((3, 3, 3), -1.0, np.float32)
    vol[1, 1, 1] = np.inf
    v, t = marching_cubes_ref(vol, 0.0, rows=rows)
    assert len(v) == 6 and len(t) == 8 and np.isfinite(v).all()
    # towards +inf from -1: t = 1 / inf = 0, a legal t; from +inf towards -1: -inf / -inf = NaN -> 0.5
    assert sorted(map(tuple, v.tolist())) == sorted([(0, 1, 1), (1.5, 1, 1), (1, 0, 1), (1, 1.5, 1), (1, 1, 0),
                                                     (1, 1, 1.5)])
    assert_closed_and_oriented(t)
    assert signed_volume(v, t) > 0
    vol[1, 1, 1] = np.nan
    v, t = marching_cubes_ref(vol, 0.0, rows=rows)
    assert len(v) == 0 and t.shape == (0, 3)
    # a corner exactly at iso is inside, its vertices sit ON the corner, the triangles are degenerate and kept
    vol[1, 1, 1] = 0.0
    v, t = marching_cubes_ref(vol, 0.0, rows=rows)
    assert len(v) == 6 and len(t) == 8 and np.all(v == 1.0)
