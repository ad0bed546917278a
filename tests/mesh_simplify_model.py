"""A NumPy restatement of include/mi3d.h Part 14 (mesh simplification by vertex clustering), for
tests/test_mesh_simplify_cpu.py and tests/test_mesh_simplify_gpu.py: the yardstick the kernels of csrc/meshsimplify.hip are
compared with, exactly - integer arrays equal, float rows bit-identical.  float32, int64 and float64 stand where the
contract says binary32, int64 and binary64; NumPy rounds every array operation on its own, which is what the contract
asks (no fused multiply-add).  Below the model: the inputs both test files share."""
import numpy as np

CLAMP_LO, CLAMP_HI = -2 ** 30, 2 ** 30 - 1
FRACTION = 2 ** 20
COUNTS = ("vertices", "triangles", "bad_triangles", "gave_up", "non_finite_vertices", "clusters", "degenerate",
          "duplicate")


def clusters(vertices, origin, cell):
    """(finite bool [nv], c int32 [nv, 3], q int64 [nv, 3]): the cluster and the fixed-point fraction of every vertex
    (rows of non-finite vertices hold garbage)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    o = np.asarray(origin, np.float32).reshape(3)
    cell = np.float32(cell)
    finite = np.isfinite(v).all(1)
    with np.errstate(all="ignore"):
        g = (v - o[None, :]) / cell                                   # float32: subtraction, then division
        assert g.dtype == np.float32
        fl = np.where(np.isnan(g), np.float32(0), np.floor(g))
        c = np.clip(fl.astype(np.float64), CLAMP_LO, CLAMP_HI).astype(np.int64).astype(np.int32)
        f = g - c.astype(np.float32)                                  # float32
        f = np.where(np.isnan(f), np.float32(0), np.clip(f, np.float32(0), np.float32(1))).astype(np.float32)
        q = np.floor(f * np.float32(FRACTION)).astype(np.int64)
    return finite, c, q


def simplify(vertices, triangles, origin, cell):
    """Returns (vertices float32 [kv, 3], triangles int32 [kt, 3], vertex_map int32 [nv], counts: list of 8 ints)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    nv, nt = len(v), len(t)
    o = np.asarray(origin, np.float32).reshape(3)
    finite, c, q = clusters(v, o, cell)

    # leaders: the smallest vertex index of every cluster
    lead = np.full(nv, -1, np.int64)
    idx = np.nonzero(finite)[0]
    if len(idx):
        _, first, inverse = np.unique(c[idx], axis=0, return_index=True, return_inverse=True)
        lead[idx] = idx[first[inverse.reshape(-1)]]                   # np.unique reports the FIRST occurrence
    leaders = np.nonzero(lead == np.arange(nv))[0]

    # accumulators in the leader's row
    S = np.zeros((nv, 3), np.int64)
    n = np.zeros(nv, np.int64)
    np.add.at(S, lead[idx], q[idx])
    np.add.at(n, lead[idx], 1)

    # triangles
    t64 = t.astype(np.int64)
    in_range = ((t64 >= 0) & (t64 < nv)).all(1)
    lt = np.full((nt, 3), -1, np.int64)
    if nv:
        lt[in_range] = lead[t64[in_range]]
    bad = ~in_range | (lt < 0).any(1)
    degenerate = ~bad & ((lt[:, 0] == lt[:, 1]) | (lt[:, 1] == lt[:, 2]) | (lt[:, 0] == lt[:, 2]))
    cand = np.nonzero(~bad & ~degenerate)[0]
    survivors = np.zeros(0, np.int64)
    if len(cand):
        _, first = np.unique(np.sort(lt[cand], axis=1), axis=0, return_index=True)
        survivors = np.sort(cand[first])
    duplicate = len(cand) - len(survivors)

    # output: the cited clusters by ascending leader, the survivors by ascending index
    cited = np.unique(lt[survivors]) if len(survivors) else np.zeros(0, np.int64)
    new_id = np.full(nv, -1, np.int64)
    new_id[cited] = np.arange(len(cited))
    vertex_map = np.where(lead >= 0, new_id[np.maximum(lead, 0)], -1).astype(np.int32) if nv else np.zeros(0, np.int32)
    s = S[cited].astype(np.float64) / n[cited].astype(np.float64)[:, None]
    s = s * np.float64(1.0 / FRACTION)
    s = c[cited].astype(np.float64) + s
    s = np.float64(np.float32(cell)) * s
    s = o.astype(np.float64)[None, :] + s
    out_v = s.astype(np.float32).reshape(-1, 3)
    out_t = new_id[lt[survivors]].astype(np.int32).reshape(-1, 3)
    counts = [len(cited), len(survivors), int(bad.sum()), 0, int((~finite).sum()), len(leaders), int(degenerate.sum()),
              int(duplicate)]
    assert counts[1] + counts[6] + counts[7] + counts[2] == nt
    return out_v, out_t, vertex_map, counts


def export_lattice(R, d):
    """The lattice export_mesh clusters on: origin -1 - h/4 in float32, cell = float32(d h), h = 2 / (R - 1)."""
    h = 2.0 / (R - 1)
    o = np.float32(-1.0) - np.float32(h) / np.float32(4.0)
    return np.array([o, o, o], np.float32), np.float32(d * h)


# ------------------------------------------------------------------------------------------------ checks without the model

def check_geometry(vertices, origin, cell, out_v, out_t, vertex_map, radius=None):
    """What must hold of any output, stated without simplify(): every output vertex lies in the cell of the vertices
    mapped to it, up to one float32 ulp of its coordinate (the final rounding); with `radius`, it lies within a cell
    diagonal of that sphere; every triangle has three distinct indices in [0, kv), no two share a vertex set, every
    output vertex is cited.  The inputs here lie away from +-2^30 cells and their g away from binary32 ties, so the cell
    of a vertex is taken in float64."""
    v = np.asarray(vertices, np.float64)
    o, cell = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(cell))
    out_v, out_t, vertex_map = np.asarray(out_v), np.asarray(out_t), np.asarray(vertex_map)
    kv = len(out_v)
    assert out_v.dtype == np.float32 and out_t.dtype == np.int32 and vertex_map.dtype == np.int32
    assert vertex_map.shape == (len(v),) and vertex_map.min(initial=-1) >= -1 and vertex_map.max(initial=-1) == kv - 1
    mapped = np.nonzero(vertex_map >= 0)[0]
    c = np.floor((v[mapped] - o) / cell)
    first = np.full(kv, -1, np.int64)
    first[vertex_map[mapped][::-1]] = np.arange(len(mapped))[::-1]      # a member of every output vertex
    assert (first >= 0).all()
    assert np.array_equal(c, c[first][vertex_map[mapped]])               # one cell per output vertex
    g = (out_v.astype(np.float64) - o) / cell - c[first]
    tol = np.spacing(np.abs(out_v)).astype(np.float64) / cell
    assert np.all(g >= -tol) and np.all(g <= 1 + tol), (g.min(), g.max())
    if radius is not None:
        assert np.all(np.abs(np.linalg.norm(out_v.astype(np.float64), axis=1) - radius) <= cell * np.sqrt(3.0))
    assert out_t.min(initial=0) >= 0 and out_t.max(initial=-1) < kv
    assert np.all((out_t[:, 0] != out_t[:, 1]) & (out_t[:, 1] != out_t[:, 2]) & (out_t[:, 0] != out_t[:, 2]))
    assert len(np.unique(np.sort(out_t, axis=1), axis=0)) == len(out_t)
    assert np.array_equal(np.unique(out_t), np.arange(kv))


# ------------------------------------------------------------------------------------------------ the inputs

def sphere_volume(R, r0=0.6, centre=(0.0, 0.0, 0.0)):
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (r0 - d).astype(np.float32)


def torus_volume(R=32, major=0.55, minor=0.22):
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (minor - np.sqrt((np.sqrt(x ** 2 + y ** 2) - major) ** 2 + z ** 2)).astype(np.float32)


VOLUMES = {                                                           # name -> (R, volume maker); iso = 0
    "sphere24": (24, lambda: sphere_volume(24, 0.6)),
    "sphere48": (48, lambda: sphere_volume(48, 0.6)),
    "torus32": (32, torus_volume),
    "two_spheres32": (32, lambda: np.maximum(sphere_volume(32, 0.3, (0.45, 0, 0)), sphere_volume(32, 0.3, (-0.45, 0, 0)))),
    # The model finds NO duplicate triangle on a plain sphere (a triangle is smaller than a cell: around a lattice point
    # one triangle spans three cells) and 3 744 vertices on the 48^3 one.  So two surfaces more: a shell thinner than the
    # coarser cells, whose two sheets fall into the same clusters (duplicates, with opposite orientations), and a sphere
    # with more than 10 000 vertices.
    "shell32": (32, lambda: np.minimum(sphere_volume(32, 0.6), -sphere_volume(32, 0.47))),
    "sphere96": (96, lambda: sphere_volume(96, 0.6)),
}
SURFACE_D = (1.5, 2, 3.7)                                             # export lattice, in grid steps
OWN_ORIGIN_STEPS = 3                                                  # origin=None: cell = 3 h


def lattices(R, vertices):
    """[(name, origin float32[3], cell float32)] a surface at resolution R is clustered with."""
    h = 2.0 / (R - 1)
    out = [(f"d={d}", *export_lattice(R, d)) for d in SURFACE_D]
    out.append(("own origin", np.asarray(vertices, np.float32).min(0), np.float32(OWN_ORIGIN_STEPS * h)))
    return out


SHEET = 600                                                           # vertices per side
SHEET_CELLS = (2.5, 7.0)                                              # in lattice steps
SCAN_ROUND = 1024 * 256                                               # elements per round of scan_row (csrc/mi3d_scan.h)


def sheet(n=SHEET):
    """A planar lattice sheet of n x n vertices at unit steps, two triangles per square: n^2 vertices, 2 (n - 1)^2
    triangles (360 000 and 717 602 at n = 600)."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    t = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)]).astype(np.int32)
    return v, t


def sheet_lattice(steps):
    return np.array([-0.25, -0.25, -0.25], np.float32), np.float32(steps)


def boundary_case():
    """Vertices exactly on cell boundaries, just below them (one with g = -1e-10, whose fraction rounds to 1.0), below the
    origin and past the +-2^30 clamp; two fans of triangles over them.  origin (0, -0.25, 1), cell 0.25: g is exact
    for the coordinates chosen."""
    origin, cell = np.array([0.0, -0.25, 1.0], np.float32), np.float32(0.25)
    xs = [0.0, 0.25, 0.5, 1.0,                                        # g = 0, 1, 2, 4: on boundaries
          float(np.nextafter(np.float32(0.25), np.float32(0.0))),     # just below g = 1
          float(np.nextafter(np.float32(0.5), np.float32(0.0))),      # just below g = 2
          -2.5e-11,                                                   # g = -1e-10: c = -1, f rounds to 1.0
          -0.25, -1.0, -3.5,                                          # below the origin: c = -1, -4, -14
          0.125, 0.375]                                               # mid-cell
    v = [(x, -0.25 + 0.25 * (k % 3), 1.0 + 0.25 * (k % 2)) for k, x in enumerate(xs)]
    v += [(3.0e9, 0.0, 1.0), (-3.0e9, 0.0, 1.0), (3.0e38, -3.0e38, 1.0)]   # g beyond +-2^30 (the last: g overflows)
    v = np.array(v, np.float32)
    nv = len(v)
    t = np.array([(k, (k + 1) % nv, (k + 5) % nv) for k in range(nv)] + [(k, (k + 2) % nv, (k + 7) % nv) for k in range(nv)],
                 np.int32)
    return v, t, origin, cell


def fans_case():
    """Unit cells at origin 0.  Clusters A = (0,0,0), B = (1,0,0), C = (0,1,0), D = (1,1,0), E = (3,3,0), F = (5,5,0).
    Triangles 0 and 1 collapse onto {A, B, C} with the SAME orientation, 2 onto it with the OPPOSITE one; triangles 3 and 4
    onto {B, C, D} with opposite orientations, the reversed one first; 5 has two corners in A (degenerate); 6 is the only
    one that cites E, and is degenerate, so E is a cluster cited by dropped triangles alone; vertex 12 (F) is cited by no
    triangle."""
    v = np.array([(0.2, 0.2, 0.5), (1.2, 0.2, 0.5), (0.2, 1.2, 0.5),        # 0 A, 1 B, 2 C
                  (0.7, 0.6, 0.5), (1.7, 0.6, 0.5), (0.7, 1.6, 0.5),        # 3 A, 4 B, 5 C
                  (1.5, 1.5, 0.5), (1.1, 1.9, 0.5),                         # 6 D, 7 D
                  (0.9, 0.1, 0.5),                                          # 8 A
                  (3.5, 3.5, 0.5), (3.6, 3.1, 0.5),                         # 9 E, 10 E
                  (1.9, 0.9, 0.5),                                          # 11 B
                  (5.5, 5.5, 0.5)], np.float32)                             # 12 F
    t = np.array([(3, 4, 5), (0, 1, 2), (2, 1, 0),                          # {A,B,C}: 0 survives, as (A, B, C)
                  (7, 5, 4), (1, 2, 6),                                     # {B,C,D}: 3 survives, as (D, C, B)
                  (0, 8, 1),                                                # A, A, B
                  (9, 10, 0)], np.int32)                                    # E, E, A
    return v, t, np.zeros(3, np.float32), np.float32(1.0)


def bad_case():
    """Corner indices -1, nv and INT32_MAX; a NaN and an inf vertex, each cited by one triangle and one of them by none."""
    rng = np.random.default_rng(14)
    nv, nt = 300, 120
    v = rng.uniform(-1, 1, size=(nv, 3)).astype(np.float32)
    t = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    v[17, 1], v[200, 0], v[250, 2] = np.nan, np.inf, -np.inf
    t[t == 17] = 18
    t[t == 200] = 201
    t[t == 250] = 251
    t[5, 1], t[40, 2], t[77, 0] = -1, nv, 2 ** 31 - 1
    t[9, 0], t[90, 2] = 17, 200                                      # vertex 250 is cited by no triangle
    return v, t, np.array([-1.0, -1.0, -1.0], np.float32), np.float32(0.2)
