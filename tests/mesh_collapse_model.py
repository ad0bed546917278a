"""A restatement of include/mi3d.h Part 19 (quadric edge-collapse decimation), for tests/test_mesh_collapse_cpu.py and
tests/test_mesh_collapse_gpu.py: the yardstick the kernels of csrc/meshcollapse.hip are compared with, exactly - integer
arrays equal, float rows bit-identical.  Python floats stand where the contract says binary64 (every operation rounded
on its own, no fused multiply-add), np.float32 where it says binary32.  The model follows the contract's words, one
edge at a time; it is not fast.  Below the model: the inputs both test files share."""
import numpy as np

import mesh_smooth_model as SM

MAX_DEGREE = 64                                                       # MI3D_COLLAPSE_MAX_DEGREE
MAX_ROW = 1024                                                        # MI3D_COLLAPSE_MAX_ROW
NONE = 2 ** 64 - 1
INF = float("inf")
COUNTS = ("vertices", "triangles", "unusable_triangles", "rounds", "non_finite_vertices", "collapses", "locked_vertices",
          "errors")
PAIRS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))   # the ten entries of a quadric


def f32(x):
    return float(np.float32(x))


def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def normal(p0, p1, p2):
    u = (p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2])
    v = (p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2])
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def plane_quadric(p0, p1, p2):
    """K of the triangle's plane, or None if s is 0 or not finite."""
    n = normal(p0, p1, p2)
    s = dot(n, n)
    if not (0.0 < s < INF):
        return None
    e = (n[0], n[1], n[2], -dot(n, p0))
    return [e[i] * e[j] / s for i, j in PAIRS]


def error(q, x, y, z):
    """E(x) = x^T A x + 2 b^T x + c in the order Part 19 states."""
    t0 = (q[0] * x + q[1] * y) + q[2] * z
    t1 = (q[1] * x + q[4] * y) + q[5] * z
    t2 = (q[2] * x + q[5] * y) + q[7] * z
    quad = (x * t0 + y * t1) + z * t2
    lin = (q[3] * x + q[6] * y) + q[8] * z
    return (quad + 2.0 * lin) + q[9]


def placement(q, pa, pb):
    """(x* as three binary32 values, E(x*)) or None: the candidates in order, the smallest E, ties to the earlier."""
    d = (pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2])
    mid = ((pa[0] + pb[0]) * 0.5, (pa[1] + pb[1]) * 0.5, (pa[2] + pb[2]) * 0.5)
    cands = [pa, pb, (f32(mid[0]), f32(mid[1]), f32(mid[2]))]
    a00, a01, a02, b0, a11, a12, b1, a22, b2 = q[:9]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    tr = ((a00 + a11) + a22) / 3.0
    if abs(det) > 1e-3 * ((tr * tr) * tr) and det != 0.0:
        o = (-((c00 * b0 + c01 * b1) + c02 * b2) / det, -((c01 * b0 + c11 * b1) + c12 * b2) / det,
             -((c02 * b0 + c12 * b1) + c22 * b2) / det)
        w = (o[0] - mid[0], o[1] - mid[1], o[2] - mid[2])
        if dot(w, w) <= dot(d, d):
            cands.append((f32(o[0]), f32(o[1]), f32(o[2])))
    best = None
    for c in cands:
        e = error(q, c[0], c[1], c[2])
        if e == e and (best is None or e < best[1]):
            best = (c, e)
    return best


def edge_hash(a, b, r):
    m = 0xFFFFFFFF
    return ((((a * 2654435761) & m) ^ ((b * 2246822519) & m) ^ ((r * 3266489917) & m)) >> 7) & 0xFFFFF


def collapse(vertices, triangles, target_faces, max_error=None, max_rounds=256, return_rounds=False):
    """Returns (vertices float32 [kv, 3], triangles int32 [kt, 3], vertex_map int32 [nv], counts: list of 8 ints)."""
    v0 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t0s = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    nv, nt = len(v0), len(t0s)
    target = int(target_faces)
    limit = np.float32(np.inf if max_error is None else max_error)
    assert target >= 0 and limit >= 0
    limit = float(limit)
    usable = SM.usable_triangles(v0, t0s)
    finite = np.isfinite(v0).all(1)
    P = [tuple(float(x) for x in row) for row in v0]
    tri = t0s.astype(np.int64).tolist()
    live = usable.tolist()

    # quadrics: ascending triangle index, from zero
    Q = [[0.0] * 10 for _ in range(nv)]
    deg0 = [0] * nv
    planeless = 0
    for t in range(nt):
        if not live[t]:
            continue
        c = tri[t]
        K = plane_quadric(P[c[0]], P[c[1]], P[c[2]])
        planeless += K is None
        for x in c:
            deg0[x] += 1
            if K is not None:
                q = Q[x]
                for k in range(10):
                    q[k] = q[k] + K[k]
    for x in range(nv):
        if deg0[x] > MAX_ROW:
            Q[x] = [float("nan")] * 10

    rep = list(range(nv))
    L = sum(live)
    rounds = collapses = locked_last = 0
    per_round = []
    for r in range(int(max_rounds)):
        if L <= target:
            break
        inc = [[] for _ in range(nv)]
        for t in range(nt):
            if live[t]:
                for k in range(3):
                    inc[tri[t][k]].append((t, k))
        deg = [len(row) for row in inc]
        nbr = [None] * nv                                            # the other two corners of every triangle at v
        locked = [False] * nv
        for x in range(nv):
            if deg[x] == 0:
                continue
            if deg[x] > MAX_DEGREE:
                locked[x] = True
                continue
            row = []
            for t, k in inc[x]:
                row.append(tri[t][(k + 1) % 3])
                row.append(tri[t][(k + 2) % 3])
            nbr[x] = row
            locked[x] = any(row.count(y) == 1 for y in row)
        locked_last = sum(locked)

        claim = [NONE] * nv
        cands = []                                                   # (key, a, b, x*)
        for t in range(nt):
            if not live[t]:
                continue
            for i in range(3):
                a, b, c = tri[t][i], tri[t][(i + 1) % 3], tri[t][(i + 2) % 3]
                if not a < b or locked[a] or locked[b]:
                    continue
                holders = [(u, k) for u, k in inc[a] if b in tri[u]]
                if len(holders) != 2:
                    continue
                (u, k), = [h for h in holders if h[0] != t]
                if tri[u][(k + 2) % 3] != b:                         # the other one must traverse b -> a
                    continue
                d = tri[u][(k + 1) % 3]
                if c == d:
                    continue
                nb = set(nbr[b])
                if any(y in nb and y != c and y != d for y in nbr[a]):
                    continue
                if not 3 <= deg[a] + deg[b] - 4 <= MAX_DEGREE:
                    continue
                if deg[c] < 4 or deg[d] < 4:
                    continue
                q = [Q[a][k] + Q[b][k] for k in range(10)]
                best = placement(q, P[a], P[b])
                if best is None:
                    continue
                x, e = best
                ok = True
                for end in (a, b):
                    for w, k in inc[end]:
                        if w == t or w == u:
                            continue
                        p = [P[y] for y in tri[w]]
                        n_old = normal(*p)
                        p[k] = x
                        n_new = normal(*p)
                        if not (dot(n_old, n_new) > 0.0 and dot(n_new, n_new) > 0.0):
                            ok = False
                if not ok:
                    continue
                c32 = np.float32(e if e > 0.0 else 0.0)
                if not c32 <= limit:
                    continue
                hi = (int(c32.view(np.uint32)) & 0xFFF00000) | edge_hash(a, b, r)
                key = (hi << 32) | (3 * t + i)
                cands.append((key, a, b, x))
                claim[a] = min(claim[a], key)
                claim[b] = min(claim[b], key)
        winners = []
        for key, a, b, x in cands:
            if claim[a] == key and claim[b] == key and all(claim[y] >= key for y in nbr[a] + nbr[b]):
                winners.append((key & 0xFFFFFFFF, a, b, x))
        per_round.append((L, len(cands), len(winners)))
        if not winners:
            break
        rounds += 1
        winners.sort()
        quota = (L - target + 1) // 2
        for _, a, b, x in winners[:quota]:
            rep[b] = a
            P[a] = x
            Q[a] = [Q[a][k] + Q[b][k] for k in range(10)]
            collapses += 1
        for t in range(nt):
            if live[t]:
                c = tri[t] = [rep[y] for y in tri[t]]
                if c[0] == c[1] or c[1] == c[2] or c[0] == c[2]:
                    live[t] = False
        rep = [rep[rep[x]] for x in range(nv)]
        L = sum(live)

    keep = [t for t in range(nt) if live[t]]
    cited = sorted({y for t in keep for y in tri[t]})
    new_id = np.full(nv, -1, np.int64)
    new_id[cited] = np.arange(len(cited))
    out_v = np.array([P[y] for y in cited], np.float32).reshape(-1, 3)
    out_t = np.array([[new_id[y] for y in tri[t]] for t in keep], np.int32).reshape(-1, 3)
    vertex_map = new_id[np.array(rep, np.int64)].astype(np.int32) if nv else np.zeros(0, np.int32)
    counts = [len(cited), len(keep), int((~usable).sum()) | (int(planeless) << 32), rounds, int((~finite).sum()), collapses,
              locked_last, 0]
    out = (out_v, out_t, vertex_map, counts)
    return out + (per_round,) if return_rounds else out


# ------------------------------------------------------------------------------------------------ measures

def centroid_radial_rms(v, t, radius=1.0):
    """RMS distance of the triangle centroids from the sphere of `radius` about the origin, float64."""
    v = np.asarray(v, np.float64)
    c = (v[t[:, 0]] + v[t[:, 1]] + v[t[:, 2]]) / 3.0
    return float(np.sqrt(np.mean((np.linalg.norm(c, axis=1) - radius) ** 2)))


enclosed_volume = SM.enclosed_volume


# ------------------------------------------------------------------------------------------------ the inputs

def cube(n):
    """The surface of [-1, 1]^3, n x n quads per face, two triangles per quad, outward: 6 n^2 + 2 vertices, 12 n^2
    triangles.  The coordinates are k * (2 / n) - 1 in float64 rounded to float32; the faces lie exactly on +-1."""
    ax = (np.arange(n + 1) * (2.0 / n) - 1.0).astype(np.float32)
    ax[0], ax[-1] = -1.0, 1.0
    index, verts, tris = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        g = [0, 0, 0]
                        g[axis], g[(axis + 1) % 3], g[(axis + 2) % 3] = side, i + di, j + dj
                        quad.append(vid(tuple(g)))
                    if side == 0:
                        quad.reverse()
                    tris += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    v = np.array([[ax[g] for g in p] for p in verts], np.float32)
    return v, np.array(tris, np.int32)


def octa_sphere(levels=4):
    """The octahedron subdivided `levels` times, every vertex pushed to the unit sphere: 8 * 4^levels triangles, outward."""
    verts = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, new = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.add(verts[a], verts[b])
                verts.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in tris:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            new += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        tris = new
    return np.array(verts, np.float32), np.array(tris, np.int32)


def tetrahedron():
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float32)
    return v, np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)


open_sheet = SM.open_sheet                                            # 20 x 20, bumpy: 76 border vertices


def fan100():
    """A closed fan whose centre has degree 100 > MAX_DEGREE: locked and counted; every rim vertex is on an open edge."""
    return SM.fan(100)


def bad_case():
    """The bumpy sheet of the smoothing tests with indices out of range, a repeated index and non-finite vertices."""
    return SM.bad_case()


SPHERE_CELLS = (0.30, 0.37, 0.45)                                     # clustering cells the sphere comparison uses
SPHERE_ORIGIN = -1.07
STALL_ERROR = 3e-3                                                    # octa_sphere(3) to 60 faces stalls at about 300
