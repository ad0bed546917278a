"""A NumPy restatement of include/mi3d.h Part 16 (Taubin smoothing of a mesh's vertices), for
tests/test_mesh_smooth_cpu.py and tests/test_mesh_smooth_gpu.py: the yardstick the kernels of csrc/meshsmooth.hip are
compared with, exactly - vertices bit for bit, all counts equal.  int64 and float64 stand where the contract says 64-bit
integers and binary64; NumPy rounds every array operation on its own, which is what the contract asks (no fused
multiply-add).  Below the model: the inputs both test files share."""
import numpy as np

import mesh_simplify_model as S

SATURATE = 2 ** 40
MAX_DEGREE = 1024                                                     # MI3D_SMOOTH_MAX_DEGREE
COUNTS = ("unusable_triangles", "non_finite_vertices", "isolated_vertices", "border_vertices", "over_degree_vertices",
          "clamped_vertices", "errors")
LAMBDA, MU = 0.5, -0.53


def fraction_bits(extent):
    """The e mesh.smooth chooses for coordinates up to `extent`: extent <= 2^x, e = 38 - x taken into [0, 40]."""
    x = int(np.frexp(float(extent))[1]) if extent > 0 else -40
    return min(max(38 - x, 0), 40)


def usable_triangles(vertices, triangles):
    """bool [nt]: indices in [0, nv), pairwise distinct, three vertices finite in the input."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3).astype(np.int64)
    nv = len(v)
    ok = ((t >= 0) & (t < nv)).all(1)
    ok &= (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    finite = np.isfinite(v).all(1)
    if nv:
        ok &= finite[np.clip(t, 0, nv - 1)].all(1)
    return ok


def quantise(p, e):
    """q of Part 16: int64, saturated at +-2^40, 0 for NaN."""
    with np.errstate(all="ignore"):
        x = p.astype(np.float64) * np.float64(2.0 ** e)
        r = np.where(np.isnan(x), 0.0, np.clip(np.rint(x), -float(SATURATE), float(SATURATE)))
    return r.astype(np.int64)                                         # np.rint: to nearest, ties to even


def border_vertices(ut, nv):
    """bool [nv]: on an edge that exactly one of the usable triangles `ut` (int64 [m, 3]) has."""
    on = np.zeros(nv, bool)
    if len(ut):
        e = np.concatenate([ut[:, [0, 1]], ut[:, [1, 2]], ut[:, [2, 0]]])
        e = np.sort(e, axis=1)
        uniq, cnt = np.unique(e, axis=0, return_counts=True)
        on[uniq[cnt == 1].reshape(-1)] = True
    return on


def smooth(vertices, triangles, iterations, lam=LAMBDA, mu=MU, pin_border=True, max_move=None, e=None):
    """Returns (vertices float32 [nv, 3], counts: list of 7 ints).  `e` None: fraction_bits of the largest finite
    |coordinate|, what mesh.smooth reads from the device."""
    v0 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    nv = len(v0)
    if e is None:
        e = fraction_bits(np.abs(np.where(np.isfinite(v0), v0, np.float32(0))).max(initial=0.0))
    ok = usable_triangles(v0, t)
    ut = t[ok].astype(np.int64)
    deg = np.zeros(nv, np.int64)
    np.add.at(deg, ut.reshape(-1), 1)
    finite = np.isfinite(v0).all(1)
    over = deg > MAX_DEGREE
    border = border_vertices(ut, nv) & ~over if pin_border else np.zeros(nv, bool)
    moves = finite & (deg > 0) & ~over & ~border
    w = (2 * deg).astype(np.float64)
    cur = v0.copy()
    held = np.zeros(nv, bool)
    with np.errstate(all="ignore"):
        if max_move is not None:
            lo, hi = v0 - np.float32(max_move), v0 + np.float32(max_move)      # float32
        for _ in range(int(iterations)):
            for k in (lam, mu):
                if k == 0:
                    continue
                q = quantise(cur, e)
                acc = np.zeros((nv, 3), np.int64)
                for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                    np.add.at(acc, ut[:, a], q[ut[:, b]] + q[ut[:, c]])
                m = acc.astype(np.float64) / w[:, None]
                m = m * np.float64(2.0 ** -e)
                p = cur.astype(np.float64)
                d = m - p
                d = np.float64(k) * d
                new = (p + d).astype(np.float32)
                held = np.zeros(nv, bool)
                if max_move is not None:
                    kept = np.where(new < lo, lo, np.where(new > hi, hi, new))
                    held = moves & (kept != new).any(1)
                    new = kept
                cur = np.where(moves[:, None], new, cur)
    counts = [int((~ok).sum()), int((~finite).sum()), int((deg == 0).sum()), int(border.sum()), int(over.sum()),
              int(held.sum()), 0]
    return cur, counts


# ------------------------------------------------------------------------------------------------ measures

def radial_rms(v, radius):
    r = np.linalg.norm(np.asarray(v, np.float64), axis=1)
    return float(np.sqrt(np.mean((r - radius) ** 2)))


def enclosed_volume(v, t):
    """The signed volume of a closed mesh, float64."""
    v = np.asarray(v, np.float64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------------------------------------ the inputs

VOLUMES = S.VOLUMES                                                   # the surfaces of the simplification tests
EXTENT_E = fraction_bits(1.0)                                         # surfaces in [-1, 1]^3, as export_mesh passes it
# (iterations, lam, mu, pin_border, max_move in units of the grid step h) every surface is smoothed with
SURFACE_RUNS = ((1, LAMBDA, MU, True, None), (7, LAMBDA, MU, True, None), (3, LAMBDA, 0.0, True, None),
                (7, LAMBDA, MU, True, 0.1), (4, 0.63, -0.67, False, None))
NOISE = 0.03                                                          # radial, relative, on the sphere the properties use


def noisy_sphere(v, seed=16, noise=NOISE):
    """`v` scaled radially by 1 + noise * U(-1, 1) per vertex, float32."""
    rng = np.random.default_rng(seed)
    return (v.astype(np.float64) * (1.0 + noise * rng.uniform(-1, 1, size=(len(v), 1)))).astype(np.float32)


def open_sheet(n=20):
    """n x n vertices of a bumpy open sheet: 4 (n - 1) border vertices (76 at n = 20)."""
    v, t = S.sheet(n)
    rng = np.random.default_rng(20)
    v = v.copy()
    v[:, 2] = rng.uniform(-0.3, 0.3, size=len(v)).astype(np.float32)
    v[:, :2] += rng.uniform(-0.2, 0.2, size=(len(v), 2)).astype(np.float32)
    return v, t


def fan(n, centre=(0.0, 0.0, 0.5), first=0):
    """A closed fan of n triangles: vertex `first` is the centre (degree n, interior), the n rim vertices follow."""
    ang = 2 * np.pi * np.arange(n) / n
    rng = np.random.default_rng(n)
    r = 1.0 + 0.2 * rng.uniform(-1, 1, size=n)
    v = np.concatenate([[centre], np.stack([centre[0] + r * np.cos(ang), centre[1] + r * np.sin(ang),
                                            0.1 * rng.uniform(-1, 1, size=n)], 1)]).astype(np.float32)
    k = np.arange(n)
    t = np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], 1) + first
    return v, t.astype(np.int32)


def fan300():
    """The centre has degree 300: a row of 600 entries, longer than a wave, and 360 000 comparisons of the border rule.
    The fan is closed, so the centre is interior and moves; every rim vertex lies on an open edge."""
    return fan(300)


def degree_limit_case():
    """Two closed fans: the centre of the first has degree 1024 = MAX_DEGREE and moves, the centre of the second has
    degree 1025 and is pinned and counted."""
    v1, t1 = fan(MAX_DEGREE)
    v2, t2 = fan(MAX_DEGREE + 1, centre=(5.0, 0.0, 0.7), first=len(v1))
    return np.concatenate([v1, v2]), np.concatenate([t1, t2])


def fans_case():
    """The non-manifold mesh of the simplification tests: edges with three triangles, a vertex no triangle cites."""
    v, t, _, _ = S.fans_case()
    return v, t


def bad_case():
    """A bumpy 12 x 12 sheet with: an index out of range (-1, nv, INT32_MAX), a triangle with a repeated index, a NaN
    and an infinite vertex (each cited by triangles, which become unusable), an isolated vertex, and a coordinate of
    3e30 that saturates the fixed point."""
    v, t = open_sheet(12)
    nv0 = len(v)
    v = np.concatenate([v, [[40.0, 40.0, 40.0]]]).astype(np.float32)  # nv0: cited by nothing
    nv = len(v)
    t = t.copy()
    t[3, 1], t[50, 2], t[77, 0] = -1, nv, 2 ** 31 - 1
    t[100, 2] = t[100, 0]                                             # repeated index
    v[40, 1], v[90, 0] = np.nan, np.inf
    v[65, 2] = 3.0e30                                                 # saturates; its neighbours sum 2^40
    assert nv0 == 144
    return v, t


def big_sheet():
    """The 600 x 600 sheet of the simplification tests with a bump per vertex: 360 000 vertices, more than one round of
    the 1024-wide scan over the per-workgroup degree sums (S.SCAN_ROUND vertices per round)."""
    v, t = S.sheet()
    v = v.copy()
    v[:, 2] = np.random.default_rng(600).uniform(-0.5, 0.5, size=len(v)).astype(np.float32)
    return v, t


# name -> (maker, the extent the case is smoothed with: a power of two above its coordinates - but for "bad", whose
# 3e30 is to saturate while the sheet keeps 31 fraction bits)
HAND_MADE = {"open_sheet": (open_sheet, 32.0), "fan300": (fan300, 8.0), "fans": (fans_case, 8.0), "bad": (bad_case, 64.0),
             "degree_limit": (degree_limit_case, 8.0)}
# (iterations, lam, mu, pin_border, max_move) the hand-made cases are smoothed with
HAND_RUNS = ((2, LAMBDA, MU, True, None), (2, LAMBDA, MU, False, 0.05))
