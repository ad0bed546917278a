"""The area-adaptive atlas of include/mi3d.h Part 20 restated in NumPy float32 (no test in this file): measure, plan,
sort, ownership, UVs and the texel -> point map, written from the header's text and independent of csrc/.  The CPU tests
hold the library's host plan and ownership rule against it, the GPU tests every kernel output bit for bit.  Also the
meshes the tests build and the texel density a plan gives a mesh."""
import numpy as np

F = np.float32
LEGS = (2, 3, 4, 6, 8, 11, 16, 23, 32, 45, 64, 91, 128, 181, 256, 362)
PLAN_WORDS = 3472
GROUPS, RECORDS, INDEX = 16, 144, 3216


# ------------------------------------------------------------------------------------------------ meshes

def graded_plane():
    """Six rows of squares of side 0.5 * 2^-k over x in [-0.5, 0.5], stacked in y from -0.5, z = 0.1; every square split
    in two: 252 triangles with edge lengths spanning 32 x."""
    v, t, y = [], [], -0.5
    for k in range(6):
        side, n, base = 0.5 * 2.0 ** -k, 2 ** (k + 1), len(v)
        for j in range(2):
            for i in range(n + 1):
                v.append((-0.5 + i * side, y + j * side, 0.1))
        for i in range(n):
            a, b, c, d = base + i, base + i + 1, base + n + 1 + i + 1, base + n + 1 + i
            t += [(a, b, c), (a, c, d)]
        y += side
    return np.array(v, F), np.array(t, np.int32)


def latlong_sphere(nlon=64, nlat=32, radius=0.7):
    """nlon x nlat latitude-longitude sphere: 2 nlon (nlat - 1) triangles, slivers at the poles."""
    v = [(0.0, 0.0, radius)]
    for j in range(1, nlat):
        th = np.pi * j / nlat
        for i in range(nlon):
            ph = 2 * np.pi * i / nlon
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)))
    v.append((0.0, 0.0, -radius))
    ring = lambda j, i: 1 + (j - 1) * nlon + i % nlon
    t = [(0, ring(1, i), ring(1, i + 1)) for i in range(nlon)]
    for j in range(1, nlat - 1):
        for i in range(nlon):
            t += [(ring(j, i), ring(j + 1, i), ring(j + 1, i + 1)), (ring(j, i), ring(j + 1, i + 1), ring(j, i + 1))]
    last = len(v) - 1
    t += [(last, ring(nlat - 1, i + 1), ring(nlat - 1, i)) for i in range(nlon)]
    return np.array(v, F), np.array(t, np.int32)


# ------------------------------------------------------------------------------------------------ 1. measure

def bins_of(l):
    """The bin of binary32 squared lengths: biased exponent - 127 clamped to [-60, 3], + 60; exponent 0 or 255: 0."""
    e = ((np.ascontiguousarray(l, F).view(np.uint32) >> 23) & 0xff).astype(np.int64)
    return np.where((e == 0) | (e == 255), 0, np.clip(e - 127, -60, 3) + 60)


def measure(vertices, triangles):
    """-> (shape uint32 [nt], hist uint32 [64, 64] indexed [binAC, binAB], bad)."""
    vertices, t = np.ascontiguousarray(vertices, F), np.asarray(triangles, np.int64)
    nv = len(vertices)
    bad = ((t < 0) | (t >= nv)).any(1)
    p = vertices[np.where(bad[:, None], 0, t)]                         # [nt, 3, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        l = []
        for k in range(3):                                             # edge k: opposite corner k
            d = p[:, (k + 2) % 3] - p[:, (k + 1) % 3]
            l.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        assert all(x.dtype == F for x in l)
        rot = np.where(l[1] > l[0], 1, 0)
        longest = np.where(l[1] > l[0], l[1], l[0])
        rot = np.where(l[2] > longest, 2, rot)
    l = np.stack(l, 1)
    i = np.arange(len(t))
    binAB, binAC = bins_of(l[i, (rot + 2) % 3]), bins_of(l[i, (rot + 1) % 3])
    rot, binAB, binAC = (np.where(bad, 0, x) for x in (rot, binAB, binAC))
    shape = (rot | (binAB << 8) | (binAC << 16) | (bad.astype(np.int64) << 31)).astype(np.uint32)
    hist = np.zeros((64, 64), np.uint32)
    np.add.at(hist, (binAC, binAB), 1)
    return shape, hist, int(bad.sum())


# ------------------------------------------------------------------------------------------------ 2. plan

def kmax_of(T):
    return max(k for k in range(16) if LEGS[k] + 3 <= T)


def classes_of(hist, s, kmax):
    """-> (count int64 [16, 16] indexed [kb, ka], legs clamped at the smallest class, legs clamped at the largest)."""
    count, lo, hi = np.zeros((16, 16), np.int64), 0, 0
    for bc, bb in zip(*np.nonzero(hist)):
        n = int(hist[bc, bb])
        count[min(max(bc - s, 0), kmax), min(max(bb - s, 0), kmax)] += n
        for b in (bb, bc):
            lo += n if b - s < 0 else 0
            hi += n if b - s > kmax else 0
    return count, lo, hi


def shelves(count, T):
    """Shelf packing, cell by cell as the header words it -> (rows used, groups, records)."""
    y, groups, records = 0, [], []
    for kb in range(15, -1, -1):
        if not count[kb].any():
            continue
        h, shelf, x, first = LEGS[kb] + 3, 0, 0, len(records)
        for ka in range(15, -1, -1):
            n = int(count[kb, ka])
            if n == 0:
                continue
            w, cells = LEGS[ka] + 3, (n + 1) // 2
            if T - x < w:
                shelf, x = shelf + 1, 0
            records.append(dict(key=kb * 16 + ka, a=LEGS[ka], b=LEGS[kb], x0=x, shelf0=shelf, n0=(T - x) // w, per=T // w,
                                count=n, y0=y, cells=cells))
            for _ in range(cells):                                     # one cell at a time
                if T - x < w:
                    shelf, x = shelf + 1, 0
                x += w
        groups.append(dict(y0=y, h=h, shelves=shelf + 1, first=first, count=len(records) - first, kb=kb))
        y += (shelf + 1) * h
    return y, groups, records


def plan(hist, T):
    """The plan for a bin histogram [64, 64] and T, or None: a dict with the flat int32 array of the header's layout
    under "words"."""
    hist = np.asarray(hist)
    nt = int(hist.astype(np.int64).sum())
    if not 64 <= T <= 16384 or nt == 0 or nt > 2 ** 31 - 1:
        return None
    kmax = kmax_of(T)
    for s in range(64):
        count, lo, hi = classes_of(hist, s, kmax)
        rows, groups, records = shelves(count, T)
        if rows <= T:
            break
    else:
        return None
    start, by_key = 0, {r["key"]: r for r in records}
    owned = 0
    for key in sorted(by_key):
        r = by_key[key]
        r["start"], start = start, start + r["count"]
        owned += r["count"] * int(half0_mask(r["a"], r["b"]).sum())
    words = np.zeros(PLAN_WORDS, np.int32)
    words[INDEX:] = -1
    words[:10] = [s, T, kmax, rows, len(groups), len(records), nt, owned, lo, hi]
    for g, gr in enumerate(groups):
        words[GROUPS + 8 * g:GROUPS + 8 * g + 6] = [gr["y0"], gr["h"], gr["shelves"], gr["first"], gr["count"], gr["kb"]]
    for j, r in enumerate(records):
        words[RECORDS + 12 * j:RECORDS + 12 * j + 11] = [r["key"], r["a"], r["b"], r["x0"], r["shelf0"], r["n0"], r["per"],
                                                         r["count"], r["start"], r["y0"], r["cells"]]
        words[INDEX + r["key"]] = j
    return dict(shift=s, T=T, kmax=kmax, rows=rows, groups=groups, records=records, by_key=by_key, nt=nt, owned=owned,
                clamped_small=lo, clamped_large=hi, classes=count, words=words)


def cell_origin(r, q):
    """Top-left texel (X0, Y0) of cells q (an array) of class record r."""
    q = np.asarray(q, np.int64)
    w, h = r["a"] + 3, r["b"] + 3
    rest = np.maximum(q - r["n0"], 0)
    first = q < r["n0"]
    X0 = np.where(first, r["x0"] + q * w, (rest % r["per"]) * w)
    Y0 = r["y0"] + np.where(first, r["shelf0"], r["shelf0"] + 1 + rest // r["per"]) * h
    return X0, Y0


# ------------------------------------------------------------------------------------------------ 3. sort

def keys_of(shape, s, kmax):
    binAB, binAC = (shape.astype(np.int64) >> 8) & 63, (shape.astype(np.int64) >> 16) & 63
    return np.clip(binAC - s, 0, kmax) * 16 + np.clip(binAB - s, 0, kmax)


def sort(shape, p):
    """-> (slot uint32 [nt], triangle_of uint32 [nt]): stable by key."""
    triangle_of = np.argsort(keys_of(shape, p["shift"], p["kmax"]), kind="stable")
    slot = np.empty(len(shape), np.int64)
    slot[triangle_of] = np.arange(len(shape))
    return slot.astype(np.uint32), triangle_of.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ 4. ownership, UVs

def half0_mask(a, b):
    """bool [b + 3, a + 3] indexed [y, x]: the texels half 0 owns."""
    y, x = np.meshgrid(np.arange(b + 3), np.arange(a + 3), indexing="ij")
    return (x <= a) & (y <= b) & (b * np.maximum(x - 1, 0) + a * np.maximum(y - 1, 0) < a * b)


def half1_mask(a, b):
    return half0_mask(a, b)[::-1, ::-1]


def bilinear_footprint(a, b):
    """bool [b + 3, a + 3]: the texels a bilinear lookup touches with non-zero weight at some point of the closed UV
    triangle with corners at the centres of texels (0, 0), (a, 0), (0, b) - by sampling, in exact integers.

    Coordinates are counted in units of 1 / S, S = 4 a b.  The sample points are, per axis and per integer c, c itself,
    c + 1 / S and c + 1 / 2, kept where they lie in the closed triangle (b x + a y <= a b).  A point's taps are the texels
    floor and floor + 1 per axis, the latter only with a non-zero fraction.  The samples miss nothing: the taps are the
    same for every interior point of a unit square of the texel lattice, and a unit square whose interior meets the
    triangle has its lower left corner (cx, cy) with b cx + a cy <= a b - 1, so that (cx + 1 / S, cy + 1 / S) lies in
    the triangle; points on lattice lines only touch subsets of what a neighbouring interior point touches."""
    S = 4 * a * b
    px = np.array([c * S + e for c in range(a + 1) for e in (0, 1, S // 2)], np.int64)
    py = np.array([c * S + e for c in range(b + 1) for e in (0, 1, S // 2)], np.int64)
    Y, X = np.meshgrid(py, px, indexing="ij")
    inside = (X <= a * S) & (Y <= b * S) & (b * X + a * Y <= a * b * S)
    X, Y = X[inside], Y[inside]
    m = np.zeros((b + 3, a + 3), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            weight = np.where(dx, X % S, S - X % S) * np.where(dy, Y % S, S - Y % S)
            m[(Y // S + dy)[weight > 0], (X // S + dx)[weight > 0]] = True
    return m


def layout(vertices, triangles, T, ssaa, p=None):
    """Steps 1 - 5 -> dict(shape, hist, bad, plan, slot, triangle_of, vt [3 nt, 2], owner [T, T], xyz [T, T, ssaa^2, 3]),
    or None when no shift fits."""
    vertices, triangles = np.ascontiguousarray(vertices, F), np.asarray(triangles, np.int64)
    nt, nv = len(triangles), len(vertices)
    shape, hist, bad = measure(vertices, triangles)
    p = plan(hist, T) if p is None else p
    if p is None:
        return None
    slot, triangle_of = sort(shape, p)
    keys, rot = keys_of(shape, p["shift"], p["kmax"]), (shape & 3).astype(np.int64)
    is_bad = (shape >> 31).astype(bool)
    vt = np.zeros((nt, 3, 2), F)
    owner = np.full((T, T), -1, np.int32)
    xyz = np.zeros((T, T, ssaa * ssaa, 3), F)
    for key, r in p["by_key"].items():
        a, b = r["a"], r["b"]
        tri = np.flatnonzero(keys == key)
        rank = slot[tri].astype(np.int64) - r["start"]
        assert len(tri) == r["count"] and rank.min() >= 0 and rank.max() < r["count"]
        X0, Y0 = cell_origin(r, rank // 2)
        half = (rank & 1).astype(bool)
        for k in range(3):                                             # row 3 i + k: the ORIGINAL corner k
            j = (k - rot[tri]) % 3
            lx, ly = np.where(j == 1, a, 0), np.where(j == 2, b, 0)
            x, y = np.where(half, a + 2 - lx, lx), np.where(half, b + 2 - ly, ly)
            vt[tri, k, 0] = ((X0 + x).astype(F) + F(0.5)) / F(T)
            vt[tri, k, 1] = F(1.0) - ((Y0 + y).astype(F) + F(0.5)) / F(T)
        for h, mask in ((0, half0_mask(a, b)), (1, half1_mask(a, b))):
            sel = (half == bool(h)) & ~is_bad[tri]
            if not sel.any():
                continue
            ys, xs = np.nonzero(mask)                                  # local texels of the half
            u, v = (a + 2 - xs, b + 2 - ys) if h else (xs, ys)
            t, gx, gy = tri[sel], X0[sel][:, None] + xs, Y0[sel][:, None] + ys
            assert (owner[gy, gx] == -1).all()                         # cells and halves are disjoint
            owner[gy, gx] = t[:, None]
            ids = triangles[t]
            r_ = rot[t]
            n = np.arange(len(t))
            A, B, C = (vertices[ids[n, (r_ + c) % 3]] for c in range(3))
            e1, e2 = (B - A)[:, None, :], (C - A)[:, None, :]
            with np.errstate(invalid="ignore", over="ignore"):
                for j in range(ssaa):
                    for i in range(ssaa):
                        s = (u.astype(F) + F((i + 0.5) / ssaa - 0.5)) / F(a)
                        tt = (v.astype(F) + F((j + 0.5) / ssaa - 0.5)) / F(b)
                        q = (A[:, None, :] + s[None, :, None] * e1) + tt[None, :, None] * e2
                        assert q.dtype == F
                        xyz[gy, gx, j * ssaa + i] = np.fmin(np.fmax(q, F(-1)), F(1))      # fmax, fmin: NaN -> -1
    assert nv > 0
    return dict(shape=shape, hist=hist, bad=bad, plan=p, slot=slot, triangle_of=triangle_of, vt=vt.reshape(-1, 2),
                owner=owner, xyz=xyz)


# ------------------------------------------------------------------------------------------------ density

def densities(vertices, triangles, shape, p):
    """Texels per unit length along A'B' and A'C' of every triangle, [nt, 2] float64, and which of them are clamped
    (bin - s outside [0, kmax]) [nt, 2] bool."""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    rot = (shape & 3).astype(np.int64)
    i = np.arange(len(t))
    A, B, C = (v[t[i, (rot + c) % 3]] for c in range(3))
    bins = np.stack([(shape.astype(np.int64) >> 8) & 63, (shape.astype(np.int64) >> 16) & 63], 1) - p["shift"]
    legs = np.array(LEGS)[np.clip(bins, 0, p["kmax"])]
    lengths = np.stack([np.linalg.norm(B - A, axis=1), np.linalg.norm(C - A, axis=1)], 1)
    return legs / lengths, (bins < 0) | (bins > p["kmax"])


# ------------------------------------------------------------------------------------------------ reading a texture back

def surface_samples(vertices, triangles, n, seed):
    """n area-weighted random surface points: (triangle index [n], barycentric weights [n, 3], points [n, 3]), float64."""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    p = v[t]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    rng = np.random.default_rng(seed)
    tri = rng.choice(len(t), size=n, p=area / area.sum())
    w = rng.dirichlet(np.ones(3), size=n)
    return tri, w, np.einsum("nb,nbd->nd", w, p[tri])


def bilinear_lookup(image, vt, tri, w):
    """The texture read through vt at barycentric weights w of triangles tri, as a renderer reads it: gx = u T - 0.5,
    gy = (1 - v) T - 0.5, four taps clamped to the image; float64 [n, 3] in [0, 1]."""
    T = image.shape[0]
    uv = np.einsum("nb,nbd->nd", w, np.asarray(vt, np.float64).reshape(-1, 3, 2)[tri])
    gx, gy = uv[:, 0] * T - 0.5, (1.0 - uv[:, 1]) * T - 0.5
    i0, j0 = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64)
    fx, fy = (gx - i0)[:, None], (gy - j0)[:, None]
    tap = lambda j, i: image[np.clip(j, 0, T - 1), np.clip(i, 0, T - 1)].astype(np.float64)
    top = tap(j0, i0) * (1 - fx) + tap(j0, i0 + 1) * fx
    bot = tap(j0 + 1, i0) * (1 - fx) + tap(j0 + 1, i0 + 1) * fx
    return (top * (1 - fy) + bot * fy) / 255.0


def stripes(points, frequency=20.0):
    """The analytic albedo of the sharpness test: 0.5 + 0.5 sin(2 pi f x) per coordinate."""
    return 0.5 + 0.5 * np.sin(2.0 * np.pi * frequency * np.asarray(points, np.float64))
