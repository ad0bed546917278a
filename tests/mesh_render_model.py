"""include/mi3d.h Part 17 in NumPy: the visibility buffer of a mesh and its shading - in binary32 with the header's
operation order (the restatement the GPU tests compare against bit for bit), or, with F = np.float64 and bounds=True, the
same definitions in binary64 together with first-order running bounds on what binary32 rounding can do to them (what
tests/test_mesh_render_cpu.py checks the restatement with).  Built on texture_views_model: its `project`, `_edge` and
`_pixels` are Part 15's projection, edge function, coverage test and depth, which Part 17 uses as they stand.

THE RUNNING BOUNDS (u = 2^-24), by the method of Part 15's "ERROR AGAINST EXACT ARITHMETIC": `project` gives E(x), E(y),
E(z) of every corner and `_edge` E(w_k) of every edge function.  On top of them, each operation adding its own rounding:
    s = (w0 + w1) + w2        E(s)   = sum E(w_k) + 2 u sum |w_k|
    b_k = w_k / s             E(b_k) = (E(w_k) + |b_k| E(s)) / |s| + u |b_k|
    r_k = b_k / z_k           E(r_k) = (E(b_k) + |r_k| E(z_k)) / |z_k| + u |r_k|
    S = (r0 + r1) + r2        E(S)   = sum E(r_k) + 2 u sum |r_k|
    d = 1 / S                 E(d)   = d^2 E(S) + u |d|
    l_k = r_k d               E(l_k) = |d| E(r_k) + |r_k| E(d) + u |l_k|
    a = (l0 a0 + l1 a1) + l2 a2    E(a) = sum |a_k| E(l_k) + 3 u sum |l_k a_k|       (two roundings per product chain and the
                                                                                       two of the sums, counted as 3 per term)
A pixel is UNDECIDED when some |w_k| <= 2 E(w_k): binary32 may decide its coverage the other way.

Not a test module: helpers only."""
import numpy as np

import texture_views_model as M

U = M.U
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _boxes(P, H, W, F):
    xs, ys = np.stack([P[k][0] for k in range(3)]), np.stack([P[k][1] for k in range(3)])
    xlo = np.maximum(np.ceil(xs.min(0) - F(0.5)), F(0))
    xhi = np.minimum(np.floor(xs.max(0) - F(0.5)), F(W - 1))
    ylo = np.maximum(np.ceil(ys.min(0) - F(0.5)), F(0))
    yhi = np.minimum(np.floor(ys.max(0) - F(0.5)), F(H - 1))
    some = (xlo <= xhi) & (ylo <= yhi)
    i0, j0 = np.where(some, xlo, 0).astype(np.int64), np.where(some, ylo, 0).astype(np.int64)
    wd = np.where(some, xhi - xlo + 1, 0).astype(np.int64)
    hg = np.where(some, yhi - ylo + 1, 0).astype(np.int64)
    return some, i0, j0, wd, hg


def visibility(vertices, triangles, records, H, W, F=np.float32):
    """The nearest triangle at every pixel centre: (depth [V, H, W] of dtype F, +inf where nothing is drawn; tri int64
    [V, H, W], -1 there; (bad, skipped) as mi3d_mesh_visibility counts them).  For every pixel `_pixels` writes, the
    candidates (d, triangle index) are ordered by depth, then by index - for F = np.float32 the order of the keys
    (bits(d) << 32) | index, since positive floats order like their bits."""
    vertices, triangles = np.asarray(vertices, np.float32), np.asarray(triangles)
    nv, V = len(vertices), len(records)
    ok = ((triangles >= 0) & (triangles < nv)).all(1) if len(triangles) else np.zeros(0, bool)
    bad, skipped = int((~ok).sum()), 0
    index = np.flatnonzero(ok)
    tri = triangles[ok].astype(np.int64)
    depth, winner = np.full((V, H * W), np.inf, F), np.full((V, H * W), -1, np.int64)
    pv = vertices.astype(F)
    for v in range(V):
        pr = M.project(records[v], pv, F)
        with np.errstate(invalid="ignore"):
            good = (pr[2] > 0) & np.isfinite(pr[0]) & np.isfinite(pr[1]) & np.isfinite(pr[2])
        drawn = good[tri].all(1) if len(tri) else np.zeros(0, bool)
        skipped += int((~drawn).sum())
        t, name = tri[drawn], index[drawn]
        if len(t) == 0:
            continue
        ids = [t[:, k] for k in range(3)]
        P = [tuple(pr[c][t[:, k]] for c in range(3)) for k in range(3)]
        some, i0, j0, wd, hg = _boxes(P, H, W, F)
        at, dd, who = [], [], []

        def put(m, ii, jj):
            write, d = M._pixels([i[m] for i in ids], [tuple(c[m] for c in p) for p in P], ii.astype(F) + F(0.5),
                                 jj.astype(F) + F(0.5), F)
            at.append((jj * W + ii)[write])
            dd.append(d[write])
            who.append((name[m] + 0 * ii)[write])

        small = some & (wd * hg <= M.BIG)
        n = np.flatnonzero(small)
        if len(n):
            for dj in range(int(hg[n].max())):
                for di in range(int(wd[n].max())):
                    m = n[(dj < hg[n]) & (di < wd[n])]
                    if len(m):
                        put(m, i0[m] + di, j0[m] + dj)
        for m in np.flatnonzero(some & ~small):
            jj, ii = np.meshgrid(np.arange(j0[m], j0[m] + hg[m]), np.arange(i0[m], i0[m] + wd[m]), indexing="ij")
            put(m, ii.ravel(), jj.ravel())
        at, dd, who = np.concatenate(at), np.concatenate(dd), np.concatenate(who)
        order = np.lexsort((who, dd, at))                       # by pixel, then depth, then triangle index
        at, dd, who = at[order], dd[order], who[order]
        first = np.ones(len(at), bool)
        first[1:] = at[1:] != at[:-1]
        depth[v][at[first]], winner[v][at[first]] = dd[first], who[first]
    return depth.reshape(V, H, W), winner.reshape(V, H, W), (bad, skipped)


def keys(depth, tri):
    """The uint64 keys of mi3d_mesh_visibility from visibility()'s binary32 depth and winner: all-ones where tri < 0."""
    bits = np.ascontiguousarray(depth, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(tri >= 0, (bits << np.uint64(32)) | np.maximum(tri, 0).astype(np.uint64), EMPTY)


def _mix(lam, a):
    """((l0 a0 + l1 a1) + l2 a2) for a = three arrays [n] or [n, c]."""
    ex = (lambda x, y: x[:, None] * y) if a[0].ndim == 2 else (lambda x, y: x * y)
    return (ex(lam[0], a[0]) + ex(lam[1], a[1])) + ex(lam[2], a[2])


def _tap(g, T, F):
    i0 = np.fmin(np.fmax(np.floor(g), F(0)), F(T - 2))
    f = np.fmin(np.fmax(g - i0, F(0)), F(1))
    return i0.astype(np.int64), f


def shade(vertices, triangles, records, H, W, tri, colors=None, vt=None, texture=None, vn=None, background=(1, 1, 1),
          F=np.float32, bounds=False):
    """mi3d_mesh_shade from the winners tri int64 [V, H, W] (-1: nothing drawn): a dict of image [V, H, W, 3], depth,
    tri int32, bary [V, H, W, 3], alpha uint8, normal (None without vn) of dtype F and, with a texture, gx, gy (the
    texel coordinates).  With bounds (F = np.float64) also `undecided` bool [V, H, W], `Ebary` [V, H, W, 3] and, with
    vt, `Euv` [V, H, W, 2]: the bounds of the module's header."""
    vertices, triangles = np.asarray(vertices, np.float32), np.asarray(triangles)
    V = len(records)
    out = dict(image=np.empty((V, H, W, 3), F), depth=np.full((V, H, W), np.inf, F), tri=tri.astype(np.int32),
               bary=np.zeros((V, H, W, 3), F), alpha=(tri >= 0).astype(np.uint8),
               normal=None if vn is None else np.zeros((V, H, W, 3), F))
    out["image"][:] = np.asarray(background, np.float32).astype(F)
    if texture is not None:
        out["gx"], out["gy"] = np.zeros((V, H, W), F), np.zeros((V, H, W), F)
    if bounds:
        out["undecided"], out["Ebary"] = np.zeros((V, H, W), bool), np.zeros((V, H, W, 3))
        out["Euv"] = np.zeros((V, H, W, 2))
    pv = vertices.astype(F)
    for v in range(V):
        jj, ii = np.nonzero(tri[v] >= 0)
        if len(jj) == 0:
            continue
        t = tri[v][jj, ii]
        idx = triangles[t].astype(np.int64)
        pr = M.project(records[v], pv, F, bounds)
        ids = [idx[:, k] for k in range(3)]
        P = [tuple(pr[c][idx[:, k]] for c in range(3)) for k in range(3)]
        E = [tuple(pr[3 + c][idx[:, k]] for c in range(3)) for k in range(3)] if bounds else None
        px, py = ii.astype(F) + F(0.5), jj.astype(F) + F(0.5)
        w, Ew = [], []
        for a, b in ((1, 2), (2, 0), (0, 1)):
            r = M._edge(ids[a], P[a][0], P[a][1], ids[b], P[b][0], P[b][1], px, py,
                        None if E is None else E[a], None if E is None else E[b])
            w.append(r[0] if bounds else r)
            if bounds:
                Ew.append(r[1])
        s = (w[0] + w[1]) + w[2]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            bk = [w[k] / s for k in range(3)]
            r = [bk[k] / P[k][2] for k in range(3)]
            S = (r[0] + r[1]) + r[2]
            d = F(1.0) / S
            lam = [r[k] * d for k in range(3)]
        out["depth"][v][jj, ii] = d
        out["bary"][v][jj, ii] = np.stack(lam, -1)
        if bounds:
            Es = Ew[0] + Ew[1] + Ew[2] + 2 * U * (abs(w[0]) + abs(w[1]) + abs(w[2]))
            Eb = [(Ew[k] + abs(bk[k]) * Es) / abs(s) + U * abs(bk[k]) for k in range(3)]
            Er = [(Eb[k] + abs(r[k]) * E[k][2]) / abs(P[k][2]) + U * abs(r[k]) for k in range(3)]
            ES = Er[0] + Er[1] + Er[2] + 2 * U * (abs(r[0]) + abs(r[1]) + abs(r[2]))
            Ed = d * d * ES + U * abs(d)
            El = [abs(d) * Er[k] + abs(r[k]) * Ed + U * abs(lam[k]) for k in range(3)]
            out["undecided"][v][jj, ii] = (abs(w[0]) <= 2 * Ew[0]) | (abs(w[1]) <= 2 * Ew[1]) | (abs(w[2]) <= 2 * Ew[2])
            out["Ebary"][v][jj, ii] = np.stack(El, -1)
        if colors is not None:
            c = np.asarray(colors, np.float32).astype(F)
            out["image"][v][jj, ii] = _mix(lam, [c[idx[:, k]] for k in range(3)])
        else:
            uv = np.asarray(vt, np.float32).astype(F).reshape(-1, 3, 2)[t]
            u, vv = _mix(lam, [uv[:, k, 0] for k in range(3)]), _mix(lam, [uv[:, k, 1] for k in range(3)])
            if bounds:
                out["Euv"][v][jj, ii] = np.stack(
                    [sum(abs(uv[:, k, c]) * El[k] + 3 * U * abs(lam[k] * uv[:, k, c]) for k in range(3)) for c in (0, 1)], -1)
                out["u"] = out.get("u", np.zeros((V, H, W)))
                out["v"] = out.get("v", np.zeros((V, H, W)))
                out["u"][v][jj, ii], out["v"][v][jj, ii] = u, vv
            T = len(texture)
            gx, gy = u * F(T) - F(0.5), (F(1.0) - vv) * F(T) - F(0.5)
            (i0, fx), (j0, fy) = _tap(gx, T, F), _tap(gy, T, F)
            hx, hy = F(1.0) - fx, F(1.0) - fy
            tex = np.asarray(texture).astype(F)
            c00, c10, c01, c11 = tex[j0, i0], tex[j0, i0 + 1], tex[j0 + 1, i0], tex[j0 + 1, i0 + 1]
            top = c00 * hx[:, None] + c10 * fx[:, None]
            bot = c01 * hx[:, None] + c11 * fx[:, None]
            out["image"][v][jj, ii] = (top * hy[:, None] + bot * fy[:, None]) / F(255.0)
            out["gx"][v][jj, ii], out["gy"][v][jj, ii] = gx, gy
        if vn is not None:
            n = np.asarray(vn, np.float32).astype(F)
            out["normal"][v][jj, ii] = _mix(lam, [n[idx[:, k]] for k in range(3)])
    return out


def render(vertices, triangles, records, H, W, F=np.float32, bounds=False, **source):
    """visibility() and shade() in one: shade's dict plus `vis` (the uint64 keys, binary32 only) and `counts`."""
    depth, tri, counts = visibility(vertices, triangles, records, H, W, F)
    out = shade(vertices, triangles, records, H, W, tri, F=F, bounds=bounds, **source)
    out["counts"] = counts
    if F == np.float32:
        out["vis"] = keys(depth, tri)
    out["vis_depth"] = depth
    return out
