"""include/mi3d.h Part 15 in NumPy: the view records, the depth maps of a mesh, and per atlas sample the colour and the
hit count of the projection - in binary32 with the header's operation order (the restatement the GPU tests compare
against bit for bit), or, with F = np.float64, the same definitions in binary64 together with first-order running
bounds on what binary32 rounding can do to them (what tests/test_texture_views_cpu.py checks the restatement with).

Not a test module: helpers only."""
import numpy as np

U = 2.0 ** -24          # the unit roundoff of binary32
BIG = 64                # a bounding box of more pixels than this is walked on its own, smaller ones in batches


def view_records(c2w, K):
    """float32 [V, 24]: rows of [R | t] of inv(c2w) (binary64 inverse), K, the camera centre; each rounded once."""
    c2w, K = np.asarray(c2w, np.float64), np.asarray(K, np.float64)
    rec = np.empty((len(c2w), 24))
    for v, pose in enumerate(c2w):
        w2c = np.linalg.inv(pose)
        rec[v] = np.concatenate([w2c[:3, :3].ravel(), w2c[:3, 3], K.ravel(), pose[:3, 3]])
    return rec.astype(np.float32)


def project(rec, p, F=np.float32, bounds=False):
    """One view record, points p [n, 3] of dtype F -> (x, y, z); with bounds also (Ex, Ey, Ez), the first-order bounds
    on the binary32 results' errors: 4 roundings per component of cam, 4 more per q, one per division."""
    rec = rec.astype(F)
    R, t, K = rec[:9].reshape(3, 3), rec[9:12], rec[12:21].reshape(3, 3)
    cam = [((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)]
    q = [(K[r, 0] * cam[0] + K[r, 1] * cam[1]) + K[r, 2] * cam[2] for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x, y, z = q[0] / q[2], q[1] / q[2], q[2]
        if not bounds:
            return x, y, z
        Ecam = [4 * U * (abs(R[r, 0] * p[:, 0]) + abs(R[r, 1] * p[:, 1]) + abs(R[r, 2] * p[:, 2]) + abs(t[r]))
                for r in range(3)]
        Eq = [4 * U * sum(abs(K[r, k] * cam[k]) for k in range(3)) + sum(abs(K[r, k]) * Ecam[k] for k in range(3))
              for r in range(3)]
        Ex = U * abs(x) + (Eq[0] + abs(x) * Eq[2]) / abs(z)
        Ey = U * abs(y) + (Eq[1] + abs(y) * Eq[2]) / abs(z)
    return x, y, z, Ex, Ey, Eq[2]


def _edge(ia, ax, ay, ib, bx, by, px, py, Ea=None, Eb=None):
    """The edge function of a -> b with the watertight rule; with Ea = (Ex, Ey) of a and Eb of b also its error bound."""
    fwd = ia <= ib
    lx, ly, hx, hy = np.where(fwd, ax, bx), np.where(fwd, ay, by), np.where(fwd, bx, ax), np.where(fwd, by, ay)
    a, b, c, d = hx - lx, py - ly, hy - ly, px - lx
    e = a * b - c * d
    e = np.where(fwd, e, -e)
    if Ea is None:
        return e
    Elx, Ely = np.where(fwd, Ea[0], Eb[0]), np.where(fwd, Ea[1], Eb[1])
    Ehx, Ehy = np.where(fwd, Eb[0], Ea[0]), np.where(fwd, Eb[1], Ea[1])
    EA, EB, EC, ED = Ehx + Elx + U * abs(a), Ely + U * abs(b), Ehy + Ely + U * abs(c), Elx + U * abs(d)
    return e, abs(a) * EB + abs(b) * EA + abs(c) * ED + abs(d) * EC + U * (abs(a * b) + abs(c * d)) + U * abs(e)


def _pixels(ids, P, px, py, F, E=None):
    """Coverage and depth of triangles at pixel centres (shapes broadcast).  ids: 3 index arrays; P: 3 x (x, y, z);
    E: 3 x (Ex, Ey, Ez) or None.  Returns (write, depth) and with E also (maybe, surely, depth error, lowest depth):
    covered for some / for every perturbation of the edge functions within their bounds."""
    w, Ew = [], []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        r = _edge(ids[a], P[a][0], P[a][1], ids[b], P[b][0], P[b][1], px, py,
                  None if E is None else E[a], None if E is None else E[b])
        if E is None:
            w.append(r)
        else:
            w.append(r[0])
            Ew.append(r[1])
    covered = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
    s = (w[0] + w[1]) + w[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = [(w[k] / s) / P[k][2] for k in range(3)]
        S = (t[0] + t[1]) + t[2]
        d = F(1.0) / S
        write = covered & (s != 0) & (d > 0) & np.isfinite(d)
        if E is None:
            return write, d
        maybe = ((w[0] >= -Ew[0]) & (w[1] >= -Ew[1]) & (w[2] >= -Ew[2])) | \
                ((w[0] <= Ew[0]) & (w[1] <= Ew[1]) & (w[2] <= Ew[2]))
        surely = ((w[0] > Ew[0]) & (w[1] > Ew[1]) & (w[2] > Ew[2])) | ((w[0] < -Ew[0]) & (w[1] < -Ew[1]) & (w[2] < -Ew[2]))
        Es = Ew[0] + Ew[1] + Ew[2] + 2 * U * (abs(w[0]) + abs(w[1]) + abs(w[2]))
        # the b_k = w_k / s sum to 1 up to their own roundings whatever the errors of the w_k, so an error of b_k moves
        # S = sum b_k / z_k only through 1 / z_k - 1 / z_0; the roundings of b_k, t_k and the two sums are 6 u sum |t_k|
        ES = 6 * U * (abs(t[0]) + abs(t[1]) + abs(t[2]))
        for k in range(3):
            bk = w[k] / s
            Eb = (Ew[k] + abs(bk) * Es) / abs(s)
            ES = ES + Eb * abs(F(1.0) / P[k][2] - F(1.0) / P[0][2]) + abs(bk) * E[k][2] / (P[k][2] * P[k][2])
        Ed = d * d * ES + U * abs(d)
        valid = (d > 0) & np.isfinite(d)
        usable = valid & np.isfinite(Ed)
        surely = surely & usable
        # one edge in doubt, the two others surely of one sign: the triangle across that edge (the same two indices) sees
        # exactly the opposite value, so if it stands on the other side the two of them surely cover the pixel together
        doubt = [abs(w[k]) <= Ew[k] for k in range(3)]
        pos, neg = [w[k] > Ew[k] for k in range(3)], [w[k] < -Ew[k] for k in range(3)]
        edge, sign = np.full(np.shape(d), -1), np.zeros(np.shape(d), np.int64)
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            one = doubt[k] & usable & ((pos[a] & pos[b]) | (neg[a] & neg[b]))
            edge, sign = np.where(one, k, edge), np.where(one, np.where(pos[a], 1, -1), sign)
        # a covered pixel's depth is a convex combination of the vertices' (the b_k of one sign, each at most 1): where the
        # error bound of d is of no use (s next to 0) the lowest vertex depth still bounds it from below
        zlow = np.minimum(np.minimum(P[0][2], P[1][2]), P[2][2]) * (1 - 8 * U) + 0 * d
    return write, d, maybe, surely, np.where(usable, Ed, 0.0), np.where(usable, d, zlow), edge, sign


def depth_maps(vertices, triangles, records, H, W, F=np.float32, bounds=False):
    """depth [V, H, W] of dtype F (+inf: nothing drawn) and (bad, skipped) as mi3d_mesh_depth counts them.  With bounds
    (F = np.float64) also `doubtful` bool [V, H, W] - a pixel where binary32 rounding could change WHETHER anything
    is drawn - and `err` [V, H, W], a bound on the binary32 depth's error there: the largest bound of the triangles
    that may cover the pixel, plus the gap between the nearest that may and the nearest that surely does."""
    vertices, triangles = np.asarray(vertices, np.float32), np.asarray(triangles)
    nv, V = len(vertices), len(records)
    ok = ((triangles >= 0) & (triangles < nv)).all(1) if len(triangles) else np.zeros(0, bool)
    bad, skipped = int((~ok).sum()), 0
    tri = triangles[ok].astype(np.int64)
    depth = np.full((V, H * W), np.inf, F)
    lowest, surest, err = np.full((V, H * W), np.inf), np.full((V, H * W), np.inf), np.zeros((V, H * W))
    pv = vertices.astype(F)
    for v in range(V):
        pr = project(records[v], pv, F, bounds)
        with np.errstate(invalid="ignore"):
            good = (pr[2] > 0) & np.isfinite(pr[0]) & np.isfinite(pr[1]) & np.isfinite(pr[2])
        drawn = good[tri].all(1) if len(tri) else np.zeros(0, bool)
        skipped += int((~drawn).sum())
        t = tri[drawn]
        if len(t) == 0:
            continue
        ids = [t[:, k] for k in range(3)]
        P = [tuple(pr[c][t[:, k]] for c in range(3)) for k in range(3)]
        E = [tuple(pr[3 + c][t[:, k]] for c in range(3)) for k in range(3)] if bounds else None
        xs, ys = np.stack([P[k][0] for k in range(3)]), np.stack([P[k][1] for k in range(3)])
        xlo = np.maximum(np.ceil(xs.min(0) - F(0.5)), F(0))
        xhi = np.minimum(np.floor(xs.max(0) - F(0.5)), F(W - 1))
        ylo = np.maximum(np.ceil(ys.min(0) - F(0.5)), F(0))
        yhi = np.minimum(np.floor(ys.max(0) - F(0.5)), F(H - 1))
        some = (xlo <= xhi) & (ylo <= yhi)
        i0, j0 = np.where(some, xlo, 0).astype(np.int64), np.where(some, ylo, 0).astype(np.int64)
        wd = np.where(some, xhi - xlo + 1, 0).astype(np.int64)
        hg = np.where(some, yhi - ylo + 1, 0).astype(np.int64)

        def put(sel, ii, jj, res):
            at = (jj * W + ii)[res[0]]
            np.minimum.at(depth[v], at, res[1][res[0]])
            if bounds:                                          # the binary32 depth lies in [lowest - err, surest + err]
                np.minimum.at(lowest[v], (jj * W + ii)[res[2]], res[5][res[2]])
                np.minimum.at(surest[v], (jj * W + ii)[res[3]], res[1][res[3]])
                np.maximum.at(err[v], (jj * W + ii)[res[2]], res[4][res[2]])
                one = res[6] >= 0
                if one.any():
                    a, b = (res[6][one] + 1) % 3, (res[6][one] + 2) % 3
                    tri3 = np.stack([ids[k][sel] + 0 * ii for k in range(3)], 1)[one]
                    ia, ib = tri3[np.arange(len(a)), a], tri3[np.arange(len(a)), b]
                    shared.append(np.stack([(jj * W + ii)[one], np.minimum(ia, ib), np.maximum(ia, ib), res[7][one]], 1))
                    shared_d.append(res[1][one])

        shared, shared_d = [], []
        small = some & (wd * hg <= BIG)
        n = np.flatnonzero(small)
        if len(n):
            for dj in range(int(hg[n].max())):
                for di in range(int(wd[n].max())):
                    m = n[(dj < hg[n]) & (di < wd[n])]
                    if len(m) == 0:
                        continue
                    ii, jj = i0[m] + di, j0[m] + dj
                    res = _pixels([i[m] for i in ids], [tuple(c[m] for c in p) for p in P], ii.astype(F) + F(0.5),
                                  jj.astype(F) + F(0.5), F, None if E is None else [tuple(c[m] for c in e) for e in E])
                    put(m, ii, jj, res)
        for m in np.flatnonzero(some & ~small):
            jj, ii = np.meshgrid(np.arange(j0[m], j0[m] + hg[m]), np.arange(i0[m], i0[m] + wd[m]), indexing="ij")
            jj, ii = jj.ravel(), ii.ravel()
            res = _pixels([i[m] for i in ids], [tuple(c[m] for c in p) for p in P], ii.astype(F) + F(0.5),
                          jj.astype(F) + F(0.5), F, None if E is None else [tuple(c[m] for c in e) for e in E])
            put(m, ii, jj, res)
        if shared:
            key, dd = np.concatenate(shared), np.concatenate(shared_d)
            _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)       # the sign is in the key
            inv = inv.ravel()
            far = np.full(len(cnt), -np.inf)
            np.maximum.at(far, inv, dd)
            two = cnt[inv] == 2
            np.minimum.at(surest[v], key[two, 0], far[inv][two])
    depth = depth.reshape(V, H, W)
    if bounds:
        with np.errstate(invalid="ignore"):
            doubtful = np.isfinite(surest) != np.isfinite(lowest)
            err = np.where(np.isfinite(surest), err + (surest - lowest), err)
        doubtful |= ~np.isfinite(err)
        return depth, (bad, skipped), doubtful.reshape(V, H, W), np.where(np.isfinite(err), err, 0).reshape(V, H, W)
    return depth, (bad, skipped)


def project_views(xyz, owner, vertices, triangles, records, H, W, depth, images, masks, weights, power, min_cos2,
                  depth_tol, base, F=np.float32, bounds=None):
    """Per sample: xyz [n, 3] float32, owner [n] (the owner triangle of the sample's texel, -1: none).  depth [V, H, W] of
    dtype F, images float32 [V, H, W, 3], masks uint8 [V, H, W] or None, weights float32 [V], base float32 [n, 3].
    Returns (colour [n, 3] of dtype F, hits uint8 [n]).  With bounds = (doubtful, err) of depth_maps (F = np.float64) also
    `undecided` bool [n] - some comparison in (b), (c) or (e) lies within twice its error bound - and `Ecol` [n], twice
    the first-order bound on the binary32 colour's error."""
    xyz, vertices, triangles = np.asarray(xyz, np.float32), np.asarray(vertices, np.float32), np.asarray(triangles)
    n, V, nv, nt = len(xyz), len(records), len(vertices), len(triangles)
    owner = np.asarray(owner).astype(np.int64)
    has = (owner >= 0) & (owner < nt)
    tri = triangles[np.where(has, owner, 0)].astype(np.int64)
    has &= ((tri >= 0) & (tri < nv)).all(1)
    tri = np.where(has[:, None], tri, 0)
    A, B, C = (vertices[tri[:, k]].astype(F) for k in range(3))
    e1, e2 = B - A, C - A
    N = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
         e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
    nn = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
    live = has & (nn > 0) & np.isfinite(nn)
    p = xyz.astype(F)
    sw, sc, hits = np.zeros(n, F), np.zeros((n, 3), F), np.zeros(n, np.int64)
    tol, mc2 = F(np.float32(depth_tol)), F(np.float32(min_cos2))
    if bounds is not None:
        doubtful, derr = bounds
        EN = [4 * U * (abs(e1[:, (k + 1) % 3] * e2[:, (k + 2) % 3]) + abs(e1[:, (k + 2) % 3] * e2[:, (k + 1) % 3]))
              for k in range(3)]
        Enn = sum(2 * abs(N[k]) * EN[k] for k in range(3)) + 3 * U * nn
        undecided, Ec, Ew = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for v in range(V):
            rec = records[v].astype(F)
            pr = project(records[v], p, F, bounds is not None)
            x, y, z = pr[:3]
            inb = (x >= F(0.5)) & (x <= F(W) - F(0.5)) & (y >= F(0.5)) & (y <= F(H) - F(0.5))
            ok = live & (z > 0) & inb
            gx, gy = x - F(0.5), y - F(0.5)
            i0 = np.minimum(np.floor(np.where(ok, gx, 0)).astype(np.int64), W - 2)
            j0 = np.minimum(np.floor(np.where(ok, gy, 0)).astype(np.int64), H - 2)
            taps = [depth[v][j0 + b, i0 + a] for b in (0, 1) for a in (0, 1)]               # d00 d10 d01 d11
            fin = np.isfinite(taps[0]) & np.isfinite(taps[1]) & np.isfinite(taps[2]) & np.isfinite(taps[3])
            m4 = np.minimum(np.minimum(taps[0], taps[1]), np.minimum(taps[2], taps[3]))
            ok_c = fin & (z <= m4 + tol)
            ok_d = np.ones(n, bool)
            if masks is not None:
                for b in (0, 1):
                    for a in (0, 1):
                        ok_d &= masks[v][j0 + b, i0 + a] != 0
            d = [rec[21 + k] - p[:, k] for k in range(3)]
            nd = (N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]
            dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            cos2 = (nd * nd) / (nn * dd)
            ok_e = (nd > 0) & (cos2 >= mc2)
            c = ok & ok_c & ok_d & ok_e
            cp = cos2
            e = 2
            while e < power:
                cp = cp * cp
                e *= 2
            w = F(weights[v]) * cp
            fx, fy = gx - i0.astype(F), gy - j0.astype(F)
            hx, hy = F(1.0) - fx, F(1.0) - fy
            img = images[v].astype(F)
            c00, c10, c01, c11 = img[j0, i0], img[j0, i0 + 1], img[j0 + 1, i0], img[j0 + 1, i0 + 1]
            top = c00 * hx[:, None] + c10 * fx[:, None]
            bot = c01 * hx[:, None] + c11 * fx[:, None]
            col = top * hy[:, None] + bot * fy[:, None]
            sw = np.where(c, sw + w, sw)
            sc = np.where(c[:, None], sc + w[:, None] * col, sc)
            hits += c
            if bounds is not None:
                Ex, Ey, Ez = pr[3:]
                front = live & (z > 2 * Ez)
                u = live & (abs(z) <= 2 * Ez)
                for g, E, hi in ((x, Ex, W - 0.5), (y, Ey, H - 0.5)):
                    Eg = 2 * (E + U * abs(g))
                    u |= front & ((abs(g - 0.5) <= Eg) | (abs(g - hi) <= Eg))
                    u |= front & inb & (abs((g - 0.5) - np.rint(g - 0.5)) <= Eg)            # the choice of the taps
                tap_doubt = np.zeros(n, bool)
                tap_err = np.zeros(n)
                for b in (0, 1):
                    for a in (0, 1):
                        tap_doubt |= doubtful[v][j0 + b, i0 + a]
                        tap_err = np.maximum(tap_err, derr[v][j0 + b, i0 + a])
                Ecmp = 2 * (Ez + tap_err + 2 * U * (abs(m4) + tol))
                u |= ok & (tap_doubt | (fin & (abs(z - (m4 + tol)) <= Ecmp)))
                End = sum(EN[k] * abs(d[k]) for k in range(3)) + 4 * U * sum(abs(N[k] * d[k]) for k in range(3))
                rel = 2 * End / abs(nd) + Enn / nn + 5 * U + 3 * U
                u |= live & ((abs(nd) <= 2 * End) | ((nd > 0) & (abs(cos2 - mc2) <= 2 * cos2 * rel)))
                undecided |= u
                Ec = np.where(c, np.maximum(Ec, (Ex + Ey) + 2 * U * (abs(x) + abs(y) + 1) + 8 * U), Ec)
                Ew = np.where(c, np.maximum(Ew, (power // 2) * (rel + U) + 2 * U), Ew)
        seen = sw > 0
        colour = np.where(seen[:, None], sc / sw[:, None], np.asarray(base, np.float32).astype(F))
    hits = hits.astype(np.uint8)
    if bounds is None:
        return colour, hits
    return colour, hits, undecided, 2 * (Ec + 2 * Ew + (2 * V + 6) * U)


def pack(colour, owner, ssaa):
    """mi3d_texture_pack: colour float32 [T, T, ssaa^2, 3], owner [T, T] -> uint8 [T, T, 3]."""
    F = np.float32
    colour = np.asarray(colour, F)
    s = colour[:, :, 0]
    for k in range(1, ssaa * ssaa):
        s = s + colour[:, :, k]
    a = s * F(1.0 / (ssaa * ssaa))
    with np.errstate(invalid="ignore"):
        v = a * F(255)
        q = np.where(v >= 255, 255, np.where(v >= 0, np.floor(v), 0)).astype(np.uint8)
    return np.where((np.asarray(owner) >= 0)[:, :, None], q, 0).astype(np.uint8)


def orbit(V, radius=2.4, elevation=0.3, start=0.0):
    """c2w [V, 4, 4] float64 of cameras on a circle, looking at the origin: camera +z forward, +x right, +y down (the
    convention of pointcloud.project: x to the right, y downwards in the image, z the depth)."""
    out = []
    for k in range(V):
        a = start + 2 * np.pi * k / V
        eye = radius * np.array([np.cos(a) * np.cos(elevation), np.sin(a) * np.cos(elevation), np.sin(elevation)])
        out.append(look_at(eye))
    return np.stack(out)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    if np.linalg.norm(r) < 1e-9:
        r = np.cross(f, (0.0, 1.0, 0.0))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    return c2w


def pinhole(focal, H, W):
    """pointcloud.intrinsics with a normalised focal length."""
    return np.array([[focal * W, 0, 0.5 * W], [0, focal * H, 0.5 * H], [0, 0, 1]], np.float64)
