"""A NumPy restatement of include/mi3d.h Part 13 (mesh components and the floater filter), for tests/test_mesh_clean_cpu.py
and tests/test_mesh_clean_gpu.py: the yardstick the kernels of csrc/meshclean.hip are compared with, exactly - integer
arrays equal, float rows bit-identical.  Written from the header's contract, sequential and slow on purpose: a union-find
with one Python step per triangle, no device code read."""
import numpy as np


def float_key(x):
    """The order-preserving integer image of binary32: a < b as floats <=> key(a) < key(b) as uint32; -0 below +0."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_float(k):
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def valid_triangles(triangles, nv):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < nv)).all(1)


def components(vertices, triangles):
    """(label int32 [nv], faces int32 [nv], box_min float32 [nv, 3], box_max float32 [nv, 3], bad): per-component values at
    the row of the label vertex, 0 in every other row; `bad` = the triangles with an index outside [0, nv)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    nv = len(v)
    ok = valid_triangles(t, nv)
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in t[ok].tolist():
        for other in (b, c):
            ra, rb = find(a), find(other)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)       # the smaller index stays the root: label = the minimum
    label = np.array([find(x) for x in range(nv)], np.int64).reshape(nv)
    faces = np.zeros(nv, np.int64)
    np.add.at(faces, label[t[ok, 0]], 1)

    keys, num = float_key(v), ~np.isnan(v)
    kmin = np.full((nv, 3), 0xFFFFFFFF, np.uint32)
    kmax = np.zeros((nv, 3), np.uint32)
    for c in range(3):
        rows = label[num[:, c]]
        np.minimum.at(kmin[:, c], rows, keys[num[:, c], c])
        np.maximum.at(kmax[:, c], rows, keys[num[:, c], c])
    seen = np.zeros((nv, 3), bool)                      # an axis without a number: [0, 0]
    for c in range(3):
        seen[label[num[:, c]], c] = True
    box_min = np.where(seen, key_float(kmin), np.float32(0)).astype(np.float32)
    box_max = np.where(seen, key_float(kmax), np.float32(0)).astype(np.float32)
    return label.astype(np.int32), faces.astype(np.int32), box_min, box_max, int((~ok).sum())


def diag2(box_min, box_max):
    """dx*dx + dy*dy + dz*dz in binary32, one rounding per operation, left to right; a NaN extent (inf - inf) is 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(box_max, np.float32) - np.asarray(box_min, np.float32)
        d = np.where(np.isnan(d), np.float32(0), d).astype(np.float32)
        return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + d[..., 2] * d[..., 2]).astype(np.float32)


def keep_rule(labels, faces, d2, min_faces=0, min_diagonal=0.0, largest=False):
    """The keep rule on a component table: labels, faces, d2 (diag2, float32) one entry per component -> bool per entry."""
    labels, faces = np.asarray(labels, np.int64), np.asarray(faces, np.int64)
    d2 = np.asarray(d2, np.float32)
    md = np.float32(min_diagonal)
    if int(min_faces) < 0 or not md >= 0:
        raise ValueError("min_faces and min_diagonal must be >= 0 and not NaN")
    with np.errstate(over="ignore"):
        thr = np.float32(md * md)
    keep = (faces >= 1) & (faces >= int(min_faces)) & (d2 >= thr)
    if largest:
        best = np.zeros(len(labels), bool)
        if (faces >= 1).any():
            top = faces.max()
            best[labels == labels[faces == top].min()] = True      # the most faces; ties: the smaller label
        keep &= best
    return keep


def clean(vertices, triangles, min_faces=0, min_diagonal=0.0, largest=False, comps=None):
    """(vertices, triangles, vertex_map, bad): the kept rows in their original order, triangles renumbered.  `comps`:
    what components(vertices, triangles) returned, where a caller has it already."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    nv = len(v)
    label, faces, box_min, box_max, bad = components(v, t) if comps is None else comps
    roots = np.flatnonzero(label == np.arange(nv))
    keep_root = np.zeros(nv, bool)
    keep_root[roots] = keep_rule(roots, faces[roots], diag2(box_min[roots], box_max[roots]), min_faces, min_diagonal,
                                 largest)
    keep_v = keep_root[label] if nv else np.zeros(0, bool)
    vertex_map = np.where(keep_v, np.cumsum(keep_v) - 1, -1).astype(np.int32)
    ok = valid_triangles(t, nv)
    keep_t = ok.copy()
    keep_t[ok] = keep_v[t[ok, 0]]
    out_t = vertex_map[t[keep_t]].astype(np.int32).reshape(-1, 3)
    return v[keep_v].reshape(-1, 3), out_t, vertex_map, bad
