"""CPU: tests/mesh_components_model.py - the NumPy restatement of include/mi3d.h Part 13 that tests/test_mesh_clean_gpu.py
compares the kernels with - against an independent brute force (the closure of the adjacency matrix, plain Python minima),
the keep rule's edge cases on hand-written component tables, and the argument checks of mesh.components / mesh.clean /
export_mesh that need no GPU."""
import inspect
import math

import numpy as np
import pytest

import mesh_components_model as M

SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0, 0.0)


def random_mesh(seed):
    """nv <= 40, with unreferenced vertices, duplicate and degenerate triangles, a few non-finite and signed-zero
    coordinates, and in every third mesh a triangle with a bad index."""
    rng = np.random.default_rng(seed)
    nv = int(rng.integers(1, 41))
    nt = int(rng.integers(0, max(1, nv)))                        # sparse: several components, some vertices uncited
    v = rng.normal(size=(nv, 3)).astype(np.float32)
    hit = rng.random((nv, 3)) < 0.12
    v[hit] = rng.choice(np.array(SPECIALS, np.float32), size=int(hit.sum()))
    t = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    if nt >= 3:
        t[1] = t[0]                                              # a duplicate
        t[2, 1] = t[2, 0]                                        # a degenerate one
    if nt >= 4 and seed % 3 == 0:
        t[3, int(rng.integers(0, 3))] = (-1, nv)[seed % 2]
    return v, t


def total_order(x):
    """Sort key of a binary32 value that is no NaN: by value, -0 below +0."""
    return (x, 0 if math.copysign(1.0, x) < 0 else 1)


def brute_force(v, t):
    """label, faces, box_min, box_max, bad by the closure of the adjacency matrix and Python min / max."""
    nv = len(v)
    ok = [all(0 <= i < nv for i in row) for row in t.tolist()]
    A = np.eye(nv, dtype=bool)
    for row, good in zip(t.tolist(), ok):
        if good:
            for i in row:
                for j in row:
                    A[i, j] = True
    while True:
        B = (A.astype(np.int64) @ A.astype(np.int64)) > 0
        if np.array_equal(A, B):
            break
        A = B
    label = np.array([int(np.flatnonzero(A[i])[0]) for i in range(nv)], np.int64).reshape(nv)
    faces = np.zeros(nv, np.int64)
    for row, good in zip(t.tolist(), ok):
        if good:
            faces[label[row[0]]] += 1
    box_min, box_max = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.float32)
    for r in set(label.tolist()):
        for c in range(3):
            xs = [float(x) for x in v[label == r, c] if not math.isnan(x)]
            if xs:
                box_min[r, c], box_max[r, c] = min(xs, key=total_order), max(xs, key=total_order)
    return label, faces, box_min, box_max, ok.count(False)


@pytest.mark.parametrize("seed", range(36))
def test_model_against_the_adjacency_closure(seed):
    v, t = random_mesh(seed)
    label, faces, bmin, bmax, bad = M.components(v, t)
    rl, rf, rmin, rmax, rbad = brute_force(v, t)
    assert label.dtype == np.int32 and faces.dtype == np.int32 and bmin.dtype == np.float32
    assert np.array_equal(label, rl) and np.array_equal(faces, rf) and bad == rbad
    assert bmin.tobytes() == rmin.tobytes() and bmax.tobytes() == rmax.tobytes()      # signed zeros included
    assert np.all(label <= np.arange(len(v))) and np.array_equal(label[label], label)
    assert faces.sum() == len(t) - bad and np.all(faces[label != np.arange(len(v))] == 0)

    # clean against the same brute force: the rule spelled out per component, compaction by Python lists
    roots = [r for r in range(len(v)) if rl[r] == r]
    for min_faces, min_diagonal, largest in ((0, 0.0, False), (2, 0.0, False), (0, 1.5, False), (1, 0.0, True), (3, 0.5, True)):
        d2 = {}
        for r in roots:
            with np.errstate(invalid="ignore", over="ignore"):
                d = [np.float32(0) if np.isnan(e) else e for e in (rmax[r] - rmin[r])]
                d2[r] = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        thr = np.float32(np.float32(min_diagonal) * np.float32(min_diagonal))
        kept = {r for r in roots if rf[r] >= 1 and rf[r] >= min_faces and d2[r] >= thr}
        if largest:
            faced = [r for r in roots if rf[r] >= 1]
            best = min(faced, key=lambda r: (-rf[r], r)) if faced else None
            kept &= {best}
        new, vmap = 0, []
        for i in range(len(v)):
            vmap.append(new if rl[i] in kept else -1)
            new += rl[i] in kept
        rows = [[vmap[i] for i in row] for row in t.tolist() if all(0 <= i < len(v) for i in row) and rl[row[0]] in kept]
        with np.errstate(invalid="ignore", over="ignore"):
            cv, ct, cmap, cbad = M.clean(v, t, min_faces, min_diagonal, largest)
        assert cbad == rbad and cmap.tolist() == vmap and ct.tolist() == rows
        assert cv.tobytes() == v[[i for i in range(len(v)) if vmap[i] >= 0]].reshape(-1, 3).tobytes()
        assert cv.shape == (new, 3) and ct.shape == (len(rows), 3) and ct.dtype == np.int32 and cmap.dtype == np.int32


def test_diag2_is_binary32_left_to_right():
    lo = np.array([[0.1, -0.3, 1e-3]], np.float32)
    hi = np.array([[0.7, 0.9, 0.3]], np.float32)
    d = hi - lo
    want = np.float32(np.float32(np.float32(d[0, 0] * d[0, 0]) + np.float32(d[0, 1] * d[0, 1])) + np.float32(d[0, 2] * d[0, 2]))
    got = M.diag2(lo, hi)
    assert got.dtype == np.float32 and got.tobytes() == np.array([want]).tobytes()
    inf = np.float32(np.inf)
    assert M.diag2(np.array([[inf, 0, 0]], np.float32), np.array([[inf, 0, 0]], np.float32))[0] == 0      # inf - inf
    assert M.diag2(np.array([[-inf, 0, 0]], np.float32), np.array([[1, 0, 0]], np.float32))[0] == inf


def test_float_key_orders_like_the_floats():
    xs = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    k = M.float_key(xs)
    assert np.all(k[:-1] < k[1:]) and M.key_float(k).tobytes() == xs.tobytes()


# ------------------------------------------------------------------------------------------------ the keep rule

def test_equality_keeps():
    labels, faces = [0, 5, 9], [10, 4, 3]
    d2 = M.diag2(np.zeros((3, 3), np.float32), np.array([[3, 4, 0], [0.3, 0.4, 0], [1, 1, 1]], np.float32))
    assert M.keep_rule(labels, faces, d2, min_faces=4).tolist() == [True, True, False]
    assert M.keep_rule(labels, faces, d2, min_faces=5).tolist() == [True, False, False]
    assert M.keep_rule(labels, faces, d2, min_faces=3).tolist() == [True, True, True]
    assert d2[0] == 25.0
    assert M.keep_rule(labels, faces, d2, min_diagonal=5.0).tolist() == [True, False, False]     # diag2 == 25 == 5 * 5
    assert M.keep_rule(labels, faces, d2, min_diagonal=float(np.nextafter(np.float32(5), np.float32(6)))).tolist() == \
        [False, False, False]
    assert M.keep_rule(labels, faces, d2, min_faces=10, min_diagonal=5.0).tolist() == [True, False, False]


def test_the_threshold_product_is_binary32():
    md = 0.1                                              # float32(0.1)^2 rounded to binary32, not 0.01 in binary64
    thr = np.float32(np.float32(md) * np.float32(md))
    below = np.nextafter(thr, np.float32(0))
    assert M.keep_rule([0, 1], [1, 1], np.array([thr, below], np.float32), min_diagonal=md).tolist() == [True, False]


def test_ties_go_to_the_smaller_label():
    assert M.keep_rule([7, 2, 11], [5, 5, 4], np.ones(3, np.float32), largest=True).tolist() == [False, True, False]
    assert M.keep_rule([7, 2, 11], [5, 4, 5], np.ones(3, np.float32), largest=True).tolist() == [True, False, False]
    assert M.keep_rule([3], [1], np.zeros(1, np.float32), largest=True).tolist() == [True]


def test_largest_with_excluding_thresholds_keeps_nothing():
    labels, faces, d2 = [0, 4, 8], [9, 6, 2], np.array([0.01, 4.0, 4.0], np.float32)
    assert M.keep_rule(labels, faces, d2, largest=True).tolist() == [True, False, False]
    assert M.keep_rule(labels, faces, d2, min_diagonal=1.0, largest=True).tolist() == [False, False, False]
    assert M.keep_rule(labels, faces, d2, min_faces=10, largest=True).tolist() == [False, False, False]
    assert M.keep_rule(labels, faces, d2, min_diagonal=1.0).tolist() == [False, True, True]      # not the runner-up either


def test_zero_face_components_never_survive():
    labels, faces, d2 = [0, 1, 2], [0, 0, 3], np.array([9.0, 0.0, 1.0], np.float32)
    assert M.keep_rule(labels, faces, d2).tolist() == [False, False, True]
    assert M.keep_rule(labels, faces, d2, min_faces=0, min_diagonal=0.0).tolist() == [False, False, True]
    assert M.keep_rule([0, 1], [0, 0], np.ones(2, np.float32), largest=True).tolist() == [False, False]
    v = np.zeros((5, 3), np.float32)                      # vertices 0 and 4 are cited by no one
    cv, ct, vmap, bad = M.clean(v, np.array([[1, 2, 3]], np.int32))
    assert vmap.tolist() == [-1, 0, 1, 2, -1] and ct.tolist() == [[0, 1, 2]] and len(cv) == 3 and bad == 0


def test_model_refuses_negative_and_nan_thresholds():
    for kw in ({"min_faces": -1}, {"min_diagonal": -0.5}, {"min_diagonal": float("nan")}):
        with pytest.raises(ValueError):
            M.keep_rule([0], [1], np.ones(1, np.float32), **kw)


# ------------------------------------------------------------------------------------------------ the product, no GPU

def test_clean_and_components_refuse_cpu_tensors_and_bad_arguments(monkeypatch):
    import torch
    from mi3d import _lib, mesh
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for fn in (mesh.components, mesh.clean):
        with pytest.raises(_lib.Mi3dError, match="GPU"):
            fn(v, t)
        with pytest.raises(TypeError):
            fn(np.zeros((4, 3), np.float32), t)
    assert calls == []


@pytest.mark.parametrize("kw", [{"min_faces": -1}, {"min_faces": 2.5}, {"min_faces": True}, {"min_faces": 2 ** 32},
                                {"min_diagonal": -1e-9}, {"min_diagonal": float("nan")}, {"min_diagonal": "1"},
                                {"largest": 1}, {"largest": None}])
def test_keep_rule_arguments_are_checked(kw):
    from mi3d import _lib, mesh
    args = {"min_faces": 0, "min_diagonal": 0.0, "largest": False, **kw}
    with pytest.raises(_lib.Mi3dError, match=next(iter(kw))):
        mesh._check_keep_rule(**args)


def test_keep_rule_arguments_accepted():
    from mi3d import mesh
    assert mesh._check_keep_rule(0, 0.0, False) == (0, 0.0, False)
    assert mesh._check_keep_rule(np.int64(7), np.float32(0.5), np.bool_(True)) == (7, 0.5, True)
    assert mesh._check_keep_rule(3, 2, True) == (3, 2.0, True)
    assert mesh._check_keep_rule(0, float("inf"), False)[1] == float("inf")


def test_export_mesh_accepts_the_three_arguments(tmp_path):
    import torch
    from mi3d import _lib, mesh, network, renderer, sds_step
    for fn in (renderer.NeRFRenderer.export_mesh, mesh.export):
        p = inspect.signature(fn).parameters
        assert p["min_faces"].default is None and p["min_diagonal"].default is None and p["largest"].default is False
    torch.manual_seed(0)
    model = network.NeRFNetwork(sds_step.make_opt(fp16=False))
    with pytest.raises(_lib.Mi3dError, match="GPU"):         # a CPU model is refused as before, whatever the arguments
        model.export_mesh(str(tmp_path), resolution=8, min_faces=10, min_diagonal=0.1, largest=True)


def test_part13_is_declared_bound_and_built_without_contraction():
    import importlib.util
    import os
    from conftest import PKG
    from mi3d import _lib
    lib = _lib.lib()
    for name in ("mi3d_mesh_components", "mi3d_mesh_clean_count", "mi3d_mesh_clean_emit"):
        assert name in _lib._SIGNATURES and hasattr(lib, name)
    assert "mi3d_mesh_components_workspace" in _lib._LATE_SIGNATURES
    spec = importlib.util.spec_from_file_location("mi3d_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("meshclean.hip", ["-ffp-contract=off"]) in b.UNITS
    assert lib.mi3d_abi_version() == 5


def test_workspace_query_is_host_only():
    from mi3d import _lib
    ws = _lib.lib().mi3d_mesh_components_workspace
    assert ws(0, 0) == 0
    assert ws(1, 1) == 8 + 8 + 8                          # one block sum each, padded to 8 bytes, and one flag byte padded
    assert ws(257, 4099) == 8 + 72 + 264                  # 2 and 17 block sums of 4 bytes, 257 flag bytes, each padded to 8
    assert ws(2 ** 31 - 1, 2 ** 31 - 1) > 2 ** 31 and ws(2 ** 31, 1) == 0 and ws(1, 2 ** 31) == 0
