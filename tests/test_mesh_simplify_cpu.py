"""CPU: tests/mesh_simplify_model.py - the NumPy restatement of include/mi3d.h Part 14 that tests/test_mesh_simplify_gpu.py
holds the kernels to - against an independent brute-force version (Python dicts keyed by the cluster triple and by the
frozenset of a triangle's clusters), on the very inputs the GPU tests use; that these inputs contain what their names
say; and the argument checks of mesh.simplify and export_mesh that need no GPU."""
import math

import numpy as np
import pytest

import mesh_simplify_model as M
from test_mc_tables_cpu import load_table, marching_cubes_ref


# ------------------------------------------------------------------------------------------------ brute force

def brute(vertices, triangles, origin, cell):
    """Part 14 once more, an element at a time: scalar float32 / float64 arithmetic, dicts for the clusters."""
    v = np.asarray(vertices, np.float32)
    o = [np.float32(x) for x in origin]
    cell = np.float32(cell)
    nv, nt = len(v), len(triangles)
    members, cluster = {}, [None] * nv                      # cluster triple -> vertex indices, ascending
    qs = [None] * nv
    non_finite = 0
    with np.errstate(all="ignore"):
        for i in range(nv):
            if not all(math.isfinite(float(x)) for x in v[i]):
                non_finite += 1
                continue
            key, q = [], []
            for k in range(3):
                g = np.float32(np.float32(v[i, k] - o[k]) / cell)
                fl = math.floor(float(g)) if math.isfinite(float(g)) else (2 ** 40 if g > 0 else -2 ** 40)
                c = min(max(fl, -2 ** 30), 2 ** 30 - 1)
                f = np.float32(g - np.float32(c))
                f = np.float32(min(max(float(f), 0.0), 1.0))
                key.append(c)
                q.append(math.floor(float(np.float32(f * np.float32(2 ** 20)))))
            cluster[i], qs[i] = tuple(key), q
            members.setdefault(cluster[i], []).append(i)
    seen, survivors, bad, degenerate, duplicate = set(), [], 0, 0, 0
    for j in range(nt):
        idx = [int(x) for x in triangles[j]]
        if not all(0 <= x < nv for x in idx) or any(cluster[x] is None for x in idx):
            bad += 1
            continue
        key = frozenset(cluster[x] for x in idx)
        if len(key) < 3:
            degenerate += 1
        elif key in seen:
            duplicate += 1
        else:
            seen.add(key)
            survivors.append(j)
    cited = {cluster[int(x)] for j in survivors for x in triangles[j]}
    order = sorted(cited, key=lambda key: members[key][0])  # by leader
    new_id = {key: n for n, key in enumerate(order)}
    out_v = np.zeros((len(order), 3), np.float32)
    for n_, key in enumerate(order):
        for k in range(3):
            S = sum(qs[i][k] for i in members[key])         # exact Python integers
            s = np.float64(S) / np.float64(len(members[key]))
            s = s * np.float64(2.0 ** -20)
            s = np.float64(key[k]) + s
            s = np.float64(cell) * s
            s = np.float64(o[k]) + s
            out_v[n_, k] = np.float32(s)
    out_t = np.array([[new_id[cluster[int(x)]] for x in triangles[j]] for j in survivors], np.int32).reshape(-1, 3)
    vmap = np.array([new_id.get(cluster[i], -1) if cluster[i] is not None else -1 for i in range(nv)], np.int32)
    counts = [len(order), len(survivors), bad, 0, non_finite, len(members), degenerate, duplicate]
    return out_v, out_t, vmap, counts


def same(a, b):
    return (a[0].tobytes() == b[0].tobytes() and a[0].shape == b[0].shape and np.array_equal(a[1], b[1])
            and a[1].dtype == b[1].dtype == np.int32 and np.array_equal(a[2], b[2]) and list(a[3]) == list(b[3]))


@pytest.fixture(scope="module")
def surfaces():
    rows, _ = load_table()
    out = {}
    for name, (R, make) in M.VOLUMES.items():
        h = np.float32(2.0 / (R - 1))
        out[name] = (R,) + marching_cubes_ref(make(), 0.0, (-1, -1, -1), (h, h, h), rows)
    return out


# ------------------------------------------------------------------------------------------------ model vs brute force

@pytest.mark.parametrize("name", list(M.VOLUMES))
def test_model_equals_brute_force_on_the_surfaces(surfaces, name):
    R, v, t = surfaces[name]
    assert len(v) > 500 and len(t) > 1000
    for what, origin, cell in M.lattices(R, v):
        got = M.simplify(v, t, origin, cell)
        assert same(got, brute(v, t, origin, cell)), what
        assert 0 < got[3][1] < len(t) and 0 < got[3][0] <= got[3][5] < len(v), what
        assert got[3][6] > 0, (what, got[3])                            # degenerate triangles on every surface
        M.check_geometry(v, origin, cell, *got[:3], radius=0.6 if name.startswith("sphere") else None)
        if name == "shell32" and what in ("d=3.7", "own origin"):
            assert got[3][7] > 0, (what, got[3])                        # duplicates where the cell exceeds the shell


def test_the_larger_spheres_span_several_workgroups(surfaces):
    """What the model says about the spheres: several workgroups at 48^3 (3 744 vertices, not 10 000), more than 10 000
    vertices at 96^3 - and no duplicate triangle on either, which is why shell32 is among the surfaces."""
    R, v, t = surfaces["sphere48"]
    assert len(v) > 4 * 256 and len(t) > 4 * 256
    R, v, t = surfaces["sphere96"]
    assert len(v) > 10_000 and len(t) > 20_000


@pytest.mark.parametrize("case", [M.boundary_case, M.fans_case, M.bad_case])
def test_model_equals_brute_force_on_the_hand_made_cases(case):
    v, t, origin, cell = case()
    assert same(M.simplify(v, t, origin, cell), brute(v, t, origin, cell))


@pytest.mark.parametrize("steps", M.SHEET_CELLS)
def test_model_equals_brute_force_on_the_sheet(steps):
    v, t = M.sheet()
    assert len(v) == 360_000 and len(t) == 717_602
    origin, cell = M.sheet_lattice(steps)
    got = M.simplify(v, t, origin, cell)
    assert same(got, brute(v, t, origin, cell))
    # both rows of block sums (one per 256 elements) need a second round of the 1024-wide scan
    assert len(v) > M.SCAN_ROUND and len(t) > M.SCAN_ROUND
    assert -(-len(v) // 256) > 1024 and -(-len(t) // 256) > 1024
    assert got[3][0] > 256 and got[3][1] > 256 and got[3][6] > 0             # the outputs span workgroups too


def test_everything_collapses_and_empty_input():
    v, t = M.sheet(8)
    out_v, out_t, vmap, counts = M.simplify(v, t, (-0.25, -0.25, -0.25), 100.0)
    assert out_v.shape == (0, 3) and out_t.shape == (0, 3) and np.all(vmap == -1)
    assert counts == [0, 0, 0, 0, 0, 1, len(t), 0]
    assert same(M.simplify(v, t, (-0.25, -0.25, -0.25), 100.0), brute(v, t, (-0.25, -0.25, -0.25), 100.0))
    e = M.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), (0, 0, 0), 1.0)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0,) and e[3] == [0] * 8


# ------------------------------------------------------------------------------------------------ the inputs are what they claim

def test_boundary_case_holds_what_it_names():
    v, t, origin, cell = M.boundary_case()
    finite, c, q = M.clusters(v, origin, cell)
    assert finite.all()
    with np.errstate(over="ignore"):
        g = (v - origin) / cell
    assert list(g[:4, 0]) == [0.0, 1.0, 2.0, 4.0] and list(c[:4, 0]) == [0, 1, 2, 4] and not q[:4, 0].any()  # on boundaries
    assert 0 < 1 - g[4, 0] < 1e-6 and 0 < 2 - g[5, 0] < 1e-6 and list(c[4:6, 0]) == [0, 1]                     # just below
    assert np.all(q[4:6, 0] == 2 ** 20 - 1)                                                                    # the last fixed-point step
    assert abs(float(g[6, 0]) + 1e-10) < 1e-16 and c[6, 0] == -1 and q[6, 0] == 2 ** 20                       # f rounds to 1.0
    assert list(c[7:10, 0]) == [-1, -4, -14]                                                                   # below the origin
    assert c[12, 0] == 2 ** 30 - 1 and c[13, 0] == -2 ** 30 and c[14, 0] == 2 ** 30 - 1 and c[14, 1] == -2 ** 30
    assert np.isinf(g[14, 0]) and np.isinf(g[14, 1])
    out_v, out_t, vmap, counts = M.simplify(v, t, origin, cell)
    assert counts[1] > 0 and {vmap[6], vmap[12], vmap[13], vmap[14]} != {-1}
    assert np.isfinite(out_v).all()


def test_fans_case_holds_what_it_names():
    v, t, origin, cell = M.fans_case()
    out_v, out_t, vmap, counts = M.simplify(v, t, origin, cell)
    assert counts == [4, 2, 0, 0, 0, 6, 2, 3]
    # leaders: A 0, B 1, C 2, D 6 -> new ids 0 .. 3; triangle 0 = (A, B, C) and triangle 3 = (D, C, B) survive as they are
    assert out_t.tolist() == [[0, 1, 2], [3, 2, 1]]
    assert vmap.tolist() == [0, 1, 2, 0, 1, 2, 3, 3, 0, -1, -1, 1, -1]
    # the mean of A's members 0, 3, 8 up to the 2^-20 fixed point
    assert np.allclose(out_v[0], v[[0, 3, 8]].astype(np.float64).mean(0), atol=2 ** -19)


def test_bad_case_holds_what_it_names():
    v, t, origin, cell = M.bad_case()
    nv = len(v)
    assert (t == -1).sum() == 1 and (t == nv).sum() == 1 and (t == 2 ** 31 - 1).sum() == 1
    assert np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
    counts = M.simplify(v, t, origin, cell)[3]
    assert counts[2] == 5 and counts[4] == 3 and counts[1] > 0          # three bad indices, two cited non-finite vertices


# ------------------------------------------------------------------------------------------------ argument checks

def test_ladder_is_strictly_increasing():
    from mi3d import mesh
    lad = mesh.DECIMATE_LADDER
    assert lad == (1.5, 2, 2.5, 3, 3.5, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64)
    assert all(a < b for a, b in zip(lad, lad[1:]))
    assert all(float(2 * d).is_integer() for d in lad)                  # multiples of 0.5: the quarter-step offset holds


def test_export_lattice_is_the_models():
    from mi3d import mesh
    for R in (24, 48, 256):
        for d in (1.5, 2, 3.7, 64):
            origin, cell = mesh.export_lattice(R, d)
            mo, mc = M.export_lattice(R, d)
            assert np.float32(cell) == mc and all(np.float32(x) == y for x, y in zip(origin, mo))


def test_no_grid_plane_meets_a_cell_boundary():
    """With the origin a quarter step below the grid, grid plane i lies at (i + 1/4) / d cells: never an integer for a d
    that is a multiple of 0.5, and at least 1 / (4 d) cells from one - far above binary32 rounding."""
    from mi3d import mesh
    R = 256
    i = np.arange(R, dtype=np.float64)
    for d in mesh.DECIMATE_LADDER:
        g = (i + 0.25) / d
        assert np.abs(g - np.round(g)).min() >= 0.25 / d - 1e-12


@pytest.mark.parametrize("cell", [0, -1, float("nan"), float("inf"), "2", None, True, 1e-50, 1e50])
def test_simplify_checks_cell_first_on_any_device(cell):
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="cell"):
        mesh.simplify(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), cell)
    with pytest.raises(_lib.Mi3dError, match="cell"):
        mesh.simplify("no tensor", None, cell)                          # before the tensors are looked at


def test_simplify_refuses_cpu_tensors_after_the_cell():
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="GPU"):
        mesh.simplify(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), 0.5)


class _CpuModel:
    """What export looks at before it needs a GPU."""
    import torch as _torch
    aabb_train = _torch.zeros(6)
    grid_size, cuda_ray, mean_density, density_thresh = 16, False, 0.0, 10.0


@pytest.mark.parametrize("kw, match", [
    ({"decimate": 2, "target_faces": 100}, "mutually exclusive"),
    ({"decimate": 0}, "decimate"), ({"decimate": -1.5}, "decimate"), ({"decimate": float("nan")}, "decimate"),
    ({"decimate": float("inf")}, "decimate"), ({"decimate": "2"}, "decimate"), ({"decimate": True}, "decimate"),
    ({"target_faces": 0}, "target_faces"), ({"target_faces": -3}, "target_faces"), ({"target_faces": 2.5}, "target_faces"),
    ({"target_faces": 100.0}, "target_faces"), ({"target_faces": "100"}, "target_faces"),
    ({"target_faces": True}, "target_faces"),
])
def test_export_checks_the_new_arguments_before_the_device(tmp_path, kw, match):
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match=match):
        mesh.export(_CpuModel(), str(tmp_path), **kw)


@pytest.mark.parametrize("kw", [{"decimate": 2}, {"decimate": 1.5}, {"target_faces": 100}, {"target_faces": np.int64(7)},
                                {"decimate": None, "target_faces": None}])
def test_export_with_good_arguments_reaches_the_device_check(tmp_path, kw):
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="export_mesh needs the model on the GPU"):
        mesh.export(_CpuModel(), str(tmp_path), **kw)


def test_export_mesh_passes_the_arguments_on(tmp_path):
    """NeRFRenderer.export_mesh hands both arguments to mesh.export."""
    import inspect
    from mi3d import mesh, renderer
    sig = inspect.signature(renderer.NeRFRenderer.export_mesh).parameters
    assert sig["decimate"].default is None and sig["target_faces"].default is None
    sig = inspect.signature(mesh.export).parameters
    assert sig["decimate"].default is None and sig["target_faces"].default is None


def test_binding_build_and_workspace_query():
    import importlib.util
    import os
    from conftest import PKG
    from mi3d import _lib
    for name in ("mi3d_mesh_simplify_count", "mi3d_mesh_simplify_emit"):
        assert name in _lib._SIGNATURES
    assert "mi3d_mesh_simplify_workspace" in _lib._LATE_SIGNATURES
    spec = importlib.util.spec_from_file_location("mi3d_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("meshsimplify.hip", ["-ffp-contract=off"]) in b.UNITS
    ws = _lib.lib().mi3d_mesh_simplify_workspace
    pad8 = lambda n: (n + 7) // 8 * 8                                   # noqa: E731
    above = lambda n: 1 << int(n).bit_length()                          # noqa: E731  the smallest power of two > n
    for nv, nt in ((1, 0), (0, 1), (3, 1), (255, 256), (256, 257), (1000, 2000), (360_000, 717_602)):
        # S and n, marks, lead, tslot; per workgroup of 256: two rows of counts for the vertices, three for the triangles
        fixed = (pad8(32 * nv) + pad8(nv) + pad8(4 * nv) + pad8(4 * nt) + 2 * pad8(4 * -(-nv // 256))
                 + 3 * pad8(4 * -(-nt // 256)))
        assert ws(nv, nt, 1) == fixed + pad8(4 * above(nv)) + pad8(4 * above(nt)), (nv, nt)
        assert ws(nv, nt, 0) == fixed + pad8(8 * above(nv)) + pad8(8 * above(nt)), (nv, nt)
        assert above(nv) > nv and above(nt) > nt and 2 * above(nv) >= 2 * nv
    assert ws(0, 0, 0) == 0 and ws(0, 0, 1) == 0 and ws(2 ** 31, 1, 0) == 0 and ws(1, 2 ** 31, 1) == 0
    big = 2 ** 31 - 1                                                    # capacities stop at 2^31 slots
    assert ws(big, big, 0) == ws(big, big, 1)
