"""CPU: tests/mesh_collapse_model.py, the restatement of include/mi3d.h Part 19 (quadric edge-collapse decimation), held to
what must be true of ANY correct output - stated with NumPy alone, without the model's data structures - and to the
figures the contract was chosen by: cubes that come back as 12 triangles with their corners bit for bit, a sphere closer
to the sphere than vertex clustering at equal faces, a thin shell whose sheets stay apart.  Then the argument checks of
mesh.collapse and of export_mesh's `collapse`, which need no GPU.  tests/test_mesh_collapse_gpu.py compares the kernels
with this model byte for byte."""
import numpy as np
import pytest

import mesh_collapse_model as M
import mesh_simplify_model as S
from test_mc_tables_cpu import load_table, marching_cubes_ref


# ------------------------------------------------------------------------------------------------ properties, NumPy alone

def edge_table(t):
    """(undirected edges [ne, 2], how many triangles hold each, directed edges that occur more than once)."""
    t = np.asarray(t, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    lo, hi = d.min(1), d.max(1)
    packed, cnt = np.unique((lo << 32) | hi, return_counts=True)       # indices are below 2^31
    repeated = len(d) - len(np.unique((d[:, 0] << 32) | d[:, 1]))
    return np.stack([packed >> 32, packed & 0xFFFFFFFF], 1), cnt, repeated


def components(edges, n):
    """label [n]: the smallest index connected to every index, by hooking and pointer jumping."""
    parent = np.arange(n)
    while True:
        a, b = parent[edges[:, 0]], parent[edges[:, 1]]
        new = parent.copy()
        np.minimum.at(new, np.maximum(a, b), np.minimum(a, b))
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, parent):
            return parent
        parent = new


def topology(t, nv):
    """(Euler characteristic, component count, border edges, non-manifold edges, repeated directed edges) of the
    triangles' own vertices."""
    t = np.asarray(t, np.int64)
    if len(t) == 0:
        return 0, 0, 0, 0, 0
    uniq, cnt, repeated = edge_table(t)
    cited = np.unique(t)
    label = components(uniq, nv)
    return (len(cited) - len(uniq) + len(t), len(np.unique(label[cited])), int((cnt == 1).sum()), int((cnt > 2).sum()),
            repeated)


def check_output(v, t, out_v, out_t, vertex_map, closed=True):
    """What holds of every output: types, indices, every vertex cited, vertex_map onto [0, kv); the Euler characteristic
    and the component count of the usable input; with `closed`, two triangles on every edge, once in each direction."""
    assert out_v.dtype == np.float32 and out_t.dtype == np.int32 and vertex_map.dtype == np.int32
    kv = len(out_v)
    assert out_v.shape == (kv, 3) and out_t.ndim == 2 and out_t.shape[1] == 3 and vertex_map.shape == (len(v),)
    assert np.array_equal(np.unique(out_t), np.arange(kv))              # no index cited that is not emitted, and none idle
    assert np.all((out_t[:, 0] != out_t[:, 1]) & (out_t[:, 1] != out_t[:, 2]) & (out_t[:, 0] != out_t[:, 2]))
    assert vertex_map.min(initial=-1) >= -1 and vertex_map.max(initial=-1) == kv - 1
    ok = M.SM.usable_triangles(v, t)
    before, after = topology(t[ok], len(v)), topology(out_t, max(kv, 1))
    assert after[:2] == before[:2], (before, after)                     # Euler characteristic, components
    assert after[3] == before[3] == 0 and after[4] == before[4] == 0    # manifold, consistently oriented
    assert after[2] == before[2]
    if closed:
        assert after[2] == 0
    assert np.isfinite(out_v).all()


def marched(name):
    rows, _ = load_table()
    R, make = S.VOLUMES[name]
    h = np.float32(2.0 / (R - 1))
    return marching_cubes_ref(make(), 0.0, (-1, -1, -1), (h, h, h), rows)


# ------------------------------------------------------------------------------------------------ the cubes

@pytest.mark.parametrize("n", [2, 3, 6])
def test_cube_comes_back_as_twelve_triangles_with_its_corners(n):
    v, t = M.cube(n)
    assert len(v) == 6 * n * n + 2 and len(t) == 12 * n * n and M.enclosed_volume(v, t) == 8.0
    out_v, out_t, vm, counts = M.collapse(v, t, 12)
    check_output(v, t, out_v, out_t, vm)
    assert counts[:2] == [8, 12] and counts[2] == 0 and counts[4] == 0 and counts[6] == 0 and counts[7] == 0
    assert counts[5] == (len(t) - 12) // 2                              # every collapse removes two triangles
    corners = {(x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)}
    assert {tuple(p) for p in out_v.tolist()} == corners                # bit for bit
    assert np.all(np.abs(out_v).max(1) == 1.0)                          # every vertex on the surface
    assert M.enclosed_volume(out_v, out_t) == 8.0
    for x in np.nonzero(np.abs(v).min(1) == 1.0)[0]:                    # an input corner stays itself
        if (np.abs(v[x]) == 1.0).all():
            assert tuple(out_v[vm[x]]) == tuple(v[x])


def test_cube_halfway_is_a_closed_manifold_on_the_surface():
    v, t = M.cube(6)
    out_v, out_t, vm, counts = M.collapse(v, t, 100)
    check_output(v, t, out_v, out_t, vm)
    assert counts[1] == 100 and M.enclosed_volume(out_v, out_t) == 8.0 and np.all(np.abs(out_v).max(1) == 1.0)


# ------------------------------------------------------------------------------------------------ the sphere

@pytest.fixture(scope="module")
def sphere():
    return M.octa_sphere(4)


@pytest.mark.parametrize("cell, faces", zip(M.SPHERE_CELLS, (333, 234, 157)))
def test_sphere_is_closer_to_the_sphere_than_clustering_at_equal_faces(sphere, cell, faces):
    """RMS distance of the triangle centroids from the unit sphere, clustering | collapse: 0.0237 | 0.0103 at 333 faces,
    0.0364 | 0.0138 at 234, 0.0573 | 0.0207 at 157 (collapse lands on 332, 234, 156).  The bound is clustering's own
    figure, no margin."""
    v, t = sphere
    assert len(t) == 2048
    sv, st, _, _ = S.simplify(v, t, np.full(3, M.SPHERE_ORIGIN, np.float32), cell)
    assert len(st) == faces
    out_v, out_t, vm, counts = M.collapse(v, t, faces)
    check_output(v, t, out_v, out_t, vm)
    assert counts[1] in (faces, faces - 1)
    assert topology(st, len(sv))[3] > 0                                 # clustering's output is not manifold
    ours, theirs = M.centroid_radial_rms(out_v, out_t), M.centroid_radial_rms(sv, st)
    print(f"faces {faces}: clustering {theirs:.4f}, collapse {ours:.4f}")
    assert ours <= theirs
    assert 4.0 < M.enclosed_volume(out_v, out_t) < M.enclosed_volume(v, t) < 4.0 / 3.0 * np.pi


def test_sphere_down_to_four_faces_is_a_tetrahedron_of_positive_volume(sphere):
    v, t = sphere
    out_v, out_t, vm, counts = M.collapse(v, t, 4)
    check_output(v, t, out_v, out_t, vm)
    assert counts[:2] == [4, 4] and M.enclosed_volume(out_v, out_t) > 0.0


def test_tetrahedron_does_not_collapse():
    v, t = M.tetrahedron()
    out_v, out_t, vm, counts = M.collapse(v, t, 0)
    assert out_v.tobytes() == v.tobytes() and np.array_equal(out_t, t) and np.array_equal(vm, np.arange(4))
    assert counts == [4, 4, 0, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ borders, shells, limits

def test_open_sheet_keeps_its_border_bit_for_bit():
    v, t = M.open_sheet()
    n = 20
    out_v, out_t, vm, counts = M.collapse(v, t, len(t) // 4)
    check_output(v, t, out_v, out_t, vm, closed=False)
    i, j = np.divmod(np.arange(n * n), n)
    border = np.nonzero((i == 0) | (i == n - 1) | (j == 0) | (j == n - 1))[0]
    assert len(border) == 76 and np.all(vm[border] >= 0)
    assert out_v[vm[border]].tobytes() == v[border].tobytes()
    assert counts[1] < len(t) and counts[6] == 76                       # interior reduced; the border locked, counted
    assert topology(out_t, len(out_v))[2] == 76                         # still 76 border edges


def test_thin_shell_stays_two_components():
    """The shell of thickness 0.13: vertex clustering at d = 3.7 grid steps joins its two sheets (one component, edges
    with four triangles); collapse to the same face count keeps two closed manifolds."""
    v, t = marched("shell32")
    origin, cell = S.export_lattice(32, 3.7)
    sv, st, _, _ = S.simplify(v, t, origin, cell)
    assert topology(t, len(v))[1] == 2 and topology(st, len(sv))[1] == 1
    out_v, out_t, vm, counts = M.collapse(v, t, len(st))
    check_output(v, t, out_v, out_t, vm)
    assert topology(out_t, len(out_v))[1] == 2 and counts[1] in (len(st), len(st) - 1)


def test_target_at_or_above_the_face_count_returns_the_usable_triangles_untouched():
    v, t = M.bad_case()
    ok = M.SM.usable_triangles(v, t)
    for target in (int(ok.sum()), len(t), 10 ** 12):
        out_v, out_t, vm, counts = M.collapse(v, t, target)
        cited = np.unique(t[ok])
        assert out_v.tobytes() == v[cited].tobytes() and np.array_equal(cited[out_t], t[ok])
        assert counts[3] == counts[5] == 0 and counts[2] == int((~ok).sum()) and counts[4] == 2


def test_degree_limit_locks_and_counts():
    v, t = M.fan100()
    out_v, out_t, vm, counts = M.collapse(v, t, 10)
    assert np.array_equal(out_t, t) and out_v.tobytes() == v.tobytes()  # the centre and the whole rim are locked
    assert counts[6] == 101 and counts[3] == 0


def test_max_error_stops_the_run_early():
    """The 512-face sphere: the cheapest collapse costs between 3e-4 and 1e-3 (a sum over about ten unit-weight planes),
    so max_error = 3e-3 lets a hundred-odd through and then stalls, far above the target."""
    v, t = M.octa_sphere(3)
    free = M.collapse(v, t, 60)[3]
    assert M.collapse(v, t, 60, max_error=3e-4)[3][5] == 0
    held = M.collapse(v, t, 60, max_error=M.STALL_ERROR)
    check_output(v, t, *held[:3])
    assert free[1] in (60, 59) and 60 < held[3][1] < len(t) and 0 < held[3][5] < free[5]


def test_key_hash_is_the_contracts():
    assert M.edge_hash(0, 0, 0) == 0 and M.edge_hash(1, 0, 0) == (2654435761 >> 7) & 0xFFFFF
    assert M.edge_hash(3, 5, 7) == ((((3 * 2654435761) ^ (5 * 2246822519) ^ (7 * 3266489917)) & 0xFFFFFFFF) >> 7) & 0xFFFFF


# ------------------------------------------------------------------------------------------------ argument checks

BAD_ARGUMENTS = [
    ({"target_faces": -1}, "target_faces"), ({"target_faces": 2.0}, "target_faces"), ({"target_faces": True}, "target_faces"),
    ({"target_faces": "9"}, "target_faces"), ({"target_faces": 9, "max_error": -1e-3}, "max_error"),
    ({"target_faces": 9, "max_error": float("nan")}, "max_error"), ({"target_faces": 9, "max_error": "1"}, "max_error"),
    ({"target_faces": 9, "max_rounds": -1}, "max_rounds"), ({"target_faces": 9, "max_rounds": 1.5}, "max_rounds"),
]


@pytest.mark.parametrize("kw, match", BAD_ARGUMENTS + [({"target_faces": 9, "rounds_per_read": 0}, "rounds_per_read"),
                                                       ({"target_faces": 9, "rounds_per_read": 5000}, "rounds_per_read")])
def test_collapse_checks_its_arguments_first_on_any_device(kw, match):
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match=match):
        mesh.collapse(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), **kw)
    with pytest.raises(_lib.Mi3dError, match=match):
        mesh.collapse("no tensor", None, **kw)


def test_collapse_refuses_cpu_tensors_after_the_arguments():
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="GPU"):
        mesh.collapse(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), 9, max_error=0.1)


class _CpuModel:
    """What export looks at before it needs a GPU."""
    import torch as _torch
    aabb_train = _torch.zeros(6)
    grid_size, cuda_ray, mean_density, density_thresh = 16, False, 0.0, 10.0


@pytest.mark.parametrize("collapse, match", [(kw["target_faces"] if len(kw) == 1 else kw, m) for kw, m in BAD_ARGUMENTS]
                         + [(0, "target_faces"), ({"max_error": 0.5}, "target_faces is required"),
                            ({"target_faces": 9, "rounds_per_read": 2}, "unknown keys")])
def test_export_checks_collapse_before_the_device(tmp_path, collapse, match):
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match=match):
        mesh.export(_CpuModel(), str(tmp_path), collapse=collapse)


@pytest.mark.parametrize("collapse", [None, 1, np.int64(5000), {"target_faces": 100},
                                      {"target_faces": 100, "max_error": 1e-4, "max_rounds": 64}])
def test_export_with_a_good_collapse_reaches_the_device_check(tmp_path, collapse):
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="export_mesh needs the model on the GPU"):
        mesh.export(_CpuModel(), str(tmp_path), collapse=collapse, decimate=2)     # both may be given


def test_export_mesh_passes_the_argument_on():
    import inspect
    from mi3d import mesh, renderer
    assert inspect.signature(renderer.NeRFRenderer.export_mesh).parameters["collapse"].default is None
    assert inspect.signature(mesh.export).parameters["collapse"].default is None
    assert "collapse" in renderer.NeRFRenderer.export_mesh.__doc__ and mesh.COLLAPSE_COUNTS == M.COUNTS


def test_binding_build_and_workspace_query():
    import importlib.util
    import os
    from conftest import PKG
    from mi3d import _lib
    for name in ("begin", "rounds", "count", "emit"):
        assert "mi3d_mesh_collapse_" + name in _lib._SIGNATURES
    assert "mi3d_mesh_collapse_workspace" in _lib._LATE_SIGNATURES
    spec = importlib.util.spec_from_file_location("mi3d_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("meshcollapse.hip", ["-ffp-contract=off"]) in b.UNITS and "mi3d_incidence.h" in b.HEADERS
    ws = _lib.lib().mi3d_mesh_collapse_workspace                         # host only: no GPU here
    assert ws(0, 0) == 0 and ws(2 ** 31, 1) == 0 and ws(1, 2 ** 30 + 1) == 0
    for nv, nt in ((1, 0), (0, 1), (3, 1), (255, 256), (1000, 2000), (360_000, 717_602), (2 ** 31 - 1, 2 ** 30)):
        need = int(ws(nv, nt))
        assert need % 8 == 0 and need > 113 * nv + 85 * nt      # every array of the unit's layout
    assert _lib.lib().mi3d_abi_version() == 5
