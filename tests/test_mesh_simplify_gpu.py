"""GPU: mesh simplification by vertex clustering (csrc/meshsimplify.hip through mi3d.mesh.simplify and the C ABI,
include/mi3d.h Part 14).  Every comparison is exact with tests/mesh_simplify_model.py, the NumPy restatement of the
contract: vertices bit for bit, triangles, vertex_map and all eight counts equal.  The inputs are those
tests/test_mesh_simplify_cpu.py shows to contain what they claim: surfaces of the product's own marching cubes, hand-made
boundary, duplicate / degenerate and bad-input meshes, and a 600 x 600 sheet whose rows of block sums need a second
round of the scan, run with the recommended and with the tight workspace.  Then export_mesh with `decimate` and
`target_faces`, end to end."""
import os

import numpy as np
import pytest

import mesh_simplify_model as M
from test_mesh_clean_gpu import R_EXPORT, floaters, model  # noqa: F401  (fixtures: the field and volume of the clean tests)
from test_mesh_cpu import parse_obj

pytestmark = pytest.mark.gpu


def upload(cuda, v, t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).to(cuda), torch.from_numpy(np.ascontiguousarray(t)).to(cuda)


def host(out):
    return tuple(x.cpu().numpy() for x in out[:3])


def assert_same(got, ref, what=""):
    """got: (vertices, triangles, vertex_map, counts) from the GPU as NumPy / list; ref: the model's."""
    assert list(got[3]) == list(ref[3]), (what, got[3], ref[3])
    assert got[0].shape == ref[0].shape and got[0].tobytes() == ref[0].tobytes(), what
    assert got[1].dtype == np.int32 and np.array_equal(got[1], ref[1]), what
    assert got[2].dtype == np.int32 and np.array_equal(got[2], ref[2]), what


def simplify_with_counts(gv, gt, origin, cell):
    from mi3d import mesh
    *out, stats = mesh.simplify(gv, gt, float(cell), origin=[float(o) for o in origin], return_stats=True)
    assert tuple(stats) == M.COUNTS == mesh.SIMPLIFY_COUNTS
    return host(out) + (list(stats.values()),)


def through_the_abi(gv, gt, origin, cell, tight=False, caps=None, fill=None):
    """count, one host read, emit - without mesh.simplify's refusals: (vertices, triangles, vertex_map, counts, lost)."""
    import ctypes as C
    import torch
    from mi3d import _lib
    nv, nt, p, dev = len(gv), len(gt), _lib.ptr, gv.device
    need = int(_lib.lib().mi3d_mesh_simplify_workspace(nv, nt, 1 if tight else 0))
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    counts = torch.full((8,), 99, dtype=torch.int64, device=dev)
    org, cell = (C.c_float * 3)(*[float(o) for o in origin]), float(np.float32(cell))
    _lib.launch("mi3d_mesh_simplify_count", gv, p(gv), nv, p(gt), nt, org, cell, p(ws), need, p(counts))
    c = counts.tolist()
    kv, kt = c[:2] if caps is None else caps
    out_v = torch.full((kv, 3), -7.0 if fill is None else fill, dtype=torch.float32, device=dev)
    out_t = torch.full((kt, 3), -7, dtype=torch.int32, device=dev)
    vmap = torch.full((nv,), -7, dtype=torch.int32, device=dev)
    lost = torch.full((1,), 99, dtype=torch.int64, device=dev)
    _lib.launch("mi3d_mesh_simplify_emit", gv, p(gv), nv, p(gt), nt, org, cell, p(ws), need, p(out_v), kv, p(out_t), kt,
                p(vmap), p(lost))
    return out_v.cpu().numpy(), out_t.cpu().numpy(), vmap.cpu().numpy(), c, int(lost)


# ------------------------------------------------------------------------------------------------ 1, 9: general surfaces

@pytest.fixture(scope="module")
def surfaces(cuda):
    """name -> (R, vertices, triangles as NumPy, the two on the GPU): the product's marching cubes, run once."""
    import torch
    from mi3d import mesh
    out = {}
    for name, (R, make) in M.VOLUMES.items():
        h = 2.0 / (R - 1)
        gv, gt = mesh.marching_cubes(torch.from_numpy(make()).to(cuda), 0.0, origin=(-1.0, -1.0, -1.0), spacing=(h, h, h))
        out[name] = (R, gv.cpu().numpy(), gt.cpu().numpy(), gv, gt)
    return out


@pytest.mark.parametrize("name", list(M.VOLUMES))
def test_surfaces_against_the_model(cuda, surfaces, name):
    from mi3d import mesh
    R, v, t, gv, gt = surfaces[name]
    assert len(v) > 500 and len(t) > 1000
    for what, origin, cell in M.lattices(R, v):
        ref = M.simplify(v, t, origin, cell)
        got = simplify_with_counts(gv, gt, origin, cell)
        assert_same(got, ref, what)
        assert got[3][1] + got[3][6] + got[3][7] + got[3][2] == len(t)
        M.check_geometry(v, origin, cell, *got[:3], radius=0.6 if name.startswith("sphere") else None)
    # origin=None is vertices.amin(0)
    origin, cell = M.lattices(R, v)[-1][1:]
    assert_same(host(mesh.simplify(gv, gt, float(cell))) + ([],), M.simplify(v, t, origin, cell)[:3] + ([],))


# ------------------------------------------------------------------------------------------------ 2, 3: by hand

@pytest.mark.parametrize("case", [M.boundary_case, M.fans_case])
def test_hand_made_cases_against_the_model(cuda, case):
    v, t, origin, cell = case()
    gv, gt = upload(cuda, v, t)
    ref = M.simplify(v, t, origin, cell)
    assert_same(simplify_with_counts(gv, gt, origin, cell), ref)
    got = through_the_abi(gv, gt, origin, cell, tight=True)
    assert_same(got[:4], ref)
    assert got[4] == 0


def test_fans_keep_the_smaller_index_and_its_corner_order(cuda):
    v, t, origin, cell = M.fans_case()
    out_v, out_t, vmap, counts = simplify_with_counts(*upload(cuda, v, t), origin, cell)
    assert out_t.tolist() == [[0, 1, 2], [3, 2, 1]] and counts == [4, 2, 0, 0, 0, 6, 2, 3]
    assert vmap.tolist() == [0, 1, 2, 0, 1, 2, 3, 3, 0, -1, -1, 1, -1]   # E: cited by a dropped triangle; F: by none


# ------------------------------------------------------------------------------------------------ 4: everything collapses

def test_everything_collapses_and_empty_input(cuda, monkeypatch):
    import torch
    from mi3d import _lib, mesh
    v, t = M.sheet(8)
    gv, gt = upload(cuda, v, t)
    out_v, out_t, vmap, stats = mesh.simplify(gv, gt, 100.0, origin=(-0.25, -0.25, -0.25), return_stats=True)
    assert tuple(out_v.shape) == (0, 3) and tuple(out_t.shape) == (0, 3) and out_v.dtype == torch.float32
    assert out_t.dtype == torch.int32 and torch.all(vmap == -1) and len(vmap) == len(v)
    assert stats["degenerate"] == len(t) and stats["clusters"] == 1 and stats["triangles"] == stats["vertices"] == 0
    assert list(stats.values()) == M.simplify(v, t, (-0.25, -0.25, -0.25), 100.0)[3]
    monkeypatch.setattr(_lib, "launch", lambda *a: pytest.fail("an empty mesh launches nothing"))
    e = mesh.simplify(gv[:0], gt[:0], 1.0, return_stats=True)
    assert tuple(e[0].shape) == (0, 3) and tuple(e[1].shape) == (0, 3) and tuple(e[2].shape) == (0,)
    assert e[0].device == gv.device and list(e[3].values()) == [0] * 8


# ------------------------------------------------------------------------------------------------ 5: the sheet

@pytest.fixture(scope="module")
def sheet(cuda):
    v, t = M.sheet()
    return (v, t) + upload(cuda, v, t)


@pytest.mark.parametrize("steps", M.SHEET_CELLS)
def test_sheet_with_the_recommended_and_the_tight_workspace(cuda, sheet, steps):
    from mi3d import _lib
    v, t, gv, gt = sheet
    assert len(v) == 360_000 and len(t) == 717_602 and len(v) > M.SCAN_ROUND and len(t) > M.SCAN_ROUND
    ws = _lib.lib().mi3d_mesh_simplify_workspace
    assert ws(len(v), len(t), 1) < ws(len(v), len(t), 0)
    origin, cell = M.sheet_lattice(steps)
    ref = M.simplify(v, t, origin, cell)
    wide = through_the_abi(gv, gt, origin, cell, tight=False)
    tight = through_the_abi(gv, gt, origin, cell, tight=True)
    assert wide[3][3] == 0 and tight[3][3] == 0 and wide[4] == 0 and tight[4] == 0
    for a, b in zip(wide[:3], tight[:3]):
        assert a.tobytes() == b.tobytes()
    assert wide[3] == tight[3]
    assert_same(wide[:4], ref)


# ------------------------------------------------------------------------------------------------ 6: run to run

@pytest.mark.parametrize("name", ["sphere48", "sphere96"])
def test_run_to_run_and_on_a_side_stream(cuda, surfaces, name):
    import torch
    from mi3d import mesh
    R, v, t, gv, gt = surfaces[name]
    origin, cell = M.export_lattice(R, 2)
    o = [float(x) for x in origin]
    first = host(mesh.simplify(gv, gt, float(cell), origin=o))
    second = host(mesh.simplify(gv, gt, float(cell), origin=o))
    side = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize(cuda)
    with torch.cuda.stream(side):
        third = mesh.simplify(gv, gt, float(cell), origin=o)
    side.synchronize()
    third = host(third)
    for a, b, c in zip(first, second, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()


# ------------------------------------------------------------------------------------------------ 7: bad input

def test_bad_input_is_counted_and_never_dereferenced(cuda):
    """Indices -1, nv and INT32_MAX, a NaN and two infinite vertices: the indices are compared with nv before any load
    (k_sp_insert_t), a non-finite vertex joins no table.  This checks the guard; nothing here reads out of bounds."""
    from mi3d import _lib, mesh
    v, t, origin, cell = M.bad_case()
    gv, gt = upload(cuda, v, t)
    ref = M.simplify(v, t, origin, cell)
    assert ref[3][2] == 5 and ref[3][4] == 3
    got = through_the_abi(gv, gt, origin, cell)
    assert_same(got[:4], ref)
    assert got[4] == 0
    assert got[3][1] + got[3][6] + got[3][7] + got[3][2] == len(t)
    with pytest.raises(_lib.Mi3dError, match=rf"\b3 of the {len(v)} vertices.*\b5 of the {len(t)} triangles"):
        mesh.simplify(gv, gt, float(cell), origin=[float(o) for o in origin])
    with pytest.raises(_lib.Mi3dError, match=r"\b3 of the 300 vertices"):
        mesh.simplify(gv, gt, float(cell))                              # origin=None skips the non-finite coordinates


# ------------------------------------------------------------------------------------------------ 8: the C ABI's checks

def test_c_abi_argument_checks_launch_nothing(cuda):
    """hipErrorInvalidValue (1) for NULL pointers, a bad cell or origin, a workspace below the tight size or misaligned and
    sizes out of range; success (0) without a launch for an empty mesh.  Nothing refused touches its buffers."""
    import ctypes as C
    import torch
    from mi3d import _lib
    lib, p = _lib.lib(), _lib.ptr
    nv, nt = 6, 2
    v = torch.zeros(nv, 3, device=cuda)
    t = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device=cuda)
    vmap = torch.full((nv,), -7, dtype=torch.int32, device=cuda)
    counts = torch.full((8,), 99, dtype=torch.int64, device=cuda)
    lost = torch.full((2,), 99, dtype=torch.int64, device=cuda)
    need, tight = int(lib.mi3d_mesh_simplify_workspace(nv, nt, 0)), int(lib.mi3d_mesh_simplify_workspace(nv, nt, 1))
    assert 0 < tight < need
    ws = torch.full((need // 8 + 2,), -7, dtype=torch.int64, device=cuda)
    out_v, out_t = torch.full((nv, 3), -7.0, device=cuda), torch.full((nt, 3), -7, dtype=torch.int32, device=cuda)
    org = (C.c_float * 3)(0.0, 0.0, 0.0)
    s = _lib.stream(v)
    big = 2 ** 31
    with torch.cuda.device(cuda):
        count = lambda **k: lib.mi3d_mesh_simplify_count(*[k.get(n, d) for n, d in (  # noqa: E731
            ("v", p(v)), ("nv", nv), ("t", p(t)), ("nt", nt), ("org", org), ("cell", 1.0), ("ws", p(ws)), ("need", need),
            ("counts", p(counts)))], s)
        emit = lambda **k: lib.mi3d_mesh_simplify_emit(*[k.get(n, d) for n, d in (  # noqa: E731
            ("v", p(v)), ("nv", nv), ("t", p(t)), ("nt", nt), ("org", org), ("cell", 1.0), ("ws", p(ws)), ("need", need),
            ("out_v", p(out_v)), ("nv_cap", nv), ("out_t", p(out_t)), ("nt_cap", nt), ("vmap", p(vmap)),
            ("lost", p(lost)))], s)
        for k in ("v", "t", "org", "ws", "counts"):
            assert count(**{k: None}) == 1, k
        for k in ("v", "t", "org", "ws", "out_v", "out_t", "vmap", "lost"):
            assert emit(**{k: None}) == 1, k
        for fn in (count, emit):
            for cell in (0.0, -1.0, float("nan"), float("inf")):
                assert fn(cell=cell) == 1, cell
            for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, -float("inf"))):
                assert fn(org=(C.c_float * 3)(*bad)) == 1, bad
            assert fn(need=tight - 1) == 1 and fn(ws=C.c_void_p(ws.data_ptr() + 4)) == 1
            assert fn(nv=big) == 1 and fn(nt=big) == 1
        assert count(counts=C.c_void_p(counts.data_ptr() + 4)) == 1 and emit(lost=C.c_void_p(lost.data_ptr() + 4)) == 1
        # an empty mesh: success, and nothing is launched
        assert count(nv=0, nt=0, v=None, t=None, ws=None, need=0, counts=None) == 0
        assert emit(nv=0, nt=0, v=None, t=None, ws=None, need=0, out_v=None, nv_cap=0, out_t=None, nt_cap=0, vmap=None,
                    lost=None) == 0
    torch.cuda.synchronize(cuda)
    assert torch.all(counts == 99) and torch.all(ws == -7) and torch.all(lost == 99)
    for x in (vmap, out_v, out_t):
        assert torch.all(x == -7)


def test_emit_counts_what_does_not_fit_and_writes_nothing_past_the_caps(cuda, surfaces):
    R, v, t, gv, gt = surfaces["sphere24"]
    origin, cell = M.export_lattice(R, 2)
    rv, rt, rmap, rc = M.simplify(v, t, origin, cell)
    out_v, out_t, vmap, counts, lost = through_the_abi(gv, gt, origin, cell, caps=(len(rv) + 4, len(rt) + 4))
    assert counts == rc and lost == 0                                   # larger buffers: the tail is not touched
    assert out_v[:-4].tobytes() == rv.tobytes() and np.all(out_v[-4:] == -7) and np.all(out_t[-4:] == -7)
    out_v, out_t, vmap, counts, lost = through_the_abi(gv, gt, origin, cell, caps=(len(rv) - 3, len(rt) - 2))
    assert counts == rc and lost == 5
    assert out_v.tobytes() == rv[:-3].tobytes() and np.array_equal(out_t, rt[:-2]) and np.array_equal(vmap, rmap)


def test_python_argument_checks_launch_nothing(cuda, monkeypatch):
    import torch
    from mi3d import _lib, mesh
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    v = torch.zeros(6, 3, device=cuda)
    t = torch.zeros(2, 3, dtype=torch.int32, device=cuda)
    for bv, bt in ((v.cpu(), t), (v, t.cpu()), (v.double(), t), (v, t.long()), (v[:, :2].contiguous(), t), (v, t[0])):
        with pytest.raises(_lib.Mi3dError):
            mesh.simplify(bv, bt, 1.0)
    for kw in ({"cell": 0}, {"cell": float("nan")}, {"cell": "2"}, {"cell": 1.0, "origin": (0, 0)},
               {"cell": 1.0, "origin": (0, float("nan"), 0)}):
        with pytest.raises(_lib.Mi3dError):
            mesh.simplify(v, t, **kw)
    assert calls == []


# ------------------------------------------------------------------------------------------------ 10: export_mesh

def by_hand(uv, ut, d, R=R_EXPORT):
    from mi3d import mesh
    origin, cell = mesh.export_lattice(R, d)
    return mesh.simplify(uv, ut, cell, origin=origin)


def test_export_mesh_decimate_writes_the_simplified_mesh(cuda, model, floaters, tmp_path):
    import torch
    uv, ut = floaters
    ref = M.simplify(uv.cpu().numpy(), ut.cpu().numpy(), *M.export_lattice(R_EXPORT, 2))
    v, f, c = model.export_mesh(str(tmp_path), resolution=R_EXPORT, decimate=2)
    assert v.dtype == np.float32 and f.dtype == np.int32 and c.dtype == np.float32 and c.shape == v.shape
    assert v.tobytes() == ref[0].tobytes() and np.array_equal(f, ref[1]) and 0 < len(f) == ref[3][1] < len(ut)
    with torch.no_grad():
        albedo = model.density(torch.from_numpy(v).to(cuda))["albedo"].float()
    assert c.tobytes() == albedo.cpu().numpy().tobytes()                # the colours of the new vertices
    mtllib, pv, pc, pf, usemtl = parse_obj(tmp_path / "mesh.obj")
    assert len(pf) == ref[3][1] and pf.min() == 1 and pf.max() == len(pv) == len(v)
    assert np.array_equal(pv.astype(np.float32), v) and np.array_equal(pf, f.astype(np.int64) + 1)


def test_export_mesh_textures_and_normals_follow_the_simplified_mesh(cuda, model, floaters, tmp_path):
    from mi3d import mesh
    uv, ut = floaters
    sv, st, _ = by_hand(uv, ut, 2)
    T = 256
    cell, cell_all = mesh.atlas_cell(len(st), T), mesh.atlas_cell(len(ut), T)
    assert cell > cell_all > 0                                          # fewer triangles, larger patches
    v, f, c, vt, image, vn = model.export_mesh(str(tmp_path), resolution=R_EXPORT, texture_size=T, normals=True,
                                               decimate=2)
    assert np.array_equal(f, st.cpu().numpy()) and v.tobytes() == sv.cpu().numpy().tobytes()
    assert c.shape == (len(sv), 3) and vt.shape == (3 * len(st), 2) and image.shape == (T, T, 3) and vn.shape == (len(sv), 3)
    assert round(float(vt[1, 0] - vt[0, 0]) * T) == cell - 2            # include/mi3d.h Part 9, as the clean test reads it
    bi, bvt, _ = mesh.bake_texture(model, sv, st, T)
    assert vt.tobytes() == bvt.cpu().numpy().tobytes() and image.tobytes() == bi.cpu().numpy().tobytes()
    assert vn.tobytes() == mesh.vertex_normals(model, sv).cpu().numpy().tobytes()
    lines = open(tmp_path / "mesh.obj").read().splitlines()
    count = lambda tag: sum(1 for ln in lines if ln.startswith(tag + " "))     # noqa: E731
    assert count("v") == len(sv) and count("vn") == len(sv) and count("vt") == 3 * len(st) and count("f") == len(st)


def test_export_mesh_drops_the_floaters_before_it_clusters(cuda, model, floaters, tmp_path):
    from mi3d import mesh
    uv, ut = floaters
    cv, ct, _ = mesh.clean(uv, ut, min_faces=9)
    assert len(ct) < len(ut)
    sv, st, _ = by_hand(cv, ct, 2)
    v, f, c = model.export_mesh(str(tmp_path), resolution=R_EXPORT, min_faces=9, decimate=2)
    assert v.tobytes() == sv.cpu().numpy().tobytes() and np.array_equal(f, st.cpu().numpy())
    dv, dt, _ = by_hand(uv, ut, 2)                                       # with the specks in: another mesh
    assert len(dt) != len(st)


def test_export_mesh_target_faces_takes_the_first_rung_that_reaches_it(cuda, model, floaters, tmp_path):
    from mi3d import _lib, mesh
    uv, ut = floaters
    rungs = [by_hand(uv, ut, d) for d in mesh.DECIMATE_LADDER[:10]]
    taken = []
    for n, N in enumerate((len(ut) // 2, len(ut) // 8)):                # half, as a user would ask; an eighth: a later rung
        v, f, c = model.export_mesh(str(tmp_path / f"a{n}"), resolution=R_EXPORT, target_faces=N)
        assert 0 < len(f) <= N
        k = next(i for i, (_, st, _) in enumerate(rungs) if len(st) <= N)
        assert np.array_equal(f, rungs[k][1].cpu().numpy()) and v.tobytes() == rungs[k][0].cpu().numpy().tobytes()
        assert len(rungs[k - 1][1]) > N if k > 0 else len(ut) > N       # the next finer rung does not reach it
        taken.append(k)
    assert taken[1] > 0
    # a mesh that already has no more faces stays as it is
    a = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, target_faces=len(ut))
    b = model.export_mesh(str(tmp_path / "c"), resolution=R_EXPORT)
    assert len(a[1]) == len(ut) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # a target nothing reaches
    with pytest.raises(_lib.Mi3dError, match=r"target_faces=1 is not reached"):
        model.export_mesh(str(tmp_path / "d"), resolution=R_EXPORT, target_faces=1)
    assert not os.path.exists(tmp_path / "d" / "mesh.obj")
    with pytest.raises(_lib.Mi3dError, match=r"nothing survives decimate=100: .* 1 clusters"):
        model.export_mesh(str(tmp_path / "d"), resolution=R_EXPORT, decimate=100)


def test_export_mesh_defaults_do_not_touch_the_new_entry_points(cuda, model, floaters, tmp_path, monkeypatch):
    from mi3d import _lib, mesh
    uv, ut = floaters

    def refuse(*a, **k):
        raise AssertionError("the simplifier must not run")
    for name in ("simplify", "_simplify_count", "_simplify_emit", "_decimate"):
        monkeypatch.setattr(mesh, name, refuse)
    seen, launch = [], _lib.launch

    def spy(name, *a):
        seen.append(name)
        return launch(name, *a)
    monkeypatch.setattr(_lib, "launch", spy)
    a = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT)
    b = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, decimate=None, target_faces=None)
    assert "mi3d_mc_emit" in seen and not [n for n in seen if n.startswith("mi3d_mesh_")]
    assert len(a[1]) == len(ut) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for name in ("mesh.obj", "mesh.mtl"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
