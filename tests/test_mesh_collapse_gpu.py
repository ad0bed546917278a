"""GPU: quadric edge-collapse decimation (csrc/meshcollapse.hip through mi3d.mesh.collapse and the C ABI, include/mi3d.h
Part 19).  Every comparison is exact with tests/mesh_collapse_model.py, the restatement of the contract: the vertices bit
for bit, the triangles, the vertex map and all eight counts equal.  The inputs are those tests/test_mesh_collapse_cpu.py
holds to the contract's properties: surfaces of the product's own marching cubes, the cubes, an open sheet, a fan above the
degree limit, bad indices and non-finite vertices.  Then the batching of the rounds, run to run, the raw ABI, emit into
short buffers, a 600 x 600 sheet whose scans need a second and a third round, and export_mesh with `collapse`."""
import numpy as np
import pytest

import mesh_collapse_model as M
import mesh_simplify_model as S
from test_mesh_clean_gpu import R_EXPORT, floaters, model  # noqa: F401  (fixtures: the field and volume of the clean tests)
from test_mesh_collapse_cpu import check_output, topology
from test_mesh_cpu import parse_obj

pytestmark = pytest.mark.gpu

SURFACES = ("sphere24", "torus32", "two_spheres32", "shell32")


def upload(cuda, v, t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).to(cuda), torch.from_numpy(np.ascontiguousarray(t)).to(cuda)


def collapse_gpu(gv, gt, target, **kw):
    """mesh.collapse -> (vertices, triangles, vertex_map as NumPy, the eight counts as the ABI packs them, stats)."""
    from mi3d import mesh
    out_v, out_t, vm, stats = mesh.collapse(gv, gt, target, return_stats=True, **kw)
    assert tuple(stats)[:8] == M.COUNTS == mesh.COLLAPSE_COUNTS
    counts = [stats[k] for k in M.COUNTS]
    counts[2] |= stats["planeless_triangles"] << 32
    return out_v.cpu().numpy(), out_t.cpu().numpy(), vm.cpu().numpy(), counts, stats


def assert_same(got, ref, what=""):
    assert list(got[3]) == list(ref[3]), (what, got[3], ref[3])
    for g, r, dtype in zip(got[:3], ref[:3], (np.float32, np.int32, np.int32)):
        assert g.dtype == r.dtype == dtype and g.shape == r.shape and g.tobytes() == r.tobytes(), what


def against_the_model(cuda, v, t, target, **kw):
    ref = M.collapse(v, t, target, **kw)
    got = collapse_gpu(*upload(cuda, v, t), target, **kw)
    assert_same(got, ref, (target, kw))
    return got, ref


# ------------------------------------------------------------------------------------------------ against the model

@pytest.fixture(scope="module")
def surfaces(cuda):
    """name -> (vertices, triangles as NumPy, the two on the GPU): the product's marching cubes, run once."""
    import torch
    from mi3d import mesh
    out = {}
    for name in SURFACES + ("sphere96",):
        R, make = S.VOLUMES[name]
        h = 2.0 / (R - 1)
        gv, gt = mesh.marching_cubes(torch.from_numpy(make()).to(cuda), 0.0, origin=(-1.0, -1.0, -1.0), spacing=(h, h, h))
        out[name] = (gv.cpu().numpy(), gt.cpu().numpy(), gv, gt)
    return out


@pytest.mark.parametrize("part", [2, 10])
@pytest.mark.parametrize("name", SURFACES)
def test_surfaces_against_the_model(cuda, surfaces, name, part):
    v, t, gv, gt = surfaces[name]
    target = len(t) // part
    ref = M.collapse(v, t, target)
    got = collapse_gpu(gv, gt, target)
    assert_same(got, ref, name)
    check_output(v, t, *got[:3])
    assert got[3][1] in (target, target - 1) and got[4]["done"] and not got[4]["stalled"]
    assert got[3][5] == (len(t) - got[3][1]) // 2 and got[3][7] == 0


@pytest.mark.parametrize("n", [2, 3, 6])
def test_cubes_against_the_model(cuda, n):
    v, t = M.cube(n)
    got, ref = against_the_model(cuda, v, t, 12)
    assert got[3][:2] == [8, 12] and M.enclosed_volume(got[0], got[1]) == 8.0


def test_open_sheet_against_the_model(cuda):
    v, t = M.open_sheet()
    got, ref = against_the_model(cuda, v, t, len(t) // 4)
    check_output(v, t, *got[:3], closed=False)
    assert got[3][6] == 76 and got[3][1] < len(t)


def test_fan_above_the_degree_limit_is_locked_and_counted(cuda):
    v, t = M.fan100()
    got, ref = against_the_model(cuda, v, t, 10)
    assert got[3][6] == 101 and got[3][5] == 0 and np.array_equal(got[1], t) and got[4]["stalled"]


def test_bad_indices_and_non_finite_vertices_are_counted_and_never_dereferenced(cuda):
    v, t = M.bad_case()
    got, ref = against_the_model(cuda, v, t, 60)
    assert got[3][2] == int((~M.SM.usable_triangles(v, t)).sum()) > 0 and got[3][4] == 2
    # a triangle without a plane: three collinear vertices, counted in the upper word
    v2 = np.concatenate([v, [[50, 50, 50], [51, 51, 51], [52, 52, 52]]]).astype(np.float32)
    t2 = np.concatenate([t, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    got, ref = against_the_model(cuda, v2, t2, 60)
    assert got[3][2] >> 32 == 1 and got[4]["planeless_triangles"] == 1
    # the triangle soup of the simplification tests: indices -1, nv and INT32_MAX, a NaN and two infinite vertices
    v, t = S.bad_case()[:2]
    got, ref = against_the_model(cuda, v, t, 10)
    assert got[3][2] & 0xFFFFFFFF == int((~M.SM.usable_triangles(v, t)).sum()) == 6 and got[3][4] == 3


def test_target_at_or_above_the_face_count_returns_the_usable_triangles(cuda):
    v, t = M.bad_case()
    for target in (int(M.SM.usable_triangles(v, t).sum()), len(t), 10 ** 12):
        got, ref = against_the_model(cuda, v, t, target)
        assert got[3][3] == 0 and got[4]["done"]
    v, t = M.tetrahedron()
    got, ref = against_the_model(cuda, v, t, 0)
    assert got[3] == [4, 4, 0, 0, 0, 0, 0, 0] and got[4]["stalled"] and not got[4]["done"]


def test_sphere_down_to_a_tetrahedron(cuda):
    v, t = M.octa_sphere(3)
    got, ref = against_the_model(cuda, v, t, 4)
    assert got[3][:2] == [4, 4] and M.enclosed_volume(got[0], got[1]) > 0.0


def test_a_finite_max_error_stops_the_run_early(cuda):
    v, t = M.octa_sphere(3)
    got, ref = against_the_model(cuda, v, t, 60, max_error=M.STALL_ERROR)
    assert 60 < got[3][1] < len(t) and got[3][5] > 0 and got[4]["stalled"] and not got[4]["done"]
    got, ref = against_the_model(cuda, v, t, 60, max_error=0.0)
    assert got[4]["stalled"]
    got, ref = against_the_model(cuda, v, t, 60, max_rounds=3)          # out of rounds: neither done nor stalled
    assert got[3][3] == 3 and not got[4]["done"] and not got[4]["stalled"]


def test_empty_input_launches_nothing(cuda, monkeypatch):
    import torch
    from mi3d import _lib, mesh
    v = torch.zeros(0, 3, device=cuda)
    t = torch.zeros(0, 3, dtype=torch.int32, device=cuda)
    monkeypatch.setattr(_lib, "launch", lambda *a: pytest.fail("an empty mesh launches nothing"))
    out_v, out_t, vm, stats = mesh.collapse(v, t, 5, return_stats=True)
    assert tuple(out_v.shape) == (0, 3) and tuple(out_t.shape) == (0, 3) and tuple(vm.shape) == (0,)
    assert [stats[k] for k in M.COUNTS] == [0] * 8 == M.collapse(np.zeros((0, 3)), np.zeros((0, 3)), 5)[3]


def test_vertices_without_triangles_and_triangles_without_vertices(cuda):
    import torch
    v = np.arange(15, dtype=np.float32).reshape(5, 3)
    got, ref = against_the_model(cuda, v, np.zeros((0, 3), np.int32), 3)
    assert got[3] == [0] * 8 and np.array_equal(got[2], np.full(5, -1))
    got, ref = against_the_model(cuda, np.zeros((0, 3), np.float32), np.array([[0, 1, 2], [2, 1, 0]], np.int32), 3)
    assert got[3] == [0, 0, 2, 0, 0, 0, 0, 0]
    torch.cuda.synchronize(cuda)


# ------------------------------------------------------------------------------------------------ batching, run to run

def test_rounds_per_read_changes_no_byte(cuda, surfaces):
    v, t, gv, gt = surfaces["torus32"]
    eight = collapse_gpu(gv, gt, len(t) // 10)
    one = collapse_gpu(gv, gt, len(t) // 10, rounds_per_read=1)
    many = collapse_gpu(gv, gt, len(t) // 10, rounds_per_read=100)
    assert_same(one, eight)
    assert_same(many, eight)
    assert one[4]["rounds_launched"] == one[3][3] + 1 and eight[4]["rounds_launched"] % 8 == 0


def through_the_abi(gv, gt, target, max_error, rounds, poison):
    """begin, `rounds` rounds in one call, count, emit - with poisoned workspace, counts and outputs."""
    import torch
    from mi3d import _lib
    nv, nt, p, dev = len(gv), len(gt), _lib.ptr, gv.device
    need = int(_lib.lib().mi3d_mesh_collapse_workspace(nv, nt))
    assert need % 8 == 0
    ws = torch.full((need // 8,), poison, dtype=torch.int64, device=dev)
    counts = torch.full((8,), 99, dtype=torch.int64, device=dev)
    _lib.launch("mi3d_mesh_collapse_begin", gv, p(gv), nv, p(gt), nt, p(ws), need, p(counts))
    _lib.launch("mi3d_mesh_collapse_rounds", gv, nv, nt, target, max_error, rounds, p(ws), need, p(counts))
    _lib.launch("mi3d_mesh_collapse_count", gv, nv, nt, p(ws), need, p(counts))
    kv, kt = counts.tolist()[:2]
    out_v = torch.full((kv + 1, 3), -7.0, dtype=torch.float32, device=dev)
    out_t = torch.full((kt + 1, 3), -7, dtype=torch.int32, device=dev)
    vm = torch.full((nv,), -7, dtype=torch.int32, device=dev)
    _lib.launch("mi3d_mesh_collapse_emit", gv, nv, nt, p(ws), need, p(out_v), kv, p(out_t), kt, p(vm), p(counts))
    assert torch.all(out_v[kv] == -7.0) and torch.all(out_t[kt] == -7)          # nothing past the caps
    return out_v[:kv].cpu().numpy(), out_t[:kt].cpu().numpy(), vm.cpu().numpy(), counts.tolist(), (ws, need, counts)


def test_run_to_run_on_a_side_stream_and_through_the_abi(cuda, surfaces):
    import torch
    v, t, gv, gt = surfaces["sphere96"]
    target = len(t) // 10
    first = collapse_gpu(gv, gt, target)
    second = collapse_gpu(gv, gt, target)
    side = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize(cuda)
    with torch.cuda.stream(side):
        third = collapse_gpu(gv, gt, target)
    side.synchronize()
    assert_same(second, first)
    assert_same(third, first)
    check_output(v, t, *first[:3])
    assert first[3][1] in (target, target - 1)
    # poisoned buffers through the ABI, with two poisons; 64 rounds in one call, the no-op rounds included
    assert first[3][3] < 64
    a = through_the_abi(gv, gt, target, float("inf"), 64, -0x0101010101010102)
    b = through_the_abi(gv, gt, target, float("inf"), 64, 0x7FF8000000000001)
    assert_same(a, first)
    assert_same(b, first)


def test_emit_into_short_buffers_writes_nothing_past_them_and_counts(cuda, surfaces):
    import torch
    from mi3d import _lib
    v, t, gv, gt = surfaces["sphere24"]
    full = through_the_abi(gv, gt, len(t) // 2, float("inf"), 16, 0)
    ws, need, counts = full[4]
    kv, kt = full[3][:2]
    nv, nt, p = len(gv), len(gt), _lib.ptr
    out_v = torch.full((kv, 3), -7.0, dtype=torch.float32, device=cuda)
    out_t = torch.full((kt, 3), -7, dtype=torch.int32, device=cuda)
    vm = torch.full((nv,), -7, dtype=torch.int32, device=cuda)
    _lib.launch("mi3d_mesh_collapse_emit", gv, nv, nt, p(ws), need, p(out_v), kv - 5, p(out_t), kt - 9, p(vm), p(counts))
    assert counts.tolist()[7] == 5 + 9
    assert torch.all(out_v[kv - 5:] == -7.0) and torch.all(out_t[kt - 9:] == -7)
    assert out_v[:kv - 5].cpu().numpy().tobytes() == full[0][:kv - 5].tobytes()
    assert np.array_equal(out_t[:kt - 9].cpu().numpy(), full[1][:kt - 9]) and np.array_equal(vm.cpu().numpy(), full[2])


def test_c_abi_argument_checks_launch_nothing(cuda):
    """hipErrorInvalidValue (1) for NULL pointers, a max_error that is negative or NaN, too many rounds, a workspace that
    is too small or misaligned, a misaligned counts and sizes out of range; success (0) without a launch for an empty
    mesh.  Nothing refused touches its buffers."""
    import ctypes as C
    import torch
    from mi3d import _lib
    lib, p = _lib.lib(), _lib.ptr
    nv, nt = 6, 2
    v = torch.zeros(nv, 3, device=cuda)
    t = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device=cuda)
    counts = torch.full((8,), 99, dtype=torch.int64, device=cuda)
    need = int(lib.mi3d_mesh_collapse_workspace(nv, nt))
    assert need > 0
    ws = torch.full((need // 8 + 2,), -7, dtype=torch.int64, device=cuda)
    out_v = torch.full((nv, 3), -7.0, device=cuda)
    out_t = torch.full((nt, 3), -7, dtype=torch.int32, device=cuda)
    vm = torch.full((nv,), -7, dtype=torch.int32, device=cuda)
    s = _lib.stream(v)
    state = (("nv", nv), ("nt", nt))
    tail = (("ws", p(ws)), ("need", need))
    entries = {
        "begin": (lib.mi3d_mesh_collapse_begin, (("v", p(v)), ("nv", nv), ("t", p(t)), ("nt", nt)) + tail + (("counts", p(counts)),)),
        "rounds": (lib.mi3d_mesh_collapse_rounds, state + (("target", 1), ("err", float("inf")), ("n", 2)) + tail
                   + (("counts", p(counts)),)),
        "count": (lib.mi3d_mesh_collapse_count, state + tail + (("counts", p(counts)),)),
        "emit": (lib.mi3d_mesh_collapse_emit, state + tail + (("out_v", p(out_v)), ("nv_cap", nv), ("out_t", p(out_t)),
                                                              ("nt_cap", nt), ("vm", p(vm)), ("counts", p(counts)))),
    }
    with torch.cuda.device(cuda):
        for name, (fn, args) in entries.items():
            call = lambda **k: fn(*[k.get(n, d) for n, d in args], s)   # noqa: E731
            pointers = [n for n, _ in args if n in ("v", "t", "ws", "counts", "out_v", "out_t", "vm")]
            for k in pointers:
                assert call(**{k: None}) == 1, (name, k)
            bad = [{"nv": 2 ** 31}, {"nt": 2 ** 30 + 1}, {"need": need - 1}, {"ws": C.c_void_p(ws.data_ptr() + 4)},
                   {"counts": C.c_void_p(counts.data_ptr() + 4)}]
            if name == "rounds":
                bad += [{"err": -1.0}, {"err": float("nan")}, {"n": 4097}]
            for b in bad:
                assert call(**b) == 1, (name, b)
            empty = {n: None for n in pointers}
            assert call(nv=0, nt=0, need=0, **empty) == 0, name          # an empty mesh: success, nothing launched
    torch.cuda.synchronize(cuda)
    assert torch.all(counts == 99) and torch.all(ws == -7) and torch.all(out_v == -7) and torch.all(out_t == -7)
    assert torch.all(vm == -7)


# ------------------------------------------------------------------------------------------------ the big sheet

def test_big_sheet_reaches_the_later_rounds_of_the_scans(cuda):
    """360 000 vertices are 1 407 workgroups, 717 602 triangles 2 804: scan_row's second and third round of 1 024.  The
    model is not asked (it is not fast): two runs give the same bytes, and the properties hold."""
    v, t = S.sheet()
    n = S.SHEET
    assert len(v) == 360_000 > S.SCAN_ROUND and len(t) == 717_602 > 2 * S.SCAN_ROUND
    gv, gt = upload(cuda, v, t)
    first = collapse_gpu(gv, gt, len(t) // 2, max_rounds=6)
    second = collapse_gpu(gv, gt, len(t) // 2, max_rounds=6, rounds_per_read=1)
    assert_same(second, first)
    out_v, out_t, vm, counts, stats = first
    assert counts[7] == 0 and 4 <= counts[3] <= 6 and counts[5] > 50_000 and counts[1] == len(t) - 2 * counts[5]
    check_output(v, t, out_v, out_t, vm, closed=False)
    assert topology(out_t, len(out_v))[:3] == (1, 1, 4 * (n - 1))      # a disc, one piece, its border edges all there
    i, j = np.divmod(np.arange(n * n), n)
    border = np.nonzero((i == 0) | (i == n - 1) | (j == 0) | (j == n - 1))[0]
    assert counts[6] == len(border) and out_v[vm[border]].tobytes() == v[border].tobytes()
    assert np.all(out_v[:, 2] == 0.0)                                   # a flat sheet stays flat
    a, b, c = (out_v[out_t[:, k]].astype(np.float64) for k in range(3))
    assert np.all(np.cross(b - a, c - a)[:, 2] > 0.0)                   # no triangle flipped


# ------------------------------------------------------------------------------------------------ export_mesh

def test_export_mesh_collapse_end_to_end(cuda, model, floaters, tmp_path):
    import torch
    from mi3d import mesh
    uv, ut = floaters
    cv, ct, _ = mesh.clean(uv, ut, min_faces=9)
    target = len(ct) // 4
    ref = M.collapse(cv.cpu().numpy(), ct.cpu().numpy(), target)
    v, f, c = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT, min_faces=9, collapse=target)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert v.tobytes() == ref[0].tobytes() and np.array_equal(f, ref[1]) and len(f) in (target, target - 1)
    with torch.no_grad():
        albedo = model.density(torch.from_numpy(v).to(cuda))["albedo"].float()
    assert c.tobytes() == albedo.cpu().numpy().tobytes()                # the colours of the new vertices, from the field
    mtllib, pv, pc, pf, usemtl = parse_obj(tmp_path / "a" / "mesh.obj")
    assert np.array_equal(pv.astype(np.float32), v) and np.array_equal(pf, f.astype(np.int64) + 1)
    # after the clustering, before the smoothing; the dict form
    origin, cell = mesh.export_lattice(R_EXPORT, 1.5)
    dv, dt, _ = mesh.simplify(cv, ct, cell, origin=origin)
    opts = dict(target_faces=len(dt) // 2, max_error=1.0, max_rounds=40)
    kv, kt, _ = mesh.collapse(dv, dt, opts["target_faces"], max_error=1.0, max_rounds=40)
    v2, f2, _ = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, min_faces=9, decimate=1.5, collapse=opts, smooth=2)
    assert np.array_equal(f2, kt.cpu().numpy()) and len(f2) < len(dt)
    assert v2.tobytes() == mesh.smooth(kv, kt, 2, extent=1.0).cpu().numpy().tobytes()
    # texture and normals see the collapsed mesh
    T = 256
    v3, f3, c3, vt, image, vn = model.export_mesh(str(tmp_path / "c"), resolution=R_EXPORT, texture_size=T, normals=True,
                                                  min_faces=9, collapse=target)
    assert v3.tobytes() == v.tobytes() and np.array_equal(f3, f) and vt.shape == (3 * len(f), 2)
    gv3, gf3 = upload(cuda, v3, f3)
    bi, bvt, _ = mesh.bake_texture(model, gv3, gf3, T)
    assert vt.tobytes() == bvt.cpu().numpy().tobytes() and image.tobytes() == bi.cpu().numpy().tobytes()
    assert vn.tobytes() == mesh.vertex_normals(model, gv3).cpu().numpy().tobytes()


def test_export_mesh_without_collapse_does_not_touch_the_new_entry_points(cuda, model, floaters, tmp_path, monkeypatch):
    from mi3d import _lib, mesh

    def refuse(*a, **k):
        raise AssertionError("the collapse must not run")
    for name in ("collapse", "_collapse_export"):
        monkeypatch.setattr(mesh, name, refuse)
    seen, launch = [], _lib.launch

    def spy(name, *a):
        seen.append(name)
        return launch(name, *a)
    monkeypatch.setattr(_lib, "launch", spy)
    a = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT, texture_size=128)
    b = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, texture_size=128, collapse=None)
    assert "mi3d_mc_emit" in seen and not any("collapse" in name for name in seen)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for name in ("mesh.obj", "mesh.mtl", "albedo.png"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
