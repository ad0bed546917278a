"""GPU: Taubin smoothing of a mesh's vertices (csrc/meshsmooth.hip through mi3d.mesh.smooth and the C ABI, include/mi3d.h
Part 16).  Every comparison is exact with tests/mesh_smooth_model.py, the NumPy restatement of the contract: vertices bit
for bit, all counts equal.  The inputs are those tests/test_mesh_smooth_cpu.py shows to contain what they claim:
surfaces of the product's own marching cubes, an open sheet, a fan of degree 300, fans at and above the degree limit, a
non-manifold and a bad-input mesh, and a 600 x 600 sheet whose degree scan needs a second round.  Then the raw ABI, and
export_mesh with `smooth`, end to end."""
import numpy as np
import pytest

import mesh_smooth_model as M
from test_mesh_clean_gpu import R_EXPORT, floaters, model  # noqa: F401  (fixtures: the field and volume of the clean tests)
from test_mesh_cpu import parse_obj

pytestmark = pytest.mark.gpu


def upload(cuda, v, t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).to(cuda), torch.from_numpy(np.ascontiguousarray(t)).to(cuda)


def smooth_with_counts(gv, gt, its, lam, mu, pin, mm, extent):
    from mi3d import mesh
    out, stats = mesh.smooth(gv, gt, its, lam=lam, mu=mu, pin_border=pin, max_move=mm, extent=extent, return_stats=True)
    assert tuple(stats) == M.COUNTS == mesh.SMOOTH_COUNTS
    return out.cpu().numpy(), list(stats.values())


def assert_same(got, ref, what=""):
    assert list(got[1]) == list(ref[1]), (what, got[1], ref[1])
    assert got[0].dtype == np.float32 and got[0].shape == ref[0].shape and got[0].tobytes() == ref[0].tobytes(), what


def through_the_abi(gv, gt, its, lam, mu, pin, mm, e, poison=-7.0):
    """mi3d_mesh_smooth with poisoned output, workspace and counts: (vertices, counts[0 .. 6]) and counts[7] == 0."""
    import torch
    from mi3d import _lib
    nv, nt, p, dev = len(gv), len(gt), _lib.ptr, gv.device
    need = int(_lib.lib().mi3d_mesh_smooth_workspace(nv, nt))
    assert need % 8 == 0
    ws = torch.full((need // 8,), -0x0101010101010102, dtype=torch.int64, device=dev)
    counts = torch.full((8,), 99, dtype=torch.int64, device=dev)
    out = torch.full((nv, 3), poison, dtype=torch.float32, device=dev)
    _lib.launch("mi3d_mesh_smooth", gv, p(gv), nv, p(gt), nt, its, lam, mu, int(pin), float("inf") if mm is None else mm, e,
                p(ws), need, p(out), p(counts))
    c = counts.tolist()
    assert c[7] == 0
    return out.cpu().numpy(), c[:7]


# ------------------------------------------------------------------------------------------------ general surfaces

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
    """1 and 7 iterations, mu = 0, a max_move that binds, pinning on and off (M.SURFACE_RUNS)."""
    R, v, t, gv, gt = surfaces[name]
    h = 2.0 / (R - 1)
    assert len(v) > 500 and len(t) > 1000
    for its, lam, mu, pin, mm in M.SURFACE_RUNS:
        mm = None if mm is None else float(np.float32(mm * h))
        ref = M.smooth(v, t, its, lam, mu, pin, mm, e=M.EXTENT_E)
        got = smooth_with_counts(gv, gt, its, lam, mu, pin, mm, 1.0)
        assert_same(got, ref, (its, lam, mu, pin, mm))
        assert (got[1][5] > 0) == (mm is not None) and not np.array_equal(got[0], v)


def test_default_extent_reads_the_largest_coordinate(cuda, surfaces):
    from mi3d import mesh
    R, v, t, gv, gt = surfaces["sphere24"]
    big = (v * np.float32(37.5)).astype(np.float32)                     # up to 22.6: e = 33, not the 37 of extent 1
    assert M.fraction_bits(np.abs(big).max()) == 33
    got = mesh.smooth(upload(cuda, big, t)[0], gt, 2).cpu().numpy()
    assert got.tobytes() == M.smooth(big, t, 2)[0].tobytes() == M.smooth(big, t, 2, e=33)[0].tobytes()


# ------------------------------------------------------------------------------------------------ by hand

@pytest.mark.parametrize("name", list(M.HAND_MADE))
def test_hand_made_cases_against_the_model(cuda, name):
    make, extent = M.HAND_MADE[name]
    v, t = make()
    gv, gt = upload(cuda, v, t)
    e = M.fraction_bits(extent)
    for its, lam, mu, pin, mm in M.HAND_RUNS:
        ref = M.smooth(v, t, its, lam, mu, pin, mm, e=e)
        assert_same(smooth_with_counts(gv, gt, its, lam, mu, pin, mm, extent), ref, (name, pin))
        assert_same(through_the_abi(gv, gt, its, lam, mu, pin, mm, e), ref, (name, pin, "abi"))


def test_open_sheet_keeps_its_border_bit_for_bit(cuda):
    v, t = M.open_sheet()
    gv, gt = upload(cuda, v, t)
    ij = np.arange(400)
    edge = (ij // 20 == 0) | (ij // 20 == 19) | (ij % 20 == 0) | (ij % 20 == 19)
    out, counts = smooth_with_counts(gv, gt, 5, M.LAMBDA, M.MU, True, None, 32.0)
    assert counts == [0, 0, 0, 76, 0, 0, 0] and out[edge].tobytes() == v[edge].tobytes()
    assert (out[~edge] != v[~edge]).any(1).all()
    out, counts = smooth_with_counts(gv, gt, 5, M.LAMBDA, M.MU, False, None, 32.0)
    assert counts == [0] * 7 and (out[edge] != v[edge]).any(1).all()


def test_degree_limit_pins_and_counts(cuda):
    v, t = M.degree_limit_case()
    out, counts = smooth_with_counts(*upload(cuda, v, t), 1, M.LAMBDA, M.MU, False, None, 8.0)
    assert counts == [0, 0, 0, 0, 1, 0, 0]
    assert out[1025].tobytes() == v[1025].tobytes() and out[0].tobytes() != v[0].tobytes()


def test_bad_input_is_counted_and_never_dereferenced(cuda):
    """Indices -1, nv and INT32_MAX, a repeated index, a NaN and an infinite vertex: the indices are compared with nv
    before any load (usable() in csrc/meshsmooth.hip), and a row holds corners of usable triangles alone.  This checks
    the guard; nothing here reads out of bounds."""
    v, t = M.bad_case()
    e = M.fraction_bits(M.HAND_MADE["bad"][1])
    ref = M.smooth(v, t, 3, pin_border=False, e=e)
    assert ref[1][0] > 6 and ref[1][1] == 2 and ref[1][2] >= 3
    out, counts = through_the_abi(*upload(cuda, v, t), 3, M.LAMBDA, M.MU, False, None, e)
    assert_same((out, counts), ref)
    assert out[40].tobytes() == v[40].tobytes() and out[90].tobytes() == v[90].tobytes() and out[144].tobytes() == v[144].tobytes()


# ------------------------------------------------------------------------------------------------ the sheet

def test_big_sheet_needs_a_second_round_of_the_scan(cuda):
    v, t = M.big_sheet()
    assert len(v) == 360_000 and len(v) > M.S.SCAN_ROUND
    gv, gt = upload(cuda, v, t)
    for its, mm in ((1, None), (2, 0.1)):
        ref = M.smooth(v, t, its, max_move=mm, e=M.fraction_bits(1024.0))
        assert_same(smooth_with_counts(gv, gt, its, M.LAMBDA, M.MU, True, mm, 1024.0), ref)
        assert ref[1][3] == 4 * 599


# ------------------------------------------------------------------------------------------------ run to run, the ABI

@pytest.mark.parametrize("name", ["sphere48", "sphere96"])
def test_run_to_run_and_on_a_side_stream(cuda, surfaces, name):
    import torch
    from mi3d import mesh
    R, v, t, gv, gt = surfaces[name]
    first = mesh.smooth(gv, gt, 5, extent=1.0).cpu().numpy()
    second = mesh.smooth(gv, gt, 5, extent=1.0).cpu().numpy()
    side = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize(cuda)
    with torch.cuda.stream(side):
        third = mesh.smooth(gv, gt, 5, extent=1.0)
    side.synchronize()
    assert first.tobytes() == second.tobytes() == third.cpu().numpy().tobytes()
    # the triangles in another order: other rows, the same bytes
    perm = torch.randperm(len(gt), device=cuda, generator=torch.Generator(device=cuda).manual_seed(3))
    shuffled = gt[perm].roll(1, dims=1).contiguous()
    assert mesh.smooth(gv, shuffled, 5, extent=1.0).cpu().numpy().tobytes() == first.tobytes()
    # poisoned buffers through the ABI, twice, with two poisons
    a = through_the_abi(gv, gt, 5, M.LAMBDA, M.MU, True, None, M.EXTENT_E, poison=-7.0)
    b = through_the_abi(gv, gt, 5, M.LAMBDA, M.MU, True, None, M.EXTENT_E, poison=float("nan"))
    assert a[0].tobytes() == b[0].tobytes() == first.tobytes() and a[1] == b[1] == [0] * 7


def test_zero_factors_copy_and_mu_zero_is_lambda_only(cuda, surfaces):
    R, v, t, gv, gt = surfaces["torus32"]
    out, counts = through_the_abi(gv, gt, 4, 0.0, 0.0, True, 0.5, M.EXTENT_E)
    assert out.tobytes() == v.tobytes() and counts == [0] * 7          # no pass is launched: the input, copied
    for lam, mu in ((M.LAMBDA, 0.0), (0.0, M.MU)):                      # an odd and an even number of launched passes
        for its in (3, 4):
            assert_same(through_the_abi(gv, gt, its, lam, mu, True, None, M.EXTENT_E), M.smooth(v, t, its, lam, mu, e=M.EXTENT_E))


def test_c_abi_argument_checks_launch_nothing(cuda):
    """hipErrorInvalidValue (1) for NULL pointers, iterations, factors, max_move and fraction bits out of range, aliasing
    output, a workspace that is too small or misaligned and sizes out of range; success (0) without a launch for an
    empty mesh.  Nothing refused touches its buffers."""
    import ctypes as C
    import torch
    from mi3d import _lib
    lib, p = _lib.lib(), _lib.ptr
    nv, nt = 6, 2
    v = torch.zeros(nv, 3, device=cuda)
    t = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device=cuda)
    counts = torch.full((8,), 99, dtype=torch.int64, device=cuda)
    need = int(lib.mi3d_mesh_smooth_workspace(nv, nt))
    assert need > 0
    ws = torch.full((need // 8 + 2,), -7, dtype=torch.int64, device=cuda)
    out = torch.full((nv, 3), -7.0, device=cuda)
    s = _lib.stream(v)
    nan, inf = float("nan"), float("inf")
    with torch.cuda.device(cuda):
        call = lambda **k: lib.mi3d_mesh_smooth(*[k.get(n, d) for n, d in (  # noqa: E731
            ("v", p(v)), ("nv", nv), ("t", p(t)), ("nt", nt), ("its", 2), ("lam", 0.5), ("mu", -0.53), ("pin", 1),
            ("mm", inf), ("e", 37), ("ws", p(ws)), ("need", need), ("out", p(out)), ("counts", p(counts)))], s)
        for k in ("v", "t", "ws", "out", "counts"):
            assert call(**{k: None}) == 1, k
        for bad in ({"its": 0}, {"its": 1001}, {"lam": 1.5}, {"lam": nan}, {"mu": -1.5}, {"mu": inf}, {"mm": -1.0},
                    {"mm": nan}, {"e": 41}, {"nv": 2 ** 31}, {"nt": 2 ** 30 + 1}, {"need": need - 1}, {"out": p(v)},
                    {"ws": C.c_void_p(ws.data_ptr() + 4)}, {"counts": C.c_void_p(counts.data_ptr() + 4)}):
            assert call(**bad) == 1, bad
        # an empty mesh: success, and nothing is launched
        assert call(nv=0, nt=0, v=None, t=None, ws=None, need=0, out=None, counts=None) == 0
        assert call(nv=0, v=None, ws=None, need=0, out=None, counts=None) == 0
    torch.cuda.synchronize(cuda)
    assert torch.all(counts == 99) and torch.all(ws == -7) and torch.all(out == -7)


def test_empty_input_launches_nothing(cuda, monkeypatch):
    import torch
    from mi3d import _lib, mesh
    v = torch.zeros(0, 3, device=cuda)
    t = torch.zeros(0, 3, dtype=torch.int32, device=cuda)
    monkeypatch.setattr(_lib, "launch", lambda *a: pytest.fail("an empty mesh launches nothing"))
    out, stats = mesh.smooth(v, t, 3, return_stats=True)
    assert tuple(out.shape) == (0, 3) and out.device == v.device and list(stats.values()) == [0] * 7


# ------------------------------------------------------------------------------------------------ export_mesh

def test_export_mesh_smooth_moves_the_vertices_alone(cuda, model, floaters, tmp_path):
    import torch
    from mi3d import mesh
    uv, ut = floaters
    v0, f0, c0 = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT)
    v, f, c = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, smooth=3)
    assert np.array_equal(f, f0) and v.shape == v0.shape and v.dtype == np.float32
    sv = mesh.smooth(uv, ut, 3, extent=1.0)
    assert v.tobytes() == sv.cpu().numpy().tobytes() == M.smooth(v0, f0, 3, e=M.EXTENT_E)[0].tobytes()
    assert not np.array_equal(v, v0)
    with torch.no_grad():
        albedo = model.density(torch.from_numpy(v).to(cuda))["albedo"].float()
    assert c.tobytes() == albedo.cpu().numpy().tobytes()                # the colours of the moved vertices
    mtllib, pv, pc, pf, usemtl = parse_obj(tmp_path / "b" / "mesh.obj")
    assert np.array_equal(pv.astype(np.float32), v) and np.array_equal(pf, f.astype(np.int64) + 1)
    # the dict form: max_move in grid steps
    h = 2.0 / (R_EXPORT - 1)
    opts = dict(iterations=4, lam=0.6, mu=-0.62, pin_border=False, max_move=0.05)
    v2 = model.export_mesh(str(tmp_path / "c"), resolution=R_EXPORT, smooth=opts)[0]
    ref = M.smooth(v0, f0, 4, 0.6, -0.62, False, float(np.float32(0.05 * h)), e=M.EXTENT_E)
    mm = np.float32(0.05 * h)
    assert v2.tobytes() == ref[0].tobytes() and ref[1][5] > 0 and np.all(v2 >= v0 - mm) and np.all(v2 <= v0 + mm)


def test_export_mesh_smooths_after_the_filter_and_the_decimation(cuda, model, floaters, tmp_path):
    from mi3d import mesh
    uv, ut = floaters
    cv, ct, _ = mesh.clean(uv, ut, min_faces=9)
    origin, cell = mesh.export_lattice(R_EXPORT, 2)
    dv, dt, _ = mesh.simplify(cv, ct, cell, origin=origin)
    v, f, c = model.export_mesh(str(tmp_path), resolution=R_EXPORT, min_faces=9, decimate=2, smooth=2)
    assert np.array_equal(f, dt.cpu().numpy())
    assert v.tobytes() == mesh.smooth(dv, dt, 2, extent=1.0).cpu().numpy().tobytes()


def test_export_mesh_texture_and_normals_see_the_smoothed_vertices(cuda, model, floaters, tmp_path):
    from mi3d import mesh
    uv, ut = floaters
    sv = mesh.smooth(uv, ut, 3, extent=1.0)
    T = 256
    v, f, c, vt, image, vn = model.export_mesh(str(tmp_path), resolution=R_EXPORT, texture_size=T, normals=True, smooth=3)
    assert v.tobytes() == sv.cpu().numpy().tobytes() and np.array_equal(f, ut.cpu().numpy())
    bi, bvt, _ = mesh.bake_texture(model, sv, ut, T)
    assert vt.tobytes() == bvt.cpu().numpy().tobytes() and image.tobytes() == bi.cpu().numpy().tobytes()
    assert vn.tobytes() == mesh.vertex_normals(model, sv).cpu().numpy().tobytes()   # the field's normal at the moved vertex
    lines = open(tmp_path / "mesh.obj").read().splitlines()
    count = lambda tag: sum(1 for ln in lines if ln.startswith(tag + " "))     # noqa: E731
    assert count("v") == len(sv) and count("vn") == len(sv) and count("vt") == 3 * len(ut) and count("f") == len(ut)


def test_export_mesh_without_smooth_does_not_touch_the_new_entry_point(cuda, model, floaters, tmp_path, monkeypatch):
    from mi3d import _lib, mesh

    def refuse(*a, **k):
        raise AssertionError("the smoother must not run")
    for name in ("smooth", "_smooth_export"):
        monkeypatch.setattr(mesh, name, refuse)
    seen, launch = [], _lib.launch

    def spy(name, *a):
        seen.append(name)
        return launch(name, *a)
    monkeypatch.setattr(_lib, "launch", spy)
    a = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT, texture_size=128)
    b = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, texture_size=128, smooth=None)
    assert "mi3d_mc_emit" in seen and "mi3d_mesh_smooth" not in seen
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for name in ("mesh.obj", "mesh.mtl", "albedo.png"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
