"""GPU: marching cubes (csrc/mesh.hip through mi3d.mesh.marching_cubes) against the NumPy restatement of
tests/test_mc_tables_cpu.py - bit for bit and in order - and against properties that do not pass through the
restatement (closed, oriented, Euler characteristic, distance to the analytic surface); then mesh export of a model:
the sampled volume against the field itself and the oracle, the files against the returned arrays."""
import os

import numpy as np
import pytest

from test_mc_tables_cpu import (assert_closed_and_oriented, edge_uses, marching_cubes_ref, signed_volume,
                                sphere_volume)
from test_mesh_cpu import parse_obj

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the volumes

def _grid(R):
    ax = np.linspace(-1, 1, R)
    return np.meshgrid(ax, ax, ax, indexing="ij")


def _box_frame(R):
    h = float(np.float32(2.0 / (R - 1)))
    return (-1.0, -1.0, -1.0), (h, h, h)


INDEX_FRAME = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
R0 = 0.6


def vol_a():
    return sphere_volume(48, R0), 0.0, _box_frame(48)


def vol_b():
    x, y, z = _grid(64)
    return (0.2 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).astype(np.float32), 0.0, _box_frame(64)


def vol_c():
    return np.maximum(sphere_volume(48, 0.3, (0.5, 0, 0)), sphere_volume(48, 0.3, (-0.5, 0, 0))), 0.0, _box_frame(48)


def vol_d():
    return np.random.default_rng(0).random((33, 40, 29), dtype=np.float32), 0.5, INDEX_FRAME


def vol_e():
    x, _, _ = _grid(32)
    return (x - 0.3).astype(np.float32), 0.0, INDEX_FRAME


def vol_f():
    return np.full((16, 16, 16), -1.0, np.float32), 0.0, INDEX_FRAME


def vol_g():
    v, iso, frame = vol_a()
    v = v.copy()
    assert v[24, 24, 24] > 0.5
    v[24, 24, 24] = np.nan                                  # outside by the rule: a cavity in the middle of the ball
    i0 = int(np.argmax(v[:, 24, 24] >= 0))                  # the first inside voxel of the row: its -x neighbour is outside
    assert i0 > 0 and v[i0 - 1, 24, 24] < 0 <= v[i0, 24, 24]
    v[i0, 24, 24] = np.inf
    return v, iso, frame


def vol_h(rest):
    v = np.full((3, 3, 3), rest, np.float32)
    v[1, 1, 1] = 0.25
    return v, 0.25, INDEX_FRAME


MC_BLOCK = 256                # kBlock of csrc/mesh.hip: grid points per workgroup of k_mc_count / k_mc_vertices / k_mc_triangles
MC_SCAN_ROUND = 1024          # block sums per round of k_mc_scan: kRowThreads of scan_row in csrc/mi3d_scan.h
FIRST_ROUND = MC_SCAN_ROUND * MC_BLOCK       # grid points whose block offsets the scan's first round makes


def _ball(shape, centre, r0):
    """r0 - distance to `centre`, both in grid units (the index frame)."""
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (r0 - np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2)).astype(np.float32)


def vol_i():
    """65 x 64 x 64 = 266 240 points, 1040 blocks: the blocks of the second scan round are the plane i = 64, whose points own
    only edges inside that plane and no cell.  The ball is pushed so far towards high i that this plane cuts it: a cap
    is missing, the cut's rim consists of vertices owned by blocks >= 1024."""
    return _ball((65, 64, 64), (59.3, 31.4, 30.7), 10.2), 0.0, INDEX_FRAME


def vol_j():
    """A closed ball across the round boundary, which needs more planes behind it: 72 x 64 x 64 = 1152 blocks, the surface
    spans i = 54.7 .. 69.9 - vertices and triangles on both sides of block 1024, so the second round's offsets start
    from a base that is not 0."""
    return _ball((72, 64, 64), (62.3, 31.4, 30.7), 7.6), 0.0, INDEX_FRAME


def vol_k():
    """3 x 300 x 300 = 270 000 points, 1055 blocks, a ragged second round; crossings everywhere.  (Coordinates above 256
    carry 15 fraction bits, so a vertex may round onto a grid point and meet a neighbour there: with this seed none does,
    which test_vertices_are_welded needs.)"""
    return np.random.default_rng(1).random((3, 300, 300), dtype=np.float32), 0.5, INDEX_FRAME


VOLUMES = {"a": vol_a, "b": vol_b, "c": vol_c, "d": vol_d, "e": vol_e, "f": vol_f, "g": vol_g,
           "h_below": lambda: vol_h(-1.0), "h_above": lambda: vol_h(1.0), "i": vol_i, "j": vol_j, "k": vol_k}
SECOND_ROUND = ("i", "j", "k")


def owned_elements(vol, iso, first, last=None):
    """(vertices, triangles) the grid points with linear index in [first, last) own, counted from the volume alone: crossing
    edges towards +axis, and the non-trivial cells they are the min corner of (a trivial cell has all corners on one side)."""
    ins = (vol >= iso).reshape(vol.shape)
    lin = np.arange(vol.size).reshape(vol.shape)
    sel = (lin >= first) & (lin < (vol.size if last is None else last))
    nv = 0
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        nv += int(((ins[tuple(lo)] != ins[tuple(hi)]) & sel[tuple(lo)]).sum())
    corners = sum(ins[a:ins.shape[0] - 1 + a, b:ins.shape[1] - 1 + b, c:ins.shape[2] - 1 + c].astype(np.int64)
                  for a in (0, 1) for b in (0, 1) for c in (0, 1))
    cells = int((((corners > 0) & (corners < 8)) & sel[:-1, :-1, :-1]).sum())
    return nv, cells


def run_gpu(cuda, vol, iso, frame):
    import torch
    from mi3d import mesh
    v, t = mesh.marching_cubes(torch.from_numpy(vol).to(cuda), iso, origin=frame[0], spacing=frame[1])
    assert v.device == cuda and t.device == cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    assert v.dim() == 2 and v.shape[1] == 3 and t.dim() == 2 and t.shape[1] == 3
    return v.cpu().numpy(), t.cpu().numpy()


def rotate_min_first(t):
    t = np.asarray(t, np.int64).reshape(-1, 3)
    k, r = t.argmin(1), np.arange(len(t))
    return np.stack([t[r, k], t[r, (k + 1) % 3], t[r, (k + 2) % 3]], 1)


@pytest.fixture(scope="module")
def meshes(cuda):
    """name -> (volume, iso, frame, vertices, triangles) from the GPU, each extracted once."""
    out = {}
    for name, make in VOLUMES.items():
        vol, iso, frame = make()
        v, t = run_gpu(cuda, vol, iso, frame)
        print(f"[mesh] {name}: volume {vol.shape} -> nv {len(v)} nt {len(t)}")
        out[name] = (vol, iso, frame, v, t)
    return out


# ------------------------------------------------------------------------------------------------ kernel level

@pytest.mark.parametrize("name", list(VOLUMES))
def test_against_the_restatement_bitwise_and_in_order(cuda, meshes, name):
    vol, iso, frame, v, t = meshes[name]
    rv, rt = marching_cubes_ref(vol, iso, frame[0], frame[1])
    print(f"[mesh] {name}: restatement nv {len(rv)} nt {len(rt)}")
    assert (len(v), len(t)) == (len(rv), len(rt))
    assert v.tobytes() == rv.tobytes()                                   # bitwise, in order
    assert np.array_equal(rotate_min_first(t), rotate_min_first(rt))     # in order, up to rotation within a triangle
    if len(t):
        assert t.min() >= 0 and t.max() < len(v)
    v2, t2 = run_gpu(cuda, vol, iso, frame)                              # deterministic: a second call, the same bytes
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()


@pytest.mark.parametrize("name", SECOND_ROUND)
def test_the_large_volumes_reach_the_second_scan_round(name):
    """The block count is the library's own (mi3d_mc_workspace: u64 + u32 per block, padded, and u32 per point); what lies
    behind the first round is counted from the volume, not taken from the kernels."""
    from mi3d import _lib
    vol, iso, _ = VOLUMES[name]()
    nb = -(-vol.size // MC_BLOCK)
    assert int(_lib.lib().mi3d_mc_workspace(*vol.shape)) == nb * 8 + (nb + 1) // 2 * 8 + vol.size * 4
    assert MC_SCAN_ROUND < nb < 2 * MC_SCAN_ROUND and vol.size > FIRST_ROUND
    early, late = owned_elements(vol, iso, 0, FIRST_ROUND), owned_elements(vol, iso, FIRST_ROUND)
    print(f"[mesh] {name}: {nb} blocks; first round owns {early} (vertices, cells with triangles), later rounds {late}")
    # a base to carry, and vertices to place by it ("i": the rim of the cut, a circle of 2 pi sqrt(10.2^2 - 4.7^2) = 57 grid
    # units in the plane i = 64, crosses more edges than that)
    assert early[0] > 100 and early[1] > 100 and late[0] > (57 if name == "i" else 100)
    if name == "j":
        assert late[1] > 100                                                     # and triangles


@pytest.mark.parametrize("name,euler", [("a", 2), ("b", 0), ("c", 4), ("j", 2)])
def test_closed_surfaces(meshes, name, euler):
    _, _, _, v, t = meshes[name]
    E = assert_closed_and_oriented(t)
    print(f"[mesh] {name}: V {len(v)} E {E} F {len(t)} signed volume {signed_volume(v, t):.6f}")
    assert len(v) - E + len(t) == euler
    assert signed_volume(v, t) > 0
    assert set(np.unique(t)) == set(range(len(v)))


def test_sphere_vertices_lie_within_one_spacing_of_the_surface(meshes):
    """A vertex lies on a grid edge of length `spacing` whose ends straddle the zero set of a 1-Lipschitz function."""
    _, _, frame, v, _ = meshes["a"]
    dist = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - R0)
    print(f"[mesh] a: max | |v| - r0 | = {dist.max():.6f}, spacing {frame[1][0]:.6f}")
    assert np.all(dist <= frame[1][0])


@pytest.mark.parametrize("name", ["d", "e", "i"])
def test_open_surfaces_have_their_boundary_on_the_box(meshes, name):
    vol, _, _, v, t = meshes[name]                     # index frame: a vertex has two integer coordinates
    uses = edge_uses(t)
    frac = v != np.floor(v)
    assert np.all(frac.sum(1) == 1), "a vertex on a grid point (t = 0 or 1) is a null event in these volumes"
    top = np.array(vol.shape, np.float32) - 1
    on_box = (((v == 0) | (v == top[None, :])) & ~frac).any(1)   # its grid edge lies in a boundary face of the volume
    once = 0
    for (a, b), n in uses.items():
        both = n + uses.get((b, a), 0)
        assert n == 1 and both <= 2, (a, b, n, both)
        if both == 1:
            once += 1
            assert on_box[a] and on_box[b], (a, b, v[a], v[b])
    print(f"[mesh] {name}: {len(uses)} directed edges, {once} boundary edges")
    assert once > 0


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "g", "i", "j", "k"])
def test_vertices_are_welded(meshes, name):
    _, _, _, v, t = meshes[name]
    assert len(np.unique(v, axis=0)) == len(v)
    assert t.min() >= 0 and t.max() < len(v)


def test_nothing_above_iso_gives_empty_tensors(meshes):
    _, _, _, v, t = meshes["f"]
    assert v.shape == (0, 3) and t.shape == (0, 3)


def test_non_finite_voxels_give_finite_coordinates(meshes):
    vol, _, _, v, t = meshes["g"]
    _, _, _, va, _ = meshes["a"]
    assert np.isnan(vol).sum() == 1 and np.isinf(vol).sum() == 1
    assert np.isfinite(v).all()
    assert len(v) == len(va) + 6                       # the NaN voxel is a cavity of six vertices
    assert_closed_and_oriented(t)


def test_degenerate_corner_is_kept(meshes):
    _, _, _, v, t = meshes["h_below"]                  # the centre alone is inside (value == iso counts as inside)
    assert len(v) == 6 and len(t) == 8 and np.all(v == 1.0)   # every vertex ON the centre point, eight null triangles
    _, _, _, v, t = meshes["h_above"]                  # everything inside: no surface
    assert v.shape == (0, 3) and t.shape == (0, 3)


def test_argument_checks_launch_nothing(cuda, monkeypatch):
    import torch
    from mi3d import _lib, mesh
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    good = torch.zeros(4, 4, 4, device=cuda)
    bad = {
        "dimension 1": torch.zeros(4, 1, 4, device=cuda),
        "dimension 1025": torch.zeros(2, 2, 1025, device=cuda),
        "cpu": torch.zeros(4, 4, 4),
        "half": good.half(),
        "non-contiguous": torch.zeros(4, 4, 8, device=cuda)[:, :, ::2],
        "2-D": torch.zeros(4, 4, device=cuda),
    }
    for what, t in bad.items():
        with pytest.raises(_lib.Mi3dError):
            mesh.marching_cubes(t, 0.5)
        assert calls == [], what
    with pytest.raises(_lib.Mi3dError):
        mesh.marching_cubes(good, float("nan"))
    assert calls == []


def test_c_abi_rejects_bad_arguments(cuda):
    """hipErrorInvalidValue (1) from the entry points themselves: sizes out of range, a short workspace, NULL pointers."""
    import torch
    from mi3d import _lib
    lib = _lib.lib()
    vol = torch.zeros(4, 4, 4, device=cuda)
    need = lib.mi3d_mc_workspace(4, 4, 4)
    assert need >= 4 * 64 and lib.mi3d_mc_workspace(1, 4, 4) == 0 and lib.mi3d_mc_workspace(4, 4, 1025) == 0
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=cuda)
    counts = torch.zeros(4, dtype=torch.int64, device=cuda)
    p, s = _lib.ptr, _lib.stream(vol)
    assert lib.mi3d_mc_count(p(vol), 1, 4, 4, 0.5, p(ws), need, p(counts), s) == 1
    assert lib.mi3d_mc_count(p(vol), 4, 4, 1025, 0.5, p(ws), need, p(counts), s) == 1
    assert lib.mi3d_mc_count(p(vol), 4, 4, 4, 0.5, p(ws), need - 1, p(counts), s) == 1
    assert lib.mi3d_mc_count(None, 4, 4, 4, 0.5, p(ws), need, p(counts), s) == 1
    assert lib.mi3d_mc_count(p(vol), 4, 4, 4, 0.5, None, need, p(counts), s) == 1
    assert lib.mi3d_mc_count(p(vol), 4, 4, 4, float("nan"), p(ws), need, p(counts), s) == 1
    assert lib.mi3d_mc_scan(4, 4, 4, p(ws), need - 1, p(counts), s) == 1
    assert lib.mi3d_mc_scan(4, 4, 4, p(ws), need, None, s) == 1


def test_caps_are_respected_and_the_overflow_is_counted(cuda):
    """emit writes nothing past nv_cap / nt_cap and counts what it could not place in counts[2]."""
    import ctypes as C
    import torch
    from mi3d import _lib
    lib = _lib.lib()
    vol_np, iso, frame = vol_a()
    rv, rt = marching_cubes_ref(vol_np, iso, frame[0], frame[1])
    vol = torch.from_numpy(vol_np).to(cuda)
    need = lib.mi3d_mc_workspace(48, 48, 48)
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=cuda)
    counts = torch.zeros(4, dtype=torch.int64, device=cuda)
    nv_cap, nt_cap = len(rv) - 100, len(rt) - 7
    verts = torch.full((len(rv), 3), -7.0, device=cuda)
    tris = torch.full((len(rt), 3), -7, dtype=torch.int32, device=cuda)
    org, spc = (C.c_float * 3)(*frame[0]), (C.c_float * 3)(*frame[1])
    p = _lib.ptr
    _lib.launch("mi3d_mc_count", vol, p(vol), 48, 48, 48, iso, p(ws), need, p(counts))
    _lib.launch("mi3d_mc_scan", vol, 48, 48, 48, p(ws), need, p(counts))
    _lib.launch("mi3d_mc_emit", vol, p(vol), 48, 48, 48, iso, org, spc, p(ws), need, p(counts), p(verts), nv_cap,
                p(tris), nt_cap)
    assert counts.tolist() == [len(rv), len(rt), 107, 0]
    assert verts[:nv_cap].cpu().numpy().tobytes() == rv[:nv_cap].tobytes()
    assert torch.all(verts[nv_cap:] == -7.0) and torch.all(tris[nt_cap:] == -7)


def test_on_a_side_stream(cuda, meshes):
    import torch
    vol, iso, frame, v, t = meshes["a"]
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        v2, t2 = run_gpu(cuda, vol, iso, frame)
    side.synchronize()
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()


# ------------------------------------------------------------------------------------------------ model level

@pytest.fixture(scope="module")
def model(cuda):
    """The field of __graft_entry__.smoke()."""
    import torch
    from mi3d import sds_step
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    m, _, _ = sds_step.build_training_state(opt, cuda, bitfield=0.5)
    with torch.no_grad():
        m.encoder.params.uniform_(-0.3, 0.3)
    return m


@pytest.fixture(scope="module")
def volume64(model):
    from mi3d import mesh
    return mesh.extract_volume(model, 64)


def test_extract_volume_is_the_field_on_the_reference_lattice(cuda, oracle, model, volume64):
    import torch
    R = 64
    assert volume64.shape == (R, R, R) and volume64.dtype == torch.float32 and volume64.device == cuda
    idx = torch.from_numpy(np.random.default_rng(1).integers(0, R ** 3, 4096))
    axis = torch.linspace(-1, 1, R)                    # on the CPU, as renderer.py:170-172 makes it
    i, j, k = idx // (R * R), (idx // R) % R, idx % R
    pts = torch.stack([axis[i], axis[j], axis[k]], -1)
    with torch.no_grad():
        direct = model.density(pts.to(cuda))["sigma"]
    got = volume64.view(-1)[idx.to(cuda)]
    diff = (got - direct).abs().max().item()
    print(f"[mesh] extract_volume vs density on 4096 points: max abs diff {diff:g}")
    assert torch.equal(got, direct)                    # bitwise: a row's sigma does not depend on its batch

    fp = oracle.FieldParams(oracle.GridConfig())
    fp.params = model.encoder.params.detach().cpu().numpy()
    fp.W = [l.weight.detach().cpu().numpy() for l in model.sigma_net.net]
    fp.B = [l.bias.detach().cpu().numpy() for l in model.sigma_net.net]
    sig, _ = oracle.field_density(pts.numpy(), fp)
    rel = np.abs(got.cpu().numpy() - sig) / np.abs(sig)
    print(f"[mesh] extract_volume vs oracle.field_density: max rel err {rel.max():.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), sig, rtol=1e-4)   # RTOL of tests/test_field_gpu.py for sigma


def test_export_mesh_writes_what_it_returns(cuda, model, volume64, tmp_path):
    import torch
    from mi3d import mesh
    R = 64
    model.mean_density = float(volume64.median())      # neither empty nor everything
    thresh = min(model.mean_density, model.density_thresh)
    out = tmp_path / "export"                          # created by export_mesh
    v, f, c = model.export_mesh(str(out), resolution=R)
    assert os.path.isfile(out / "mesh.obj") and os.path.isfile(out / "mesh.mtl")
    assert v.dtype == np.float32 and f.dtype == np.int32 and c.dtype == np.float32
    print(f"[mesh] export at {R}^3, threshold {thresh:g}: nv {len(v)} nt {len(f)}")
    assert 0 < len(f) and 0 < len(v) < 3 * R ** 3

    h = 2.0 / (R - 1)
    mv, mt = mesh.marching_cubes(mesh.extract_volume(model, R), thresh, origin=(-1.0, -1.0, -1.0), spacing=(h, h, h))
    assert mv.cpu().numpy().tobytes() == v.tobytes() and mt.cpu().numpy().tobytes() == f.tobytes()
    with torch.no_grad():
        albedo = model.density(torch.from_numpy(v).to(cuda))["albedo"].float()
    assert albedo.cpu().numpy().tobytes() == c.tobytes()
    assert c.min() >= 0 and c.max() <= 1

    mtllib, pv, pc, pf, usemtl = parse_obj(out / "mesh.obj")
    assert mtllib == "mesh.mtl" and usemtl == "mat0"
    assert np.array_equal(pv.astype(np.float32), v)    # %.9g round-trips binary32
    np.testing.assert_allclose(pc, c, atol=5e-7)       # six decimals
    assert np.array_equal(pf, f.astype(np.int64) + 1) and pf.min() >= 1 and pf.max() <= len(v)
    assert "map_Kd" not in open(out / "mesh.mtl").read()


def test_export_mesh_defaults_to_grid_size(cuda, model, volume64, tmp_path):
    from mi3d import mesh
    model.mean_density = float(volume64.median())
    thresh = min(model.mean_density, model.density_thresh)
    assert model.grid_size == 128
    v, f, _ = model.export_mesh(str(tmp_path))
    h = 2.0 / 127
    mv, mt = mesh.marching_cubes(mesh.extract_volume(model, 128), thresh, origin=(-1.0, -1.0, -1.0), spacing=(h, h, h))
    assert len(v) > 0 and mv.cpu().numpy().tobytes() == v.tobytes() and mt.cpu().numpy().tobytes() == f.tobytes()


def test_export_mesh_without_a_surface_names_the_threshold(cuda, model, volume64, tmp_path):
    from mi3d import _lib
    keep = model.mean_density, model.density_thresh
    model.mean_density = model.density_thresh = 1e30
    assert float(volume64.max()) < 1e30
    try:
        with pytest.raises(_lib.Mi3dError, match=r"1e\+30"):
            model.export_mesh(str(tmp_path), resolution=16)
    finally:
        model.mean_density, model.density_thresh = keep
    assert not os.path.exists(tmp_path / "mesh.obj")
