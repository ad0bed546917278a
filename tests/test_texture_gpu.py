"""GPU: texture baking (csrc/texture.hip through mi3d.mesh, include/mi3d.h Part 9).  The atlas layout against a NumPy
float32 restatement of the contract, bit for bit; the no-bleed property on the kernels' output alone; the image against
the field evaluated on the kernels' positions; and the exported OBJ / MTL / PNG triple against the field at the surface
points that the files' own UVs denote."""
import os

import numpy as np
import pytest

from test_mesh_gpu import vol_a, vol_b
from test_texture_cpu import cell_by_the_formula, decode_png, parse_textured_obj

pytestmark = pytest.mark.gpu

F = np.float32


# ------------------------------------------------------------------------------------------------ the restatement

def atlas_ref(vertices, triangles, T, ssaa):
    """include/mi3d.h Part 9 in NumPy float32: (c, vt [3 nt, 2], owner [T, T], xyz [T, T, ssaa^2, 3])."""
    nt = len(triangles)
    c = cell_by_the_formula(nt, T)
    assert c >= 4
    cols, rows = T // (c + 1), T // c
    # UV corners
    i = np.arange(nt)
    q, half = i // 2, (i & 1).astype(bool)
    X0, Y0 = (q % cols) * (c + 1), (q // cols) * c
    vt = np.zeros((nt, 3, 2), F)
    for k, (lx, ly) in enumerate([(0, 0), (c - 2, 0), (0, c - 2)]):
        x, y = np.where(half, c - lx, lx), np.where(half, c - 1 - ly, ly)
        vt[:, k, 0] = ((X0 + x).astype(F) + F(0.5)) / F(T)
        vt[:, k, 1] = F(1.0) - ((Y0 + y).astype(F) + F(0.5)) / F(T)
    # ownership
    Y, X = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    col, x, row, y = X // (c + 1), X % (c + 1), Y // c, Y % c
    half = ~((x <= c - 1) & (x + y <= c - 1))
    tri = 2 * (row * cols + col) + half
    owned = (col < cols) & (row < rows) & (tri < nt)
    owner = np.where(owned, tri, -1).astype(np.int32)
    # texel -> surface point
    u, v = np.where(half, c - x, x)[owned], np.where(half, c - 1 - y, y)[owned]
    corners = vertices[triangles[tri[owned]]]                      # [n, 3, 3] float32
    A, e1, e2 = corners[:, 0], corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    span = F(c - 2)
    xyz = np.zeros((T, T, ssaa * ssaa, 3), F)
    for j in range(ssaa):
        for i_ in range(ssaa):
            s = (u.astype(F) + F((i_ + 0.5) / ssaa - 0.5)) / span
            t = (v.astype(F) + F((j + 0.5) / ssaa - 0.5)) / span
            p = (A + s[:, None] * e1) + t[:, None] * e2
            sub = xyz[:, :, j * ssaa + i_]
            sub[owned] = np.clip(p, F(-1), F(1))
    assert xyz.dtype == F
    return c, vt.reshape(-1, 2), owner, xyz


# ------------------------------------------------------------------------------------------------ the kernels

def run_atlas(cuda, vertices, triangles, T, ssaa, band=37):
    """mi3d_atlas_uv and mi3d_atlas_positions over the whole image in bands of `band` rows (no multiple of the cell
    height: bands start inside cells) -> (vt, owner, xyz) as NumPy arrays, and the bad-triangle counter."""
    import torch
    from mi3d import _lib
    v = torch.from_numpy(np.ascontiguousarray(vertices, F)).to(cuda)
    t = torch.from_numpy(np.ascontiguousarray(triangles, np.int32)).to(cuda)
    nt, ss2, p = len(triangles), ssaa * ssaa, _lib.ptr
    vt = torch.full((3 * nt, 2), -7.0, device=cuda)
    owner = torch.full((T, T), -7, dtype=torch.int32, device=cuda)
    xyz = torch.full((T, T, ss2, 3), -7.0, device=cuda)
    bad = torch.zeros(1, dtype=torch.int64, device=cuda)
    _lib.launch("mi3d_atlas_uv", vt, nt, T, p(vt))
    for row0 in range(0, T, band):
        rows = min(band, T - row0)
        _lib.launch("mi3d_atlas_positions", xyz, p(v), len(vertices), p(t), nt, T, ssaa, row0, rows, p(xyz[row0]),
                    p(owner[row0]), p(bad))
    return vt.cpu().numpy(), owner.cpu().numpy(), xyz.cpu().numpy(), int(bad)


@pytest.fixture(scope="module")
def meshes(cuda):
    """name -> (vertices, triangles) of the sphere and the torus of test_mesh_gpu.py, from the GPU's marching cubes."""
    import torch
    from mi3d import mesh
    out = {}
    for name, make in (("sphere", vol_a), ("torus", vol_b)):
        vol, iso, frame = make()
        v, t = mesh.marching_cubes(torch.from_numpy(vol).to(cuda), iso, origin=frame[0], spacing=frame[1])
        out[name] = (v.cpu().numpy(), t.cpu().numpy())
        print(f"[texture] {name}: nv {len(out[name][0])} nt {len(out[name][1])}")
    return out


@pytest.fixture(scope="module")
def model(cuda):
    """The field of test_mesh_gpu.py: random hash-grid entries, so that the albedo varies from texel to texel (a
    default-initialised field is almost constant and every addressing error would pass)."""
    import torch
    from mi3d import sds_step
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    m, _, _ = sds_step.build_training_state(opt, cuda, bitfield=0.5)
    with torch.no_grad():
        m.encoder.params.uniform_(-0.3, 0.3)
    return m


def albedo_at(model, cuda, pts):
    """model.density(pts)["albedo"] as a float32 NumPy array [n, 3]; pts a NumPy array [n, 3]."""
    import torch
    from mi3d import mesh
    return mesh.vertex_albedo(model, torch.from_numpy(np.ascontiguousarray(pts, F)).to(cuda)).cpu().numpy()


def quantise(a):
    return np.minimum(F(255), np.floor(a.astype(F) * F(255))).astype(np.uint8)


SIZES = (512, 777)       # 777: no multiple of 4 and of no cell size - right / bottom margins, the byte tail of the pack


# ------------------------------------------------------------------------------------------------ layout, bit for bit

@pytest.mark.parametrize("ssaa", [1, 2])
@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("name,drop", [("sphere", 0), ("sphere", 1), ("torus", 0), ("torus", 1)])
def test_layout_against_the_restatement_bitwise(cuda, meshes, name, drop, T, ssaa):
    v, t = meshes[name]
    t = t[:len(t) - drop]                       # a closed mesh has an even triangle count: all but the last is odd
    assert len(t) % 2 == drop
    c, rvt, rowner, rxyz = atlas_ref(v, t, T, ssaa)
    vt, owner, xyz, bad = run_atlas(cuda, v, t, T, ssaa)
    print(f"[texture] {name} nt {len(t)} T {T} ssaa {ssaa}: c {c}, owned texels {(owner >= 0).sum()}")
    assert bad == 0
    assert vt.tobytes() == rvt.tobytes()
    assert np.array_equal(owner, rowner)
    assert xyz.shape == rxyz.shape and xyz.tobytes() == rxyz.tobytes()
    assert (rowner >= 0).sum() == len(t) * c * (c + 1) // 2
    if drop:
        assert not (rowner == len(t)).any()     # the missing partner of the odd last triangle owns nothing


def test_the_two_sizes_give_different_cells(meshes):
    for name, (_, t) in meshes.items():
        cs = [cell_by_the_formula(len(t), T) for T in SIZES]
        assert cs[0] >= 4 and cs[0] != cs[1], (name, cs)


# ------------------------------------------------------------------------------------------------ no bleed

@pytest.mark.parametrize("T", SIZES)
def test_no_bleed_from_the_kernels_alone(cuda, meshes, T):
    """For every triangle, at its corners, edge midpoints and 64 random interior points: each texel that bilinear
    filtering reads with non-zero weight is owned by that triangle.  Uses vt and owner of the kernels only.

    A vt is a binary32 number: it denotes its texel centre to within T * 2^-24 of a texel.  The points are therefore laid
    out from the texel centres the vt snap to (the snap distance is asserted), in float64, where corners and midpoints
    are exact and a weight below 1e-9 can only be rounding of the random points' barycentric sums."""
    from mi3d import mesh
    v, t = meshes["sphere"]
    nt = len(t)
    c = mesh.atlas_cell(nt, T)
    vt, owner, _, bad = run_atlas(cuda, v, t, T, 1)
    assert bad == 0 and c >= 4
    assert (vt > 0).all() and (vt < 1).all()
    # owned sets: one owner per texel by construction; every triangle owns c (c + 1) / 2 texels
    counts = np.bincount(owner[owner >= 0], minlength=nt)
    assert counts.shape == (nt,) and (counts == c * (c + 1) // 2).all()
    assert owner.min() == -1 and owner.max() == nt - 1

    px = np.stack([vt[:, 0].astype(np.float64) * T - 0.5, (1.0 - vt[:, 1].astype(np.float64)) * T - 0.5], -1)
    corner = np.rint(px)
    snap = np.abs(px - corner).max()
    print(f"[texture] T {T} c {c}: vt denote texel centres within {snap:.3e} texels (T * 2^-23 = {T * 2.0 ** -23:.3e})")
    assert snap <= T * 2.0 ** -23
    corner = corner.reshape(nt, 3, 2)

    rng = np.random.default_rng(T)
    w = rng.dirichlet(np.ones(3), size=(nt, 64))                                    # [nt, 64, 3]
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]], np.float64)
    w = np.concatenate([np.broadcast_to(fixed, (nt, 6, 3)), w], 1)                  # [nt, 70, 3]
    pts = np.einsum("nkb,nbd->nkd", w, corner)                                      # continuous texel coordinates
    base = np.floor(pts)
    frac = pts - base
    checked = 0
    for dx in (0, 1):
        for dy in (0, 1):
            weight = np.where(dx, frac[..., 0], 1 - frac[..., 0]) * np.where(dy, frac[..., 1], 1 - frac[..., 1])
            X, Y = base[..., 0].astype(np.int64) + dx, base[..., 1].astype(np.int64) + dy
            used = weight > 1e-9
            assert (X[used] >= 0).all() and (X[used] < T).all() and (Y[used] >= 0).all() and (Y[used] < T).all()
            got = owner[Y[used], X[used]]
            want = np.broadcast_to(np.arange(nt)[:, None], used.shape)[used]
            assert np.array_equal(got, want), (dx, dy, np.flatnonzero(got != want)[:8])
            checked += int(used.sum())
    print(f"[texture] T {T}: {checked} footprint texels checked over {nt} triangles x 70 points")
    assert checked > nt * 70


# ------------------------------------------------------------------------------------------------ colours

@pytest.mark.parametrize("ssaa", [1, 2])
@pytest.mark.parametrize("T", SIZES)
def test_colours_are_the_field(cuda, model, meshes, T, ssaa):
    """image[owner >= 0] == the quantised (mean of the) albedo the field gives at the kernel's positions, bitwise;
    unowned texels are 0.  The albedo of a row does not depend on the batch it is evaluated in (test_mesh_gpu.py relies
    on the same for sigma), so the test may evaluate the owned texels alone."""
    import torch
    from mi3d import mesh
    v, t = meshes["torus"]
    dv, dt = torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)
    image, vt, owner = mesh.bake_texture(model, dv, dt, T, ssaa)
    assert image.shape == (T, T, 3) and image.dtype == torch.uint8 and image.device == cuda
    assert vt.shape == (3 * len(t), 2) and vt.dtype == torch.float32 and owner.shape == (T, T) and owner.dtype == torch.int32
    kvt, kowner, kxyz, bad = run_atlas(cuda, v, t, T, ssaa)
    image, vt, owner = image.cpu().numpy(), vt.cpu().numpy(), owner.cpu().numpy()
    assert bad == 0 and vt.tobytes() == kvt.tobytes() and np.array_equal(owner, kowner)
    owned = owner >= 0
    assert owned.any() and (~owned).any()
    assert (image[~owned] == 0).all()
    a = albedo_at(model, cuda, kxyz[owned].reshape(-1, 3)).reshape(-1, ssaa * ssaa, 3)
    mean = a[:, 0]
    for k in range(1, ssaa * ssaa):
        mean = mean + a[:, k]                                      # float32, in sample order
    mean = mean * F(1.0 / (ssaa * ssaa))
    want = quantise(mean)
    got = image[owned]
    print(f"[texture] T {T} ssaa {ssaa}: {owned.sum()} owned texels, {(got != want).sum()} bytes differ, albedo spans "
          f"[{a.min():.4f}, {a.max():.4f}], {len(np.unique(got))} distinct byte values")
    assert np.array_equal(got, want)
    # the comparison can tell texels apart: the same check against positions one owned texel further fails
    assert not np.array_equal(got[1:], want[:-1])
    image2, _, _ = mesh.bake_texture(model, dv, dt, T, ssaa)       # deterministic
    assert image2.cpu().numpy().tobytes() == image.tobytes()


# ------------------------------------------------------------------------------------------------ through the files

@pytest.fixture(scope="module")
def volume64(model):
    from mi3d import mesh
    return mesh.extract_volume(model, 64)


@pytest.fixture()
def object_threshold(model, volume64):
    """Extraction at the 0.9 quantile of the sampled volume (the median gives a noise surface of several 10^5
    triangles); mean_density and density_thresh are restored afterwards."""
    import torch
    keep = model.mean_density, model.density_thresh
    q = float(torch.quantile(volume64.flatten(), 0.9))
    model.mean_density, model.density_thresh = q, max(model.density_thresh, q)
    yield q
    model.mean_density, model.density_thresh = keep


def _export_textured(model, out, ssaa=1):
    """export_mesh at 64^3 with the smallest T of {2048, 4096} whose cell is at least 6."""
    from mi3d import mesh
    v, f, _ = model.export_mesh(os.path.join(out, "plain"), resolution=64)
    T = next((T for T in (2048, 4096) if mesh.atlas_cell(len(f), T) >= 6), 4096)
    c = mesh.atlas_cell(len(f), T)
    print(f"[texture] export at 64^3: nv {len(v)} nt {len(f)} -> T {T} c {c}")
    assert c >= 6                                                  # interior texel centres exist from c = 5
    return T, c, model.export_mesh(os.path.join(out, "textured"), resolution=64, texture_size=T, ssaa=ssaa)


def test_exported_files_show_the_field_at_the_points_their_uvs_denote(cuda, model, object_threshold, tmp_path):
    """Independent of the restatement and of the kernels' positions: parse mesh.obj, decode albedo.png, pick >= 4096
    random (triangle, texel centre strictly inside its UV triangle) pairs, recompute the barycentric coordinates of the
    texel centre from the parsed vt and the 3-D point from the parsed v in float64, evaluate the field there, compare
    with the decoded texel.

    Tolerance: one code value (1/255: the floor may flip) plus a margin for the position differing in its last bits -
    the contract's formula rounds five times per coordinate, the float64 recomputation never.  The margin is measured
    on the field kernels, not on the code under test: twice the largest albedo change over these same points when one
    coordinate is moved by four binary32 ulps up or down.  Both numbers are printed; no point is left out.
    Figures: none recorded yet - DESIGN.md section 9 says what has and has not run on an MI355X."""
    T, c, (v, f, _, vt, image) = _export_textured(model, str(tmp_path))
    out = tmp_path / "textured"
    _, pv, _, pvt, pf, pft, _ = parse_textured_obj(out / "mesh.obj")
    png = decode_png(out / "albedo.png")
    assert png.shape == (T, T, 3)
    nt = len(pf)
    tri_px = np.stack([pvt[:, 0] * T - 0.5, (1.0 - pvt[:, 1]) * T - 0.5], -1)[pft - 1]      # [nt, 3, 2] float64
    rng = np.random.default_rng(7)
    pairs, want_pairs = [], 4096
    while sum(len(p[0]) for p in pairs) < want_pairs:
        tri = rng.integers(0, nt, 8192)
        w = rng.dirichlet(np.ones(3), size=len(tri))
        P = tri_px[tri]                                                                      # [n, 3, 2]
        texel = np.rint(np.einsum("nb,nbd->nd", w, P))                                       # a texel centre near it
        # barycentric coordinates of that centre, float64
        d1, d2, dp = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], texel - P[:, 0]
        det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
        b1 = (dp[:, 0] * d2[:, 1] - dp[:, 1] * d2[:, 0]) / det
        b2 = (d1[:, 0] * dp[:, 1] - d1[:, 1] * dp[:, 0]) / det
        bary = np.stack([1 - b1 - b2, b1, b2], -1)
        inside = (bary > 1e-3).all(1)                                  # strictly inside: at least c - 2 >= 4 texels wide
        pairs.append((tri[inside], texel[inside].astype(np.int64), bary[inside]))
    tri = np.concatenate([p[0] for p in pairs])
    texel = np.concatenate([p[1] for p in pairs])
    bary = np.concatenate([p[2] for p in pairs])
    assert len(tri) >= want_pairs and len(np.unique(tri)) > 1000
    pts = np.einsum("nb,nbd->nd", bary, pv[pf[tri] - 1])               # float64, from the parsed (exact) vertices
    pts32 = pts.astype(F)
    albedo = albedo_at(model, cuda, pts32).astype(np.float64)
    sens = 0.0
    for axis in range(3):
        for direction in (F(np.inf), F(-np.inf)):
            moved = pts32.copy()
            for _ in range(4):
                moved[:, axis] = np.nextafter(moved[:, axis], direction)
            sens = max(sens, float(np.abs(albedo_at(model, cuda, moved).astype(np.float64) - albedo).max()))
    margin = 2 * sens
    decoded = png[texel[:, 1], texel[:, 0]].astype(np.float64) / 255.0
    err = np.abs(decoded - albedo)
    print(f"[texture] files vs field over {len(tri)} (triangle, interior texel) pairs of {len(np.unique(tri))} triangles: "
          f"max |texel / 255 - albedo| {err.max():.6f}; four-ulp sensitivity of the field {sens:.3e}, margin {margin:.3e}, "
          f"bound {1 / 255 + margin:.6f}; albedo spans [{albedo.min():.4f}, {albedo.max():.4f}]")
    assert (err <= 1.0 / 255.0 + margin).all()
    # the comparison can tell points apart: paired with its neighbour's point instead, some texel misses the bound
    assert (np.abs(np.roll(decoded, 1, axis=0) - albedo) > 1.0 / 255.0 + margin).any()
    # the decoded texel never lies above the field's value by more than the margin: the quantisation is a floor
    assert (decoded - albedo <= margin).all()


def test_exported_files_match_the_returned_arrays(cuda, model, object_threshold, tmp_path):
    from mi3d import mesh
    T, c, (v, f, col, vt, image) = _export_textured(model, str(tmp_path))
    out = tmp_path / "textured"
    assert sorted(os.listdir(out)) == ["albedo.png", "mesh.mtl", "mesh.obj"]
    nt = len(f)
    assert v.dtype == F and f.dtype == np.int32 and col.dtype == F and vt.dtype == F and image.dtype == np.uint8
    assert vt.shape == (3 * nt, 2) and image.shape == (T, T, 3) and col.shape == v.shape
    mtl = open(out / "mesh.mtl").read()
    assert mtl.startswith("newmtl mat0") and mtl.rstrip().endswith("map_Kd albedo.png") and mtl.count("map_Kd") == 1
    mtllib, pv, extra, pvt, pf, pft, usemtl = parse_textured_obj(out / "mesh.obj")
    assert mtllib == "mesh.mtl" and usemtl == "mat0" and extra == 0
    assert np.array_equal(pv.astype(F), v) and len(pvt) == 3 * nt and np.array_equal(pvt.astype(F), vt)
    assert np.array_equal(pf, f.astype(np.int64) + 1)
    assert np.array_equal(pft, np.arange(3 * nt).reshape(nt, 3) + 1)           # ta = 3 i + 1, 3 i + 2, 3 i + 3
    assert np.array_equal(decode_png(out / "albedo.png"), image)
    # the mesh is the default export's mesh; the image is bake_texture's
    pv0, pf0, _ = model.export_mesh(str(tmp_path / "again"), resolution=64)
    assert pv0.tobytes() == v.tobytes() and pf0.tobytes() == f.tobytes()
    import torch
    img, kvt, _ = mesh.bake_texture(model, torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda), T)
    assert img.cpu().numpy().tobytes() == image.tobytes() and kvt.cpu().numpy().tobytes() == vt.tobytes()


def test_default_export_is_untouched(cuda, model, object_threshold, tmp_path):
    out = tmp_path / "default"
    res = model.export_mesh(str(out), resolution=64)
    assert len(res) == 3
    assert sorted(os.listdir(out)) == ["mesh.mtl", "mesh.obj"]
    obj = open(out / "mesh.obj").read()
    assert "\nvt " not in obj and "/" not in obj
    assert "map_Kd" not in open(out / "mesh.mtl").read()
    res2 = model.export_mesh(str(tmp_path / "none"), resolution=64, texture_size=None, ssaa=1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res, res2))
    assert open(tmp_path / "none" / "mesh.obj").read() == obj


# ------------------------------------------------------------------------------------------------ refusals

def test_a_texture_too_small_for_the_mesh_names_one_that_fits(cuda, model, object_threshold, tmp_path):
    from mi3d import _lib, mesh
    v, f, _ = model.export_mesh(str(tmp_path / "plain"), resolution=64)
    nt = len(f)
    fit = next(T for T in (1 << k for k in range(6, 15)) if mesh.atlas_cell(nt, T) > 0)
    assert fit > 64 and mesh.atlas_cell(nt, fit // 2) == 0
    out = tmp_path / "small"
    with pytest.raises(_lib.Mi3dError) as e:
        model.export_mesh(str(out), resolution=64, texture_size=fit // 2)
    msg = str(e.value)
    print(f"[texture] {msg}")
    assert str(nt) in msg and str(fit // 2) in msg and str(fit) in msg
    assert not os.path.exists(out)
    for ssaa in (3, 0, 8):
        with pytest.raises(_lib.Mi3dError, match="ssaa"):
            model.export_mesh(str(out), resolution=64, texture_size=fit, ssaa=ssaa)
        assert not os.path.exists(out)
    for size in (63, 16385, 100.5):
        with pytest.raises(_lib.Mi3dError, match="texture_size"):
            model.export_mesh(str(out), resolution=64, texture_size=size)
        assert not os.path.exists(out)


def test_a_vertex_index_out_of_range_is_counted_not_read(cuda, model, meshes):
    """An argument check: the kernel compares every index with nv before it reads, the triangle owns nothing, the
    counter says how many there were, bake_texture raises."""
    import torch
    from mi3d import _lib, mesh
    v, t = meshes["sphere"]
    t = t.copy()
    t[5, 1] = len(v)                # one past the end
    t[100, 0] = -1
    t[101, 2] = 2 ** 31 - 1
    _, owner, xyz, bad = run_atlas(cuda, v, t, 512, 1)
    assert bad == 3
    for i in (5, 100, 101):
        assert not (owner == i).any()
    assert (xyz[owner < 0] == 0).all() and np.isfinite(xyz).all()
    good = np.setdiff1d(np.arange(len(t)), [5, 100, 101])
    c = mesh.atlas_cell(len(t), 512)
    assert (np.bincount(owner[owner >= 0], minlength=len(t))[good] == c * (c + 1) // 2).all()
    with pytest.raises(_lib.Mi3dError, match="3 of the"):
        mesh.bake_texture(model, torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), 512)


def test_c_abi_rejects_bad_arguments(cuda, meshes):
    """hipErrorInvalidValue (1) from the entry points themselves; nothing is launched."""
    import torch
    from mi3d import _lib
    lib = _lib.lib()
    v, t = meshes["sphere"]
    dv, dt = torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)
    nv, nt, T = len(v), len(t), 512
    vt = torch.zeros(3 * nt, 2, device=cuda)
    xyz = torch.full((8 * T, 3), -7.0, device=cuda)
    owner = torch.full((8, T), -7, dtype=torch.int32, device=cuda)
    img = torch.full((8, T, 3), 7, dtype=torch.uint8, device=cuda)
    bad = torch.zeros(2, dtype=torch.int64, device=cuda)
    p, s = _lib.ptr, _lib.stream(dv)
    assert lib.mi3d_atlas_uv(nt, 63, p(vt), s) == 1
    assert lib.mi3d_atlas_uv(nt, 256, p(vt), s) == 1                  # the sphere does not fit 256^2
    assert lib.mi3d_atlas_uv(0, T, p(vt), s) == 1
    assert lib.mi3d_atlas_uv(nt, T, None, s) == 1

    def positions(**kw):
        a = dict(vertices=p(dv), nv=nv, triangles=p(dt), nt=nt, T=T, ssaa=1, row0=0, rows=8, xyz=p(xyz), owner=p(owner),
                 bad=p(bad))
        a.update(kw)
        return lib.mi3d_atlas_positions(*a.values(), s)
    for kw in (dict(ssaa=3), dict(ssaa=0), dict(rows=0), dict(row0=T), dict(row0=T - 4, rows=8), dict(T=16385), dict(nt=0),
               dict(nv=0), dict(vertices=None), dict(triangles=None), dict(xyz=None), dict(bad=None),
               dict(bad=_lib.C.c_void_p(bad.data_ptr() + 4)), dict(T=256)):
        assert positions(**kw) == 1, kw
    assert lib.mi3d_texture_pack(p(xyz), p(owner), T, 3, 8, p(img), s) == 1
    assert lib.mi3d_texture_pack(p(xyz), p(owner), T, 1, 0, p(img), s) == 1
    assert lib.mi3d_texture_pack(p(xyz), p(owner), T, 1, T + 1, p(img), s) == 1
    assert lib.mi3d_texture_pack(None, p(owner), T, 1, 8, p(img), s) == 1
    assert lib.mi3d_texture_pack(p(xyz), None, T, 1, 8, p(img), s) == 1
    assert lib.mi3d_texture_pack(p(xyz), p(owner), T, 1, 8, _lib.C.c_void_p(img.data_ptr() + 1), s) == 1
    torch.cuda.synchronize()
    assert (xyz == -7).all() and (owner == -7).all() and (img == 7).all() and (vt == 0).all() and (bad == 0).all()
    assert positions(owner=None) == 0                                  # owner is optional
    torch.cuda.synchronize()
    assert (xyz != -7).all() and (owner == -7).all()


def test_pack_writes_nothing_past_the_band(cuda):
    """A band of 3 rows of a 777-wide image has 2331 texels: 582 word groups and three texels written as bytes; the bytes
    after the band stay."""
    import torch
    from mi3d import _lib
    T, rows = 777, 3
    rng = np.random.default_rng(5)
    a = rng.random((rows * T, 3), dtype=F)
    a[:4] = [[1.0, 0.999999, 0.0], [0.5, 1.5, -0.25], [np.nan, 1 / 255, 0.00392], [254 / 255, 0.99609375, 0.99607]]
    own = np.where(rng.random(rows * T) < 0.8, 1, -1).astype(np.int32)
    own[:4] = 0
    da, do = torch.from_numpy(a).to(cuda), torch.from_numpy(own).to(cuda)
    img = torch.full((rows * T * 3 + 64,), 77, dtype=torch.uint8, device=cuda)
    _lib.launch("mi3d_texture_pack", da, _lib.ptr(da), _lib.ptr(do), T, 1, rows, _lib.ptr(img))
    got = img.cpu().numpy()
    with np.errstate(invalid="ignore"):
        v = a * F(255)
        want = np.where(v >= 255, 255, np.where(v >= 0, np.floor(v), 0)).astype(np.uint8)      # NaN, negatives: 0
    want[own < 0] = 0
    assert np.array_equal(got[:rows * T * 3].reshape(-1, 3), want)
    assert (got[rows * T * 3:] == 77).all()
    assert want[0].tolist() == [255, 254, 0] and want[1].tolist() == [127, 255, 0] and want[2, 0] == 0
