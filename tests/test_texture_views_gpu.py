"""GPU: texturing from views (csrc/textureviews.hip through mi3d.mesh, include/mi3d.h Part 15).  The depth maps and the
per-sample colour, hit count and packed image against the NumPy float32 restatement of tests/texture_views_model.py, bit
for bit; then semantics that do not pass through the restatement (occlusion, back faces, self-occlusion against the
analytic torus), the pixel conventions against the two renderers, and the exported files.

The meshes are marching_cubes of vol_a (sphere), vol_b (torus) and vol_c (two spheres) of test_mesh_gpu.py.  Of these
only vol_c fits a 256^2 atlas and only vol_a and vol_c a 333^2 one (7484, 12144 and 3736 triangles); the torus is baked
at 512^2."""
import os

import numpy as np
import pytest

import texture_views_model as M
from test_mesh_gpu import vol_a, vol_b, vol_c
from test_texture_cpu import decode_png
from test_texture_gpu import atlas_ref, run_atlas
from test_texture_views_cpu import looking_away, quad_mesh, smooth_images

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 96, 80
FOCAL = 1.2
POWER, MIN_COS, TOL = 4, 0.2, 0.05     # at 96 x 80 a pixel is 0.025 wide on the object: 0.02 would leave a cap per view
MIN_COS2 = float(F(MIN_COS) * F(MIN_COS))


@pytest.fixture(scope="module")
def meshes(cuda):
    import torch
    from mi3d import mesh
    out = {"quad": quad_mesh()}
    for name, make in (("sphere", vol_a), ("torus", vol_b), ("two", vol_c)):
        vol, iso, frame = make()
        v, t = mesh.marching_cubes(torch.from_numpy(vol).to(cuda), iso, origin=frame[0], spacing=frame[1])
        out[name] = (v.cpu().numpy(), t.cpu().numpy())
    return out


def gpu_depth(cuda, v, t, c2w, K, h=H, w=W):
    import torch
    from mi3d import mesh
    d, counts = mesh.render_depth(torch.from_numpy(np.ascontiguousarray(v, F)).to(cuda),
                                  torch.from_numpy(np.ascontiguousarray(t, np.int32)).to(cuda), c2w, K, h, w,
                                  return_counts=True)
    return d.cpu().numpy(), (counts["bad"], counts["skipped"])


def five_views():
    """V = 5: three overlapping orbit views, one that sees nothing, one from below; view 1 masked on its left half;
    unequal weights."""
    c2w = np.concatenate([M.orbit(1, 2.4, 0.3, 0.2 + 0.6 * k) for k in range(3)] +
                         [looking_away()[None], M.look_at((0.3, 0.2, -2.2))[None]])
    masks = np.ones((5, H, W), np.uint8)
    masks[1, :, : W // 2] = 0
    return dict(c2w=c2w, K=M.pinhole(FOCAL, H, W), images=smooth_images(5, H, W, seed=3), masks=masks,
                weights=np.array([1.0, 0.5, 2.0, 3.0, 0.25], F))


# ------------------------------------------------------------------------------------------------ depth maps

DEPTH_CASES = {
    "orbit": ("sphere", lambda: M.orbit(3, 2.4, 0.3, 0.2)),
    "torus": ("torus", lambda: M.orbit(2, 2.6, 0.35, 0.5)),
    "close": ("quad", lambda: np.stack([M.look_at((0.05, 0.02, 0.8), up=(0, 1, 0)),          # the quad fills the image
                                        M.look_at((0.6, 0.3, 0.9), up=(0, 1, 0))])),
    "behind": ("sphere", lambda: np.stack([M.look_at((0.0, 0.0, 0.0), target=(1, 0.2, 0.1)),  # inside the sphere
                                           M.look_at((0.55, 0.0, 0.3), target=(-1, 0, 0))])),
}


@pytest.mark.parametrize("case", list(DEPTH_CASES))
def test_depth_maps_against_the_restatement_bitwise(cuda, meshes, case):
    name, poses = DEPTH_CASES[case]
    v, t = meshes[name]
    c2w, K = poses(), M.pinhole(FOCAL, H, W)
    want, counts = M.depth_maps(v, t, M.view_records(c2w, K), H, W)
    got, got_counts = gpu_depth(cuda, v, t, c2w, K)
    drawn = np.isfinite(want).mean(axis=(1, 2))
    print(f"[texture views] depth {case}: drawn {drawn}, counts {counts}")
    assert got.dtype == F and got.shape == (len(c2w), H, W)
    assert got_counts == counts
    assert got.tobytes() == want.tobytes()
    if case == "close":
        assert drawn[0] > 0.5                                   # one thread walks most of the image
    if case == "behind":
        assert 0 < counts[1] < len(c2w) * len(t)                # some triangles behind the camera, some in front
    else:
        assert counts == (0, 0) and (drawn > 0.05).all()


def test_bad_indices_are_counted_and_degenerate_triangles_draw_nothing(cuda, meshes):
    v, t = meshes["two"]
    t = t.copy()
    t[7, 1] = len(v)
    t[300, 0] = -1
    t[301, 2] = 2 ** 31 - 1
    t[50] = [t[50, 0], t[50, 0], t[50, 1]]                      # two equal corners: no area
    c2w, K = M.orbit(2, 2.4, 0.3, 0.2), M.pinhole(FOCAL, H, W)
    want, counts = M.depth_maps(v, t, M.view_records(c2w, K), H, W)
    got, got_counts = gpu_depth(cuda, v, t, c2w, K)
    assert counts == (3, 0) and got_counts == counts            # once per triangle, not once per view
    assert got.tobytes() == want.tobytes()
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="3 of the"):
        mesh.render_depth(torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), c2w, K, H, W)
    flat = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)       # three collinear points
    d, counts = gpu_depth(cuda, flat, np.array([[0, 1, 2]], np.int32), M.look_at((0.2, 0.1, 2.0), up=(0, 1, 0))[None], K)
    want, _ = M.depth_maps(flat, np.array([[0, 1, 2]], np.int32),
                           M.view_records(M.look_at((0.2, 0.1, 2.0), up=(0, 1, 0))[None], K), H, W)
    assert d.tobytes() == want.tobytes() and counts == (0, 0)


# ------------------------------------------------------------------------------------------------ the projection

def run_project(cuda, v, t, T, ssaa, views, depth, base, band=37):
    """mi3d_atlas_positions and mi3d_texture_project over the whole image in bands of `band` rows (bands start inside
    cells) -> (colour [T, T, ssaa^2, 3], hits [T, T, ssaa^2]) as NumPy arrays."""
    import torch
    from mi3d import _lib
    ss2, p = ssaa * ssaa, _lib.ptr
    dv = torch.from_numpy(np.ascontiguousarray(v, F)).to(cuda)
    dt = torch.from_numpy(np.ascontiguousarray(t, np.int32)).to(cuda)
    rec = torch.from_numpy(M.view_records(views["c2w"], views["K"])).to(cuda)
    images, weights = torch.from_numpy(views["images"]).to(cuda), torch.from_numpy(views["weights"]).to(cuda)
    masks = None if views.get("masks") is None else torch.from_numpy(views["masks"]).to(cuda)
    depth, base = torch.from_numpy(depth).to(cuda), torch.from_numpy(base).to(cuda)
    xyz = torch.empty(T, T, ss2, 3, device=cuda)
    owner = torch.empty(T, T, dtype=torch.int32, device=cuda)
    colour = torch.full((T, T, ss2, 3), -7.0, device=cuda)
    hits = torch.full((T, T, ss2), 99, dtype=torch.uint8, device=cuda)
    bad = torch.zeros(1, dtype=torch.int64, device=cuda)
    V, h, w = views["images"].shape[:3]
    for row0 in range(0, T, band):
        rows = min(band, T - row0)
        _lib.launch("mi3d_atlas_positions", xyz, p(dv), len(v), p(dt), len(t), T, ssaa, row0, rows, p(xyz[row0]),
                    p(owner[row0]), p(bad))
        _lib.launch("mi3d_texture_project", xyz, p(xyz[row0]), p(owner[row0]), p(dv), len(v), p(dt), len(t), T, ssaa, rows,
                    p(rec), V, h, w, p(depth), p(images), p(masks), p(weights), POWER, MIN_COS2, TOL, p(base[row0]),
                    p(colour[row0]), p(hits[row0]))
    return colour.cpu().numpy(), hits.cpu().numpy()


def model_project(v, t, T, ssaa, views, depth, base):
    ss2 = ssaa * ssaa
    _, _, owner, xyz = atlas_ref(v, t, T, ssaa)
    col, hits = M.project_views(xyz.reshape(-1, 3), np.repeat(owner.ravel(), ss2), v, t,
                                M.view_records(views["c2w"], views["K"]), H, W, depth, views["images"], views.get("masks"),
                                views["weights"], POWER, MIN_COS2, TOL, base.reshape(-1, 3))
    return col.reshape(T, T, ss2, 3), hits.reshape(T, T, ss2), owner


@pytest.mark.parametrize("ssaa", [1, 2])
@pytest.mark.parametrize("name,T", [("two", 256), ("sphere", 333), ("two", 333), ("torus", 512)])
def test_colour_hits_and_image_against_the_restatement_bitwise(cuda, meshes, monkeypatch, name, T, ssaa):
    import torch
    from mi3d import mesh
    v, t = meshes[name]
    views, ss2 = five_views(), ssaa * ssaa
    base = np.random.default_rng(T + ssaa).random((T, T, ss2, 3)).astype(F)
    depth, _ = M.depth_maps(v, t, M.view_records(views["c2w"], views["K"]), H, W)
    want_col, want_hits, owner = model_project(v, t, T, ssaa, views, depth, base)
    got_depth, _ = gpu_depth(cuda, v, t, views["c2w"], views["K"])
    assert got_depth.tobytes() == depth.tobytes()
    col, hits = run_project(cuda, v, t, T, ssaa, views, depth, base)
    owned = owner >= 0
    share = np.bincount(want_hits[owned].ravel(), minlength=4)[:4] / want_hits[owned].size
    print(f"[texture views] {name} T {T} ssaa {ssaa}: samples with 0 / 1 / 2 / 3 views {share}")
    assert share[0] > 0.02 and share[1] > 0.1 and share[2] > 0.05       # every kind of sample occurs
    assert want_hits[:, :, :][owned].max() <= 4                          # view 3 sees nothing
    assert hits.tobytes() == want_hits.tobytes()
    assert col.tobytes() == want_col.tobytes()
    assert (col[~owned] == base[~owned]).all() and (hits[~owned] == 0).all()
    # the whole bake: several bands, the pack, the returned arrays
    monkeypatch.setattr(mesh, "CHUNK", T * ss2 * 36)
    image, vt, own, bhits = mesh.bake_views(torch.from_numpy(base).to(cuda), torch.from_numpy(v).to(cuda),
                                            torch.from_numpy(t).to(cuda), T, views["images"], views["c2w"], views["K"],
                                            ssaa=ssaa, masks=views["masks"], weights=views["weights"], power=POWER,
                                            min_cos=MIN_COS, depth_tol=TOL)
    assert image.dtype == torch.uint8 and tuple(image.shape) == (T, T, 3) and tuple(bhits.shape) == (T, T, ss2)
    assert own.cpu().numpy().tobytes() == owner.tobytes()
    assert bhits.cpu().numpy().tobytes() == want_hits.tobytes()
    assert image.cpu().numpy().tobytes() == M.pack(want_col, owner, ssaa).tobytes()


def test_two_runs_give_identical_bytes(cuda, meshes):
    v, t = meshes["torus"]
    views = five_views()
    base = np.zeros((512, 512, 1, 3), F)
    a, b = gpu_depth(cuda, v, t, views["c2w"], views["K"])[0], gpu_depth(cuda, v, t, views["c2w"], views["K"])[0]
    assert a.tobytes() == b.tobytes()
    c1, h1 = run_project(cuda, v, t, 512, 1, views, a, base)
    c2, h2 = run_project(cuda, v, t, 512, 1, views, a, base)
    assert c1.tobytes() == c2.tobytes() and h1.tobytes() == h2.tobytes()


# ------------------------------------------------------------------------------------------------ semantics

RED, BLUE = np.array([1.0, 0.0, 0.0], F), np.array([0.0, 0.0, 1.0], F)


def bake_one_view(cuda, v, t, T, c2w, **kw):
    """One red view over a blue base -> (is_red bool [T, T], hits [T, T], owner, xyz [T, T, 3]) as NumPy arrays."""
    import torch
    from mi3d import mesh
    images = np.broadcast_to(RED, (1, H, W, 3)).copy()
    image, _, owner, hits = mesh.bake_views(BLUE, torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), T, images,
                                            c2w[None], M.pinhole(FOCAL, H, W), **kw)
    image, owner, hits = image.cpu().numpy(), owner.cpu().numpy(), hits.cpu().numpy()[:, :, 0]
    owned = owner >= 0
    red, blue = (image == [255, 0, 0]).all(-1), (image == [0, 0, 255]).all(-1)
    assert (red | blue)[owned].all() and (red[owned] == (hits[owned] > 0)).all()
    xyz = run_atlas(cuda, v, t, T, 1)[2][:, :, 0]
    return red, hits, owner, xyz


def facing(v, t, owner, xyz, eye):
    """cos of the angle between the owner triangle's normal and the direction to `eye`, in binary64 (NaN: unowned)."""
    tri = v[t[np.maximum(owner, 0)]].astype(np.float64)
    n = np.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])
    d = np.asarray(eye, np.float64) - xyz
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (n * d).sum(-1) / (np.linalg.norm(n, axis=-1) * np.linalg.norm(d, axis=-1))
    return np.where(owner >= 0, cos, np.nan)


def test_the_near_sphere_hides_the_far_one(cuda, meshes):
    v, t = meshes["two"]
    eye = (2.4, 0.0, 0.0)
    red, hits, owner, xyz = bake_one_view(cuda, v, t, 256, M.look_at(eye), depth_tol=0.1)    # the spheres are 0.4 apart
    with np.errstate(invalid="ignore"):
        cos = facing(v, t, owner, xyz, eye)
        far_near_side = (xyz[..., 0] < 0) & (cos > 0)
        near_front = (xyz[..., 0] > 0) & (cos > 0.5)
    assert far_near_side.sum() > 5000 and near_front.sum() > 5000
    assert not red[far_near_side].any()                          # 0.3 / 1.9 > 0.3 / 2.9: wholly behind the near sphere
    assert red[near_front].mean() > 0.99
    assert not red[(xyz[..., 0] < 0) & (owner >= 0)].any()


def test_back_faces_never_take_a_views_colour(cuda, meshes):
    v, t = meshes["sphere"]
    eye = M.orbit(1, 2.4, 0.3, 0.7)[0]
    red, hits, owner, xyz = bake_one_view(cuda, v, t, 333, eye, min_cos=0.0, depth_tol=0.15)     # nothing occludes
    with np.errstate(invalid="ignore"):
        cos = facing(v, t, owner, xyz, eye[:3, 3])
        assert (cos < -1e-6).sum() > 10000 and not red[cos < -1e-6].any()
        assert red[cos > 0.3].mean() > 0.99                      # and the front does
        red2 = bake_one_view(cuda, v, t, 333, eye, min_cos=0.5, depth_tol=0.15)[0]
        assert not red2[cos < 0.5 - 1e-4].any() and red2[cos > 0.5 + 1e-4].mean() > 0.99


def torus_sdf(p):
    return np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - 0.55) ** 2 + p[..., 2] ** 2) - 0.2


def test_the_torus_hides_itself(cuda, meshes):
    """Independent of the depth maps: a texel is HIDDEN if the straight line from it to the camera passes through the
    analytic torus' body (signed distance below -0.05 somewhere, in binary64), CLEAR if it stays 0.08 outside from 0.1 on - three pixels of
    0.027, so that no tap of its bilinear footprint sees an occluder.  depth_tol = 0.1: the ring's parts are 0.7 apart."""
    v, t = meshes["torus"]
    eye = M.orbit(1, 2.6, 0.15, 0.5)[0]          # low: the near side of the ring hides the far side's inner wall
    red, hits, owner, xyz = bake_one_view(cuda, v, t, 512, eye, depth_tol=0.1)
    o = eye[:3, 3]
    with np.errstate(invalid="ignore"):
        cos = facing(v, t, owner, xyz, o)
    pts = xyz.astype(np.float64)
    s = np.linspace(0.0, 1.0, 97)[1:, None, None, None]
    along = torus_sdf(pts[None] + s * (o - pts)[None])
    dist = (s * np.linalg.norm(o - pts, axis=-1)[None, ..., None])[..., 0]
    hidden = (owner >= 0) & (along.min(0) < -0.05)
    clear = (owner >= 0) & (np.where(dist > 0.1, along, 1.0).min(0) > 0.08) & (cos > 0.5)
    front_hidden = hidden & (cos > 0.3)
    print(f"[texture views] torus: hidden {hidden.sum()}, of them facing the camera {front_hidden.sum()}, clear {clear.sum()}")
    assert front_hidden.sum() > 2000                             # texels only the depth test can reject
    assert not red[hidden].any()
    assert red[clear].mean() > 0.99


# ------------------------------------------------------------------------------------------------ conventions

def test_render_point_lights_the_pixel_the_projection_names(cuda):
    import torch
    from mi3d import refine
    S = 64
    c2w, K = M.orbit(1, 2.4, 0.3, 0.4)[0], M.pinhole(FOCAL, S, S)
    w2c = np.linalg.inv(c2w)
    for i, j in ((20, 33), (0, 0), (63, 5), (41, 63)):
        cam = np.linalg.inv(K) @ np.array([i + 0.5, j + 0.5, 1.0]) * 2.2           # the pixel's centre at depth 2.2
        p = (c2w[:3, :3] @ cam + c2w[:3, 3]).astype(F)
        x, y, z = M.project(M.view_records(c2w[None], K)[0], p[None])
        assert int(np.floor(x[0])) == i and int(np.floor(y[0])) == j and abs(z[0] - 2.2) < 1e-5
        img = refine.render_point(torch.from_numpy(p[None]).to(cuda), torch.ones(1, 3, device=cuda), S, S,
                                  torch.tensor(K, device=cuda).float(), torch.tensor(w2c, device=cuda).float(), (S, S),
                                  0.6 / S * 2.0, 4)[0, 0].cpu().numpy()
        lit = np.argwhere(img > 0)
        assert lit.tolist() == [[j, i]], (i, j, lit)


def test_pinhole_rays_hit_the_point_that_projects_to_the_pixels_centre(cuda):
    """Binary32 bound: the projection's own running bound (texture_views_model.project) plus the ray direction's
    rounding, 16 u, seen through the focal length in pixels."""
    import torch
    from mi3d import rays
    S, fov = 64, 40.0
    c2w = M.orbit(1, 2.4, 0.3, 0.4)[0]
    focal = S / (2 * np.tan(np.radians(fov) / 2))
    K = np.array([[focal, 0, S / 2], [0, focal, S / 2], [0, 0, 1]])
    o, d, _ = rays.pinhole_rays(torch.tensor(c2w, device=cuda).float()[None], S, S, fov)
    o, d = o[0].cpu().numpy().astype(np.float64), d[0].cpu().numpy().astype(np.float64)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - 0.36)
    hit = disc > 1e-3
    assert hit.sum() > 500
    p = (o + (-b - np.sqrt(np.where(hit, disc, 0)))[:, None] * d)[hit]
    x, y, z, Ex, Ey, _ = M.project(M.view_records(c2w[None], K)[0], p, np.float64, True)
    x32, y32, _ = M.project(M.view_records(c2w[None], K)[0], p.astype(F))
    j, i = np.divmod(np.flatnonzero(hit), S)
    slack = 16 * M.U * focal * 2 + M.U * S                       # the direction, and p rounded to binary32
    assert (abs(x32 - (i + 0.5)) <= 2 * Ex + slack).all() and (abs(y32 - (j + 0.5)) <= 2 * Ey + slack).all()
    assert (2 * Ex + slack).max() < 2e-3


# ------------------------------------------------------------------------------------------------ export

@pytest.fixture(scope="module")
def model(cuda):
    """The field of test_texture_gpu.py: random hash-grid entries."""
    import torch
    from mi3d import sds_step
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    m, _, _ = sds_step.build_training_state(opt, cuda, bitfield=0.5)
    with torch.no_grad():
        m.encoder.params.uniform_(-0.3, 0.3)
    return m


@pytest.fixture()
def small_surface(model):
    """A threshold and a resolution at which the surface fits a 256^2 atlas; the model's thresholds are restored."""
    import torch
    from mi3d import mesh
    keep = model.mean_density, model.density_thresh
    for R in (24, 16, 12, 8):
        vol = mesh.extract_volume(model, R)
        q = float(torch.quantile(vol.flatten(), 0.9))
        v, t = mesh.marching_cubes(vol, q)
        if 0 < t.shape[0] and mesh.atlas_cell(t.shape[0], 256) > 0:
            break
    else:
        pytest.fail("no resolution gives a surface that fits 256^2")
    model.mean_density, model.density_thresh = q, max(model.density_thresh, q)
    yield R
    model.mean_density, model.density_thresh = keep


def test_export_with_views_writes_the_views_where_they_hit_and_the_field_elsewhere(cuda, model, small_surface, tmp_path):
    R, T = small_surface, 256
    c2w = M.orbit(4, 3.2, 0.4, 0.1)                              # outside the box: its half-diagonal is 1.74
    views = dict(images=smooth_images(4, H, W, seed=9), c2w=c2w, K=M.pinhole(1.6, H, W),
                 weights=np.array([1.0, 2.0, 0.5, 1.5], F), power=POWER, min_cos=MIN_COS, depth_tol=TOL)
    field = model.export_mesh(str(tmp_path / "field"), resolution=R, texture_size=T)
    both = model.export_mesh(str(tmp_path / "views"), resolution=R, texture_size=T, views=views)
    assert sorted(os.listdir(tmp_path / "views")) == ["albedo.png", "mesh.mtl", "mesh.obj"]
    for name in ("mesh.obj", "mesh.mtl"):
        assert open(tmp_path / "views" / name, "rb").read() == open(tmp_path / "field" / name, "rb").read()
    v, t = both[0], both[1]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(field[:4], both[:4]))
    png = decode_png(str(tmp_path / "views" / "albedo.png"))
    assert png.tobytes() == both[4].tobytes()
    depth, counts = M.depth_maps(v, t, M.view_records(c2w, views["K"]), H, W)
    assert counts == (0, 0)
    col, hits, owner = model_project(v, t, T, 1, dict(views, masks=None), depth, np.zeros((T, T, 1, 3), F))
    want = M.pack(col, owner, 1)
    seen = hits[:, :, 0] > 0
    print(f"[texture views] export at {R}^3: nt {len(t)}, texels a view sees {seen.sum()} of {(owner >= 0).sum()}")
    assert seen.sum() > 500 and (~seen & (owner >= 0)).sum() > 100
    assert (png[seen] == want[seen]).all()
    assert (png[~seen] == field[4][~seen]).all()
    assert (png[seen] != field[4][seen]).any()


def test_export_without_views_is_untouched(cuda, model, small_surface, tmp_path):
    R = small_surface
    a = model.export_mesh(str(tmp_path / "a"), resolution=R, texture_size=256)
    b = model.export_mesh(str(tmp_path / "b"), resolution=R, texture_size=256, views=None)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for name in ("mesh.obj", "mesh.mtl", "albedo.png"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    from mi3d import _lib
    with pytest.raises(_lib.Mi3dError, match="texture_size"):
        model.export_mesh(str(tmp_path / "c"), resolution=R, views=dict(images=np.zeros((1, H, W, 3), F),
                                                                        c2w=M.orbit(1), K=M.pinhole(1.0, H, W)))
    assert not os.path.exists(tmp_path / "c")


def test_render_views_returns_what_bake_views_takes(cuda):
    import torch
    from mi3d import mesh, refine
    torch.manual_seed(0)
    unet = refine.UNet(num_input_channels=3, num_output_channels=3).to(cuda).eval()
    pts = torch.nn.functional.normalize(torch.randn(4000, 3, device=cuda), dim=-1) * 0.6
    c2w = M.orbit(2, 2.4, 0.3, 0.2)
    images, K = refine.render_views(unet, pts, torch.rand(4000, 3, device=cuda), c2w, FOCAL, 64, 64, 0.05, 8)
    assert tuple(images.shape) == (2, 64, 64, 3) and images.dtype == torch.float32 and not images.requires_grad
    assert 0 <= float(images.min()) and float(images.max()) <= 1
    assert np.array_equal(K, M.pinhole(FOCAL, 64, 64))
    assert mesh.check_views(images, c2w, K)[4] == (2, 64, 64)


# ------------------------------------------------------------------------------------------------ refusals

def test_c_abi_rejects_bad_arguments(cuda, meshes):
    """hipErrorInvalidValue (1) from the entry points themselves; nothing is launched."""
    import torch
    from mi3d import _lib
    lib = _lib.lib()
    v, t = meshes["two"]
    dv, dt = torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)
    T, rows, V = 256, 8, 2
    rec = torch.from_numpy(M.view_records(M.orbit(V), M.pinhole(FOCAL, H, W))).to(cuda)
    depth = torch.full((V, H, W), -7.0, device=cuda)
    counts = torch.full((3,), 7, dtype=torch.int64, device=cuda)
    images, weights = torch.zeros(V, H, W, 3, device=cuda), torch.ones(V, device=cuda)
    xyz, base = torch.zeros(rows * T, 3, device=cuda), torch.zeros(rows * T, 3, device=cuda)
    owner = torch.zeros(rows, T, dtype=torch.int32, device=cuda)
    colour = torch.full((rows * T, 3), -7.0, device=cuda)
    hits = torch.full((rows * T,), 99, dtype=torch.uint8, device=cuda)
    p, s = _lib.ptr, _lib.stream(dv)

    def mesh_depth(**kw):
        a = dict(vertices=p(dv), nv=len(v), triangles=p(dt), nt=len(t), views=p(rec), V=V, H=H, W=W, depth=p(depth),
                 counts=p(counts))
        a.update(kw)
        return lib.mi3d_mesh_depth(*a.values(), s)

    for kw in (dict(V=0), dict(V=65), dict(H=1), dict(W=1), dict(H=16385), dict(vertices=None), dict(triangles=None),
               dict(views=None), dict(depth=None), dict(counts=None), dict(counts=_lib.C.c_void_p(counts.data_ptr() + 4)),
               dict(nv=2 ** 31), dict(nt=2 ** 31)):
        assert mesh_depth(**kw) == 1, kw

    def project(**kw):
        a = dict(xyz=p(xyz), owner=p(owner), vertices=p(dv), nv=len(v), triangles=p(dt), nt=len(t), T=T, ssaa=1, rows=rows,
                 views=p(rec), V=V, H=H, W=W, depth=p(depth), images=p(images), masks=None, weights=p(weights), power=4,
                 min_cos2=0.04, depth_tol=0.02, base=p(base), colour=p(colour), hits=p(hits))
        a.update(kw)
        return lib.mi3d_texture_project(*a.values(), s)

    for kw in (dict(V=0), dict(V=65), dict(H=1), dict(W=16385), dict(power=3), dict(power=0), dict(power=32), dict(ssaa=3),
               dict(rows=0), dict(rows=T + 1), dict(T=63), dict(nv=0), dict(nt=0), dict(min_cos2=1.5),
               dict(min_cos2=float("nan")), dict(depth_tol=-1.0), dict(depth_tol=float("inf")), dict(xyz=None),
               dict(owner=None), dict(vertices=None), dict(triangles=None), dict(views=None), dict(depth=None),
               dict(images=None), dict(weights=None), dict(base=None), dict(colour=None), dict(hits=None)):
        assert project(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (depth == -7).all() and (counts == 7).all() and (colour == -7).all() and (hits == 99).all()
    assert mesh_depth(nt=0, triangles=None) == 0                 # the fill alone
    torch.cuda.synchronize()
    assert torch.isinf(depth).all() and counts.tolist() == [0, 0, 7]
