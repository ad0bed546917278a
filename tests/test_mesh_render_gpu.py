"""GPU: the rasteriser of the exported mesh (csrc/meshrender.hip through mi3d.mesh, include/mi3d.h Part 17).  The
visibility buffer and every output of the shading pass against the NumPy float32 restatement of
tests/mesh_render_model.py, bit for bit, in both colour modes; the visibility buffer against mesh.render_depth; the tie
rule, the counters, the refusals; then what does not pass through the restatement (a constant texture, supersampling)
and the files export_mesh(preview=) writes.

H x W = 37 x 53: odd, not square, and 3 x 37 x 53 pixels end in a partial wave.  V = 3: two orbit cameras and one so close
that (on the marching-cubes meshes) some triangles have a corner behind it and others span hundreds of pixels - one
thread walks them.  The meshes are those of test_texture_views_gpu.py; only `two` fits a 256^2 atlas and `sphere` a
333^2 one, the torus and the quad take texture coordinates of their own."""
import json
import os

import numpy as np
import pytest

import mesh_render_model as R
import texture_views_model as M
from test_texture_cpu import decode_png
from test_texture_gpu import atlas_ref
from test_texture_views_gpu import meshes, model, small_surface  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 37, 53
FOCAL = 1.2
U = 2.0 ** -24
BG = (0.25, 0.5, 0.75)
CLOSE = {"sphere": lambda: M.look_at((0.55, 0.0, 0.3), target=(-1, 0, 0)),
         "two": lambda: M.look_at((0.75, 0.0, 0.2), target=(-1, 0, 0)),
         "torus": lambda: M.look_at((0.6, 0.0, 0.23), target=(0.3, 0.6, 0.0)),
         "quad": lambda: M.look_at((0.05, 0.02, 0.8), up=(0, 1, 0))}
TEXTURE_SIZE = {"two": 256, "sphere": 333, "torus": 256, "quad": 256}


def cameras(name):
    return np.concatenate([M.orbit(2, 2.4, 0.3, 0.2), CLOSE[name]()[None]]), M.pinhole(FOCAL, H, W)


def sources(name, v, t):
    """Per mesh: vertex colours, vertex normals (not unit: they are interpolated as they are), texture coordinates - the
    atlas' where the mesh fits one, random ones in [0.02, 0.98] otherwise - and a random texture."""
    rng = np.random.default_rng(len(t))
    T = TEXTURE_SIZE[name]
    if name in ("two", "sphere"):
        vt = atlas_ref(v, t, T, 1)[1].reshape(-1, 2)
    else:
        vt = rng.uniform(0.02, 0.98, (3 * len(t), 2)).astype(F)
    return dict(colors=rng.random((len(v), 3)).astype(F), vn=rng.normal(size=(len(v), 3)).astype(F), vt=vt,
                texture=rng.integers(0, 256, (T, T, 3), dtype=np.uint8))


_REFERENCE = {}


def reference(name, mode, v, t):
    """The restatement of one (mesh, colour mode), computed once and shared; nobody writes to it."""
    if (name, mode) not in _REFERENCE:
        c2w, K = cameras(name)
        s = sources(name, v, t)
        src = dict(colors=s["colors"]) if mode == "colors" else dict(vt=s["vt"], texture=s["texture"])
        _REFERENCE[name, mode] = R.render(v, t, M.view_records(c2w, K), H, W, vn=s["vn"], background=BG, **src)
    return _REFERENCE[name, mode]


def dev(cuda, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(cuda)


def gpu_buffers(cuda, v, t, c2w, K, s, mode, h=H, w=W, bg=BG, normals=True):
    from mi3d import mesh
    src = dict(colors=dev(cuda, s["colors"])) if mode == "colors" else dict(uvs=dev(cuda, s["vt"]),
                                                                           texture=dev(cuda, s["texture"]))
    out = mesh._render_buffers(dev(cuda, v, F), dev(cuda, t, np.int32), dev(cuda, mesh.view_records(c2w, K)), h, w,
                               normals=dev(cuda, s["vn"]) if normals else None, bg=bg, **src)
    return {k: None if a is None else a.cpu().numpy() for k, a in out.items()}


def assert_equal_bitwise(got, want):
    assert got["vis"].view(np.uint64).tobytes() == want["vis"].tobytes()
    assert tuple(got["counts"].tolist()) == want["counts"]
    for k in ("image", "depth", "tri", "bary", "normal", "alpha"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("mode", ["colors", "texture"])
@pytest.mark.parametrize("name", ["two", "sphere", "torus", "quad"])
def test_every_buffer_against_the_restatement_bitwise(cuda, meshes, name, mode):
    from mi3d import mesh
    v, t = meshes[name]
    c2w, K = cameras(name)
    want, s = reference(name, mode, v, t), sources(name, v, t)
    drawn = (want["tri"] >= 0).mean(axis=(1, 2))
    largest = np.bincount(want["tri"][2][want["tri"][2] >= 0]).max()
    print(f"[mesh render] {name} {mode}: drawn {drawn}, counts {want['counts']}, largest triangle {largest} pixels")
    assert (drawn > 0.05).all() and largest >= 200              # the close view: one thread walks hundreds of pixels
    if name != "quad":
        assert 0 < want["counts"][1] < len(t)                   # and some triangles have a corner behind that camera
    got = gpu_buffers(cuda, v, t, c2w, K, s, mode)
    assert_equal_bitwise(got, want)
    # the public function: albedo shading hands the kernel's image through, alpha is the coverage
    src = dict(colors=dev(cuda, s["colors"])) if mode == "colors" else dict(uvs=dev(cuda, s["vt"]),
                                                                           texture=dev(cuda, s["texture"]))
    image, alpha, buf = mesh.render(dev(cuda, v, F), dev(cuda, t, np.int32), c2w, K, H, W, normals=dev(cuda, s["vn"]),
                                    bg_color=BG, return_buffers=True, **src)
    assert image.cpu().numpy().tobytes() == want["image"].tobytes()
    assert alpha.cpu().numpy().tobytes() == want["alpha"].astype(F).tobytes()
    assert sorted(buf) == ["bary", "depth", "normal", "tri"]
    assert all(buf[k].cpu().numpy().tobytes() == want[k].tobytes() for k in buf)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_key_upper_word_equals_render_depth_bitwise(cuda, meshes, name):
    from mi3d import mesh
    v, t = meshes[name]
    c2w, K = cameras(name)
    got = gpu_buffers(cuda, v, t, c2w, K, sources(name, v, t), "colors")
    depth, counts = mesh.render_depth(dev(cuda, v, F), dev(cuda, t, np.int32), c2w, K, H, W, return_counts=True)
    depth = depth.cpu().numpy()
    key = got["vis"].view(np.uint64)
    drawn = np.isfinite(depth)
    assert (key[~drawn] == R.EMPTY).all() and (key[drawn] != R.EMPTY).all()
    assert ((key[drawn] >> np.uint64(32)).astype(np.uint32) == depth.view(np.uint32)[drawn]).all()
    assert got["depth"].tobytes() == depth.tobytes()            # and the shading pass recomputes the same bits
    assert tuple(got["counts"].tolist()) == (counts["bad"], counts["skipped"])


def test_a_duplicated_triangle_list_resolves_to_the_smaller_index(cuda, meshes):
    v, t = meshes["two"]
    c2w, K = cameras("two")
    s = sources("two", v, t)
    once = gpu_buffers(cuda, v, t, c2w, K, s, "colors")
    twice = gpu_buffers(cuda, v, np.concatenate([t, t]), c2w, K, s, "colors")
    assert (twice["tri"] < len(t)).all() and (twice["tri"] >= 0).sum() > 500
    for k in ("vis", "image", "depth", "tri", "bary", "alpha"):
        assert twice[k].tobytes() == once[k].tobytes(), k
    both = np.concatenate([t[::-1], t])                          # every triangle twice, the first copies in reverse order
    back = gpu_buffers(cuda, v, both, c2w, K, s, "colors")
    depth, tri, _ = R.visibility(v, both, M.view_records(c2w, K), H, W)
    assert back["vis"].view(np.uint64).tobytes() == R.keys(depth, tri).tobytes()
    assert (back["tri"] < len(t)).all() and back["depth"].tobytes() == once["depth"].tobytes()


def test_bad_indices_are_counted_and_never_drawn_and_no_triangles_give_the_background(cuda, meshes):
    import torch
    from mi3d import _lib, mesh
    v, t = meshes["two"]
    c2w, K = cameras("two")
    s = sources("two", v, t)
    t = t.copy()
    t[7, 1] = len(v)
    t[300, 0] = -1
    t[301, 2] = 2 ** 31 - 1
    rec = M.view_records(c2w, K)
    for mode, src in (("colors", dict(colors=s["colors"])), ("texture", dict(vt=s["vt"], texture=s["texture"]))):
        want = R.render(v, t, rec, H, W, vn=s["vn"], background=BG, **src)
        got = gpu_buffers(cuda, v, t, c2w, K, s, mode)
        assert want["counts"][0] == 3                           # once per triangle, not once per view
        assert_equal_bitwise(got, want)
        assert not np.isin(got["tri"], [7, 300, 301]).any()
    with pytest.raises(_lib.Mi3dError, match="3 of the"):
        mesh.render(dev(cuda, v, F), dev(cuda, t, np.int32), c2w, K, H, W, colors=dev(cuda, s["colors"]))
    # nt = 0: the fill and the background
    none = gpu_buffers(cuda, v, np.zeros((0, 3), np.int32), c2w, K, s, "colors")
    assert (none["vis"] == -1).all() and none["counts"].tolist() == [0, 0]
    assert (none["image"] == np.array(BG, F)).all() and (none["alpha"] == 0).all() and (none["tri"] == -1).all()
    assert np.isinf(none["depth"]).all() and (none["bary"] == 0).all() and (none["normal"] == 0).all()
    image, alpha = mesh.render(dev(cuda, v, F), torch.zeros(0, 3, dtype=torch.int32, device=cuda), c2w, K, H, W,
                               colors=dev(cuda, s["colors"]), bg_color=0.5)
    assert (image == 0.5).all() and (alpha == 0).all()


def test_two_runs_give_identical_bytes(cuda, meshes):
    v, t = meshes["torus"]
    c2w, K = cameras("torus")
    s = sources("torus", v, t)
    for mode in ("colors", "texture"):
        a, b = gpu_buffers(cuda, v, t, c2w, K, s, mode), gpu_buffers(cuda, v, t, c2w, K, s, mode)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_c_abi_rejects_bad_arguments(cuda, meshes):
    """hipErrorInvalidValue (1) from the entry points themselves; nothing is launched."""
    import torch
    from mi3d import _lib
    lib = _lib.lib()
    v, t = meshes["two"]
    s = sources("two", v, t)
    dv, dt = dev(cuda, v, F), dev(cuda, t, np.int32)
    V, T = 2, 256
    rec = dev(cuda, M.view_records(M.orbit(V), M.pinhole(FOCAL, H, W)))
    vis = torch.full((V, H, W), 7, dtype=torch.int64, device=cuda)
    counts = torch.full((3,), 7, dtype=torch.int64, device=cuda)
    colors, vt, tex, vn = dev(cuda, s["colors"]), dev(cuda, s["vt"]), dev(cuda, s["texture"]), dev(cuda, s["vn"])
    image = torch.full((V, H, W, 3), -7.0, device=cuda)
    normal = torch.full((V, H, W, 3), -7.0, device=cuda)
    bg = (_lib.C.c_float * 3)(*BG)
    p, st = _lib.ptr, _lib.stream(dv)

    def visibility(**kw):
        a = dict(vertices=p(dv), nv=len(v), triangles=p(dt), nt=len(t), views=p(rec), V=V, H=H, W=W, vis=p(vis),
                 counts=p(counts))
        a.update(kw)
        return lib.mi3d_mesh_visibility(*a.values(), st)

    for kw in (dict(V=0), dict(V=65), dict(H=1), dict(W=1), dict(H=16385), dict(W=16385), dict(vertices=None),
               dict(triangles=None), dict(views=None), dict(vis=None), dict(counts=None),
               dict(counts=_lib.C.c_void_p(counts.data_ptr() + 4)), dict(vis=_lib.C.c_void_p(vis.data_ptr() + 4)),
               dict(nv=2 ** 31), dict(nt=2 ** 31), dict(nt=2 ** 32 - 1)):
        assert visibility(**kw) == 1, kw

    def shade(**kw):
        a = dict(vertices=p(dv), nv=len(v), triangles=p(dt), nt=len(t), views=p(rec), V=V, H=H, W=W, vis=p(vis),
                 colors=p(colors), vt=None, texture=None, T=0, vn=p(vn), background=bg, image=p(image), normal=p(normal),
                 depth=None, tri=None, bary=None, alpha=None)
        a.update(kw)
        return lib.mi3d_mesh_shade(*a.values(), st)

    textured = dict(colors=None, vt=p(vt), texture=p(tex), T=T)
    for kw in (dict(V=0), dict(V=65), dict(H=1), dict(W=16385), dict(vertices=None), dict(triangles=None), dict(views=None),
               dict(vis=None), dict(background=None), dict(image=None), dict(nv=2 ** 31), dict(nt=2 ** 31),
               dict(colors=None),                                                   # neither colour source
               dict(vt=p(vt), texture=p(tex), T=T),                                 # both
               dict(textured, vt=None), dict(textured, texture=None), dict(textured, T=63), dict(textured, T=16385),
               dict(vn=None)):                                                      # a normal output without normals
        assert shade(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (vis == 7).all() and (counts == 7).all() and (image == -7).all() and (normal == -7).all()
    assert visibility(nt=0, triangles=None) == 0 and shade(nt=0, triangles=None) == 0      # the fill, the background
    assert shade(nt=0, triangles=None, normal=None, vn=None, **textured) == 0
    torch.cuda.synchronize()
    assert (vis == -1).all() and counts.tolist() == [0, 0, 7] and (image == torch.tensor(BG, device=cuda)).all()


def test_a_constant_texture_gives_that_colour_and_the_background_is_exact(cuda, meshes):
    """Every covered pixel within 4 u relative of the texture's colour, the blend's first-order bound for four equal taps
    k: hx = 1 - fx is exact for gx >= 1, top = k hx + k fx and bot pass a product and a sum each, 2 u, and
    c = top hy + bot fy two more.  (The division by 255 rounds once more; with equal taps the errors observed stay below
    1 u - the test prints the figure.)  Every other pixel is exactly bg_color."""
    from mi3d import mesh
    v, t = meshes["two"]
    c2w, K = cameras("two")
    T = 256
    colour = np.array([200, 90, 31], np.uint8)
    vt = atlas_ref(v, t, T, 1)[1].reshape(-1, 2)
    image, alpha = mesh.render(dev(cuda, v, F), dev(cuda, t, np.int32), c2w, K, H, W, uvs=dev(cuda, vt),
                               texture=dev(cuda, np.broadcast_to(colour, (T, T, 3))), bg_color=BG)
    image, covered = image.cpu().numpy(), alpha.cpu().numpy() > 0
    assert covered.sum() > 2000 and (~covered).sum() > 2000
    want = colour.astype(np.float64) / 255.0
    rel = np.abs(image[covered].astype(np.float64) - want) / want
    print(f"[mesh render] constant texture: max relative error {rel.max() / U:.3f} u")
    assert rel.max() <= 4 * U
    assert (image[~covered] == np.array(BG, F)).all()


@pytest.mark.parametrize("shading", ["albedo", "lambertian"])
def test_ssaa_equals_the_box_average_of_the_larger_render(cuda, meshes, shading):
    from mi3d import mesh
    v, t = meshes["sphere"]
    c2w, K = cameras("sphere")
    s = sources("sphere", v, t)
    a = dict(colors=dev(cuda, s["colors"]), normals=dev(cuda, s["vn"]), shading=shading, bg_color=BG,
             light_d=(0.3, -0.2, 0.9))
    dv, dt = dev(cuda, v, F), dev(cuda, t, np.int32)
    image, alpha = mesh.render(dv, dt, c2w, K, H, W, ssaa=2, **a)
    big, big_alpha = mesh.render(dv, dt, c2w, K * np.array([[2.0], [2.0], [1.0]]), 2 * H, 2 * W, **a)
    assert tuple(image.shape) == (3, H, W, 3) and tuple(big.shape) == (3, 2 * H, 2 * W, 3)

    def average(x):
        x = x.cpu().numpy().reshape(3, H, 2, W, 2, -1)
        return (((x[:, :, 0, :, 0] + x[:, :, 0, :, 1]) + x[:, :, 1, :, 0]) + x[:, :, 1, :, 1]) * F(0.25)

    assert image.cpu().numpy().tobytes() == average(big).tobytes()
    assert alpha.cpu().numpy().tobytes() == average(big_alpha)[..., 0].tobytes()
    part = alpha.cpu().numpy()
    assert ((part > 0) & (part < 1)).sum() > 20                 # silhouette pixels are partly covered


def test_shadings_follow_the_fields_formulas(cuda, meshes):
    """Plain fp32 torch, not specified to the bit: against NumPy binary64 within 1e-5."""
    from mi3d import mesh
    v, t = meshes["sphere"]
    c2w, K = cameras("sphere")
    s = sources("sphere", v, t)
    dv, dt = dev(cuda, v, F), dev(cuda, t, np.int32)
    want = reference("sphere", "colors", v, t)
    covered = want["tri"] >= 0
    n = want["normal"].astype(np.float64)
    n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-10)
    light = np.array([0.3, -0.2, 0.9]) / np.linalg.norm([0.3, -0.2, 0.9])
    lam = 0.25 + 0.75 * np.maximum(n @ light, 0.1)
    # normalising amplifies the interpolated normal's binary32 error, a few 1e-7, by 1 / |n|: compare where |n| > 0.05
    covered = covered & (np.linalg.norm(want["normal"].astype(np.float64), axis=-1) > 0.05)
    assert covered.sum() > 1000
    for shading, colour in (("lambertian", want["image"] * lam[..., None]), ("textureless", np.repeat(lam[..., None], 3, -1)),
                            ("normal", (n + 1) / 2)):
        image, _ = mesh.render(dv, dt, c2w, K, H, W, colors=dev(cuda, s["colors"]), normals=dev(cuda, s["vn"]),
                               shading=shading, light_d=(0.3, -0.2, 0.9), ambient_ratio=0.25, bg_color=BG)
        image = image.cpu().numpy()
        assert np.abs(image[covered] - colour[covered]).max() < 1e-5, shading
        assert (image[want["tri"] < 0] == np.array(BG, F)).all()
    from mi3d import _lib
    with pytest.raises(_lib.Mi3dError, match="normals"):
        mesh.render(dv, dt, c2w, K, H, W, colors=dev(cuda, s["colors"]), shading="lambertian")


# ------------------------------------------------------------------------------------------------ export

def quantised(image):
    return np.clip(np.floor(image.astype(F) * F(255)), 0, 255).astype(np.uint8)


def test_export_with_preview_writes_the_images_and_the_report(cuda, model, small_surface, tmp_path):
    import torch
    from mi3d import mesh
    R_, T = small_surface, 256
    c2w, K = M.orbit(2, 3.2, 0.4, 0.1), M.pinhole(1.6, H, W)     # outside the box: its half-diagonal is 1.74
    preview = dict(c2w=c2w, K=K, H=H, W=W, fidelity=True)
    plain = model.export_mesh(str(tmp_path / "plain"), resolution=R_, texture_size=T)
    out = model.export_mesh(str(tmp_path / "preview"), resolution=R_, texture_size=T, preview=preview)
    assert len(out) == len(plain) and all(a.tobytes() == b.tobytes() for a, b in zip(plain, out))
    assert sorted(os.listdir(tmp_path / "preview")) == ["albedo.png", "mesh.mtl", "mesh.obj", "preview.json",
                                                         "preview_000.png", "preview_001.png"]
    for name in ("mesh.obj", "mesh.mtl", "albedo.png"):
        assert open(tmp_path / "preview" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
    report = json.load(open(tmp_path / "preview" / "preview.json"))
    print(f"[mesh render] export at {R_}^3: {report}")
    assert len(report["views"]) == 2
    for r in [report] + report["views"]:
        assert r["psnr_intersection"] is not None and np.isfinite(r["psnr_intersection"])
        assert 0 < r["iou"] <= 1
    v, t, _, vt, image = out
    want, alpha = mesh.render(torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), c2w, K, H, W,
                              uvs=torch.from_numpy(vt).to(cuda), texture=torch.from_numpy(image).to(cuda))
    assert (alpha > 0).float().mean() > 0.02
    for k in range(2):
        png = decode_png(str(tmp_path / "preview" / f"preview_{k:03d}.png"))
        assert png.tobytes() == quantised(want[k].cpu().numpy()).tobytes()
    # without a texture the preview shows the vertex colours; supersampled; no report unless asked for
    out = model.export_mesh(str(tmp_path / "colours"), resolution=R_, preview=dict(c2w=c2w[:1], K=K, H=H, W=W, ssaa=2))
    assert sorted(os.listdir(tmp_path / "colours")) == ["mesh.mtl", "mesh.obj", "preview_000.png"]
    want, _ = mesh.render(torch.from_numpy(out[0]).to(cuda), torch.from_numpy(out[1]).to(cuda), c2w[:1], K, H, W,
                          colors=torch.from_numpy(out[2]).to(cuda), ssaa=2)
    assert decode_png(str(tmp_path / "colours" / "preview_000.png")).tobytes() == quantised(want[0].cpu().numpy()).tobytes()


def test_export_without_preview_is_untouched(cuda, model, small_surface, tmp_path):
    R_ = small_surface
    a = model.export_mesh(str(tmp_path / "a"), resolution=R_, texture_size=256)
    b = model.export_mesh(str(tmp_path / "b"), resolution=R_, texture_size=256, preview=None)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["albedo.png", "mesh.mtl", "mesh.obj"]
    for name in ("mesh.obj", "mesh.mtl", "albedo.png"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    from mi3d import _lib
    with pytest.raises(_lib.Mi3dError, match="ssaa"):
        model.export_mesh(str(tmp_path / "c"), resolution=R_, preview=dict(c2w=M.orbit(1), K=M.pinhole(1.0, H, W), H=H, W=W,
                                                                          ssaa=3))
    assert not os.path.exists(tmp_path / "c")
