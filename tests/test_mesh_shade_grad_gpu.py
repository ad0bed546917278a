"""GPU: the gradients of the mesh render's colour sources (csrc/meshrender.hip through mi3d.mesh, include/mi3d.h Part 18).
The float-texture forward and both gradients against the NumPy restatement of tests/mesh_shade_grad_model.py, bit for bit,
fed the GPU's own visibility keys; the special cases and the refusals of the raw ABI; torch.autograd through mesh.render
against the float64 restatement; mesh.fit_texture against the float64 restatement's loop; export_mesh(views=dict(fit=)).

Sizes, meshes and cameras are those of test_mesh_render_gpu.py: 37 x 53 pixels, V = 3 with one camera so close that a
single vertex or texel collects over a thousand contributions - contention on one 64-bit word, and the headroom of the
sums."""
import json

import numpy as np
import pytest

import mesh_render_model as R
import mesh_shade_grad_model as G
import test_mesh_shade_grad_cpu as CPU
import texture_views_model as M
from test_mesh_render_gpu import BG, FOCAL, H, TEXTURE_SIZE, W, cameras, dev, sources
from test_texture_cpu import decode_png
from test_texture_views_gpu import meshes, model, small_surface  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
NAMES = ["two", "sphere", "torus", "quad"]


def winners(vis, v, t):
    """tri int64 [V, H, W] from the uint64 keys, as the kernels read them: -1 for an all-ones key, a triangle index not
    below nt, and a triangle with a vertex index outside [0, nv)."""
    key = np.ascontiguousarray(vis).view(np.uint64)
    tri = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (key != R.EMPTY) & (tri < len(t))
    idx = np.asarray(t)[np.where(ok, tri, 0)]
    ok &= ((idx >= 0) & (idx < len(v))).all(-1)
    return np.where(ok, tri, -1)


def gpu_keys(cuda, v, t, rec, h=H, w=W):
    from mi3d import mesh
    return mesh._visibility(dev(cuda, v, F), dev(cuda, t, np.int32), dev(cuda, rec), h, w)[0]


def gpu_backward(cuda, v, t, rec, vis, g, vt=None, T=None, h=H, w=W):
    from mi3d import mesh
    shape = (len(v), 3) if vt is None else (T, T, 3)
    return mesh._shade_backward(dev(cuda, v, F), dev(cuda, t, np.int32), dev(cuda, rec), h, w, vis, dev(cuda, g, F),
                                None if vt is None else dev(cuda, vt), shape).cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_f32_forward_against_the_restatement_bitwise(cuda, meshes, name):
    from mi3d import mesh
    v, t = meshes[name]
    c2w, K = cameras(name)
    s, T = sources(name, v, t), TEXTURE_SIZE[name]
    rec = M.view_records(c2w, K)
    tex = np.random.default_rng(T).random((T, T, 3), dtype=F)
    got = mesh._render_buffers(dev(cuda, v, F), dev(cuda, t, np.int32), dev(cuda, rec), H, W, uvs=dev(cuda, s["vt"]),
                               texture=dev(cuda, tex), bg=BG)
    tri = winners(got["vis"].cpu().numpy(), v, t)
    assert (tri >= 0).sum() > 800 and (got["tri"].cpu().numpy() == tri).all()
    want = G.shade_f32(G.plan(v, t, rec, H, W, tri, s["vt"], T), tex, (3, H, W), BG)
    assert got["image"].cpu().numpy().tobytes() == want.tobytes()
    # the public function takes the same route, and a float texture of bytes / 255 is not the uint8 texture's render
    image, _ = mesh.render(dev(cuda, v, F), dev(cuda, t, np.int32), c2w, K, H, W, uvs=dev(cuda, s["vt"]),
                           texture=dev(cuda, tex), bg_color=BG)
    assert image.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("mode", ["colors", "texture"])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_the_restatement_bitwise_and_twice(cuda, meshes, name, mode):
    v, t = meshes[name]
    c2w, K = cameras(name)
    s, T = sources(name, v, t), TEXTURE_SIZE[name]
    rec = M.view_records(c2w, K)
    vis = gpu_keys(cuda, v, t, rec)
    tri = winners(vis.cpu().numpy(), v, t)
    vt, size = (s["vt"], T) if mode == "texture" else (None, None)
    elements = T * T if mode == "texture" else len(v)
    p = G.plan(v, t, rec, H, W, tri, vt, size)
    most = np.bincount(p["index"].ravel()).max()
    print(f"[mesh shade grad] {name} {mode}: {len(p['pixel'])} drawn pixels, up to {most} contributions per element")
    if mode == "colors" and name == "sphere":
        assert most > 1000                                      # the close camera: one word, over a thousand adders
    for seed, scale in ((1, 1.0), (2, 3e-31), (3, 7e29)):
        g = (np.random.default_rng(seed).normal(size=(3, H, W, 3)) * scale).astype(F)
        want = G.backward(p, g, elements)
        got = gpu_backward(cuda, v, t, rec, vis, g, vt, size)
        assert got.reshape(-1, 3).tobytes() == want.tobytes(), (seed, scale)
        if seed == 1:
            assert np.abs(want).max() > 1 and gpu_backward(cuda, v, t, rec, vis, g, vt, size).tobytes() == got.tobytes()


def test_background_pixels_and_poisoned_keys_contribute_nothing(cuda, meshes):
    import torch
    v, t = meshes["two"]
    c2w, K = cameras("two")
    s, T = sources("two", v, t), TEXTURE_SIZE["two"]
    rec = M.view_records(c2w, K)
    t = t.copy()
    t[7, 1] = len(v)                                            # no visibility pass draws triangle 7 ...
    vis = gpu_keys(cuda, v, t, rec)
    clean = winners(vis.cpu().numpy(), v, t)
    assert not (clean == 7).any()
    jj, ii = np.nonzero(clean[0] >= 0)
    depth = int(np.float32(2.0).view(np.uint32)) << 32
    poison = [(jj[10], ii[10], depth | 7),                      # ... so these keys are made up: a bad vertex index,
              (jj[100], ii[100], depth | len(t)),               # a triangle index that is not below nt,
              (jj[250], ii[250], depth | 0xFFFFFFFF)]           # and the largest one
    for j, i, key in poison:
        vis[0, int(j), int(i)] = key                             # below 2^63: the same bits as an int64
    tri = winners(vis.cpu().numpy(), v, t)
    assert (tri >= 0).sum() == (clean >= 0).sum() - 3
    g = np.random.default_rng(7).normal(size=(3, H, W, 3)).astype(F)
    g[tri < 0] *= 1e3                                           # the background decides amax, and adds nothing
    only_nothing = np.where((tri < 0)[..., None], g, 0).astype(F)
    for vt, size, elements in ((None, None, len(v)), (s["vt"], T, T * T)):
        p = G.plan(v, t, rec, H, W, tri, vt, size)
        got = gpu_backward(cuda, v, t, rec, vis, g, vt, size)
        assert got.reshape(-1, 3).tobytes() == G.backward(p, g, elements).tobytes()
        zero = gpu_backward(cuda, v, t, rec, vis, only_nothing, vt, size)
        assert (zero.view(np.uint32) == 0).all()
    torch.cuda.synchronize()


def test_zero_gives_exact_zeros_and_a_non_finite_entry_poisons_everything(cuda, meshes):
    v, t = meshes["quad"]
    c2w, K = cameras("quad")
    s, T = sources("quad", v, t), TEXTURE_SIZE["quad"]
    rec = M.view_records(c2w, K)
    vis = gpu_keys(cuda, v, t, rec)
    for vt, size in ((None, None), (s["vt"], T)):
        assert (gpu_backward(cuda, v, t, rec, vis, np.zeros((3, H, W, 3), F), vt, size).view(np.uint32) == 0).all()
        assert (gpu_backward(cuda, v, t, rec, vis, -np.zeros((3, H, W, 3), F), vt, size).view(np.uint32) == 0).all()
        for bad in (np.nan, np.inf, -np.inf):
            g = np.random.default_rng(8).normal(size=(3, H, W, 3)).astype(F)
            g[1, 3, 5, 2] = bad
            assert (gpu_backward(cuda, v, t, rec, vis, g, vt, size).view(np.uint32) == G.QUIET_NAN).all()


def test_c_abi_rejects_bad_arguments_and_touches_nothing(cuda, meshes):
    """hipErrorInvalidValue (1) from the entry points themselves; nothing is launched: the poisoned buffers stay."""
    import torch
    from mi3d import _lib
    lib = _lib.lib()
    v, t = meshes["two"]
    s = sources("two", v, t)
    dv, dt = dev(cuda, v, F), dev(cuda, t, np.int32)
    V, T = 2, 256
    rec = dev(cuda, M.view_records(M.orbit(V), M.pinhole(FOCAL, H, W)))
    vis = gpu_keys(cuda, v, t, rec.cpu().numpy())
    g, vt = torch.ones(V, H, W, 3, device=cuda), dev(cuda, s["vt"])
    gc, gt = torch.full((len(v), 3), -7.0, device=cuda), torch.full((T, T, 3), -7.0, device=cuda)
    ws = torch.full((3 * T * T + 1,), 7, dtype=torch.int64, device=cuda)
    need_c, need_t = 8 * (3 * len(v) + 1), 8 * (3 * T * T + 1)
    assert lib.mi3d_mesh_shade_backward_workspace(3 * len(v)) == need_c
    p, st, vp = _lib.ptr, _lib.stream(dv), _lib.C.c_void_p

    def backward(**kw):
        a = dict(vertices=p(dv), nv=len(v), triangles=p(dt), nt=len(t), views=p(rec), V=V, H=H, W=W, vis=p(vis), dimage=p(g),
                 vt=None, T=0, grad_colors=p(gc), grad_texture=None, ws=p(ws), ws_bytes=need_c)
        a.update(kw)
        return lib.mi3d_mesh_shade_backward(*a.values(), st)

    textured = dict(vt=p(vt), T=T, grad_colors=None, grad_texture=p(gt), ws_bytes=need_t)
    for kw in (dict(V=0), dict(V=65), dict(H=1), dict(W=16385), dict(vertices=None), dict(triangles=None), dict(views=None),
               dict(vis=None), dict(vis=vp(vis.data_ptr() + 4)), dict(nv=2 ** 31), dict(nt=2 ** 31), dict(dimage=None),
               dict(grad_colors=None),                                               # neither gradient
               dict(grad_texture=p(gt)),                                             # both
               dict(vt=p(vt)), dict(T=T), dict(vt=p(vt), T=T),                       # vt without T, T without vt, vt with colours
               dict(textured, vt=None), dict(textured, T=0), dict(textured, T=63), dict(textured, T=16385),
               dict(ws=None), dict(ws=vp(ws.data_ptr() + 4)), dict(ws_bytes=need_c - 1), dict(textured, ws_bytes=need_t - 8)):
        assert backward(**kw) == 1, kw
    image = torch.full((V, H, W, 3), -7.0, device=cuda)
    tex = torch.rand(T, T, 3, device=cuda)
    bg = (_lib.C.c_float * 3)(*BG)

    def shade(**kw):
        a = dict(vertices=p(dv), nv=len(v), triangles=p(dt), nt=len(t), views=p(rec), V=V, H=H, W=W, vis=p(vis), colors=None,
                 vt=p(vt), texture=p(tex), T=T, vn=None, background=bg, image=p(image), normal=None, depth=None, tri=None,
                 bary=None, alpha=None)
        a.update(kw)
        return lib.mi3d_mesh_shade_f32(*a.values(), st)

    for kw in (dict(V=0), dict(H=1), dict(views=None), dict(vis=None), dict(background=None), dict(image=None),
               dict(texture=None), dict(vt=None), dict(T=63), dict(T=16385), dict(colors=p(gc)), dict(normal=p(image)),
               dict(vt=None, texture=None)):
        assert shade(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (gc == -7).all() and (gt == -7).all() and (ws == 7).all() and (image == -7).all()
    assert backward(nt=0, triangles=None) == 0 and backward(nt=0, triangles=None, **textured) == 0     # no triangle: zeros
    torch.cuda.synchronize()
    assert (gc.view(torch.int32) == 0).all() and (gt.view(torch.int32) == 0).all()


def test_autograd_through_render_against_the_float64_restatement(cuda, meshes):
    """mesh.render(shading="lambertian", ssaa=2) differentiated in its vertex colours, against the float64 restatement of
    the whole chain: the pass at 2 H x 2 W, the Lambertian factor from the interpolated normals, the background, the box
    average.  Within the CPU test's bound (the model's header) for the kernel, evaluated at the upstream gradient the
    kernel is given, plus 16 u sum |w| |dimage| for that upstream gradient itself, which plain binary32 torch computes:
    the normalisation (a dot product, a square root, a division: the vertex normals here are unit vectors of a sphere,
    so nothing is amplified), the product with the light, the clamp, the factor's multiply-add, the product with the
    incoming gradient and the three additions and the scale of the box average's adjoint - 14 roundings, counted as 16.
    The factor also inherits the binary32 weights' error through the interpolated normal: at most 2 (1 - ambient) sum_k
    E(lambda_k) (unit vertex normals; 2 for the normalisation of a vector of length about 1), times the incoming gradient."""
    import torch
    from mi3d import mesh
    v, t = meshes["sphere"]
    c2w, K = cameras("sphere")
    s = sources("sphere", v, t)
    vn = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)
    light, ambient = np.array([0.3, -0.2, 0.9]) / np.linalg.norm([0.3, -0.2, 0.9]), 0.25
    colors = dev(cuda, s["colors"]).requires_grad_(True)
    image, _, buf = mesh.render(dev(cuda, v, F), dev(cuda, t, np.int32), c2w, K, H, W, colors=colors, normals=dev(cuda, vn),
                                shading="lambertian", light_d=light, ambient_ratio=ambient, bg_color=BG, ssaa=2,
                                return_buffers=True)
    assert image.requires_grad and tuple(image.shape) == (3, H, W, 3)
    up = np.random.default_rng(9).normal(size=(3, H, W, 3))
    image.backward(dev(cuda, up, F))
    got = colors.grad.cpu().numpy()
    # the restatement, in float64, on the winners the GPU drew
    h2, w2 = 2 * H, 2 * W
    rec = M.view_records(c2w, K * np.array([[2.0], [2.0], [1.0]]))
    tri = buf["tri"].cpu().numpy().astype(np.int64)
    p32 = G.plan(v, t, rec, h2, w2, tri)
    p64 = G.plan(v, t, rec, h2, w2, tri, dtype=np.float64, bounds=True)
    n = R.shade(v, t, rec, h2, w2, tri, colors=s["colors"], vn=vn, F=np.float64)["normal"]
    n = n / np.sqrt(np.maximum((n * n).sum(-1, keepdims=True), 1e-20))
    factor = ambient + (1 - ambient) * np.maximum(n @ light, 0.1)
    source = torch.from_numpy(s["colors"].astype(np.float64)).requires_grad_(True)
    shaded = G.render_torch(source, G.torch_plan(p64, torch.float64), (3, h2, w2), BG) * torch.from_numpy(factor)[..., None]
    shaded = torch.where(torch.from_numpy(tri >= 0)[..., None], shaded, torch.tensor(BG, dtype=torch.float64))
    small = shaded.reshape(3, H, 2, W, 2, 3).sum((2, 4)) * 0.25
    small.backward(torch.from_numpy(up))
    want = source.grad.numpy()
    dimage = np.repeat(np.repeat(up, 2, 1), 2, 2) * 0.25 * factor[..., None] * (tri >= 0)[..., None]
    bound = G.bound(p64, p32, dimage.astype(F), len(v), got)
    glue = np.zeros((len(v), 3))
    incoming = np.abs(np.repeat(np.repeat(up, 2, 1), 2, 2) * 0.25).reshape(-1, 3)[p64["pixel"]]
    slack = 16 * U * np.abs(dimage).reshape(-1, 3)[p64["pixel"]] + \
        2 * (1 - ambient) * p64["Eweight"].sum(1)[:, None] * incoming
    for k in range(3):
        np.add.at(glue, p64["index"][:, k], np.abs(p64["weight"][:, k, None]) * slack)
    err = np.abs(got - want)
    print(f"[mesh shade grad] autograd, lambertian, ssaa 2: max |grad| {np.abs(want).max():.3g}, max error {err.max():.3g}, "
          f"max error / bound {np.max(err / np.maximum(bound + glue, 1e-300)):.3g}")
    assert np.abs(want).max() > 1 and (err <= bound + glue).all()


def test_requires_grad_on_geometry_raises(cuda, meshes):
    from mi3d import _lib, mesh
    v, t = meshes["quad"]
    c2w, K = cameras("quad")
    s = sources("quad", v, t)
    dv, dt = dev(cuda, v, F), dev(cuda, t, np.int32)
    with pytest.raises(_lib.Mi3dError, match="only colors and a float32 texture are differentiable"):
        mesh.render(dev(cuda, v, F).requires_grad_(True), dt, c2w, K, H, W, colors=dev(cuda, s["colors"]))
    with pytest.raises(_lib.Mi3dError, match="uvs requires grad"):
        mesh.render(dv, dt, c2w, K, H, W, uvs=dev(cuda, s["vt"]).requires_grad_(True), texture=dev(cuda, s["texture"]))
    with pytest.raises(_lib.Mi3dError, match="normals requires grad"):
        mesh.render(dv, dt, c2w, K, H, W, colors=dev(cuda, s["colors"]), normals=dev(cuda, s["vn"]).requires_grad_(True))
    # without requires_grad nothing changes: the bits of a plain call, and no graph
    plain, _ = mesh.render(dv, dt, c2w, K, H, W, colors=dev(cuda, s["colors"]), bg_color=BG)
    tracked, _ = mesh.render(dv, dt, c2w, K, H, W, colors=dev(cuda, s["colors"]).requires_grad_(True), bg_color=BG)
    assert not plain.requires_grad and tracked.requires_grad
    assert plain.cpu().numpy().tobytes() == tracked.detach().cpu().numpy().tobytes()


def test_fit_texture_follows_the_float64_restatements_loss_history(cuda):
    """mesh.fit_texture on the quad of the CPU test's fit_case(), from a grey start against the float64 restatement's
    renders of a smooth texture, 40 iterations at lr 0.05: the loss before every step against the float64 restatement's
    (tests/test_mesh_shade_grad_cpu.py holds that run to its RECORDED values).  A binary32 run of the restatement on the
    CPU drifts from the binary64 one by at most 4.74e-07 of the loss over these iterations (DRIFT, measured there); this
    binary32 run is allowed four times that, 1.9e-06.  Texels no usable pixel touches keep their bytes."""
    import torch
    from mi3d import mesh
    v, t = CPU.case("quad")[:2]
    target, start, masks, weights = CPU.fit_case()
    T = CPU.T
    value, history = mesh.fit_texture(dev(cuda, v, F), dev(cuda, t, np.int32), dev(cuda, CPU.quad_uv(v, t)),
                                      dev(cuda, start.reshape(T, T, 3), F), target, CPU.slanted_views(),
                                      M.pinhole(CPU.FOCAL, H, W), masks=masks, weights=weights, iterations=CPU.ITERATIONS,
                                      lr=CPU.LR, bg_color=CPU.BG, return_history=True)
    want = CPU.run_fit(torch.float64)[1]
    drift = max(abs(a - b) / b for a, b in zip(history, want))
    print(f"[mesh shade grad] fit_texture: loss {history[0]:.6g} -> {history[-1]:.6g}; largest relative difference from the "
          f"float64 restatement {drift:.3g} (allowed {4 * CPU.DRIFT:.3g})")
    assert len(history) == CPU.ITERATIONS and drift <= 4 * CPU.DRIFT
    value = value.cpu().numpy().reshape(-1, 3)
    p32 = CPU.plans("quad")[0]
    touched = np.zeros(T * T, bool)
    touched[p32["index"].ravel()] = True
    assert (~touched).sum() > 100 and (value[~touched].view(np.uint32) == F(0.5).view(np.uint32)).all()


def test_fit_colors_lowers_the_loss_and_leaves_unseen_vertices_alone(cuda, meshes):
    from mi3d import mesh
    v, t = meshes["sphere"]
    c2w, K = cameras("sphere")
    s = sources("sphere", v, t)
    dv, dt = dev(cuda, v, F), dev(cuda, t, np.int32)
    target, _ = mesh.render(dv, dt, c2w[:2], K, H, W, colors=dev(cuda, s["colors"]), bg_color=BG)
    start = np.full((len(v), 3), 0.5, F)
    value, history = mesh.fit_colors(dv, dt, dev(cuda, start), target, c2w[:2], K, iterations=12, lr=0.05, bg_color=BG,
                                     return_history=True)
    tri = winners(gpu_keys(cuda, v, t, M.view_records(c2w[:2], K)).cpu().numpy(), v, t)
    seen = np.zeros(len(v), bool)
    seen[t[tri[tri >= 0]].ravel()] = True
    value = value.cpu().numpy()
    print(f"[mesh shade grad] fit_colors: loss {history[0]:.4g} -> {history[-1]:.4g}, {seen.sum()} of {len(v)} vertices seen")
    assert history[-1] < 0.5 * history[0] and 100 < seen.sum() < len(v) - 100
    assert value[~seen].tobytes() == start[~seen].tobytes() and (value[seen] != 0.5).any()


# ------------------------------------------------------------------------------------------------ export

def test_export_with_fit_does_not_lower_the_fidelity_and_without_it_is_untouched(cuda, model, small_surface, tmp_path):
    import torch
    from mi3d import mesh
    R_, T = small_surface, 256
    c2w, K = M.orbit(3, 3.2, 0.4, 0.1), M.pinhole(1.6, H, W)     # outside the box: its half-diagonal is 1.74
    images, _ = mesh.render_field(model, c2w, K, H, W)           # the views the preview's fidelity is measured against
    views = dict(images=images.clamp(0, 1), c2w=c2w, K=K)
    preview = dict(c2w=c2w, K=K, H=H, W=W, fidelity=True)
    plain = model.export_mesh(str(tmp_path / "plain"), resolution=R_, texture_size=T, views=views, preview=preview)
    fitted = model.export_mesh(str(tmp_path / "fit"), resolution=R_, texture_size=T, preview=preview,
                               views=dict(views, fit=dict(iterations=30, lr=0.02)))
    a, b = (json.load(open(tmp_path / d / "preview.json")) for d in ("plain", "fit"))
    print(f"[mesh shade grad] export at {R_}^3: union PSNR {a['psnr_union']:.3f} -> {b['psnr_union']:.3f} dB with fit, "
          f"intersection {a['psnr_intersection']:.3f} -> {b['psnr_intersection']:.3f} dB")
    assert b["psnr_union"] >= a["psnr_union"]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain[:4], fitted[:4]))
    for name in ("mesh.obj", "mesh.mtl"):
        assert open(tmp_path / "fit" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
    assert decode_png(str(tmp_path / "fit" / "albedo.png")).tobytes() == fitted[4].tobytes()
    # a texel no pixel of any view touched keeps its byte; some texels moved
    dv, dt = torch.from_numpy(plain[0]).to(cuda), torch.from_numpy(plain[1]).to(cuda)
    tri = winners(gpu_keys(cuda, plain[0], plain[1], M.view_records(c2w, K)).cpu().numpy(), plain[0], plain[1])
    p = G.plan(plain[0], plain[1], M.view_records(c2w, K), H, W, tri, plain[3], T)
    touched = np.zeros(T * T, bool)
    touched[p["index"].ravel()] = True
    touched = touched.reshape(T, T)
    assert (~touched).sum() > 1000 and (fitted[4][~touched] == plain[4][~touched]).all()
    assert (fitted[4][touched] != plain[4][touched]).any()
    # without fit: what bake_views gives, as before
    image = mesh.bake_views(model, dv, dt, T, **views)[0].cpu().numpy()
    assert plain[4].tobytes() == image.tobytes()
    none = model.export_mesh(str(tmp_path / "none"), resolution=R_, texture_size=T, views=dict(views, fit=None))
    for name in ("mesh.obj", "mesh.mtl", "albedo.png"):
        assert open(tmp_path / "none" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, none))
