"""CPU: tests/mesh_shade_grad_model.py - the restatement of include/mi3d.h Part 18 that tests/test_mesh_shade_grad_gpu.py
compares the kernels with bit for bit - checked on its own: the binary32 fixed-point gradient against float64 autograd
within the bound counted from the rounding chain (the model's header), the adjoint identity, the exponent rule, the two
special cases, the fitting loop, and the refusals that need no device.

Sizes: 37 x 53 pixels, the cameras of test_mesh_render_cpu.py and test_mesh_render_gpu.py (the close one included)."""
import numpy as np
import pytest

import mesh_render_model as R
import mesh_shade_grad_model as G
import texture_views_model as M
from test_mesh_render_cpu import quad_uv, slanted_views
from test_texture_views_cpu import quad_mesh, sphere_mesh

F = np.float32
H, W = 37, 53
FOCAL = 1.2
U = 2.0 ** -24
BG = (0.25, 0.5, 0.75)
T = 64

_CASES = {}


def case(name):
    """(v, t, records, tri, vt or None, elements): the quad with its affine atlas at 64^2 from three slanted cameras, the
    sphere with vertex colours from two orbit cameras and one 0.05 above its surface.  Computed once; nobody writes."""
    if name not in _CASES:
        if name == "quad":
            v, t = quad_mesh()
            c2w, vt = slanted_views(), quad_uv(*quad_mesh())
        else:
            v, t = sphere_mesh()
            c2w, vt = np.concatenate([M.orbit(2, 2.4, 0.3, 0.2), M.look_at((0.55, 0.0, 0.3), target=(-1, 0, 0))[None]]), None
        rec = M.view_records(c2w, M.pinhole(FOCAL, H, W))
        _, tri, _ = R.visibility(v, t, rec, H, W)
        _CASES[name] = (v, t, rec, tri, vt, T * T if vt is not None else len(v))
    return _CASES[name]


def plans(name):
    v, t, rec, tri, vt, _ = case(name)
    key = name + "/plans"
    if key not in _CASES:
        _CASES[key] = (G.plan(v, t, rec, H, W, tri, vt, T), G.plan(v, t, rec, H, W, tri, vt, T, np.float64, bounds=True))
    return _CASES[key]


@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e30])
@pytest.mark.parametrize("name", ["quad", "sphere"])
def test_fixed_point_gradient_against_float64_autograd_within_the_counted_bound(name, scale):
    import torch
    elements = case(name)[5]
    p32, p64 = plans(name)
    rng = np.random.default_rng(3)
    g = (rng.normal(size=(3, H, W, 3)) * scale).astype(F)
    got = G.backward(p32, g, elements)
    source = torch.zeros(elements, 3, dtype=torch.float64, requires_grad=True)
    image = G.render_torch(source, G.torch_plan(p64, torch.float64), (3, H, W), BG)
    image.backward(torch.from_numpy(g.astype(np.float64)))
    want = source.grad.numpy()
    bound = G.bound(p64, p32, g, elements, got)
    err = np.abs(got.astype(np.float64) - want)
    touched = np.bincount(p32["index"].ravel(), minlength=elements)
    print(f"[mesh shade grad] {name} x {scale:g}: {len(p32['pixel'])} drawn pixels, up to {touched.max()} contributions per "
          f"element, max error {err.max() / scale:.3g}, max error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert len(p32["pixel"]) > 1500 and (err <= bound).all()
    assert (got[touched == 0].view(np.uint32) == 0).all()       # nothing touched: exactly +0
    if name == "sphere":
        assert touched.max() > 1000                             # the close camera: contention and headroom


@pytest.mark.parametrize("name", ["quad", "sphere"])
def test_adjoint_identity_in_float64(name):
    import torch
    elements = case(name)[5]
    p64 = plans(name)[1]
    rng = np.random.default_rng(4)
    c, g = rng.normal(size=(elements, 3)), rng.normal(size=(3 * H * W, 3))
    Jc = G.render_torch(torch.from_numpy(c), G.torch_plan(p64, torch.float64), (3, H, W), (0, 0, 0)).numpy().reshape(-1, 3)
    JTg = np.zeros((elements, 3))
    for k in range(p64["index"].shape[1]):
        np.add.at(JTg, p64["index"][:, k], p64["weight"][:, k, None] * g[p64["pixel"]])
    a, b = (Jc * g).sum(), (c * JTg).sum()
    assert abs(a - b) <= 1e-12 * (np.abs(Jc * g).sum() + np.abs(c * JTg).sum())


@pytest.mark.parametrize("N", [1, 5883, 2 ** 34])
@pytest.mark.parametrize("amax", [1e-30, 1.0, 1e30, 2.0 ** -140, float(np.finfo(F).max)])
def test_exponent_rule_never_overflows_and_keeps_26_bits(amax, N):
    amax = F(amax)
    bits, L = G.amax_bits(np.array([amax, -amax / 3])), G.levels(N)
    assert 2 ** L >= N and (L == 0 or 2 ** (L - 1) < N)
    e = G.exponent(bits, N)
    assert np.ldexp(1.0, e - L + 60) > float(amax)               # 2^(E + 1) > amax
    heavy = F(1.0) + 8 * F(U * 2)                                # a weight 8 ulp above 1
    q = int(G.contributions(np.array([heavy, -heavy]), np.array([amax, amax]), e, L).max())
    with np.errstate(over="ignore"):
        overflows = not np.isfinite(heavy * amax)               # binary32 itself gives up: the product saturates
    assert q == 2 ** (61 - L) if overflows else 0 < q <= 2 ** (60 - L) * (1 + 2 ** -19)
    assert 3 * N * q < 2 ** 63                                  # every pixel, thrice, at the largest value
    cap = int(G.contributions(np.array([F(3e38)]), np.array([F(3e38)]), e, L)[0])
    assert cap == 2 ** (61 - L) and 3 * N * cap < 2 ** 63        # the saturation bound, whatever the weights are
    assert G.contributions(np.array([F(np.nan)]), np.array([amax]), e, L)[0] == 0
    if float(amax) >= 2.0 ** -126:                               # a normal amax: half a unit is 26 bits below it
        assert np.ldexp(1.0, e - 1) <= float(amax) * 2.0 ** -26


def test_zero_and_non_finite_upstream_gradients():
    elements = case("quad")[5]
    p32 = plans("quad")[0]
    zero = G.backward(p32, np.zeros((3, H, W, 3), F), elements)
    assert (zero.view(np.uint32) == 0).all()
    assert (G.backward(p32, -np.zeros((3, H, W, 3), F), elements).view(np.uint32) == 0).all()
    for poison in (np.nan, np.inf, -np.inf):
        g = np.random.default_rng(5).normal(size=(3, H, W, 3)).astype(F)
        g[2, 0, 0, 1] = poison                                   # a background pixel: the rule does not ask where
        assert (G.backward(p32, g, elements).view(np.uint32) == G.QUIET_NAN).all()


def test_f32_forward_restatement_equals_part_17s_up_to_the_division():
    """shade_f32 on a texture of whole numbers 0 .. 255 is mesh_render_model's uint8 blend before its / 255."""
    v, t, rec, tri, vt, _ = case("quad")
    tex = np.random.default_rng(6).integers(0, 256, (T, T, 3), dtype=np.uint8)
    got = G.shade_f32(plans("quad")[0], tex.astype(F), (3, H, W), BG)
    want = R.shade(v, t, rec, H, W, tri, vt=vt, texture=tex, background=BG)["image"]
    drawn = tri >= 0
    assert ((got[drawn] / F(255.0)).tobytes() == want[drawn].tobytes()) and (got[~drawn] == np.array(BG, F)).all()


# ------------------------------------------------------------------------------------------------ the fitting loop

ITERATIONS, LR = 40, 0.05
# the float64 restatement's loss before steps 0, 9, 19, 29 and 39 of fit_case(): recorded from this test, which holds the
# restatement to them; tests/test_mesh_shade_grad_gpu.py compares mesh.fit_texture's history with the same run
RECORDED = {0: 0.0321652560371162, 9: 0.001233398800610383, 19: 0.0014116108006313947, 29: 0.00043043695163870406,
            39: 9.455335931334641e-05}
# the largest relative difference between the losses of a binary32 and the binary64 run of the restatement over those
# iterations, measured by test_fit_drift_of_a_binary32_run; the GPU test allows four times as much
DRIFT = 4.74e-07


def smooth_texture():
    y, x = np.meshgrid((np.arange(T) + 0.5) / T, (np.arange(T) + 0.5) / T, indexing="ij")
    return np.stack([0.5 + 0.4 * np.sin(5 * x + 2 * y), 0.5 + 0.4 * np.cos(3 * x - 4 * y), 0.5 + 0.4 * np.sin(6 * y + 1)], -1)


def fit_case():
    """The quad from the three slanted cameras: (target float32 [3, H, W, 3]: the float64 restatement's render of
    smooth_texture() over BG, rounded once; the grey start [T T, 3]; masks: view 1's left half is unusable; weights)."""
    import torch
    p64 = plans("quad")[1]
    truth = torch.from_numpy(smooth_texture().reshape(-1, 3))
    target = G.render_torch(truth, G.torch_plan(p64, torch.float64), (3, H, W), BG).numpy().astype(F)
    masks = np.ones((3, H, W), np.uint8)
    masks[1, :, :W // 2] = 0
    return target, np.full((T * T, 3), 0.5), masks, np.array([1.0, 2.0, 0.5], F)


def run_fit(dtype):
    import torch
    target, start, masks, weights = fit_case()
    p = plans("quad")[0 if dtype == torch.float32 else 1]
    return G.fit(start, G.torch_plan(p, dtype), (3, H, W), BG, target, G.pixel_weights(weights, masks, (3, H, W)),
                 ITERATIONS, LR, dtype)


def test_fit_on_the_float64_restatement_recovers_a_smooth_texture():
    """Adam at lr 0.05 moves a texel by about 0.05 a step, and the texture lies within 0.4 of the grey start: 40 steps
    reach it.  The loss falls a hundredfold, the texels the views touch end nearer to the texture than they began, and
    the others have not moved at all."""
    import torch
    value, history = run_fit(torch.float64)
    print(f"[mesh shade grad] fit, float64: loss {[history[k] for k in sorted(RECORDED)]}")
    assert history[-1] < history[0] / 100
    p64 = plans("quad")[1]
    masked = G.pixel_weights(np.array([1.0, 2.0, 0.5]), fit_case()[2], (3, H, W)).reshape(-1)[p64["pixel"]] > 0
    touched = np.zeros(T * T, bool)
    touched[p64["index"][masked].ravel()] = True
    truth, value = smooth_texture().reshape(-1, 3), value.numpy()
    assert touched.sum() > 500 and (~touched).sum() > 100
    assert np.abs(value - truth)[touched].mean() < 0.25 * np.abs(0.5 - truth)[touched].mean()
    assert (value[~touched] == 0.5).all()
    for k, want in RECORDED.items():
        assert want is not None and abs(history[k] - want) <= 1e-9 * want, (k, history[k])


def test_fit_drift_of_a_binary32_run():
    """How far a binary32 run of the same loop drifts from the binary64 one: the figure the GPU test's tolerance is four
    times of.  Another binary32 run - this one on another machine, the GPU's - gets the same allowance: four times the
    recorded DRIFT."""
    import torch
    h32, h64 = run_fit(torch.float32)[1], run_fit(torch.float64)[1]
    drift = max(abs(a - b) / b for a, b in zip(h32, h64))
    print(f"[mesh shade grad] fit, binary32 against binary64 over {ITERATIONS} iterations: largest relative difference "
          f"of the loss {drift:.3g}")
    assert 0 < drift <= 4 * DRIFT


# ------------------------------------------------------------------------------------------------ refusals without a device

def test_fit_and_render_check_their_arguments_before_the_mesh(tmp_path):
    from mi3d import mesh
    images, c2w, K = np.zeros((2, 8, 6, 3), F), M.orbit(2), M.pinhole(1.0, 8, 6)
    for kw, words in ((dict(iterations=0), "iterations"), (dict(iterations=2.5), "iterations"), (dict(lr=0.0), "lr"),
                      (dict(lr=float("nan")), "lr"), (dict(ssaa=3), "ssaa"), (dict(images=images[..., :2]), "images"),
                      (dict(weights=np.zeros(2)), "weights"), (dict(masks=np.ones((2, 8, 7))), "masks"),
                      (dict(c2w=c2w[:1]), "c2w"), (dict(bg_color=(1.0, 2.0)), "bg_color")):
        args = dict(images=images, c2w=c2w, K=K)
        args.update(kw)
        with pytest.raises(mesh.Mi3dError) as e:
            mesh.fit_texture(None, None, 0, None, **args)         # no mesh, no device: the options are refused first
        assert words in str(e.value)
        with pytest.raises(mesh.Mi3dError) as e:
            mesh.fit_colors(None, None, None, **args)
        assert words in str(e.value)
    good = dict(images=images, c2w=c2w, K=K)
    for fit, words in ((dict(steps=3), "fit"), ([3], "fit"), (dict(iterations=0), "iterations"), (dict(lr=2.0), "lr")):
        with pytest.raises(mesh.Mi3dError) as e:
            mesh.export(None, str(tmp_path), texture_size=256, views=dict(good, fit=fit))
        assert words in str(e.value)
    assert not any(tmp_path.iterdir())


def test_workspace_query_and_the_refusals_that_reach_no_device():
    from mi3d import _lib
    lib = _lib.lib()
    ws = lib.mi3d_mesh_shade_backward_workspace
    assert ws(0) == 8 and ws(12) == 8 * 13 and ws(3 * 4096 * 4096) == 8 * (3 * 4096 * 4096 + 1)
    assert ws(3 * (2 ** 31 - 1)) == 8 * (3 * (2 ** 31 - 1) + 1) and ws(3 * (2 ** 31 - 1) + 1) == 0
    # every pointer is a made-up address that is never dereferenced: a refused call launches nothing
    p = _lib.C.c_void_p
    a = dict(vertices=p(64), nv=4, triangles=p(64), nt=2, views=p(64), V=2, H=H, W=W, vis=p(64), dimage=p(64), vt=None, T=0,
             grad_colors=p(64), grad_texture=None, ws=p(64), ws_bytes=8 * 13)
    textured = dict(vt=p(64), T=64, grad_colors=None, grad_texture=p(64), ws_bytes=8 * (3 * 64 * 64 + 1))
    for kw in (dict(V=0), dict(V=65), dict(H=1), dict(W=16385), dict(vertices=None), dict(triangles=None), dict(views=None),
               dict(vis=None), dict(vis=p(68)), dict(nv=2 ** 31), dict(nt=2 ** 31), dict(dimage=None),
               dict(grad_colors=None),                                               # neither gradient
               dict(grad_texture=p(64)),                                             # both
               dict(vt=p(64)), dict(T=64), dict(vt=p(64), T=64),                     # vt without T, T without vt, vt with colours
               dict(textured, vt=None), dict(textured, T=0), dict(textured, T=63), dict(textured, T=16385),
               dict(ws=None), dict(ws=p(68)), dict(ws_bytes=8 * 13 - 1), dict(ws_bytes=0),
               dict(textured, ws_bytes=8 * 3 * 64 * 64)):
        b = dict(a)
        b.update(kw)
        assert lib.mi3d_mesh_shade_backward(*b.values(), None) == 1, kw
