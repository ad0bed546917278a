"""GPU: the position gradient of the refine-stage point renderer (csrc/raster.hip k_points_composite_bwd_dists and
k_raster_bwd_points, include/mi3d.h Part 7; mi3d.refine.rasterize_points / render_point / refine_train_step) against the
float64 model of tests/raster_grad_model.py fed the GPU's own idx.

Tolerance of the parity tests: the same model run in float32 on the CPU has a maximum error against float64, relative to
the largest gradient magnitude - the yardstick of what fp32 rounding does to this formula on these shapes.  The kernels
get 4 x that (atomic arrival order; the sqrt and the division of a different library).  Nothing of the bound comes from
the kernels' own output.  Every case prints both figures and appends them to refine_positions.json BEFORE it asserts -
in the directory MI3D_REPORT_DIR names, or in test_reports/ at the root of the repository (git-ignored); the kept copy
is the `parity` entry of profiles/refine_positions.json."""
import ctypes as C
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raster_grad_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

P = 6000
FOCAL = 1.0 / (2 * np.tan(np.radians(20) / 2))
CASES = [(64, 64, 8, 19), (33, 70, 3, 19), (40, 40, 1, 19), (64, 64, 8, 3),
         (70, 33, 3, 19)]                       # portrait: k_raster_bwd_points recomputes the pixel centre with H > W
COINCIDENT, PLANTED, PLANT_DEPTH = 40, slice(300, 330), 0.8     # the planted block sits in front of the shell
REPORT_PATH = os.path.join(os.environ.get("MI3D_REPORT_DIR") or os.path.join(ROOT, "test_reports"),
                           "refine_positions.json")
_REPORT = {}


def _record(key, **figures):
    print(key, " ".join(f"{k}={v:.3e}" for k, v in figures.items()))
    _REPORT[key] = figures
    os.makedirs(os.path.dirname(REPORT_PATH), exist_ok=True)
    with open(REPORT_PATH, "w") as f:
        json.dump({"parity": _REPORT}, f, indent=1)


def _cloud(rng, n, spread=0.35):
    """tests/test_raster_gpu.py's recipe: points on a noisy sphere shell around the origin"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * spread * (1 + 0.05 * rng.normal(size=(n, 1)))).astype(np.float32)


def scene(H, W, K, Cn):
    """CPU tensors only: the cloud (with a block of coincident points and a block unprojected from pixel centres, where
    the clamp binds), the camera of tests/test_raster_gpu.py, features and an upstream gradient."""
    from mi3d import rays as R
    rng = np.random.default_rng(H * 100 + K + Cn)
    pts = _cloud(rng, P)
    pts[:COINCIDENT] = pts[COINCIDENT:2 * COINCIDENT]
    w2c = torch.linalg.inv(R.orbit_pose(1.25, 80.0, 30.0)[0])
    xf, yf = M.pixel_centres(H, W)
    # every fifth pixel of the part of the image the projection reaches: the planted discs (2 px) do not overlap, so each
    # planted point is alone in front of its pixel
    ys, xs = np.nonzero(((np.abs(yf.numpy()) < 0.9) & (np.arange(H) % 5 == 2))[:, None]
                        & ((np.abs(xf.numpy()) < 0.9) & (np.arange(W) % 5 == 2))[None, :])
    pick = rng.choice(ys.size, PLANTED.stop - PLANTED.start, replace=False)
    ys, xs = ys[pick], xs[pick]
    # x_ndc = -2 f Xc / Zc (render_point's projection), so the camera-space point of a pixel centre at depth Zc is
    cam = np.stack([-xf.numpy()[xs] * PLANT_DEPTH / (2 * FOCAL), -yf.numpy()[ys] * PLANT_DEPTH / (2 * FOCAL),
                    np.full(xs.size, PLANT_DEPTH)], -1)
    Rm, t = w2c[:3, :3].double().numpy(), w2c[:3, 3].double().numpy()
    pts[PLANTED] = ((cam - t) @ Rm).astype(np.float32)           # R^T (p_cam - t), rows
    feats = rng.uniform(0, 1, (P, Cn)).astype(np.float32)
    gout = rng.normal(size=(Cn, H, W)).astype(np.float32)
    return SimpleNamespace(H=H, W=W, K=K, Cn=Cn, radius=2.0 / H * 2.0, pts=torch.from_numpy(pts), w2c=w2c,
                           feats=torch.from_numpy(feats), gout=torch.from_numpy(gout), plant_yx=(ys, xs))


def guard_clamp(u_used):
    """The condition of the parity tests: no used slot has the model's float64 u within 1e-5 relative of 1e-3, where the
    fp32 kernel and the model could disagree about the clamp."""
    assert float((u_used / 1e-3 - 1).abs().min()) >= 1e-5


@functools.lru_cache(maxsize=None)
def ndc_case(H, W, K, Cn):
    """Shared by the tests at the level of NDC points: the GPU's rasterisation of the projected cloud, with the planted
    block moved EXACTLY onto its pixel centres, and the model's d loss / d dists in float64 and float32."""
    from mi3d import refine
    dev = torch.device("cuda:0")
    s = scene(H, W, K, Cn)
    Kmat = refine.intrinsics(FOCAL, H, W, dev)
    ndc = M.project(s.pts.to(dev), s.w2c.to(dev), Kmat, H, W)
    xf32, yf32 = M.pixel_centres(H, W, torch.float32)
    ys, xs = s.plant_yx
    ndc[PLANTED, 0], ndc[PLANTED, 1] = xf32[xs].to(dev), yf32[ys].to(dev)
    ndc = ndc.contiguous()
    idx, _, dists = refine.rasterize_points(ndc, (H, W), s.radius, K)
    idx_c = idx.cpu()
    grads = {}
    for dt in (torch.float64, torch.float32):
        d = M.dists_from_idx(ndc.cpu().to(dt), idx_c).requires_grad_(True)
        (M.render_from_dists(d, idx_c, s.feats.to(dt), s.radius) * s.gout.to(dt)).sum().backward()
        grads[dt] = d.grad.double()
    u = M.clamp_argument(M.dists_from_idx(ndc.cpu().double(), idx_c), s.radius)
    return SimpleNamespace(s=s, ndc=ndc, idx=idx, dists=dists, idx_c=idx_c, g64=grads[torch.float64],
                           g32=grads[torch.float32], u=u)


@pytest.mark.parametrize("H,W,K,Cn", CASES)
def test_grad_dists_matches_the_model(cuda, H, W, K, Cn):
    from mi3d import _lib as L
    c = ndc_case(H, W, K, Cn)
    s, used = c.s, c.idx_c >= 0
    assert float(used[..., 0].float().mean()) > 0.05 and bool(used[..., K - 1].any())
    guard_clamp(c.u[used])
    feats, gout = s.feats.to(cuda), s.gout.to(cuda)
    gd = torch.full((H, W, K), float("nan"), device=cuda)               # every slot must be written
    L.launch("mi3d_points_composite_backward_dists", gout, L.ptr(c.idx), L.ptr(c.dists), H, W, K, L.ptr(gout),
             L.ptr(feats), Cn, C.c_double(s.radius), L.ptr(gd))
    gd = gd.cpu().double()
    scale = float(c.g64.abs().max())
    yard = float((c.g32 - c.g64).abs().max()) / scale
    err = float((gd - c.g64).abs().max()) / scale
    _record(f"grad_dists[{H}x{W},K={K},C={Cn}]", fp32_model_rel_err=yard, kernel_rel_err=err, bound=4 * yard)
    assert bool(torch.isfinite(gd).all())
    assert bool((gd[~used] == 0).all())
    clamped = used & (c.u < 1e-3)
    assert int(clamped.sum()) >= PLANTED.stop - PLANTED.start and bool((gd[clamped] == 0).all())
    assert bool((c.g64[clamped] == 0).all()) and bool((gd[used & ~clamped] != 0).any())
    ys, xs = s.plant_yx                                                 # the planted block is in front and clamped
    front = c.idx_c[ys, xs, 0]
    assert bool(((front >= PLANTED.start) & (front < PLANTED.stop)).all()) and bool(clamped[ys, xs, 0].all())
    assert err <= 4 * yard, (err, yard)


def _render_with_idx(monkeypatch, *args):
    """render_point(*args) and the idx its rasterisation produced."""
    from mi3d import refine
    seen, orig = [], refine.rasterize_points

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(out[0])
        return out
    monkeypatch.setattr(refine, "rasterize_points", spy)
    out = refine.render_point(*args)
    monkeypatch.undo()
    return out, seen[0]


@pytest.mark.parametrize("H,W,K,Cn", CASES)
def test_render_point_backward_matches_the_model(cuda, monkeypatch, H, W, K, Cn):
    from mi3d import refine
    s = scene(H, W, K, Cn)
    Kmat = refine.intrinsics(FOCAL, H, W, cuda)
    pts = s.pts.to(cuda).requires_grad_(True)
    w2c = s.w2c.to(cuda).requires_grad_(True)
    feats = s.feats.to(cuda)
    out, idx = _render_with_idx(monkeypatch, pts, feats, H, W, Kmat, w2c, (H, W), s.radius, K)
    out.backward(s.gout.to(cuda)[None])
    idx_c = idx.cpu()
    ref = {}
    for dt in (torch.float64, torch.float32):
        x, cam = s.pts.to(dt).clone().requires_grad_(True), s.w2c.to(dt).clone().requires_grad_(True)
        img = M.render(x, s.feats.to(dt), idx_c, cam, Kmat.cpu().to(dt), H, W, s.radius)
        (img * s.gout.to(dt)).sum().backward()
        ref[dt] = (x.grad.double(), cam.grad.double(), img.detach().double())
    with torch.no_grad():
        u = M.clamp_argument(M.dists_from_idx(M.project(s.pts.double(), s.w2c.double(), Kmat.cpu().double(), H, W),
                                              idx_c), s.radius)
    guard_clamp(u[idx_c >= 0])
    figures, ok = {}, True
    for name, got, i in (("points", pts.grad, 0), ("world2cam", w2c.grad, 1)):
        want, scale = ref[torch.float64][i], float(ref[torch.float64][i].abs().max())
        yard = float((ref[torch.float32][i] - want).abs().max()) / scale
        err = float((got.cpu().double() - want).abs().max()) / scale
        figures.update({f"{name}_fp32_model_rel_err": yard, f"{name}_kernel_rel_err": err, f"{name}_bound": 4 * yard})
        ok = ok and scale > 0 and err <= 4 * yard
    _record(f"render_point_backward[{H}x{W},K={K},C={Cn}]", **figures)
    # the forward the gradients belong to is the model's: same visibility, same image
    assert float((out[0].detach().cpu().double() - ref[torch.float64][2]).abs().max()) <= 1e-4
    assert bool((w2c.grad[3] == 0).all())
    assert ok, figures


def test_zero_upstream_gradient_and_the_z_column(cuda):
    from mi3d import refine
    H, W, K, Cn = CASES[0]
    s = scene(H, W, K, Cn)
    Kmat = refine.intrinsics(FOCAL, H, W, cuda)
    pts = s.pts.to(cuda).requires_grad_(True)
    w2c = s.w2c.to(cuda).requires_grad_(True)
    refine.render_point(pts, s.feats.to(cuda), H, W, Kmat, w2c, (H, W), s.radius, K).backward(
        torch.zeros(1, Cn, H, W, device=cuda))
    assert bool((pts.grad == 0).all()) and bool((w2c.grad == 0).all())
    # NDC points as the leaf: depth decides only the order, so the z column is exactly 0 whatever arrives
    c = ndc_case(H, W, K, Cn)
    ndc = c.ndc.clone().requires_grad_(True)
    idx, zbuf, dists = refine.rasterize_points(ndc, (H, W), s.radius, K)
    assert torch.equal(idx, c.idx) and torch.equal(dists.detach(), c.dists)
    assert dists.requires_grad and not idx.requires_grad and not zbuf.requires_grad
    refine._PointComposite.apply(s.feats.to(cuda), idx, dists, s.radius).backward(s.gout.to(cuda))
    assert bool((ndc.grad[:, 2] == 0).all()) and float(ndc.grad[:, :2].abs().max()) > 0
    assert bool(torch.isfinite(ndc.grad).all())


def test_fixed_positions_take_the_old_path(cuda):
    """Positions not requiring grad: render_point returns the bits of _PointComposite on the plain rasterize_points
    output for the reference's in-place projection, nothing is saved for a position gradient, and the feature gradient
    stays within tests/test_raster_gpu.py's 2e-5 x max of the oracle's closed form."""
    from mi3d import refine
    from oracle import raster_ref as O
    H, W, K, Cn = CASES[0]
    s = scene(H, W, K, Cn)
    Kmat = refine.intrinsics(FOCAL, H, W, cuda)
    x, w2c = s.pts.to(cuda), s.w2c.to(cuda)
    f = s.feats.to(cuda).requires_grad_(True)
    out = refine.render_point(x, f, H, W, Kmat, w2c, (H, W), s.radius, K)
    proj = torch.matmul(x, w2c[:3, :3].T) + w2c[:3, 3]
    proj = torch.matmul(proj, Kmat.T)
    proj[:, 0:2] = proj[:, 0:2] / proj[:, 2:]
    proj[:, 0] = proj[:, 0] / W * 2 - 1.0
    proj[:, 1] = proj[:, 1] / H * 2 - 1.0
    proj[:, 0] = proj[:, 0] * -1
    proj[:, 1] = proj[:, 1] * -1
    idx, _, dists = refine.rasterize_points(proj, (H, W), s.radius, K)
    assert not dists.requires_grad
    plain = refine._PointComposite.apply(s.feats.to(cuda), idx, dists, s.radius)
    assert torch.equal(out[0].detach(), plain)
    assert len(out.grad_fn.next_functions[0][0].saved_tensors) == 2         # idx, dists: no features kept
    out.backward(s.gout.to(cuda)[None])
    idx_n = idx.cpu().numpy()
    _, w_o = O.alpha_composite(idx_n, O.point_alphas(dists.cpu().numpy(), s.radius), s.feats.numpy())
    g_o = O.alpha_composite_backward(idx_n, w_o, s.gout.numpy(), P)
    assert np.abs(f.grad.cpu().numpy() - g_o).max() <= 2e-5 * np.abs(g_o).max()


def test_refine_train_step_moves_learnable_points(cuda):
    """One front-view and one novel-view step at 64 x 64 with the points an nn.Parameter of the optimiser and an origin
    to regularise towards; then the same calls with a plain tensor, which behave as they did."""
    from mi3d import rays as R, refine, sd_standin as S
    n, H = 4000, 64
    g = S.StableDiffusionStandIn(cuda, dtype=torch.float32, unet_kw=dict(ch=(64, 64, 64, 64), ctx_dim=32, layers=1),
                                 vae_kw=dict(ch=(32, 32, 32, 32), layers=1))
    text_z = torch.randn(2, 77, 32, device=cuda)
    w2c = torch.linalg.inv(R.orbit_pose(1.25, 80.0, 30.0, device=cuda)[0])
    ref_rgb = torch.rand(1, 3, H, H, device=cuda)
    gt_mask = (torch.rand(1, 1, H, H, device=cuda) > 0.3).float()
    for learnable in (True, False):
        torch.manual_seed(1)
        d = torch.randn(n, 3, device=cuda)
        start = (d / d.norm(dim=-1, keepdim=True) * 0.35).contiguous()
        points = torch.nn.Parameter(start.clone()) if learnable else start.clone()
        colour = torch.nn.Parameter(torch.rand(n, 3, device=cuda))
        feat = torch.nn.Parameter(torch.randn(n, 16, device=cuda))
        unet = refine.UNet(num_input_channels=19).to(cuda).train()
        opt = torch.optim.Adam([colour, feat] + ([points] if learnable else []) + list(unet.parameters()), lr=1e-3)
        args = (unet, {"colour": colour, "feat": feat}, opt, g, text_z, points, w2c, FOCAL, H, H, 2.0 / H * 2.0, 8,
                colour.detach().clone())
        kw = dict(points_origin=start, lambda_points=1e3) if learnable else {}
        c0, f0 = colour.detach().clone(), feat.detach().clone()
        loss = refine.refine_train_step(*args, is_front=True, ref_rgb=ref_rgb, gt_mask=gt_mask, **kw)
        assert torch.isfinite(loss) and float(loss) > 0
        assert float((colour - c0).abs().max()) > 0 and float((feat - f0).abs().max()) > 0
        moved = (points.detach() - start).abs()
        if learnable:
            assert bool(torch.isfinite(points).all()) and bool(torch.isfinite(points.grad).all())
            assert float(moved.max()) > 0 and float(points.grad.abs().max()) > 0
        else:
            assert float(moved.max()) == 0 and points.grad is None
        assert torch.isfinite(refine.refine_train_step(*args, t=500, **kw))           # the guidance's own backward first
        assert bool(torch.isfinite(points).all()) and bool(torch.isfinite(colour).all() and torch.isfinite(feat).all())
