"""GPU: the depth gradient of the training compositor (raymarching.composite_rays_train_depth, C ABI
mi3d_composite_rays_train_backward_depth), its switch in the renderer (run_cuda(depth_grad=...)) and the reference-view
training step that needs it (mi3d.sds_step.ref_view_train_step).

The oracle's C composite backward restates the reference's, which has no depth term, so the reference here is a torch
restatement of the forward in binary64 and autograd through it (`composite64` below).

Tolerances: grad_rgbs and grad_sigmas under the bounds tests/test_raymarching_gpu.py uses for this kernel (rtol 1e-4 /
atol 1e-6, and 2e-4 x max|reference|: the bracket of grad_sigmas sums terms of mixed sign).  Both sides must stop a ray
at the same sample for those bounds to mean anything, so every input asserts that no transmittance lies within 1 % of
T_thresh (the kernel's fp32 running product over <= 256 samples is good to ~1e-4 relative)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-4
STEPS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 256, 64, 128, 192)  # chunk carry, stops in any lane, exact multiples
SCALES = (3.0, 60.0, 400.0, 0.0)
MARGIN = 1e-2
# (T_thresh, seed): seeds chosen on the CPU so that every T_incl of the input is >= 3 % away from T_thresh (5.7 % and
# 3.4 %; the test asserts MARGIN on what it builds); 22 and 25 of the 56 rays stop early
KERNEL_CASES = [(1e-4, 7), (1e-2, 108)]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------- the binary64 reference


def composite64(sig, d0, d1, rgb, T_thresh):
    """One ray in binary64 torch: weights_sum, depth, image, the stop sample, and min |T_incl / T_thresh - 1|."""
    n = sig.shape[0]
    alpha = 1 - torch.exp(-sig * d0)
    T_incl = torch.cumprod(1 - alpha, 0)
    T_excl = torch.cat([torch.ones(1, dtype=torch.float64), T_incl[:-1]])
    t = torch.cumsum(d1, 0)
    below = torch.nonzero(T_incl.detach() < T_thresh)
    stop = int(below[0]) if below.numel() else n - 1  # the crossing sample is accumulated, then the ray stops
    w = torch.where(torch.arange(n) <= stop, alpha * T_excl, torch.zeros((), dtype=torch.float64))
    margin = float((T_incl.detach() / T_thresh - 1).abs().min())
    return w.sum(), (w * t).sum(), (w[:, None] * rgb).sum(0), stop, margin


def reference64(sig, rgb, deltas, rays, T_thresh, g_ws, g_d, g_img, post=None):
    """autograd of sum(g_ws ws + g_d depth + g_img image) over every ray whose slab fits (g_d None: no depth term).
    `post(ws, depth, index) -> depth'` lets the wiring test restate what the renderer does to depth.
    Returns grad_sigmas, grad_rgbs (binary64 numpy), live[M] (True on rows up to a ray's stop sample), the number of
    early-stopped rays and the smallest margin."""
    M = sig.shape[0]
    s = torch.tensor(sig, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(rgb, dtype=torch.float64, requires_grad=True)
    dl = torch.tensor(deltas, dtype=torch.float64)
    live = np.zeros(M, bool)
    total, stopped, margin = torch.zeros((), dtype=torch.float64), 0, np.inf
    for index, offset, count in np.asarray(rays).tolist():
        if count == 0 or offset + count > M:
            continue
        sl = slice(offset, offset + count)
        ws, dep, img, stop, m = composite64(s[sl], dl[sl, 0], dl[sl, 1], c[sl], T_thresh)
        live[offset:offset + stop + 1] = True
        stopped += stop < count - 1
        margin = min(margin, m)
        total = total + float(g_ws[index]) * ws + (torch.tensor(g_img[index], dtype=torch.float64) * img).sum()
        if g_d is not None:
            total = total + float(g_d[index]) * (dep if post is None else post(ws, dep, index))
    total.backward()
    return s.grad.numpy(), c.grad.numpy(), live, stopped, margin


# ---------------------------------------------------------------------------- the kernel's input


@functools.lru_cache(maxsize=None)
def kernel_case(seed):
    """56 rays = STEPS x SCALES (ray id = scale-major), one slab each, M = 5676; a 57th ray whose slab overflows M.
    Slabs are laid out with the scale-400 block last, so that the in-bounds rows of the overflowing ray are rows past the
    stop sample of the last ray: they stay zero only if the overflowing ray is skipped.  Rows of `rays` are a permutation
    of the ray ids (index != row)."""
    rng = np.random.default_rng(seed)
    ids = [(k, n, sc) for k, (sc, n) in enumerate((sc, n) for sc in SCALES for n in STEPS)]
    layout = [r for r in ids if r[2] != 400.0] + [r for r in ids if r[2] == 400.0]
    M = sum(n for _, n, _ in ids)
    assert M == 5676 and len(ids) == 56
    scale, first, rows, off = np.zeros(M), [], np.zeros((57, 3), np.int32), 0
    for k, n, sc in layout:
        rows[k] = (k, off, n)
        scale[off:off + n] = sc
        if n:
            first.append(off)
        off += n
    rows[56] = (56, M - 32, 64)
    d0 = rng.uniform(0.003, 0.02, M).astype(np.float32)
    sig = (rng.exponential(1.0, M) * scale).astype(np.float32)
    d1 = d0.copy()
    d1[first] = 0
    rgb = rng.random((M, 3)).astype(np.float32)
    rays = rows[rng.permutation(57)]
    assert (rays[:, 0] != np.arange(57)).any()
    g = dict(ws=rng.normal(size=57).astype(np.float32), d=rng.normal(size=57).astype(np.float32),
             img=rng.normal(size=(57, 3)).astype(np.float32))
    return sig, rgb, np.stack([d0, d1], 1), rays, g


@functools.lru_cache(maxsize=None)
def kernel_reference(seed, T_thresh):
    sig, rgb, deltas, rays, g = kernel_case(seed)
    with_d = reference64(sig, rgb, deltas, rays, T_thresh, g["ws"], g["d"], g["img"])
    without = reference64(sig, rgb, deltas, rays, T_thresh, g["ws"], None, g["img"])
    return with_d, without[0]


def _backward(fn, case, dev, T_thresh, g_d="given", use_depth=True):
    sig, rgb, deltas, rays, g = case
    s_t, c_t = T(sig, dev).requires_grad_(True), T(rgb, dev).requires_grad_(True)
    ws, dep, img = fn(s_t, c_t, T(deltas, dev), T(rays, dev), T_thresh)
    if use_depth:
        gd = T(g["d"], dev) if g_d == "given" else torch.zeros_like(dep)
        torch.autograd.backward([ws, dep, img], [T(g["ws"], dev), gd, T(g["img"], dev)])
    else:  # a loss that never touches depth: grad_depth arrives as None
        ((ws * T(g["ws"], dev)).sum() + (img * T(g["img"], dev)).sum()).backward()
    return s_t.grad, c_t.grad


@pytest.mark.parametrize("T_thresh,seed", KERNEL_CASES)
def test_depth_backward_kernel_against_binary64(cuda, T_thresh, seed):
    """On the MI355X: grad_sigmas 7.5e-8 / 7.8e-8 x the scale (bound 2e-4), grad_rgbs 1.3e-7 absolute; against the same
    reference without its depth term 0.79 / 0.56 x the scale."""
    import raymarching
    case = kernel_case(seed)
    (gs_r, gc_r, live, stopped, margin), gs_nodepth = kernel_reference(seed, T_thresh)
    M = case[0].shape[0]
    print(f"T_thresh {T_thresh}: {stopped} early-stopped rays, margin {margin:.3g}")
    assert margin >= MARGIN and stopped >= 22
    assert not live[M - 32:].any()  # the overflowing ray's in-bounds rows lie past the last ray's stop sample

    gs, gc = _backward(raymarching.composite_rays_train_depth, case, cuda, T_thresh)
    gs, gc = gs.cpu().numpy(), gc.cpu().numpy()
    scale = np.abs(gs_r).max()
    err, err_nodepth = np.abs(gs - gs_r).max() / scale, np.abs(gs - gs_nodepth).max() / scale
    print(f"grad_sigmas: err {err:.3g} x scale; against a reference without the depth term {err_nodepth:.3g} x scale; "
          f"grad_rgbs max abs err {np.abs(gc - gc_r).max():.3g}")
    assert (gs[~live] == 0).all() and (gc[~live] == 0).all()  # past the stop sample, and the overflowing ray's rows
    assert (gs_r[~live] == 0).all()
    np.testing.assert_allclose(gc, gc_r, rtol=RTOL, atol=1e-6)
    assert err <= 2e-4
    assert err_nodepth > 0.1  # a kernel that ignores grad_depth cannot pass


def test_depth_off_means_off(cuda):
    """grad_depth of zeros: bit-identical to composite_rays_train; a loss that never touches depth: the same, and through
    the existing backward entry (the kernel a novel-view step runs today)."""
    import raymarching
    from mi3d import _lib
    T_thresh, seed = KERNEL_CASES[0]
    case = kernel_case(seed)
    gs0, gc0 = _backward(raymarching.composite_rays_train, case, cuda, T_thresh)
    assert float(gs0.abs().max()) > 0
    gs1, gc1 = _backward(raymarching.composite_rays_train_depth, case, cuda, T_thresh, g_d="zeros")
    assert torch.equal(gs1, gs0) and torch.equal(gc1, gc0)

    launched, orig = [], _lib.launch
    _lib.launch = lambda name, *a: (launched.append(name), orig(name, *a))[1]
    try:
        gs2, gc2 = _backward(raymarching.composite_rays_train_depth, case, cuda, T_thresh, use_depth=False)
    finally:
        _lib.launch = orig
    assert torch.equal(gs2, gs0) and torch.equal(gc2, gc0)
    assert launched == ["mi3d_composite_rays_train_forward", "mi3d_composite_rays_train_backward"]


# ---------------------------------------------------------------------------- renderer wiring


def _render_depth_grad(dev, depth_grad):
    """sum(g * outputs["depth"]) back-propagated through run_cuda on an untrained field; returns the compositor's
    captured inputs, d loss / d sigmas, g, depth_scale and max_depth."""
    import raymarching
    from mi3d import rays as R, sds_step
    # the untrained field is its density blob.  The default blob (density 5, radius 0.1) puts a transmittance within
    # 0.03 % of T_thresh on these rays whatever the view; density 4 / radius 0.2 gives 52 early-stopped rays of 256 and a
    # margin of 3.8 % (worked out with the CPU oracle's march and field; asserted below on what the GPU produced)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0, fp16=False, blob_density=4.0, blob_radius=0.2)
    model, _, _ = sds_step.build_training_state(opt, dev, bitfield=0.5)
    ro, rd, ds = R.view_rays(16, 16, device=dev)
    assert float(ds.max() - ds.min()) > 1e-4  # a depth_scale that is not all ones
    name = "composite_rays_train_depth" if depth_grad else "composite_rays_train"
    other = "composite_rays_train" if depth_grad else "composite_rays_train_depth"
    cap, orig = {}, getattr(raymarching, name)

    def spy(sigmas, rgbs, deltas, rays, T_thresh):
        sigmas.retain_grad()
        cap.update(sigmas=sigmas, rgbs=rgbs, deltas=deltas, rays=rays, T_thresh=T_thresh)
        return orig(sigmas, rgbs, deltas, rays, T_thresh)

    def never(*a):
        raise AssertionError(f"{other} called with depth_grad={depth_grad}")

    saved = getattr(raymarching, other)
    setattr(raymarching, name, spy)
    setattr(raymarching, other, never)
    try:
        out = model.render(ro, rd, depth_scale=ds, bg_color=torch.ones(3, device=dev), perturb=False,
                           force_all_rays=True, max_steps=64, depth_grad=depth_grad)
        g = torch.randn(out["depth"].shape, generator=torch.Generator().manual_seed(3)).to(dev)
        (g * out["depth"]).sum().backward()
    finally:
        setattr(raymarching, name, orig)
        setattr(raymarching, other, saved)
    return cap, cap["sigmas"].grad, g.reshape(-1), ds.reshape(-1), opt.max_depth


def _wiring_reference(cap, g, ds, max_depth):
    sig, rgb = cap["sigmas"].detach().cpu().numpy(), cap["rgbs"].detach().cpu().numpy()
    deltas, rays = cap["deltas"].cpu().numpy(), cap["rays"].cpu().numpy()
    g, ds = g.cpu().numpy().astype(np.float64), ds.cpu().numpy().astype(np.float64)
    N = rays.shape[0]
    return reference64(sig, rgb, deltas, rays, cap["T_thresh"], np.zeros(N), g, np.zeros((N, 3)),
                       post=lambda ws, dep, i: (dep + (1 - ws) * max_depth) * ds[i])


def test_renderer_depth_grad_switch(cuda):
    """run_cuda(depth_grad=True): d sum(g depth) / d sigmas is the binary64 gradient of
    (depth + (1 - weights_sum) max_depth) depth_scale on the tensors the compositor was given; with the switch off the
    same loss gives the reference op's gradient, which lacks the depth term."""
    cap, gs, g, ds, max_depth = _render_depth_grad(cuda, True)
    gs_r, _, live, stopped, margin = _wiring_reference(cap, g, ds, max_depth)
    rays = cap["rays"].cpu().numpy()
    print(f"{int((rays[:, 2] > 0).sum())} rays hit, {int(cap['sigmas'].shape[0])} rows, {stopped} early-stopped, "
          f"margin {margin:.3g}, sigma max {float(cap['sigmas'].detach().max()):.3g}")
    assert margin >= MARGIN and (rays[:, 2] > 0).sum() >= 32
    scale = np.abs(gs_r).max()
    err = np.abs(gs.cpu().numpy() - gs_r).max() / scale
    print(f"depth_grad on: err {err:.3g} x scale")
    assert err <= 2e-4

    # rows arrive in another order in every run (one slab atomic per wave), so the second render is compared with the
    # same restatement on ITS captured tensors
    cap0, gs0, g0, ds0, _ = _render_depth_grad(cuda, False)
    gs_r0, _, _, _, margin0 = _wiring_reference(cap0, g0, ds0, max_depth)
    assert margin0 >= MARGIN
    err0 = np.abs(gs0.cpu().numpy() - gs_r0).max() / np.abs(gs_r0).max()
    print(f"depth_grad off: differs by {err0:.3g} x scale")
    assert err0 > 0.1


# ---------------------------------------------------------------------------- the reference-view step


def _ref_view_step(dev, fp16, depth_grad):
    from mi3d import rays as R, sds_step
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0, fp16=fp16)
    model, optimizer, scaler = sds_step.build_training_state(opt, dev, bitfield=0.5, init_scale=8.0 if fp16 else None)
    ro, rd, ds = R.view_rays(16, 16, device=dev)
    gen = torch.Generator().manual_seed(11)
    S = 32
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    r2 = xx ** 2 + yy ** 2
    ref_imgs = torch.cat([torch.rand(1, 3, S, S, generator=gen), (r2 < 0.5).float()[None, None]], 1).to(dev)
    ref_depth = (1.2 - 0.3 * torch.sqrt((0.5 - r2).clamp(min=0)) + 0.01 * torch.rand(S, S, generator=gen)).to(dev)
    depth_mask = (r2 >= 0.5).to(dev)  # True = no prior there
    before = model.encoder.params.detach().clone()
    torch.manual_seed(5)
    loss = sds_step.ref_view_train_step(model, optimizer, scaler, ro, rd, ds, 16, 16, opt, ref_imgs, ref_depth, depth_mask,
                                        depth_grad=depth_grad)
    return loss, model.encoder.params.grad.detach().clone(), before, model.encoder.params.detach().clone()


@pytest.mark.parametrize("fp16", [True, False])
def test_ref_view_train_step(cuda, fp16):
    """One reference-view step: finite loss, a hash-table gradient, parameters that move, and a gradient that depends on
    the switch from identical state and RNG.  Without the smoothness jitter two identical steps differ only through
    the order of atomic adds (the hash-table gradient is accumulated in fixed point: none; the MLP's fp32 atomics reach
    it through the clip factor: ~1e-7 of the scale), so 1e-4 x the scale separates switch from noise; lambda_img = 1e3
    against lambda_depth = 1 leaves the depth term 5.7e-4 (autocast) and 5.9e-4 (fp32) x the scale on the MI355X."""
    loss1, g1, before, after = _ref_view_step(cuda, fp16, True)
    loss0, g0, _, _ = _ref_view_step(cuda, fp16, False)
    scale = float(g0.abs().max())
    diff = float((g1 - g0).abs().max())
    print(f"fp16 {fp16}: loss {float(loss1):.6g} / {float(loss0):.6g}, grad scale {scale:.3g}, on - off {diff / scale:.3g} x")
    assert torch.isfinite(loss1) and torch.isfinite(loss0)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0 and scale > 0
    assert diff > 1e-4 * scale
    assert not torch.equal(before, after)
