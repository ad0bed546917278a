"""What the depth gradient costs: the composite backward with and without it, and the reference-view step.

    python tools/ref_view_bench.py [--out profiles/ref_view_step.json]

1. The C2 dense sample set (bench.py's headline shapes: a 128 x 128 view, max_steps 1024, dense occupancy, the untrained
   field's sigmas and colours).  mi3d_composite_rays_train_backward (the parent's code: the baseline) and
   mi3d_composite_rays_train_backward_depth with a non-zero grad_depth are launched alternately in one process, each
   timed with HIP events; the medians and their ratio are recorded.
2. mi3d.sds_step.ref_view_train_step at 128 x 128 rays against a 512 x 512 reference image, depth_grad off and on,
   alternating, host clock around a synchronised step.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]
import torch  # noqa: E402


def capture_composite_inputs(model, rays):
    """The tensors run_cuda hands the training compositor for these rays."""
    import raymarching
    cap, orig = {}, raymarching.composite_rays_train

    def spy(sigmas, rgbs, deltas, rays_, T_thresh=1e-4):
        cap.update(sigmas=sigmas.float().contiguous(), rgbs=rgbs.float().contiguous(), deltas=deltas, rays=rays_,
                   T_thresh=T_thresh)
        return orig(sigmas, rgbs, deltas, rays_, T_thresh)
    raymarching.composite_rays_train = spy
    try:
        with torch.no_grad():
            model.render(rays[0], rays[1], depth_scale=rays[2], bg_color=torch.ones(3, device=rays[0].device),
                         perturb=False, force_all_rays=True, max_steps=model.opt.max_steps, depth_grad=False)
    finally:
        raymarching.composite_rays_train = orig
    return cap


def time_backward_kernels(cap, warmup, runs):
    import raymarching
    from mi3d import _lib as L
    sig, rgb, deltas, rays, T_thresh = cap["sigmas"], cap["rgbs"], cap["deltas"], cap["rays"], cap["T_thresh"]
    M, N = sig.shape[0], rays.shape[0]
    ws, depth, image = raymarching.composite_rays_train(sig, rgb, deltas, rays, T_thresh)
    gen = torch.Generator(device=sig.device).manual_seed(0)
    g_ws, g_d = (torch.randn(N, device=sig.device, generator=gen) for _ in range(2))
    g_img = torch.randn(N, 3, device=sig.device, generator=gen)
    gs, gc = torch.zeros_like(sig), torch.zeros_like(rgb)
    p = L.ptr

    def plain():
        L.launch("mi3d_composite_rays_train_backward", sig, p(g_ws), p(g_img), p(sig), p(rgb), p(deltas), p(rays), p(ws),
                 p(image), M, N, float(T_thresh), p(gs), p(gc))

    def with_depth():
        L.launch("mi3d_composite_rays_train_backward_depth", sig, p(g_ws), p(g_d), p(g_img), p(sig), p(rgb), p(deltas),
                 p(rays), p(ws), p(depth), p(image), M, N, float(T_thresh), p(gs), p(gc))

    times = {"plain": [], "depth": []}
    for i in range(warmup + runs):
        for name, fn in (("plain", plain), ("depth", with_depth)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    a, b = statistics.median(times["plain"]), statistics.median(times["depth"])
    return {"samples": M, "rays": N, "runs_each": runs, "warmup_each": warmup,
            "backward_ms": a, "backward_ms_min_max": [min(times["plain"]), max(times["plain"])],
            "backward_depth_ms": b, "backward_depth_ms_min_max": [min(times["depth"]), max(times["depth"])],
            "ratio_depth_over_plain": b / a}


def time_ref_view_step(dev, hw, warmup, runs):
    from mi3d import rays as R, sds_step
    opt = sds_step.make_opt()
    S = 512
    gen = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    r2 = xx ** 2 + yy ** 2
    ref_imgs = torch.cat([torch.rand(1, 3, S, S, generator=gen), (r2 < 0.5).float()[None, None]], 1).to(dev)
    ref_depth = (1.2 - 0.3 * torch.sqrt((0.5 - r2).clamp(min=0))).to(dev)
    depth_mask = (r2 >= 0.5).to(dev)
    rays = R.view_rays(hw, hw, device=dev)
    states = {flag: sds_step.build_training_state(opt, dev, bitfield="dense", init_scale=8.0) for flag in (False, True)}
    times = {False: [], True: []}
    for i in range(warmup + runs):
        for flag in (False, True):
            model, optimizer, scaler = states[flag]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = sds_step.ref_view_train_step(model, optimizer, scaler, rays[0], rays[1], rays[2], hw, hw, opt, ref_imgs,
                                                ref_depth, depth_mask, depth_grad=flag)
            torch.cuda.synchronize()
            if i >= warmup:
                times[flag].append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(loss)
    off, on = statistics.median(times[False]), statistics.median(times[True])
    return {"rays": hw * hw, "ref_size": S, "fp16": bool(opt.fp16), "bitfield": "dense", "max_steps": opt.max_steps,
            "runs_each": runs, "warmup_each": warmup, "step_ms_depth_grad_off": off, "step_ms_depth_grad_on": on,
            "step_ms_off_min_max": [min(times[False]), max(times[False])],
            "step_ms_on_min_max": [min(times[True]), max(times[True])], "ratio_on_over_off": on / off}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_view_step.json"))
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.runs < 9:
        raise SystemExit("--runs: the medians are over >= 9 runs each")
    if not torch.cuda.is_available():
        raise SystemExit("ref_view_bench needs a GPU")
    from mi3d import network, rays as R, sds_step
    dev = torch.device("cuda:0")
    model = network.NeRFNetwork(sds_step.make_opt(max_steps=1024)).to(dev)
    model.train()
    sds_step.set_bitfield(model, "dense")
    cap = capture_composite_inputs(model, R.view_rays(128, 128, device=dev))
    del model
    out = {"device": torch.cuda.get_device_name(0),
           "composite_backward_c2_dense": time_backward_kernels(cap, a.warmup, a.runs)}
    del cap
    torch.cuda.empty_cache()
    out["ref_view_train_step_128"] = time_ref_view_step(dev, 128, a.warmup, a.runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
