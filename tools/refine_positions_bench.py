"""What learnable point positions cost the refine stage: render_point and the whole refine_train_step, positions fixed
against positions learnable.

    python tools/refine_positions_bench.py [--out profiles/refine_positions.json] [--fixed-only]

BASELINE config 5's shapes (bench.py's c5_refine recipe): 512 x 512, 500 000 points on a noisy sphere shell, 8 points per
pixel, 19 feature channels, radius 2 px, the stand-in guidance at its full size.
1. mi3d.refine.render_point forward + backward (a random upstream gradient, the features requiring grad as in training)
   with the positions a plain tensor and with the positions requiring grad, alternating in one process, each timed with
   HIP events; medians, spreads and the ratio.
2. mi3d.refine.refine_train_step (novel view, SDS branch) with the points a plain tensor and with the points an
   nn.Parameter of the optimiser plus `points_origin`, alternating, host clock around a synchronised step.
The fixed-positions figures are the check that the default path did not move: compare them with this tool's figures on
the commit before the position gradient, on the same machine - `--fixed-only` measures just those (there the learnable
variants raise).  An existing `parity` entry of the output file (the figures tests/test_raster_positions_gpu.py records) is
kept.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

H = W = 512
POINTS, PPP, CHANNELS, RADIUS_PX, T_FIXED = 500_000, 8, 19, 2.0, 500
FOCAL = 1.0 / (2 * np.tan(np.radians(20) / 2))
RADIUS = RADIUS_PX / H * 2.0


def cloud(dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    d = torch.randn(POINTS, 3, device=dev, generator=gen)
    return (d / d.norm(dim=-1, keepdim=True) * 0.35 * (1 + 0.05 * torch.randn(POINTS, 1, device=dev, generator=gen))
            ).contiguous()


def summary(times, names):
    out = {}
    for n in names:
        out[f"{n}_ms"] = statistics.median(times[n])
        out[f"{n}_ms_min_max"] = [min(times[n]), max(times[n])]
    if len(names) == 2:
        out[f"ratio_{names[1]}_over_{names[0]}"] = out[f"{names[1]}_ms"] / out[f"{names[0]}_ms"]
    return out


def time_render_point(dev, w2c, variants, warmup, runs):
    from mi3d import refine
    Kmat = refine.intrinsics(FOCAL, H, W, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    feats = torch.rand(POINTS, CHANNELS, device=dev, generator=gen).requires_grad_(True)
    gout = torch.randn(1, CHANNELS, H, W, device=dev, generator=gen)
    pts = {"fixed": cloud(dev, 0), "learnable": cloud(dev, 0).requires_grad_(True)}
    times = {n: [] for n in variants}
    for i in range(warmup + runs):
        for n in variants:
            feats.grad = pts[n].grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            refine.render_point(pts[n], feats, H, W, Kmat, w2c, (H, W), RADIUS, PPP).backward(gout)
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[n].append(e0.elapsed_time(e1))
    assert pts["fixed"].grad is None and ("learnable" not in variants or float(pts["learnable"].grad.abs().max()) > 0)
    return {"what": "render_point forward + backward, HIP events", "runs_each": runs, "warmup_each": warmup,
            **summary(times, variants)}


def time_train_step(dev, w2c, variants, warmup, runs):
    from mi3d import refine, sd_standin
    guidance = sd_standin.StableDiffusionStandIn(dev)
    text_z = guidance.get_text_embeds()
    states = {}
    for n in variants:
        torch.manual_seed(0)
        start = cloud(dev, 0)
        points = torch.nn.Parameter(start.clone()) if n == "learnable" else start
        colour = torch.nn.Parameter(torch.rand(POINTS, 3, device=dev))
        feat = torch.nn.Parameter(torch.randn(POINTS, 16, device=dev))
        unet = refine.UNet(num_input_channels=CHANNELS).to(dev).train()
        groups = [{"params": [colour, feat], "lr": 1e-3}, {"params": unet.parameters(), "lr": 1e-3}]
        if n == "learnable":
            groups.append({"params": [points], "lr": 1e-5})
        optimizer = torch.optim.Adam(groups, betas=(0.9, 0.99), eps=1e-15)
        kw = dict(points_origin=start, lambda_points=1e3) if n == "learnable" else {}
        states[n] = ((unet, {"colour": colour, "feat": feat}, optimizer, guidance, text_z, points, w2c, FOCAL, H, W,
                      RADIUS, PPP, colour.detach().clone()), kw)
    times = {n: [] for n in variants}
    for i in range(warmup + runs):
        for n in variants:
            args, kw = states[n]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = refine.refine_train_step(*args, guidance_scale=5.0, t=T_FIXED, **kw)
            torch.cuda.synchronize()
            if i >= warmup:
                times[n].append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(loss)
    return {"what": "refine_train_step, novel view, t = 500 (SDS branch), host clock around a synchronised step",
            "runs_each": runs, "warmup_each": warmup, **summary(times, variants)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_positions.json"))
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fixed-only", action="store_true", help="only the fixed-positions figures (any commit)")
    a = ap.parse_args()
    if a.runs < 9:
        raise SystemExit("--runs: the medians are over >= 9 runs each")
    if not torch.cuda.is_available():
        raise SystemExit("refine_positions_bench needs a GPU")
    from mi3d import rays as R
    dev = torch.device("cuda:0")
    variants = ("fixed",) if a.fixed_only else ("fixed", "learnable")
    w2c = torch.linalg.inv(R.orbit_pose(1.25, 80.0, 30.0, device=dev)[0])
    out = {"device": torch.cuda.get_device_name(0),
           "shapes": {"H": H, "W": W, "points": POINTS, "points_per_pixel": PPP, "channels": CHANNELS,
                      "radius_px": RADIUS_PX},
           "render_point": time_render_point(dev, w2c, variants, a.warmup, a.runs)}
    torch.cuda.empty_cache()
    out["refine_train_step"] = time_train_step(dev, w2c, variants, a.warmup, a.runs)
    if os.path.exists(a.out):
        with open(a.out) as f:
            kept = json.load(f)
        out.update({k: kept[k] for k in ("parity", "parent_commit_fixed_only") if k in kept})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
