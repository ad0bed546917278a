"""What the analytic density gradient costs: analytic_normal against normal(), and the hash grid's input-gradient kernel
against its forward gather.

    python tools/density_gradient_bench.py [--out profiles/density_gradient.json]

1. A trained-shaped field (the default grid, the table redrawn U(-0.3, 0.3) as bench.py's field is, the seeded default
   MLP) at 2^20 points uniform in [-1, 1]^3: NeRFNetwork.analytic_normal (one forward + one backward per point) and
   NeRFNetwork.normal (the seven-point finite-difference stencil, forward only, under no_grad) alternate in one process,
   host clock around a synchronised call.
2. The same points mapped to [0, 1]: mi3d_hashgrid_backward_input (k_grid_backward_input) and mi3d_hashgrid_forward
   (k_grid_encode) alternate, each timed with HIP events; gather bytes are 8 corners x 8 bytes per (point, level) for both.
Medians over the runs, with min and max.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]
import torch  # noqa: E402


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def time_normals(model, x, warmup, runs):
    def analytic():
        return model.analytic_normal(x)

    def stencil():
        with torch.no_grad():
            return model.normal(x)

    times = {"analytic_normal": [], "normal": []}
    for i in range(warmup + runs):
        for name, fn in (("analytic_normal", analytic), ("normal", stencil)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
            assert out.shape == x.shape
    res = {k: _stats(v) for k, v in times.items()}
    res["ratio_analytic_over_stencil"] = res["analytic_normal"]["median_ms"] / res["normal"]["median_ms"]
    with torch.no_grad():
        cos = (analytic() * stencil()).sum(-1)
    res["cosine_analytic_vs_stencil_median"] = float(cos.median())
    return res


def time_kernels(model, x01, warmup, runs):
    from mi3d import _lib as L
    cfg, table = model.encoder.cfg, model.encoder.params.detach()
    grid = (cfg["n_levels"], cfg["base_resolution"], cfg["per_level_scale"], cfg["log2_hashmap_size"])
    n = x01.shape[0]
    out = torch.empty(n, cfg["n_levels"] * 2, device=x01.device)
    dout = torch.randn(n, cfg["n_levels"] * 2, device=x01.device, generator=torch.Generator(device=x01.device).manual_seed(1))
    gx = torch.empty(n, 3, device=x01.device)
    p = L.ptr

    def forward():
        L.launch("mi3d_hashgrid_forward", x01, p(x01), n, p(table), *grid, p(out))

    def backward_input():
        L.launch("mi3d_hashgrid_backward_input", x01, p(x01), n, p(dout), p(table), *grid, p(gx))

    times = {"hashgrid_forward": [], "hashgrid_backward_input": []}
    for i in range(warmup + runs):
        for name, fn in (("hashgrid_forward", forward), ("hashgrid_backward_input", backward_input)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    res = {k: _stats(v) for k, v in times.items()}
    gather_bytes = n * cfg["n_levels"] * 8 * 8
    res["gather_bytes"] = gather_bytes
    for k in times:
        res[k]["gather_GBps"] = gather_bytes / (res[k]["median_ms"] * 1e-3) / 1e9
    res["ratio_backward_input_over_forward"] = (res["hashgrid_backward_input"]["median_ms"] /
                                                res["hashgrid_forward"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_gradient.json"))
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.runs < 9:
        raise SystemExit("--runs: the medians are over >= 9 runs each")
    if not torch.cuda.is_available():
        raise SystemExit("density_gradient_bench needs a GPU")
    from mi3d import network, sds_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = network.NeRFNetwork(sds_step.make_opt(fp16=False)).to(dev)
    with torch.no_grad():
        model.encoder.params.uniform_(-0.3, 0.3)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(a.points, 3, device=dev, generator=gen) * 2 - 1
    out = {"device": torch.cuda.get_device_name(0), "points": a.points, "runs_each": a.runs, "warmup_each": a.warmup,
           "field": "default grid, table U(-0.3, 0.3), seeded default MLP, fp32",
           "normals": time_normals(model, x, a.warmup, a.runs),
           "kernels": time_kernels(model, ((x + 1) * 0.5).contiguous(), a.warmup, a.runs)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
