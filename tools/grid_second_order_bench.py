"""What the hash grid's second-order pass costs, beside the launches it would replace.

    python tools/grid_second_order_bench.py [--out profiles/grid_second_order.json]

The default grid (16 levels, 2^19 entries per hashed level, base 16 up to 2048), table U(-0.3, 0.3), at 2^20 and 2^22
points uniform in [0, 1]^3, with dense random dout and r.  Timed with HIP events, alternating in one process, after a
warm-up: mi3d_hashgrid_forward, mi3d_hashgrid_backward_input, mi3d_hashgrid_backward, and the two kernels of
mi3d_hashgrid_backward_input_backward - the rows kernel (grad_dout and grad_x asked for) and the table kernel (grad_params
alone).  Beside them the finite-difference route's grid work at the same n: mi3d_grid_encode_points and
mi3d_grid_scatter_points over the 7-point stencil (centre and +-eps per axis) of the same points in [-1, 1]^3.

    ratio = (forward + backward_input + rows + table at one point) / (encode_points + scatter_points at 7 points)

is the figure that says whether a trainable analytic normal - one evaluation plus the second-order pass - is worth wiring
into the fused field; it covers the GRID only: the MLP between grid and density has no second-order pass yet.  Medians over
the runs, with min and max; nothing is gated.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]
import torch  # noqa: E402

CFG = dict(n_levels=16, base_resolution=16, log2_hashmap_size=19)


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread": (max(ms) - min(ms)) / statistics.median(ms)}


def measure(n, warmup, runs, dev):
    import numpy as np
    import tinycudann as tcnn
    from mi3d import _lib as L
    from mi3d import grid_ops
    scale = float(np.float32(np.exp2(np.log2(2048 / 16) / 15)))
    grid = (CFG["n_levels"], CFG["base_resolution"], scale, CFG["log2_hashmap_size"])
    total = tcnn.grid_levels(*grid)[0]
    F = 2 * CFG["n_levels"]
    gen = torch.Generator(device=dev).manual_seed(n)
    table = (torch.rand(total * 2, device=dev, generator=gen) * 2 - 1) * 0.3
    x01 = torch.rand(n, 3, device=dev, generator=gen)
    xw = (x01 * 2 - 1).contiguous()
    dout, r = torch.randn(n, F, device=dev, generator=gen), torch.randn(n, 3, device=dev, generator=gen)
    out, gd, gx = torch.empty(n, F, device=dev), torch.empty(n, F, device=dev), torch.empty(n, 3, device=dev)
    gp = torch.zeros(total * 2, device=dev)
    offs, P0 = grid_ops.stencil_offsets(center=True, second=False)
    P = offs.shape[0]
    offs_p = offs.ctypes.data_as(C.c_void_p)
    out7 = torch.empty(P * n, F, device=dev)
    dout7 = torch.randn(P * n, F, device=dev, generator=gen)
    p = L.ptr
    launches = {
        "hashgrid_forward": lambda: L.launch("mi3d_hashgrid_forward", x01, p(x01), n, p(table), *grid, p(out)),
        "hashgrid_backward_input": lambda: L.launch("mi3d_hashgrid_backward_input", x01, p(x01), n, p(dout), p(table), *grid,
                                                    p(gx)),
        "hashgrid_backward": lambda: L.launch("mi3d_hashgrid_backward", x01, p(x01), n, p(dout), *grid, p(gp)),
        "second_order_rows": lambda: L.launch("mi3d_hashgrid_backward_input_backward", x01, p(x01), n, p(dout), p(table), p(r),
                                              *grid, p(gd), p(gx), None),
        "second_order_table": lambda: L.launch("mi3d_hashgrid_backward_input_backward", x01, p(x01), n, p(dout), p(table), p(r),
                                               *grid, None, None, p(gp)),
        "encode_points_7": lambda: L.launch("mi3d_grid_encode_points", xw, p(xw), None, n, None, offs_p, int(P0), P, 1.0,
                                            p(table), *grid, p(out7)),
        "scatter_points_7": lambda: L.launch("mi3d_grid_scatter_points", xw, p(xw), None, n, None, offs_p, int(P0), P, 1.0,
                                             p(dout7), *grid, 0.0, p(gp)),
    }
    times = {k: [] for k in launches}
    for i in range(warmup + runs):
        for name, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    res = {k: _stats(v) for k, v in times.items()}
    med = lambda k: res[k]["median_ms"]      # noqa: E731
    analytic = med("hashgrid_forward") + med("hashgrid_backward_input") + med("second_order_rows") + med("second_order_table")
    stencil = med("encode_points_7") + med("scatter_points_7")
    res["analytic_route_ms"] = analytic
    res["stencil_route_ms"] = stencil
    res["ratio_analytic_over_stencil"] = analytic / stencil
    assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gx).all())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_second_order.json"))
    ap.add_argument("--points", type=int, nargs="+", default=[1 << 20, 1 << 22])
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("--runs: the medians are over >= 20 runs each")
    if not torch.cuda.is_available():
        raise SystemExit("grid_second_order_bench needs a GPU")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "runs_each": a.runs, "warmup_each": a.warmup,
           "grid": "default16 (16 levels, base 16 -> 2048, 2^19 entries per hashed level), table U(-0.3, 0.3), dense random "
                   "dout and r, points uniform in the box",
           "ratio": "(forward + backward_input + second_order_rows + second_order_table at 1 point) / (encode_points + "
                    "scatter_points at the 7-point stencil); grid work only, the MLP has no second-order pass yet",
           "points": {str(n): measure(n, a.warmup, a.runs, dev) for n in a.points}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
