"""What the fused MLP's second-order pass costs, and what a trainable analytic normal costs with it.

    python tools/mlp_second_order_bench.py [--out profiles/mlp_second_order.json]

Two measurements at 2^20 and 2^22 rows, fp32, HIP events, alternating in one process after a warm-up; medians with min and
max; nothing is gated.

kernels   the product's MLP 32 -> 64 -> 64 -> 4 (seeded nn.Linear initialisation) on random rows: mi3d_mlp_forward,
          mi3d_mlp_backward (dx + all six parameter gradients - unchanged here: the yardstick), and
          mi3d_mlp_backward_backward with both outputs, with grad_dout alone and with the weight gradients alone.
chains    the default field (table U(-0.3, 0.3)) at points uniform in the box, a scalar loss <normal, a> and .backward() into
          the table and the MLP's weights: the trainable ANALYTIC normal - analytic_normal(x, create_graph=True), one
          evaluation per point and the second-order passes of grid and MLP - against the trainable FINITE-DIFFERENCE normal -
          normal(x), the 7-point stencil.  Both are the pointwise routes; neither is the training step.

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]
import torch  # noqa: E402

DIMS = (32, 64, 4)


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread": (max(ms) - min(ms)) / statistics.median(ms)}


def _alternate(launches, warmup, runs):
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
    return {k: _stats(v) for k, v in times.items()}


def measure_kernels(n, warmup, runs, dev):
    from mi3d import _lib as L
    torch.manual_seed(0)
    lin = [torch.nn.Linear(32, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 4)]
    ws = [t.detach().to(dev).contiguous() for l in lin for t in (l.weight, l.bias)]
    gen = torch.Generator(device=dev).manual_seed(n)
    x = 0.5 * torch.randn(n, 32, device=dev, generator=gen)
    dout, r = torch.randn(n, 4, device=dev, generator=gen), torch.randn(n, 32, device=dev, generator=gen)
    y, dx, gd = torch.empty(n, 4, device=dev), torch.empty(n, 32, device=dev), torch.empty(n, 4, device=dev)
    grads = [torch.zeros_like(t) for t in ws]
    gW = [torch.zeros_like(ws[i]) for i in (0, 2, 4)]
    p = L.ptr
    wp = [p(t) for t in ws]

    def bwd2(rows, weights):
        return lambda: L.launch("mi3d_mlp_backward_backward", x, p(x), p(dout), p(r), n, *wp, *DIMS, p(gd) if rows else None,
                                *[p(g) if weights else None for g in gW])
    res = _alternate({
        "mlp_forward": lambda: L.launch("mi3d_mlp_forward", x, p(x), 0, 0, n, *wp, *DIMS, 0, p(y)),
        "mlp_backward": lambda: L.launch("mi3d_mlp_backward", x, p(x), 0, 0, p(dout), n, *wp, *DIMS, 0, p(dx), 0,
                                         *[p(g) for g in grads]),
        "mlp_backward_backward": bwd2(True, True),
        "mlp_backward_backward_rows_only": bwd2(True, False),
        "mlp_backward_backward_weights_only": bwd2(False, True),
    }, warmup, runs)
    med = lambda k: res[k]["median_ms"]      # noqa: E731
    res["ratio_second_order_over_backward"] = med("mlp_backward_backward") / med("mlp_backward")
    res["ratio_second_order_over_forward"] = med("mlp_backward_backward") / med("mlp_forward")
    assert bool(torch.isfinite(gd).all()) and all(bool(torch.isfinite(g).all()) for g in gW)
    return res


def measure_chains(model, n, warmup, runs, dev):
    gen = torch.Generator(device=dev).manual_seed(n + 1)
    x = torch.rand(n, 3, device=dev, generator=gen) * 2 - 1
    a = torch.randn(n, 3, device=dev, generator=gen)

    def analytic():
        model.zero_grad(set_to_none=True)
        (model.analytic_normal(x, create_graph=True) * a).sum().backward()

    def stencil():
        model.zero_grad(set_to_none=True)
        (model.normal(x) * a).sum().backward()
    res = _alternate({"analytic_normal_trainable": analytic, "finite_difference_normal_trainable": stencil}, warmup, runs)
    res["ratio_analytic_over_stencil"] = (res["analytic_normal_trainable"]["median_ms"] /
                                          res["finite_difference_normal_trainable"]["median_ms"])
    analytic()
    assert all(bool(torch.isfinite(t.grad).all()) for t in [model.encoder.params] + [l.weight for l in model.sigma_net.net])
    model.zero_grad(set_to_none=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_second_order.json"))
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 22])
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("--runs: the medians are over >= 20 runs each")
    if not torch.cuda.is_available():
        raise SystemExit("mlp_second_order_bench needs a GPU")
    from mi3d import network, sds_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = network.NeRFNetwork(sds_step.make_opt(fp16=False)).to(dev)
    with torch.no_grad():
        model.encoder.params.uniform_(-0.3, 0.3)
    out = {"device": torch.cuda.get_device_name(0), "runs_each": a.runs, "warmup_each": a.warmup,
           "kernels_setup": "32 -> 64 -> 64 -> 4, seeded nn.Linear initialisation, x ~ 0.5 N(0,1), dout and r ~ N(0,1), fp32 "
                            "rows; mlp_backward is the unchanged first-order launch, timed in this process as the yardstick",
           "chains_setup": "default grid, table U(-0.3, 0.3), seeded default MLP, points uniform in the box, loss <normal, a>, "
                           ".backward() into table and weights; analytic_normal(create_graph=True) against normal() over the "
                           "7-point stencil; pointwise routes, not the training step",
           "kernels": {str(n): measure_kernels(n, a.warmup, a.runs, dev) for n in a.rows},
           "chains": {str(n): measure_chains(model, n, a.warmup, a.runs, dev) for n in a.rows}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
