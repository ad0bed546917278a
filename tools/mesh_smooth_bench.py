"""The smoother of mesh export (mi3d.mesh.smooth, csrc/meshsmooth.hip, include/mi3d.h Part 16) on the two surfaces of
256^3 the other mesh tools use.
    python tools/mesh_smooth_bench.py [--out profiles/mesh_smooth.json]
  sphere_256   the radius-0.6 sphere: what an object looks like
  field_256    the volume tools/mesh_bench.py uses (the random-weight field of __graft_entry__.smoke(), threshold = the
               volume's median): a noise surface through nearly every cell - the worst case for the triangle count
Per surface, with Taubin's pair and e of extent 1: mi3d_mesh_smooth at 1 and at 11 iterations by HIP events on the
current stream (2 warm-ups, 7 repetitions; median, minimum, maximum), with and without pin_border.  The entry point is
one call, so the two parts are told apart by the two iteration counts: `pass_ms` = (t(11) - t(1)) / 20 from the medians,
`setup_ms` = t(1) - 2 pass_ms (the incidence, the scan, the fill, the flags).  `pass_bytes_per_s`: what a pass must
move at the least - the row (8 bytes per entry), 24 bytes per vertex read and written - over pass_ms.  The counts of
Part 16, and that two runs give the same bytes.  `export_mesh` = one wall-clock run of NeRFRenderer.export_mesh at 256 on
that volume without and with smooth=10 (files to a temporary directory)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]

import torch  # noqa: E402

ITERATIONS = (1, 11)


def timed(fn, warmup=2, repeats=7):
    """Median / min / max of HIP-event times (ms) of fn() on the current stream."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "repeats": repeats}


def sphere(R, dev):
    ax = torch.linspace(-1, 1, R, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (0.6 - torch.sqrt(x * x + y * y + z * z)).float()


def measure(model, vol, iso, dev):
    from mi3d import _lib, mesh
    R = vol.shape[0]
    h = 2.0 / (R - 1)
    verts, tris = mesh.marching_cubes(vol, iso, (-1.0,) * 3, (h,) * 3)
    nv, nt, p = verts.shape[0], tris.shape[0], _lib.ptr
    e = mesh.smooth_fraction_bits(1.0)
    ws_bytes = int(_lib.lib().mi3d_mesh_smooth_workspace(nv, nt))
    res = {"resolution": R, "nv": nv, "nt": nt, "fraction_bits": e, "workspace_bytes": ws_bytes}
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    out = torch.empty_like(verts)
    inf = float("inf")
    for pin in (True, False):
        r = {}
        for its in ITERATIONS:
            run = lambda: _lib.launch("mi3d_mesh_smooth", verts, p(verts), nv, p(tris), nt, its, mesh.SMOOTH_LAMBDA,  # noqa: E731
                                      mesh.SMOOTH_MU, int(pin), inf, e, p(ws), ws_bytes, p(out), p(counts))
            r[f"iterations={its}"] = timed(run)
        host = counts.tolist()
        assert host[6] == 0 and host[7] == 0, host
        r["counts"] = dict(zip(mesh.SMOOTH_COUNTS, host))
        t1, t11 = (r[f"iterations={its}"]["ms_median"] for its in ITERATIONS)
        r["pass_ms"] = (t11 - t1) / (2 * (ITERATIONS[1] - ITERATIONS[0]))
        r["setup_ms"] = t1 - 2 * r["pass_ms"]
        usable = nt - host[0]
        r["pass_bytes_per_s"] = (3 * usable * 8 + nv * 24) / (r["pass_ms"] * 1e-3) if r["pass_ms"] > 0 else None
        again = mesh.smooth(verts, tris, ITERATIONS[1], pin_border=pin, extent=1.0)
        r["two_runs_same_bytes"] = bool(torch.equal(again.view(torch.int32), out.view(torch.int32)))
        res[f"pin_border={pin}"] = r
    del ws
    extract, mesh.extract_volume = mesh.extract_volume, lambda m, r: vol     # export_mesh sees this volume
    thresh, model.density_thresh, cuda_ray, model.cuda_ray = model.density_thresh, iso, model.cuda_ray, False
    try:
        res["export_mesh"] = {}
        for name, kw in (("plain", {}), ("smooth=10", {"smooth": 10})):
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                o = model.export_mesh(tmp, resolution=R, **kw)
                res["export_mesh"][name] = {"s": time.perf_counter() - t0, "nv": len(o[0]), "nt": len(o[1])}
    except Exception as ex:  # noqa: BLE001  the kernel times above are kept
        res["export_mesh"]["error"] = f"NOT MEASURED: {type(ex).__name__}: {ex}"
    finally:
        mesh.extract_volume, model.density_thresh, model.cuda_ray = extract, thresh, cuda_ray
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_smooth.json")
    a = ap.parse_args()
    from mi3d import mesh, sds_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    model, _, _ = sds_step.build_training_state(opt, dev, bitfield=0.5)
    with torch.no_grad():
        model.encoder.params.uniform_(-0.3, 0.3)
    model.eval()
    res = {"device": torch.cuda.get_device_name(dev), "protocol": "HIP events, 2 warm-ups, 7 repetitions; median, min, max; "
           "pass_ms and setup_ms from the medians at 1 and 11 iterations; export_mesh: one wall-clock run"}
    res["sphere_256"] = measure(model, sphere(256, dev), 0.0, dev)
    vol = mesh.extract_volume(model, 256)
    res["field_256"] = measure(model, vol, float(vol.median()), dev)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
