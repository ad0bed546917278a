"""The simplifier of mesh export (mi3d.mesh.simplify, csrc/meshsimplify.hip, include/mi3d.h Part 14) on the two surfaces of
256^3 the other mesh tools use.
    python tools/mesh_simplify_bench.py [--out profiles/mesh_simplify.json]
  field_256    the volume tools/mesh_bench.py uses (the random-weight field of __graft_entry__.smoke(), threshold = the
               volume's median): a noise surface through nearly every cell - the worst case for the triangle count
  sphere_256   the radius-0.6 sphere: what an object looks like
Per surface and d = 2, 4 (the cluster cell in grid steps, on export_mesh's lattice): `count` (the launches of
mi3d_mesh_simplify_count, without the host read that follows them) and `emit` (mi3d_mesh_simplify_emit) by HIP events on
the current stream, 2 warm-ups, 7 repetitions, median, minimum and maximum; the counts of Part 14; the atlas cell c of
Part 9 at T = 2048 and 4096 before and after (0: does not fit); `atomics_per_s` = the 4 nv 64-bit adds of the accumulate
pass alone over the whole count phase's time, a lower bound of their rate.  `export_mesh` = one wall-clock run of
NeRFRenderer.export_mesh at 256 on that volume without and with decimate=2 (files to a temporary directory)."""
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

DS = (2, 4)
TEXTURES = (2048, 4096)


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
    import ctypes as C
    from mi3d import _lib, mesh
    R = vol.shape[0]
    h = 2.0 / (R - 1)
    verts, tris = mesh.marching_cubes(vol, iso, (-1.0,) * 3, (h,) * 3)
    nv, nt, p = verts.shape[0], tris.shape[0], _lib.ptr
    res = {"resolution": R, "nv": nv, "nt": nt, "atlas_cell": {str(T): mesh.atlas_cell(nt, T) for T in TEXTURES}}
    ws_bytes = int(_lib.lib().mi3d_mesh_simplify_workspace(nv, nt, 0))
    res["workspace_bytes"] = ws_bytes
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    lost = torch.empty(1, dtype=torch.int64, device=dev)
    vmap = torch.empty(nv, dtype=torch.int32, device=dev)
    for d in DS:
        origin, cell = mesh.export_lattice(R, d)
        org = (C.c_float * 3)(*origin)
        count = lambda: _lib.launch("mi3d_mesh_simplify_count", verts, p(verts), nv, p(tris), nt, org, cell, p(ws),  # noqa: E731
                                    ws_bytes, p(counts))
        count()
        host = counts.tolist()
        assert host[2] == 0 and host[3] == 0 and host[4] == 0, host
        kv, kt = host[:2]
        out_v, out_t = torch.empty(kv, 3, device=dev), torch.empty(kt, 3, dtype=torch.int32, device=dev)
        emit = lambda: _lib.launch("mi3d_mesh_simplify_emit", verts, p(verts), nv, p(tris), nt, org, cell, p(ws),  # noqa: E731
                                   ws_bytes, p(out_v), kv, p(out_t), kt, p(vmap), p(lost))
        r = {"cell": cell, "counts": dict(zip(mesh.SIMPLIFY_COUNTS, host)), "count": timed(count), "emit": timed(emit),
             "atlas_cell": {str(T): mesh.atlas_cell(kt, T) for T in TEXTURES}}
        r["atomics_per_s"] = 4 * nv / (r["count"]["ms_median"] * 1e-3)
        assert int(lost) == 0
        sv, st, _ = mesh.simplify(verts, tris, cell, origin=origin)
        assert torch.equal(sv, out_v) and torch.equal(st, out_t)
        res[f"d={d}"] = r
    del ws, vmap
    extract, mesh.extract_volume = mesh.extract_volume, lambda m, r: vol     # export_mesh sees this volume
    thresh, model.density_thresh, cuda_ray, model.cuda_ray = model.density_thresh, iso, model.cuda_ray, False
    try:
        res["export_mesh"] = {}
        for name, kw in (("plain", {}), ("decimate=2", {"decimate": 2})):
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = model.export_mesh(tmp, resolution=R, **kw)
                res["export_mesh"][name] = {"s": time.perf_counter() - t0, "nv": len(out[0]), "nt": len(out[1]),
                                            "obj_bytes": os.path.getsize(os.path.join(tmp, "mesh.obj"))}
    except Exception as e:  # noqa: BLE001  the kernel times above are kept
        res["export_mesh"]["error"] = f"NOT MEASURED: {type(e).__name__}: {e}"
    finally:
        mesh.extract_volume, model.density_thresh, model.cuda_ray = extract, thresh, cuda_ray
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_simplify.json")
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
           "export_mesh: one wall-clock run"}
    vol = mesh.extract_volume(model, 256)
    res["field_256"] = measure(model, vol, float(vol.median()), dev)
    del vol
    res["sphere_256"] = measure(model, sphere(256, dev), 0.0, dev)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
