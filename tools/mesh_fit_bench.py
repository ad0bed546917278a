"""The gradients of the mesh render's colour sources (mi3d.mesh.fit_texture, csrc/meshrender.hip, include/mi3d.h Part 18) on
the workload of tools/mesh_render_bench.py, and the fidelity report of an export with and without the fit.
    python tools/mesh_fit_bench.py [--out profiles/mesh_fit.json] [--resolution 256] [--views 32] [--side 800]
                                   [--texture-size 4096] [--export-resolution 128] [--export-texture-size 2048]
The radius-0.6 sphere at 256^3, 32 views of 800 x 800 on four rings around it, the atlas at 4096^2.
  shade_texture_u8 / shade_texture_f32  mi3d_mesh_shade and mi3d_mesh_shade_f32, the image alone: the same kernel template
  backward_texture / backward_colors    mi3d_mesh_shade_backward, the whole call: the fill, k_grad_amax, k_shade_backward,
                                        k_grad_finish; dimage is standard normal
  backward_*_launches                   the three launches one at a time (the fill counts with the first), in their order, from
                                        the development build (tools/build_dev.py: tunable 19 selects the launches); NOT
                                        MEASURED without tools/bin/libmi3d_dev.so
  atomics_per_s_in_k_shade_backward     what launch 2 sends at the most - drawn pixels x (4 taps or 3 vertices) x 3 channels; a
                                        contribution that rounds to zero is not sent - per second of launch 2, and x 8 bytes
  fit_iteration                         one iteration of mesh.fit_texture (shade, loss, backward, Adam, clamp) against renders
                                        of the analytic colour: (a run of 12 iterations - a run of 2) / 10, wall clock
HIP events on the current stream, 2 warm-ups, 7 repetitions: median, minimum and maximum.
`fidelity`: tools/mesh_render_bench.py's export of the random-weight field (a noise field, NOT a trained object) with
preview=dict(8 views of 256 x 256, fidelity=True): plain, views= (the field's own renders from 8 OTHER cameras), and
views= + fit; each entry is that export's preview.json.  Measurements; no test asserts them."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mesh_render_bench import QUANTILES  # noqa: E402
from texture_views_bench import FOCAL, R0, cameras, colour_at, timed  # noqa: E402

DEV_LIB = os.path.join(ROOT, "tools", "bin", "libmi3d_dev.so")
LAUNCHES = {1: "fill_and_k_grad_amax", 2: "k_shade_backward", 4: "k_grad_finish"}


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "repeats": len(ts)}


def launches(args, stream, warmup=2, repeats=7):
    """The three launches of one backward, each between its own pair of events, from the development build."""
    from mi3d import _lib
    if not os.path.exists(DEV_LIB):
        return {"error": f"NOT MEASURED: {os.path.relpath(DEV_LIB, ROOT)} is not built (python tools/build_dev.py)"}
    dl = C.CDLL(DEV_LIB)
    fn = dl.mi3d_mesh_shade_backward
    fn.argtypes, fn.restype = _lib._SIGNATURES["mi3d_mesh_shade_backward"], C.c_int
    ts = {m: [] for m in LAUNCHES}
    try:
        for rep in range(warmup + repeats):
            for mask in LAUNCHES:
                dl.mi3d_dev_set(19, mask)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                err = fn(*args, stream)
                b.record()
                b.synchronize()
                if err != 0:
                    return {"error": f"NOT MEASURED: hipError {err}"}
                if rep >= warmup:
                    ts[mask].append(a.elapsed_time(b))
    finally:
        dl.mi3d_dev_set(19, -1)
    return {LAUNCHES[m]: summary(ts[m]) for m in LAUNCHES}


def kernels(a, dev):
    from mi3d import _lib, mesh
    R, V, S, T, p = a.resolution, a.views, a.side, a.texture_size, _lib.ptr
    ax = torch.linspace(-1, 1, R, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    h = 2.0 / (R - 1)
    verts, tris = mesh.marching_cubes((R0 - torch.sqrt(x * x + y * y + z * z)).float(), 0.0, (-1.0,) * 3, (h,) * 3)
    del x, y, z
    nv, nt = verts.shape[0], tris.shape[0]
    K = np.array([[FOCAL * S, 0, 0.5 * S], [0, FOCAL * S, 0.5 * S], [0, 0, 1]])
    c2w = cameras(V)
    rec = torch.from_numpy(mesh.view_records(c2w, K)).to(dev)
    keys, _ = mesh._visibility(verts, tris, rec, S, S)
    n = V * S * S
    drawn = int((keys != -1).sum())
    res = {"resolution": R, "nv": nv, "nt": nt, "views": V, "view_side": S, "texture_size": T, "pixels": n, "pixels_drawn": drawn}
    vt = torch.empty(3 * nt, 2, device=dev)
    _lib.launch("mi3d_atlas_uv", vt, nt, T, p(vt))
    image = torch.empty(V, S, S, 3, device=dev)
    bg = (C.c_float * 3)(1.0, 1.0, 1.0)
    for name, entry, texture in (("shade_texture_u8", "mi3d_mesh_shade", torch.randint(0, 256, (T, T, 3), dtype=torch.uint8, device=dev)),
                                 ("shade_texture_f32", "mi3d_mesh_shade_f32", torch.rand(T, T, 3, device=dev))):
        res[name] = timed(lambda: _lib.launch(entry, verts, p(verts), nv, p(tris), nt, p(rec), V, S, S, p(keys), None, p(vt),
                                              p(texture), T, None, bg, p(image), None, None, None, None, None))
        res[name]["bytes"] = n * (8 + 12)
        res[name]["GB_per_s"] = res[name]["bytes"] / (res[name]["ms_median"] * 1e-3) / 1e9
        del texture
    dimage = torch.randn(V, S, S, 3, device=dev)
    for name, shape, uv in (("backward_texture", (T, T, 3), vt), ("backward_colors", (nv, 3), None)):
        grad = torch.empty(shape, device=dev)
        ws_bytes = int(_lib.lib().mi3d_mesh_shade_backward_workspace(grad.numel()))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        args = (p(verts), nv, p(tris), nt, p(rec), V, S, S, p(keys), p(dimage), p(uv), T if uv is not None else 0,
                p(grad if uv is None else None), p(grad if uv is not None else None), p(ws), ws_bytes)
        res[name] = timed(lambda: _lib.launch("mi3d_mesh_shade_backward", verts, *args))
        res[name].update(elements=grad.numel(), workspace_bytes=ws_bytes,
                         contributions_at_most=drawn * (12 if uv is not None else 9), elements_touched=int((grad != 0).sum()))
        with torch.cuda.device(dev):
            res[name + "_launches"] = launches(args, _lib.stream(verts))
        k2 = res[name + "_launches"].get("k_shade_backward")
        if k2:
            res[name]["atomics_per_s_in_k_shade_backward"] = res[name]["contributions_at_most"] / (k2["ms_median"] * 1e-3)
            res[name]["atomic_GB_per_s_in_k_shade_backward"] = 8 * res[name]["atomics_per_s_in_k_shade_backward"] / 1e9
        del grad, ws
    del dimage, image
    target, _ = mesh.render(verts, tris, c2w, K, S, S, colors=colour_at(verts).float().contiguous())
    start = torch.full((T, T, 3), 0.5, device=dev)
    wall = {}
    for its in (2, 12, 2, 12):                                  # the first pair warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh.fit_texture(verts, tris, vt, start, target, c2w, K, iterations=its, lr=0.01)
        torch.cuda.synchronize()
        wall[its] = time.perf_counter() - t0
    res["fit_iteration"] = {"ms": (wall[12] - wall[2]) / 10 * 1e3, "wall_s_2_iterations": wall[2], "wall_s_12_iterations": wall[12]}
    return res


def fidelity(a, dev):
    from mi3d import mesh, sds_step
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    model, _, _ = sds_step.build_training_state(opt, dev, bitfield=0.5)
    with torch.no_grad():
        model.encoder.params.uniform_(-0.3, 0.3)
    model.eval()
    R, T, S = a.export_resolution, a.export_texture_size, 256
    vol = mesh.extract_volume(model, R)
    for q in QUANTILES:
        iso = float(torch.quantile(vol.flatten()[:: max(1, vol.numel() // (1 << 22))], q))
        nt = mesh.marching_cubes(vol, iso)[1].shape[0]
        if nt and mesh.atlas_cell(nt, T) > 0:
            break
    else:
        return {"error": f"NOT MEASURED: no quantile of {QUANTILES} gives a surface that fits a {T}^2 atlas ({nt} triangles)"}
    K = np.array([[FOCAL * S, 0, 0.5 * S], [0, FOCAL * S, 0.5 * S], [0, 0, 1]])
    preview = dict(c2w=cameras(8, 3.2), K=K, H=S, W=S, fidelity=True)          # outside the box: its half-diagonal is 1.74
    src = np.concatenate([cameras(12, 3.2)[1::2], cameras(8, 3.0)[:2]])       # 8 other cameras
    model.mean_density, model.density_thresh = iso, max(model.density_thresh, iso)
    images, _ = mesh.render_field(model, src, K, S, S)
    views = dict(images=images.clamp(0, 1), c2w=src, K=K)
    fit = dict(iterations=a.fit_iterations, lr=a.fit_lr)
    res = {"resolution": R, "texture_size": T, "quantile": q, "threshold": iso, "triangles_extracted": nt,
           "preview": "8 views of 256 x 256 at distance 3.2", "field": "random-weight (not trained)", "fit": fit}
    for name, kw in (("plain", {}), ("views", dict(views=views)), ("views+fit", dict(views=dict(views, fit=fit)))):
        try:
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = model.export_mesh(tmp, resolution=R, texture_size=T, preview=preview, **kw)
                torch.cuda.synchronize()
                r = json.load(open(os.path.join(tmp, "preview.json")))
                res[name] = {"nv": len(o[0]), "nt": len(o[1]), "psnr_union": r["psnr_union"],
                             "psnr_intersection": r["psnr_intersection"], "iou": r["iou"],
                             "views_psnr_intersection": [x["psnr_intersection"] for x in r["views"]],
                             "export_wall_s": time.perf_counter() - t0}
        except Exception as ex:  # noqa: BLE001  the other rows are kept
            res[name] = {"error": f"NOT MEASURED: {type(ex).__name__}: {ex}"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_fit.json")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--texture-size", type=int, default=4096)
    ap.add_argument("--export-resolution", type=int, default=128)
    ap.add_argument("--export-texture-size", type=int, default=2048)
    ap.add_argument("--fit-iterations", type=int, default=200)
    ap.add_argument("--fit-lr", type=float, default=0.01)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "command": "python tools/mesh_fit_bench.py " + " ".join(sys.argv[1:]),
           "protocol": "HIP events, 2 warm-ups, 7 repetitions; median, min, max"}
    res["kernels"] = kernels(a, dev)
    try:
        res["fidelity"] = fidelity(a, dev)
    except Exception as ex:  # noqa: BLE001  the kernel times above are kept
        res["fidelity"] = {"error": f"NOT MEASURED: {type(ex).__name__}: {ex}"}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
