"""The rasteriser of the exported mesh (mi3d.mesh.render, csrc/meshrender.hip, include/mi3d.h Part 17) on the inputs of
tools/texture_views_bench.py, and the fidelity report of one export.
    python tools/mesh_render_bench.py [--out profiles/mesh_render.json] [--resolution 256] [--views 32] [--side 800]
                                      [--texture-size 4096] [--export-resolution 128] [--export-texture-size 2048]
The radius-0.6 sphere at 256^3, 32 views of 800 x 800 on four rings around it (that tool's `cameras`), and its close view:
ONE view from 0.75, 0.15 above the surface, where a triangle covers thousands of pixels and one thread walks them all.
  depth / depth_close_view            mi3d_mesh_depth: the fill and the rasterisation (what the visibility pass is read against)
  visibility / visibility_close_view  mi3d_mesh_visibility on the same inputs: the same walk, a 64-bit atomicMin per covered pixel
  ratio_visibility_over_depth         from the medians of this run, for both camera sets; no threshold is set on it
  shade_colors                        mi3d_mesh_shade from vertex colours, every optional output written
  shade_texture                       mi3d_mesh_shade from the atlas (mi3d_atlas_uv) and a T^2 texture, the image alone
HIP events on the current stream, 2 warm-ups, 7 repetitions: median, minimum and maximum.  `bytes` = what a pass must move at
the least (the buffers it writes and the visibility keys it reads; vertices, triangles and taps come through the caches).
`fidelity`: NeRFRenderer.export_mesh(resolution 128, texture_size 2048, preview=dict(8 views of 256 x 256, fidelity=True)) of
the random-weight field of __graft_entry__.smoke() at the lowest of a few density quantiles whose surface fits the atlas -
a noise field, NOT a trained object - plain and with decimate=2, smooth=10, views= (the field's own renders from 8 other
cameras) and all three; each entry is that export's preview.json.  Measurements; no test asserts them."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from texture_views_bench import FOCAL, R0, cameras, colour_at, timed  # noqa: E402

QUANTILES = (0.9, 0.95, 0.98, 0.99, 0.995, 0.999)


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
    orbit = torch.from_numpy(mesh.view_records(cameras(V), K)).to(dev)
    close = torch.from_numpy(mesh.view_records(cameras(4, 0.75)[:1], K)).to(dev)
    res = {"resolution": R, "nv": nv, "nt": nt, "views": V, "view_side": S, "texture_size": T}
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    for name, rec in (("", orbit), ("_close_view", close)):
        n = rec.shape[0]
        depth = torch.empty(n, S, S, device=dev)
        vis = torch.empty(n, S, S, dtype=torch.int64, device=dev)
        d = timed(lambda: _lib.launch("mi3d_mesh_depth", verts, p(verts), nv, p(tris), nt, p(rec), n, S, S, p(depth), p(counts)))
        d.update(counts_bad_skipped=counts.tolist(), pixels_drawn_share=float(torch.isfinite(depth).float().mean()),
                 bytes=4 * n * S * S + 12 * nv + 12 * nt)
        v = timed(lambda: _lib.launch("mi3d_mesh_visibility", verts, p(verts), nv, p(tris), nt, p(rec), n, S, S, p(vis),
                                      p(counts)))
        v.update(counts_bad_skipped=counts.tolist(), pixels_drawn_share=float((vis != -1).float().mean()),
                 bytes=8 * n * S * S + 12 * nv + 12 * nt,
                 upper_words_equal_depth=bool(torch.equal((vis >> 32).to(torch.int32)[vis != -1],
                                                          depth.view(torch.int32)[vis != -1])))
        res["depth" + name], res["visibility" + name] = d, v
        res["ratio_visibility_over_depth" + name] = v["ms_median"] / d["ms_median"]
        del depth
        if not name:
            keys = vis                                              # the orbit views' buffer: what the shading reads
    n = V * S * S
    colors, vn = colour_at(verts).float().contiguous(), (verts / R0).contiguous()
    out = {k: torch.empty(V, S, S, 3, device=dev) for k in ("image", "normal", "bary")}
    out.update(depth=torch.empty(V, S, S, device=dev), tri=torch.empty(V, S, S, dtype=torch.int32, device=dev),
               alpha=torch.empty(V, S, S, dtype=torch.uint8, device=dev))
    bg = (_lib.C.c_float * 3)(1.0, 1.0, 1.0)
    res["shade_colors"] = timed(lambda: _lib.launch(
        "mi3d_mesh_shade", verts, p(verts), nv, p(tris), nt, p(orbit), V, S, S, p(keys), p(colors), None, None, 0, p(vn), bg,
        p(out["image"]), p(out["normal"]), p(out["depth"]), p(out["tri"]), p(out["bary"]), p(out["alpha"])))
    res["shade_colors"]["bytes"] = n * (8 + 12 * 3 + 4 + 4 + 1)
    vt = torch.empty(3 * nt, 2, device=dev)
    _lib.launch("mi3d_atlas_uv", vt, nt, T, p(vt))
    texture = torch.randint(0, 256, (T, T, 3), dtype=torch.uint8, device=dev)
    res["shade_texture"] = timed(lambda: _lib.launch(
        "mi3d_mesh_shade", verts, p(verts), nv, p(tris), nt, p(orbit), V, S, S, p(keys), None, p(vt), p(texture), T, None, bg,
        p(out["image"]), None, None, None, None, None))
    res["shade_texture"]["bytes"] = n * (8 + 12)
    for k in ("shade_colors", "shade_texture"):
        res[k]["GB_per_s"] = res[k]["bytes"] / (res[k]["ms_median"] * 1e-3) / 1e9
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
    res = {"resolution": R, "texture_size": T, "quantile": q, "threshold": iso, "triangles_extracted": nt,
           "preview": "8 views of 256 x 256 at distance 3.2", "field": "random-weight (not trained)"}
    for name, kw in (("plain", {}), ("decimate=2", dict(decimate=2)), ("smooth=10", dict(smooth=10)),
                     ("views", dict(views=views)), ("decimate=2,smooth=10,views", dict(decimate=2, smooth=10, views=views))):
        try:
            with tempfile.TemporaryDirectory() as tmp:
                o = model.export_mesh(tmp, resolution=R, texture_size=T, preview=preview, **kw)
                r = json.load(open(os.path.join(tmp, "preview.json")))
                res[name] = {"nv": len(o[0]), "nt": len(o[1]), "psnr_union": r["psnr_union"],
                             "psnr_intersection": r["psnr_intersection"], "iou": r["iou"],
                             "views_psnr_intersection": [x["psnr_intersection"] for x in r["views"]]}
        except Exception as ex:  # noqa: BLE001  the other rows are kept
            res[name] = {"error": f"NOT MEASURED: {type(ex).__name__}: {ex}"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_render.json")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--texture-size", type=int, default=4096)
    ap.add_argument("--export-resolution", type=int, default=128)
    ap.add_argument("--export-texture-size", type=int, default=2048)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "command": "python tools/mesh_render_bench.py " + " ".join(sys.argv[1:]),
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
