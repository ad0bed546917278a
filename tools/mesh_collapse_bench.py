"""The edge-collapse decimation of mesh export (mi3d.mesh.collapse, csrc/meshcollapse.hip, include/mi3d.h Part 19) on the
two surfaces of 256^3 the other mesh tools use, at a target of 10 % of the faces.
    python tools/mesh_collapse_bench.py [--out profiles/mesh_collapse.json]
  sphere_256   the radius-0.6 sphere: what an object looks like
  field_256    the volume tools/mesh_bench.py uses (the random-weight field of __graft_entry__.smoke(), threshold = the
               volume's median): a noise surface through nearly every cell - the worst case for the triangle count
Per surface, by HIP events on the current stream (2 warm-ups, 7 repetitions; median, minimum, maximum): `begin`
(mi3d_mesh_collapse_begin alone), `begin_and_first_round`, `begin_and_all_rounds` (one call of mi3d_mesh_collapse_rounds
with the rounds a first run needed plus one, no host read in between) and `count_emit`; from the medians
`first_round_ms`, `mean_round_ms` and `total_ms`.  Next to it mi3d_mesh_simplify_count + emit at d = 2 from the same run,
the counts of Part 19, the atlas cell c of Part 9 at T = 2048 and 4096 before and after (0: does not fit), and that two runs
give the same bytes.  `export_mesh` = one wall-clock run of NeRFRenderer.export_mesh at 256 on that volume plain (what the
commit before this feature does), with decimate=2 and with collapse= at the same 10 % (files to a temporary directory).
`fidelity`: the table of tools/mesh_render_bench.py (resolution 128, texture 2048, 8 previews) with `decimate=2` and
`collapse=` at the face count decimate=2 leaves."""
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
from mesh_simplify_bench import sphere, timed  # noqa: E402
from texture_views_bench import FOCAL, cameras  # noqa: E402

TEXTURES = (2048, 4096)
INF = float("inf")


def measure(model, vol, iso, dev, export=True):
    from mi3d import _lib, mesh
    R = vol.shape[0]
    h = 2.0 / (R - 1)
    verts, tris = mesh.marching_cubes(vol, iso, (-1.0,) * 3, (h,) * 3)
    nv, nt, p = verts.shape[0], tris.shape[0], _lib.ptr
    target = nt // 10
    res = {"resolution": R, "nv": nv, "nt": nt, "target_faces": target,
           "atlas_cell_before": {str(T): mesh.atlas_cell(nt, T) for T in TEXTURES}}
    first = mesh.collapse(verts, tris, target, return_stats=True)
    stats = first[3]
    res["stats"] = stats
    res["atlas_cell_after"] = {str(T): mesh.atlas_cell(stats["triangles"], T) for T in TEXTURES}
    again = mesh.collapse(verts, tris, target, rounds_per_read=3)
    res["two_runs_same_bytes"] = bool(torch.equal(again[0].view(torch.int32), first[0].view(torch.int32))
                                      and torch.equal(again[1], first[1]) and torch.equal(again[2], first[2]))
    del again
    rounds = stats["rounds"]
    ws_bytes = int(_lib.lib().mi3d_mesh_collapse_workspace(nv, nt))
    res["workspace_bytes"] = ws_bytes
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)

    def begin():
        _lib.launch("mi3d_mesh_collapse_begin", verts, p(verts), nv, p(tris), nt, p(ws), ws_bytes, p(counts))

    def run(n):
        begin()
        _lib.launch("mi3d_mesh_collapse_rounds", verts, nv, nt, target, INF, n, p(ws), ws_bytes, p(counts))

    out_v, out_t = torch.empty_like(first[0]), torch.empty_like(first[1])
    vm = torch.empty(nv, dtype=torch.int32, device=dev)

    def count_emit():
        _lib.launch("mi3d_mesh_collapse_count", verts, nv, nt, p(ws), ws_bytes, p(counts))
        _lib.launch("mi3d_mesh_collapse_emit", verts, nv, nt, p(ws), ws_bytes, p(out_v), len(out_v), p(out_t), len(out_t),
                    p(vm), p(counts))

    res["begin"] = timed(begin)
    res["begin_and_first_round"] = timed(lambda: run(1))
    res["begin_and_all_rounds"] = timed(lambda: run(rounds + 1))
    res["count_emit"] = timed(count_emit)
    assert torch.equal(out_t, first[1]) and counts.tolist()[7] == 0
    b, b1, ball = (res[k]["ms_median"] for k in ("begin", "begin_and_first_round", "begin_and_all_rounds"))
    res["first_round_ms"] = b1 - b
    res["mean_round_ms"] = (ball - b) / rounds if rounds else None
    res["total_ms"] = ball + res["count_emit"]["ms_median"]
    res["launches_per_round"] = 14
    del ws

    # vertex clustering at d = 2 in the same run
    origin, cell = mesh.export_lattice(R, 2)
    sws_bytes = int(_lib.lib().mi3d_mesh_simplify_workspace(nv, nt, 0))
    sws = torch.empty((sws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    org = (C.c_float * 3)(*origin)
    scount = lambda: _lib.launch("mi3d_mesh_simplify_count", verts, p(verts), nv, p(tris), nt, org, cell, p(sws),  # noqa: E731
                                 sws_bytes, p(counts))
    sc = timed(scount)
    kv, kt = counts.tolist()[:2]
    sv, st = torch.empty(kv, 3, device=dev), torch.empty(kt, 3, dtype=torch.int32, device=dev)
    lost = torch.empty(1, dtype=torch.int64, device=dev)
    se = timed(lambda: _lib.launch("mi3d_mesh_simplify_emit", verts, p(verts), nv, p(tris), nt, org, cell, p(sws), sws_bytes,
                                   p(sv), kv, p(st), kt, p(vm), p(lost)))
    res["simplify_d2"] = {"count": sc, "emit": se, "total_ms": sc["ms_median"] + se["ms_median"], "nv": kv, "nt": kt}
    del sws, sv, st
    if not export:
        return res
    extract, mesh.extract_volume = mesh.extract_volume, lambda m, r: vol     # export_mesh sees this volume
    thresh, model.density_thresh, cuda_ray, model.cuda_ray = model.density_thresh, iso, model.cuda_ray, False
    try:
        res["export_mesh"] = {}
        for name, kw in (("plain", {}), ("decimate=2", {"decimate": 2}), (f"collapse={target}", {"collapse": target})):
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


def fidelity(model, dev, R=128, T=2048, S=256):
    from mi3d import mesh
    vol = mesh.extract_volume(model, R)
    for q in QUANTILES:
        iso = float(torch.quantile(vol.flatten()[:: max(1, vol.numel() // (1 << 22))], q))
        nt = mesh.marching_cubes(vol, iso)[1].shape[0]
        if nt and mesh.atlas_cell(nt, T) > 0:
            break
    else:
        return {"error": f"NOT MEASURED: no quantile of {QUANTILES} gives a surface that fits a {T}^2 atlas"}
    K = np.array([[FOCAL * S, 0, 0.5 * S], [0, FOCAL * S, 0.5 * S], [0, 0, 1]])
    preview = dict(c2w=cameras(8, 3.2), K=K, H=S, W=S, fidelity=True)
    model.mean_density, model.density_thresh = iso, max(model.density_thresh, iso)
    res = {"resolution": R, "texture_size": T, "quantile": q, "threshold": iso, "triangles_extracted": nt,
           "preview": "8 views of 256 x 256 at distance 3.2", "field": "random-weight (not trained)"}
    faces = None
    for name in ("plain", "decimate=2", "collapse", "decimate=1.5,collapse"):
        kw = {"plain": {}, "decimate=2": dict(decimate=2), "collapse": dict(collapse=faces),
              "decimate=1.5,collapse": dict(decimate=1.5, collapse=faces)}[name]
        try:
            with tempfile.TemporaryDirectory() as tmp:
                o = model.export_mesh(tmp, resolution=R, texture_size=T, preview=preview, **kw)
                r = json.load(open(os.path.join(tmp, "preview.json")))
                res[name] = {"nv": len(o[0]), "nt": len(o[1]), "psnr_union": r["psnr_union"],
                             "psnr_intersection": r["psnr_intersection"], "iou": r["iou"]}
                if name == "decimate=2":
                    faces = len(o[1])                                # the collapse rows aim at the same face count
        except Exception as ex:  # noqa: BLE001  the other rows are kept
            res[name] = {"error": f"NOT MEASURED: {type(ex).__name__}: {ex}"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_collapse.json")
    ap.add_argument("--resolution", type=int, default=256)
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
           "round times from the medians; export_mesh: one wall-clock run"}

    def save():
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)

    R = a.resolution
    res[f"sphere_{R}"] = measure(model, sphere(R, dev), 0.0, dev)
    save()
    vol = mesh.extract_volume(model, R)
    res[f"field_{R}"] = measure(model, vol, float(vol.median()), dev)
    save()
    del vol
    try:
        res["fidelity"] = fidelity(model, dev)
    except Exception as ex:  # noqa: BLE001  the kernel times above are kept
        res["fidelity"] = {"error": f"NOT MEASURED: {type(ex).__name__}: {ex}"}
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
