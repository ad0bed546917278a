"""The floater filter of mesh export (mi3d.mesh.clean, csrc/meshclean.hip, include/mi3d.h Part 13) next to the extraction it
follows.
    python tools/mesh_clean_bench.py [--out profiles/mesh_clean.json] [--specks 4000]
Three surfaces, each extracted and cleaned in this process:
  field_128, field_256   the volume tools/mesh_bench.py uses (the random-weight field of __graft_entry__.smoke(), threshold
                         = the volume's median): a noise surface of very many small components - the worst case for the
                         labelling's atomics, not what an object looks like
  sphere_specks_256      the radius-0.6 sphere at 256^3 plus `--specks` isolated one-voxel islands: what a trained field
                         looks like to the filter (one large component, a few thousand floaters of eight triangles)
Per surface: `marching_cubes` (the whole call of mesh.marching_cubes), `clean` (the whole call of mesh.clean with
min_faces=9: labelling, keep rule, compaction and its one host read), and clean's two halves - `components` (the launches
of mi3d_mesh_components: init, hook, flatten, faces, boxes, finish) and `filter` (mi3d_mesh_clean_count, the host read,
mi3d_mesh_clean_emit).  The protocol of tools/mesh_bench.py: HIP events on the current stream, 2 warm-ups, 7 repetitions,
median, minimum and maximum reported; `clean_over_marching_cubes` is the ratio of the medians.  `bytes` of the halves =
what they must move at least (components: the triangles three times and the vertices once read, label / faces / boxes
written and read back once; filter: labels and triangles read twice, the kept rows read and written), `hbm_share` =
bytes / time / 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
MIN_FACES = 9          # above a one-voxel island's eight triangles


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


def sphere_and_specks(R, n, dev):
    ax = torch.linspace(-1, 1, R, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    d = torch.sqrt(x * x + y * y + z * z)
    vol = (0.6 - d).float()
    lat = torch.arange(2, R - 2, 3, device=dev)                   # stride 3: no two islands touch
    i, j, k = (g.reshape(-1) for g in torch.meshgrid(lat, lat, lat, indexing="ij"))
    free = d[i, j, k] > 0.7
    i, j, k = i[free], j[free], k[free]
    pick = torch.from_numpy(np.random.default_rng(0).choice(len(i), n, replace=False)).to(dev)
    vol[i[pick], j[pick], k[pick]] = 0.5
    return vol


def measure(vol, iso, dev):
    from mi3d import _lib, mesh
    R = vol.shape[0]
    h = 2.0 / (R - 1)
    extract = lambda: mesh.marching_cubes(vol, iso, (-1.0,) * 3, (h,) * 3)  # noqa: E731
    verts, tris = extract()
    nv, nt = verts.shape[0], tris.shape[0]
    label, faces, bmin, bmax, counts = mesh._label_components(verts, tris)
    host = counts.tolist()
    assert host[2] == 0 and host[3] == 0, host
    cv, ct, _ = mesh.clean(verts, tris, min_faces=MIN_FACES)
    kv, kt = cv.shape[0], ct.shape[0]
    res = {"resolution": R, "nv": nv, "nt": nt, "components_with_faces": host[5], "largest_component_faces": host[4] >> 32,
           "min_faces": MIN_FACES, "kept_nv": kv, "kept_nt": kt}
    p = _lib.ptr
    ws_bytes = int(_lib.lib().mi3d_mesh_components_workspace(nv, nt))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    vmap = torch.empty(nv, dtype=torch.int32, device=dev)
    out_v, out_t = torch.empty(kv, 3, device=dev), torch.empty(kt, 3, dtype=torch.int32, device=dev)

    def filter_half():
        _lib.launch("mi3d_mesh_clean_count", verts, p(tris), nv, nt, p(label), p(faces), p(bmin), p(bmax), MIN_FACES, 0.0,
                    0, p(ws), ws_bytes, p(counts))
        counts.tolist()
        _lib.launch("mi3d_mesh_clean_emit", verts, p(verts), nv, p(tris), nt, p(label), p(ws), ws_bytes, p(counts),
                    p(out_v), kv, p(out_t), kt, p(vmap))

    res["marching_cubes"] = timed(extract)
    res["clean"] = timed(lambda: mesh.clean(verts, tris, min_faces=MIN_FACES))
    res["components"] = dict(timed(lambda: mesh._label_components(verts, tris)),
                             bytes=3 * 12 * nt + 12 * nv + 2 * (4 + 4 + 24) * nv)
    res["filter"] = dict(timed(filter_half), bytes=2 * (12 * nt + 4 * nv) + 4 * nv + 24 * (kv + kt))
    for half in ("components", "filter"):
        res[half]["hbm_share"] = res[half]["bytes"] / (res[half]["ms_median"] * 1e-3) / HBM_PEAK
    res["clean_over_marching_cubes"] = res["clean"]["ms_median"] / res["marching_cubes"]["ms_median"]
    assert torch.equal(out_v, cv) and torch.equal(out_t, ct)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_clean.json")
    ap.add_argument("--specks", type=int, default=4000)
    a = ap.parse_args()
    from mi3d import mesh, sds_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    model, _, _ = sds_step.build_training_state(opt, dev, bitfield=0.5)
    with torch.no_grad():
        model.encoder.params.uniform_(-0.3, 0.3)
    model.eval()
    res = {"device": torch.cuda.get_device_name(dev), "hbm_peak_Bps": HBM_PEAK, "protocol": "HIP events, 2 warm-ups, 7 "
           "repetitions; median, min, max"}
    for R in (128, 256):
        vol = mesh.extract_volume(model, R)
        res[f"field_{R}"] = measure(vol, float(vol.median()), dev)
        del vol
    res["sphere_specks_256"] = dict(measure(sphere_and_specks(256, a.specks, dev), 0.0, dev), specks=a.specks)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
