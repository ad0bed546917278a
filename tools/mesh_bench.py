"""Mesh export (NeRFRenderer.export_mesh -> mi3d.mesh) at the resolution main.py asks for (256), pass by pass.
    python tools/mesh_bench.py [--resolution 256] [--out profiles/mesh_export.json] [--texture-size 4096] [--texture-only]
Random-weight field (the blob + uniform(-0.3, 0.3) hash-grid entries of __graft_entry__.smoke()), fp32, threshold = the
volume's median so that the surface is large.  HIP events around every pass, 2 warm-ups, median of 7 (the volume sampling: 3; the
file writing once, the end-to-end export twice); wall clock where the host takes part (files, end to end).
`bytes` = what a pass must move at least: the volume once per kernel that reads it, 4 B per grid point of first-vertex ids
written by the vertex kernel and (at most) read back by the triangle kernel, 12 B per vertex / triangle written;
`hbm_share` = bytes / time / 8 TB/s (the MI355X's HBM3E peak).
The textured export (key `texture`; `--texture-only` keeps every other key of an existing --out file as it is) does NOT bake
the noise surface above - no atlas holds 31.6 M triangles and it is not what an object looks like - but (a) the analytic
radius-0.6 sphere of tests/test_mc_tables_cpu.sphere_volume at the same resolution, coloured by the same random-weight field
through mesh.bake_texture, stage by stage: atlas + positions kernels, field evaluation of the texels, pack (HIP events over all
bands of the image, median of 7), PNG encoding and OBJ writing (wall clock, once); and (b) `export_mesh(texture_size=T)` end to
end on the field itself at the lowest of a few high quantiles of the volume whose surface fits the atlas with a cell of at
least 6 (wall clock, median of 2).  `bytes` of the texture kernels: 12 B per sample written + 4 B per texel of owner
(positions); the same read + 3 B per texel written (pack)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, warmup, repeats):
    """Median / min of HIP-event times (ms) of fn() on the current stream."""
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
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "repeats": repeats}


def wall(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "repeats": repeats, "clock": "wall"}


def texture_bench(model, dev, R, T, ssaa=1):
    """The `texture` record: see the module docstring."""
    from mi3d import _lib, mesh
    p, ss2, h = _lib.ptr, ssaa * ssaa, 2.0 / (R - 1)
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    sphere = torch.from_numpy((0.6 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)).to(dev)
    verts, tris = mesh.marching_cubes(sphere, 0.0, (-1.0,) * 3, (h,) * 3)
    nv, nt = verts.shape[0], tris.shape[0]
    c = mesh.atlas_cell(nt, T)
    used = -(-((nt + 1) // 2) // (T // (c + 1))) * c
    band = max(4, mesh.CHUNK // (T * ss2) // 4 * 4)
    bands = [(r, min(band, used - r)) for r in range(0, used, band)]
    res = {"texture_size": T, "ssaa": ssaa, "sphere": {"nv": nv, "nt": nt, "cell": c, "image_rows_used": used,
                                                      "texels_evaluated": used * T, "bands": len(bands)}}
    vt = torch.empty(3 * nt, 2, device=dev)
    xyz = torch.empty(used * T * ss2, 3, device=dev)
    albedo = torch.empty_like(xyz)
    owner = torch.empty(used, T, dtype=torch.int32, device=dev)
    image = torch.empty(used, T, 3, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    rows_of = lambda t, r, n: t[r * T * ss2:(r + n) * T * ss2]  # noqa: E731

    def positions():
        _lib.launch("mi3d_atlas_uv", vt, nt, T, p(vt))
        for r, n in bands:
            _lib.launch("mi3d_atlas_positions", xyz, p(verts), nv, p(tris), nt, T, ssaa, r, n, p(rows_of(xyz, r, n)),
                        p(owner[r]), p(bad))

    def field():
        for r, n in bands:
            rows_of(albedo, r, n).copy_(model.density(rows_of(xyz, r, n))["albedo"])

    def pack():
        for r, n in bands:
            _lib.launch("mi3d_texture_pack", albedo, p(rows_of(albedo, r, n)), p(owner[r]), T, ssaa, n, p(image[r]))

    sph = res["sphere"]
    with torch.no_grad():
        sph["atlas_and_positions"] = dict(timed(positions, 2, 7), bytes=used * T * (12 * ss2 + 4) + 24 * nt)
        sph["field_evaluation"] = timed(field, 1, 7)
        sph["field_evaluation"]["evaluations_per_s"] = used * T * ss2 / (sph["field_evaluation"]["ms_median"] * 1e-3)
        sph["pack"] = dict(timed(pack, 2, 7), bytes=used * T * (12 * ss2 + 4 + 3))
        for name in ("atlas_and_positions", "pack"):
            sph[name]["hbm_share"] = sph[name]["bytes"] / (sph[name]["ms_median"] * 1e-3) / HBM_PEAK
        assert int(bad) == 0
        sph["bake_texture_whole_call"] = wall(lambda: mesh.bake_texture(model, verts, tris, T, ssaa), 1, 5)
        img, uv, own = mesh.bake_texture(model, verts, tris, T, ssaa)
        assert torch.equal(img[:used], image) and torch.equal(own[:used], owner)
        colours = mesh.vertex_albedo(model, verts).cpu().numpy()
    v, f, uv, img = verts.cpu().numpy(), tris.cpu().numpy(), uv.cpu().numpy(), img.cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        r = wall(lambda: mesh.write_png(os.path.join(d, "albedo.png"), img), 0, 1)
        r["png_bytes"] = os.path.getsize(os.path.join(d, "albedo.png"))
        sph["png_encoding"] = r
        r = wall(lambda: mesh.write_obj(d, v, f, colours, uvs=uv, uv_faces=np.arange(3 * nt).reshape(-1, 3),
                                        texture="albedo.png"), 0, 1)
        r["obj_bytes"] = os.path.getsize(os.path.join(d, "mesh.obj"))
        sph["obj_writing"] = r

    # ---- export_mesh(texture_size=T) end to end on the field itself, at a quantile whose surface fits with c >= 6
    vol = mesh.extract_volume(model, R)
    flat = vol.flatten()
    keep = model.mean_density, model.density_thresh
    for q in (0.9, 0.95, 0.98, 0.99, 0.995, 0.999):
        iso = float(flat.kthvalue(int(q * (flat.numel() - 1)) + 1).values)
        n = mesh.marching_cubes(vol, iso, (-1.0,) * 3, (h,) * 3)[1].shape[0]
        if mesh.atlas_cell(n, T) >= 6:
            break
    else:
        raise SystemExit(f"no quantile up to 0.999 gives a surface that fits a {T}^2 atlas with a cell of 6 ({n} triangles)")
    try:
        model.mean_density, model.density_thresh = iso, max(model.density_thresh, iso)
        with tempfile.TemporaryDirectory() as d:
            r = wall(lambda: model.export_mesh(d, resolution=R, texture_size=T, ssaa=ssaa), 0, 2)
            r.update(quantile=q, iso=iso, nt=n, cell=mesh.atlas_cell(n, T),
                     obj_bytes=os.path.getsize(os.path.join(d, "mesh.obj")),
                     png_bytes=os.path.getsize(os.path.join(d, "albedo.png")))
            res["export_mesh_textured_end_to_end"] = r
            res["export_mesh_untextured_same_surface"] = wall(lambda: model.export_mesh(d, resolution=R), 0, 2)
    finally:
        model.mean_density, model.density_thresh = keep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--out", default="profiles/mesh_export.json")
    ap.add_argument("--texture-size", type=int, default=4096)
    ap.add_argument("--texture-only", action="store_true", help="measure the textured export alone and add it to --out")
    a = ap.parse_args()
    from mi3d import _lib, mesh, sds_step
    dev = torch.device("cuda:0")
    R = a.resolution
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    model, _, _ = sds_step.build_training_state(opt, dev, bitfield=0.5)
    with torch.no_grad():
        model.encoder.params.uniform_(-0.3, 0.3)
    model.eval()
    res = {"resolution": R, "grid_points": R ** 3, "device": torch.cuda.get_device_name(dev), "hbm_peak_Bps": HBM_PEAK}
    if a.texture_only:
        if os.path.exists(a.out):
            res = json.load(open(a.out))
            assert res["resolution"] == R, (res["resolution"], R)
        res["texture"] = texture_bench(model, dev, R, a.texture_size)
        print(json.dumps(res["texture"], indent=1))
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        return

    # ---- the field alone, for scale: density() on one chunk of random points of [-1, 1]^3
    pts = torch.rand(mesh.CHUNK, 3, device=dev) * 2 - 1
    with torch.no_grad():
        r = timed(lambda: model.density(pts), 2, 7)
    r["evaluations_per_s"] = mesh.CHUNK / (r["ms_median"] * 1e-3)
    res["density_one_chunk_random_points"] = r

    # ---- volume sampling
    r = timed(lambda: mesh.extract_volume(model, R), 1, 3)
    r["evaluations_per_s"] = R ** 3 / (r["ms_median"] * 1e-3)
    res["volume_sampling"] = r
    vol = mesh.extract_volume(model, R)
    iso = float(vol.median())
    res["iso"] = iso
    res["volume_min_max"] = [float(vol.min()), float(vol.max())]

    # ---- marching cubes, pass by pass (what mesh.marching_cubes launches)
    lib = _lib.lib()
    ws_bytes = int(lib.mi3d_mc_workspace(R, R, R))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    h = 2.0 / (R - 1)
    org, spc = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(h, h, h)
    p = _lib.ptr

    def count():
        _lib.launch("mi3d_mc_count", vol, p(vol), R, R, R, iso, p(ws), ws_bytes, p(counts))

    def scan():
        _lib.launch("mi3d_mc_scan", vol, R, R, R, p(ws), ws_bytes, p(counts))

    count()
    scan()
    nv, nt = (int(c) for c in counts[:2].tolist())
    verts = torch.empty(nv, 3, device=dev)
    tris = torch.empty(nt, 3, dtype=torch.int32, device=dev)

    def emit():
        _lib.launch("mi3d_mc_emit", vol, p(vol), R, R, R, iso, org, spc, p(ws), ws_bytes, p(counts), p(verts), nv,
                    p(tris), nt)

    vol_bytes, nb = 4 * R ** 3, (R ** 3 + 255) // 256
    mc = res["marching_cubes"] = {"nv": nv, "nt": nt, "workspace_bytes": ws_bytes}
    mc["count"] = dict(timed(count, 2, 7), bytes=vol_bytes + 12 * nb)
    # scan repeated on its own output scans offsets instead of sums: the same work (its time does not depend on the
    # values), garbage results - count and scan run once more before emit is timed
    mc["scan"] = dict(timed(scan, 2, 7), bytes=2 * 12 * nb)
    count()
    scan()
    mc["emit"] = dict(timed(emit, 2, 7), bytes=2 * vol_bytes + 2 * 4 * R ** 3 + 12 * nv + 12 * nt + 12 * nb)
    for name in ("count", "scan", "emit"):
        mc[name]["hbm_share"] = mc[name]["bytes"] / (mc[name]["ms_median"] * 1e-3) / HBM_PEAK
    assert counts.tolist() == [nv, nt, 0, 0]
    mc["whole_call"] = wall(lambda: mesh.marching_cubes(vol, iso, (-1.0,) * 3, (h,) * 3), 1, 5)

    # ---- colours, files, end to end
    with torch.no_grad():
        r = timed(lambda: mesh.vertex_albedo(model, verts), 1, 5)
    r["evaluations_per_s"] = nv / (r["ms_median"] * 1e-3)
    res["vertex_colouring"] = r
    v, f = verts.cpu().numpy(), tris.cpu().numpy()
    c = mesh.vertex_albedo(model, verts).cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        r = wall(lambda: mesh.write_obj(d, v, f, c), 0, 1)
        r["obj_bytes"] = os.path.getsize(os.path.join(d, "mesh.obj"))
        res["file_writing"] = r
        keep = model.mean_density, model.density_thresh
        model.mean_density = iso
        model.density_thresh = max(model.density_thresh, iso)
        res["export_mesh_end_to_end"] = wall(lambda: model.export_mesh(d, resolution=R), 0, 2)
        model.mean_density, model.density_thresh = keep
    res["texture"] = texture_bench(model, dev, R, a.texture_size)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
