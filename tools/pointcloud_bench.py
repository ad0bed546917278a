"""The refine stage's point cloud (mi3d.pointcloud) at the reference's size: 800 x 800, 8 views of an analytic sphere.
    python tools/pointcloud_bench.py [--side 800] [--views 8] [--out profiles/pointcloud.json]      on the MI355X
    python tools/pointcloud_bench.py --reference [--out profiles/pointcloud.json]                   in the build container
Views: the sphere of radius 0.45 about the origin from distance 1.25 (tests/golden/make_golden_pointcloud.py's case B at
another size), depth quantised to uint16 millimetres, fov 40 degrees, noise images; the canonical view is (V - 1) // 2.
GPU run: HIP events around every stage on one novel view, 2 warm-ups, median of 9 - unproject (the kept pixels' count is
read by the host inside it), zmin + visible, one 15 x 15 erosion, canonical filter, colour, the coverage render of the
canonical cloud - and `build` end to end by wall clock, median of 3.  `bytes` = what a stage must move at least.
--reference: wall time of the reference's OWN z_buffer and depth2point (oracle.ref_import) on ONE view of the same size,
on the CPU of the build container, once each - two Python loops over every point.  The parent commit has no number to
compare with: it cannot do this at all.  Both runs merge their keys into --out.
The GPU run also writes `depth_edges` (the Canny depth-edge mask, mi3d.h Part 12), same clock and repeats: classify on the
novel view's quantised depth, one batch of hysteresis sweeps on the 40 / 120 classes of a noisy image (a copy of the class
map is part of the timed work: the sweeps are in place), `depth_edge_mask` whole (10 / 10: no weak pixel, so no
hysteresis; one host read), and `build` with and without `depth_edges` by wall clock."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]

import numpy as np  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_pointcloud",
                                               os.path.join(ROOT, "tests", "golden", "make_golden_pointcloud.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

HBM_PEAK = 8.0e12


def eye_of(k, V):
    a = 2 * np.pi * k / V
    e = np.array([np.sin(a) * 0.9, 0.35 * np.cos(2 * a), np.cos(a) * 0.9 + 0.2])
    return e / np.linalg.norm(e) * 1.25


def scene(side, V):
    H = W = side
    K = gen.intrinsics(40.0, H, W)
    c2ws = np.stack([gen.look_at(eye_of(k, V)) for k in range(V)])
    depths, masks = [], []
    for c2w in c2ws:
        d, hit = gen.sphere_depth(c2w, K, H, W)
        depths.append((d * 1000.0).astype(np.uint16) / 1000.0)
        masks.append(hit.astype(np.float64))
    rgbs = np.stack([gen.noise_image(40 + k, H, W) for k in range(V)])
    return H, W, K, c2ws, np.stack(depths), np.stack(masks), rgbs


def merge(path, key, value):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[key] = value
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)


def reference(a):
    from oracle import ref_import
    ref_import.install()
    import nerf.refine_utils as ref
    H, W, K, c2ws, depths, masks, rgbs = scene(a.side, a.views)
    i = (a.views - 1) // 2
    w2c = np.linalg.inv(c2ws[i])
    v = np.random.default_rng(0).uniform(-0.45, 0.45, (int(masks[i].sum()), 3))
    t0 = time.perf_counter()
    vis = ref.z_buffer(v, w2c, H, W, K)
    t1 = time.perf_counter()
    pts, _ = ref.depth2point(depths[i], masks[i] == 1, c2ws[i], rgbs[i], H, W, K)
    t2 = time.perf_counter()
    res = {"where": "CPU of the build container, one process, the reference's own functions, one run each",
           "side": a.side, "z_buffer": {"points": len(v), "visible": int(vis.sum()), "s_wall": t1 - t0},
           "depth2point": {"masked_pixels": int(masks[i].sum()), "points": len(pts), "s_wall": t2 - t1}}
    print(json.dumps(res, indent=1))
    merge(a.out, "reference_cpu_one_view", res)


def gpu(a):
    import torch
    from mi3d import pointcloud as pc, refine

    def timed(fn, warmup=2, repeats=9):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(repeats):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        return {"ms_median": statistics.median(ts), "ms_min": min(ts), "repeats": repeats}

    dev = torch.device("cuda:0")
    H, W, K, c2ws, depths, masks, rgbs = scene(a.side, a.views)
    ind, i = (a.views - 1) // 2, 0
    D = torch.from_numpy(depths[i]).to(dev)
    m8 = torch.from_numpy(masks[i] != 0).to(dev).to(torch.uint8)
    w2c = np.linalg.inv(c2ws[i])
    rt, k = pc._camera(K, w2c)
    cano_rt, _ = pc._camera(K, np.linalg.inv(c2ws[ind]))
    img = torch.from_numpy(rgbs[i]).to(dev).float().permute(2, 0, 1).contiguous()
    cano_D = torch.from_numpy(depths[ind] * masks[ind]).to(dev).float()
    mask_f = torch.from_numpy(masks[i]).to(dev).float()
    v = pc._unproject(D, m8, K, c2ws[i])
    n = v.shape[0]
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    v_cano, _ = pc.depth2point(depths[ind], masks[ind], c2ws[ind], rgbs[ind], H, W, K, device=dev)
    cano32, K32 = v_cano.float(), torch.tensor(K, device=dev).float()
    w2c32 = torch.tensor(w2c, device=dev).float()

    def cano():
        pc._lib.launch("mi3d_pc_cano_filter", v, pc._lib.ptr(v), n, cano_rt, k, pc._lib.ptr(cano_D), H, W,
                       pc._lib.ptr(keep))

    px = H * W
    st = {"points": n, "canonical_points": int(v_cano.shape[0])}
    st["unproject"] = dict(timed(lambda: pc._unproject(D, m8, K, c2ws[i])), bytes=px * 9 * 2 + n * 24,
                           note="count, scan, write and the host's read of the count")
    st["zmin_visible"] = dict(timed(lambda: pc._visible(v, rt, k, H, W)), bytes=2 * n * 24 + px * 16 + n * 16 + n)
    st["erode_15x15"] = dict(timed(lambda: pc.erode(mask_f, 15)), bytes=px * 8)
    st["cano_filter"] = dict(timed(cano), bytes=n * 24 + n * 16 + n)
    st["colour"] = dict(timed(lambda: pc._colour(v, rt, k, img, H, W)), bytes=n * 24 + n * 48 + n * 12)
    with torch.no_grad():
        st["coverage_render"] = timed(lambda: refine.render_point(cano32, torch.ones_like(cano32), H, W, K32, w2c32, (H, W),
                                                                  2.0 / H * 2.0, 8))
    for name in ("unproject", "zmin_visible", "erode_15x15", "cano_filter", "colour"):
        st[name]["hbm_share"] = st[name]["bytes"] / (st[name]["ms_median"] * 1e-3) / HBM_PEAK
    ts = []
    for r in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pc.build(rgbs[ind], rgbs, depths, masks, c2ws, K, H, W, device=dev)
        torch.cuda.synchronize()
        if r:
            ts.append(1e3 * (time.perf_counter() - t0))
    st["build_end_to_end"] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "repeats": len(ts), "clock": "wall",
                              "views": a.views, "rows": [int(t.shape[0]) for t in out],
                              "note": "host arrays in: includes the upload of every view"}
    res = {"device": torch.cuda.get_device_name(dev), "side": a.side, "views": a.views, "hbm_peak_Bps": HBM_PEAK,
           "stages_one_novel_view": st}
    print(json.dumps(res, indent=1))
    merge(a.out, "mi355x", res)

    # ---- the Canny depth-edge mask
    m = pc.erode(mask_f, 11) == 1
    q = (D * m * 255.0).trunc().to(torch.int64).remainder(256).to(torch.uint8)
    cls_q, counts_q = pc.canny_classify(q, 10, 10)
    y, x = np.mgrid[:H, :W]
    noisy = np.clip(128 + 100 * np.sin(x / 5) * np.cos(y / 7) + np.random.default_rng(0).integers(-6, 7, (H, W)), 0, 255)
    noisy = torch.from_numpy(noisy.astype(np.uint8)).to(dev)
    cls_n, counts_n = pc.canny_classify(noisy, 40, 120)
    work, flag = torch.empty_like(cls_n), torch.empty(1, dtype=torch.int32, device=dev)

    def batch():
        work.copy_(cls_n)
        pc._lib.launch("mi3d_canny_hysteresis", work, pc._lib.ptr(work), H, W, pc.HYSTERESIS_SWEEPS, pc._lib.ptr(flag))

    calls = []
    orig = pc._lib.launch
    pc._lib.launch = lambda name, *args: (calls.append(name), orig(name, *args))[1]
    try:
        settled = pc.hysteresis(cls_n)
    finally:
        pc._lib.launch = orig
    de = {"quantised_depth": {"weak_strong": counts_q.tolist(), "edge_pixels": int((cls_q == 2).sum())},
          "noisy_image_40_120": {"weak_strong": counts_n.tolist(), "strong_after_hysteresis": int((settled == 2).sum()),
                                 "host_batches_to_settle": len(calls), "sweeps_per_batch": pc.HYSTERESIS_SWEEPS}}
    de["classify"] = dict(timed(lambda: pc.canny_classify(q, 10, 10)), bytes=px * 2,
                          note="includes the in-stream zeroing of the counts and the allocation of the outputs")
    de["hysteresis_batch"] = dict(timed(batch), bytes=px * 2 * (pc.HYSTERESIS_SWEEPS + 1),
                                  note="a copy of the class map, then one call of HYSTERESIS_SWEEPS sweeps; no host read")
    de["depth_edge_mask"] = dict(timed(lambda: pc.depth_edge_mask(D, m, 10, 11)),
                                 note="quantisation (torch ops), classify, the host's read of the counts, 11 x 11 dilation")
    for name in ("classify", "hysteresis_batch"):
        de[name]["hbm_share"] = de[name]["bytes"] / (de[name]["ms_median"] * 1e-3) / HBM_PEAK
    for key, flagged in (("build_without_depth_edges", False), ("build_with_depth_edges", True)):
        ts = []
        for r in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pc.build(rgbs[ind], rgbs, depths, masks, c2ws, K, H, W, device=dev, depth_edges=flagged)
            torch.cuda.synchronize()
            if r:
                ts.append(1e3 * (time.perf_counter() - t0))
        de[key] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "repeats": len(ts), "clock": "wall",
                   "views": a.views, "rows": [int(t.shape[0]) for t in out]}
    de = {"device": torch.cuda.get_device_name(dev), "side": a.side, "views": a.views, **de}
    print(json.dumps(de, indent=1))
    merge(a.out, "depth_edges", de)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default="profiles/pointcloud.json")
    ap.add_argument("--reference", action="store_true", help="time the reference's own functions on the CPU instead")
    a = ap.parse_args()
    (reference if a.reference else gpu)(a)


if __name__ == "__main__":
    main()
