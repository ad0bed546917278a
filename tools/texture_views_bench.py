"""Texturing from views (mi3d.mesh.bake_views, csrc/textureviews.hip, include/mi3d.h Part 15) at the size an export runs.
    python tools/texture_views_bench.py [--out profiles/texture_views.json] [--resolution 256] [--texture-size 4096]
                                        [--views 32] [--side 800]
The radius-0.6 sphere at 256^3 (what an object looks like), T = 4096, 32 views of 800 x 800 on four rings around it.  The
images are rendered analytically: the colour of a pixel is a smooth function of the point where its ray meets the sphere.
  depth            mi3d_mesh_depth for all views: the fill and the rasterisation
  depth_close_view the same for ONE view from 0.75 (0.15 above the surface), where a triangle covers thousands of pixels and
                   one thread walks them all: the case a rasteriser that splits triangles would serve
  project          mi3d_texture_project over all bands of the atlas (positions made before, a constant base)
  bake_views       mesh.bake_views as a whole with the field as base: depth, then per band positions, field, projection, pack
  bake_texture     mesh.bake_texture of the same atlas: the field bake this one is read against
HIP events on the current stream, 2 warm-ups, 7 repetitions: median, minimum and maximum.  `bytes` = what the algorithm has
to move at least (12 B of position, 12 B of base, 12 B of colour and 1 B of hits per sample, 4 B of owner per texel; the
taps come through the caches and are not counted), `ops` = samples x views x about 70 floating-point operations for a view
that passes every test - rough counts from the shapes, for orders of magnitude only.
Two quality numbers, from the kernels' own per-sample output:
  coverage   of the samples whose triangle faces some camera with cos >= min_cos (binary64), the share with >= 1 hit
  rms        the RMS difference between the blended colour and the analytic colour at the sample's point, over hit samples
No threshold is set on any of them."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

R0 = 0.6
FOCAL = 1.6             # normalised: the sphere's silhouette has a radius of 0.26 x 1.6 = 0.41 of the image side
DISTANCE = 2.4


def timed(fn, warmup=2, repeats=7):
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


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    f = -eye / np.linalg.norm(eye)
    r = np.cross(f, (0.0, 0.0, 1.0))
    r /= np.linalg.norm(r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, np.cross(f, r), f, eye
    return c2w


def cameras(V, distance=DISTANCE):
    """V poses on four rings of elevation -50, -15, 15, 50 degrees, azimuths staggered from ring to ring."""
    out = []
    for k in range(V):
        ring, n = k % 4, (V + 3) // 4
        el = math.radians((-50, -15, 15, 50)[ring])
        az = 2 * math.pi * ((k // 4) + 0.25 * ring) / n
        out.append(look_at(distance * np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])))
    return np.stack(out)


def colour_at(p):
    """The analytic texture: smooth in the surface point, different per channel; p [..., 3] (any radius) -> [..., 3]."""
    p = p / p.norm(dim=-1, keepdim=True) * R0
    k = torch.tensor([[7.0, 3.0, 5.0], [4.0, 9.0, 2.0], [3.0, 5.0, 8.0]], dtype=p.dtype, device=p.device)
    return 0.5 + 0.45 * torch.sin(p @ k.T + torch.tensor([0.3, 1.1, 2.0], dtype=p.dtype, device=p.device))


def render_analytic(c2w, K, H, W, dev):
    """float32 [V, H, W, 3]: the ray through every pixel centre against the sphere, in binary64; 0 off the sphere."""
    j, i = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64) + 0.5,
                          torch.arange(W, device=dev, dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([i, j, torch.ones_like(i)], -1)
    Kinv = torch.tensor(np.linalg.inv(K), device=dev)
    out = torch.zeros(len(c2w), H, W, 3, dtype=torch.float32, device=dev)
    for v, pose in enumerate(c2w):
        pose = torch.tensor(pose, device=dev)
        d = pix @ Kinv.T @ pose[:3, :3].T
        d = d / d.norm(dim=-1, keepdim=True)
        o = pose[:3, 3]
        b = d @ o
        disc = b * b - (o @ o - R0 * R0)
        hit = disc > 0
        p = o + (-b - torch.sqrt(disc.clamp(min=0)))[..., None] * d
        out[v] = torch.where(hit[..., None], colour_at(p), torch.zeros_like(p)).float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/texture_views.json")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--texture-size", type=int, default=4096)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--side", type=int, default=800)
    a = ap.parse_args()
    from mi3d import _lib, mesh, sds_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    model, _, _ = sds_step.build_training_state(opt, dev, bitfield=0.5)
    with torch.no_grad():
        model.encoder.params.uniform_(-0.3, 0.3)
    model.eval()

    R, T, V, S, p = a.resolution, a.texture_size, a.views, a.side, _lib.ptr
    ax = torch.linspace(-1, 1, R, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    h = 2.0 / (R - 1)
    verts, tris = mesh.marching_cubes((R0 - torch.sqrt(x * x + y * y + z * z)).float(), 0.0, (-1.0,) * 3, (h,) * 3)
    del x, y, z
    nv, nt = verts.shape[0], tris.shape[0]
    c = mesh.atlas_cell(nt, T)
    assert c > 0, f"{nt} triangles do not fit {T}"
    power, min_cos, depth_tol = 4, 0.2, 0.02                     # bake_views' defaults
    c2w, K = cameras(V), np.array([[FOCAL * S, 0, 0.5 * S], [0, FOCAL * S, 0.5 * S], [0, 0, 1]])
    images = render_analytic(c2w, K, S, S, dev)
    records, weights, min_cos2, depth_tol, _ = mesh.check_views(images, c2w, K, None, None, power, min_cos, depth_tol)
    records, weights = torch.from_numpy(records).to(dev), torch.from_numpy(weights).to(dev)
    res = {"device": torch.cuda.get_device_name(dev),
           "protocol": "HIP events, 2 warm-ups, 7 repetitions; median, min, max",
           "resolution": R, "nv": nv, "nt": nt, "texture_size": T, "cell": c, "views": V, "view_side": S,
           "power": power, "min_cos": min_cos, "depth_tol": depth_tol, "focal": FOCAL, "camera_distance": DISTANCE}

    # ---- depth
    depth = torch.empty(V, S, S, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    res["depth"] = timed(lambda: _lib.launch("mi3d_mesh_depth", verts, p(verts), nv, p(tris), nt, p(records), V, S, S,
                                             p(depth), p(counts)))
    res["depth"]["counts_bad_skipped"] = counts.tolist()
    res["depth"]["pixels_drawn_share"] = float(torch.isfinite(depth).float().mean())
    res["depth"]["bytes"] = 4 * V * S * S + 12 * nv + 12 * nt
    close = torch.from_numpy(mesh.view_records(cameras(4, 0.75)[:1], K)).to(dev)
    d1 = torch.empty(1, S, S, device=dev)
    res["depth_close_view"] = timed(lambda: _lib.launch("mi3d_mesh_depth", verts, p(verts), nv, p(tris), nt, p(close), 1, S, S,
                                                        p(d1), p(counts)))
    res["depth_close_view"]["counts_bad_skipped"] = counts.tolist()
    res["depth_close_view"]["pixels_drawn_share"] = float(torch.isfinite(d1).float().mean())
    del d1
    _lib.launch("mi3d_mesh_depth", verts, p(verts), nv, p(tris), nt, p(records), V, S, S, p(depth), p(counts))

    # ---- projection over all bands
    cols = T // (c + 1)
    used = -(-((nt + 1) // 2) // cols) * c
    band = max(4, mesh.CHUNK // T // 4 * 4)
    xyz = torch.empty(used * T, 3, device=dev)
    owner = torch.empty(used, T, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    for r0 in range(0, used, band):
        n = min(band, used - r0)
        _lib.launch("mi3d_atlas_positions", xyz, p(verts), nv, p(tris), nt, T, 1, r0, n, p(xyz[r0 * T:]), p(owner[r0]), p(bad))
    base = torch.full_like(xyz, 0.5)
    colour = torch.empty_like(xyz)
    hits = torch.empty(used * T, dtype=torch.uint8, device=dev)

    def project():
        for r0 in range(0, used, band):
            n = min(band, used - r0)
            _lib.launch("mi3d_texture_project", xyz, p(xyz[r0 * T:]), p(owner[r0]), p(verts), nv, p(tris), nt, T, 1, n,
                        p(records), V, S, S, p(depth), p(images), None, p(weights), power, min_cos2, depth_tol,
                        p(base[r0 * T:]), p(colour[r0 * T:]), p(hits[r0 * T:]))

    res["project"] = timed(project)
    samples = used * T
    res["project"].update(samples=samples, bands=-(-used // band), bytes=samples * (12 * 3 + 1 + 4),
                          ops=samples * V * 70)
    res["project"]["GB_per_s"] = res["project"]["bytes"] / (res["project"]["ms_median"] * 1e-3) / 1e9

    # ---- quality, from that output
    own = owner.view(-1) >= 0
    idx = own.nonzero().view(-1)
    pts = xyz[idx].double()
    tri = verts[tris[owner.view(-1)[idx].long()].long()].double()
    nrm = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    best = torch.full((len(idx),), -1.0, dtype=torch.float64, device=dev)
    for pose in c2w:
        d = torch.tensor(pose[:3, 3], device=dev) - pts
        best = torch.maximum(best, (nrm * d).sum(-1) / d.norm(dim=-1))
    faces = best >= min_cos
    hit = hits[idx] > 0
    err = (colour[idx][hit].double() - colour_at(pts[hit])).pow(2).mean().sqrt()
    res["quality"] = {"owned_samples": int(own.sum()), "facing_some_camera": int(faces.sum()),
                      "coverage": float((hit & faces).sum() / faces.sum()), "hit_samples": int(hit.sum()),
                      "hits_mean_over_hit_samples": float(hits[idx][hit].float().mean()),
                      "rms_vs_analytic_colour": float(err)}
    del pts, tri, nrm, best, colour, base, xyz, hits

    # ---- the whole bakes
    res["bake_views"] = timed(lambda: mesh.bake_views(model, verts, tris, T, images, c2w, K), 1, 7)
    res["bake_texture"] = timed(lambda: mesh.bake_texture(model, verts, tris, T), 1, 7)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
