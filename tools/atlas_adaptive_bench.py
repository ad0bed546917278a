"""The area-adaptive atlas of mesh export (mi3d.mesh.bake_texture(atlas="adaptive"), csrc/atlasadaptive.hip,
include/mi3d.h Part 20) beside Part 9's uniform atlas, on the radius-0.6 sphere of 256^3 before and after mesh.collapse
to 10 % of its faces, at T = 4096.
    python tools/atlas_adaptive_bench.py [--out profiles/atlas_adaptive.json]
Per mesh, by HIP events on the current stream (2 warm-ups, 7 repetitions; median, minimum, maximum): `measure`, `sort`,
`uv` and `positions` (the whole image in one band, ssaa 1) of Part 20, and `uniform_uv` and `uniform_positions` of Part 9
in the same process.  Next to them what mesh.atlas_plan reports (shift, rows, fill, clamped legs), the fill of the
uniform atlas, the spread of texels per unit length (largest / smallest over the two legs of every triangle; for the
adaptive atlas over the legs that are not clamped, and over all of them) of both atlases, and that two runs give the same
bytes.  `sharpness`: the RMS errors of tests/test_atlas_adaptive_gpu.py's test_sharper_where_it_matters (stripes of
wavelength 0.05 baked into the graded plane at T = 256, read back through vt).  The bake is milliseconds against a second
of PNG encoding: there is no speed target, the measure is texel density."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import atlas_adaptive_model as M  # noqa: E402  (the restatement: meshes, densities, the texture read-back)
from mesh_simplify_bench import sphere, timed  # noqa: E402

T = 4096


def spread(d):
    d = d[np.isfinite(d) & (d > 0)]
    return {"min": float(d.min()), "max": float(d.max()), "largest_over_smallest": float(d.max() / d.min())}


def measure(verts, tris, dev):
    from mi3d import _lib, mesh
    nv, nt, p = verts.shape[0], tris.shape[0], _lib.ptr
    res = {"nv": nv, "nt": nt, "texture_size": T}
    state = mesh._AdaptiveAtlas(verts, tris, T)
    res["plan"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in mesh._plan_dict(state.words).items()}
    shape, hist, bad = state.shape, torch.zeros(4096, dtype=torch.int32, device=dev), state.bad
    ws_bytes = int(_lib.lib().mi3d_atlas_adaptive_workspace(nt))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    slot, tri_of = torch.empty(nt, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev)
    vt, uvt = torch.empty(3 * nt, 2, device=dev), torch.empty(3 * nt, 2, device=dev)
    xyz = torch.empty(T * T, 3, device=dev)
    owner = torch.empty(T, T, dtype=torch.int32, device=dev)
    res["measure"] = timed(lambda: _lib.launch("mi3d_atlas_adaptive_measure", verts, p(verts), nv, p(tris), nt, p(shape),
                                               p(hist), p(bad)))
    res["sort"] = timed(lambda: _lib.launch("mi3d_atlas_adaptive_sort", verts, p(shape), nt, p(state.plan), p(ws), ws_bytes,
                                            p(slot), p(tri_of)))
    res["uv"] = timed(lambda: _lib.launch("mi3d_atlas_adaptive_uv", verts, p(shape), p(slot), nt, p(state.plan), T, p(vt)))
    res["positions"] = timed(lambda: _lib.launch("mi3d_atlas_adaptive_positions", verts, p(verts), nv, p(tris), nt, p(shape),
                                                 p(tri_of), p(state.plan), T, 1, 0, T, p(xyz), p(owner)))
    first = (slot.clone(), vt.clone(), xyz.clone(), owner.clone())
    _lib.launch("mi3d_atlas_adaptive_sort", verts, p(shape), nt, p(state.plan), p(ws), ws_bytes, p(slot), p(tri_of))
    _lib.launch("mi3d_atlas_adaptive_uv", verts, p(shape), p(slot), nt, p(state.plan), T, p(vt))
    _lib.launch("mi3d_atlas_adaptive_positions", verts, p(verts), nv, p(tris), nt, p(shape), p(tri_of), p(state.plan), T, 1,
                0, T, p(xyz), p(owner))
    res["two_runs_same_bytes"] = bool(all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                          for a, b in zip(first, (slot, vt, xyz, owner))))
    res["adaptive_owned_texels"] = int((owner >= 0).sum())
    c = mesh.atlas_cell(nt, T)
    res["uniform_cell"] = c
    if c:
        res["uniform_uv"] = timed(lambda: _lib.launch("mi3d_atlas_uv", verts, nt, T, p(uvt)))
        res["uniform_positions"] = timed(lambda: _lib.launch("mi3d_atlas_positions", verts, p(verts), nv, p(tris), nt, T, 1,
                                                             0, T, p(xyz), p(owner), p(bad)))
        res["uniform_fill"] = int((owner >= 0).sum()) / float(T * T)
    else:
        res["uniform_uv"] = res["uniform_positions"] = "NOT MEASURED: the mesh does not fit the uniform atlas"
    v, t = verts.cpu().numpy(), tris.cpu().numpy()
    d, clamped = M.densities(v, t, shape.cpu().numpy().view(np.uint32),
                             {"shift": int(state.words[0]), "kmax": int(state.words[2])})
    res["adaptive_density_unclamped"] = spread(d[~clamped])
    res["adaptive_density_all_legs"] = spread(d)
    if c:
        p3 = v[t].astype(np.float64)
        legs = np.stack([np.linalg.norm(p3[:, 1] - p3[:, 0], axis=1), np.linalg.norm(p3[:, 2] - p3[:, 0], axis=1)], 1)
        with np.errstate(divide="ignore"):
            res["uniform_density_all_legs"] = spread((c - 2) / legs)
    return res


def sharpness(dev):
    from mi3d import mesh
    import torch as th

    class Stripes:
        def density(self, xyz):
            return {"albedo": 0.5 + 0.5 * th.sin(2.0 * np.pi * 20.0 * xyz)}

    v, t = M.graded_plane()
    dv, dt = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
    tri, w, pts = M.surface_samples(v, t, 20000, seed=11)
    want, out = M.stripes(pts), {"mesh": "graded plane, 252 triangles", "texture_size": 256, "points": len(tri)}
    for atlas in ("uniform", "adaptive"):
        image, vt, _ = mesh.bake_texture(Stripes(), dv, dt, 256, atlas=atlas)
        got = M.bilinear_lookup(image.cpu().numpy(), vt.cpu().numpy(), tri, w)
        out[f"rms_{atlas}"] = float(np.sqrt(np.mean((got - want) ** 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/atlas_adaptive.json")
    ap.add_argument("--resolution", type=int, default=256)
    a = ap.parse_args()
    from mi3d import mesh
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "protocol": "HIP events, 2 warm-ups, 7 repetitions; median, min, max; positions: the whole 4096^2 image, ssaa 1"}

    def save():
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)

    R = a.resolution
    h = 2.0 / (R - 1)
    verts, tris = mesh.marching_cubes(sphere(R, dev), 0.0, (-1.0,) * 3, (h,) * 3)
    for name, step in ((f"sphere_{R}", lambda: (verts, tris)),
                       (f"sphere_{R}_collapsed", lambda: mesh.collapse(verts, tris, tris.shape[0] // 10)[:2])):
        try:
            res[name] = measure(*step(), dev)
        except Exception as ex:  # noqa: BLE001  the other figures are kept
            res[name] = {"error": f"NOT MEASURED: {type(ex).__name__}: {ex}"}
        save()
    try:
        res["sharpness"] = sharpness(dev)
    except Exception as ex:  # noqa: BLE001
        res["sharpness"] = {"error": f"NOT MEASURED: {type(ex).__name__}: {ex}"}
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
