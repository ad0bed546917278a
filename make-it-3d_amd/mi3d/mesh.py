"""Mesh export: the trained field -> `mesh.obj` / `mesh.mtl` (the reference's `NeRFRenderer.export_mesh`,
nerf/renderer.py:157-330 of the reference tree, without its UV atlas).

  extract_volume   sigma on the reference's R^3 lattice of [-1, 1]^3, evaluated by the field kernels in chunks, kept on
                   the device
  marching_cubes   the kernels of csrc/mesh.hip (include/mi3d.h Part 8 states the conventions): device volume in,
                   welded indexed mesh out; the host reads the two counts once to size the outputs (and
                   the overflow counter once after emit)
  export           volume -> surface -> per-vertex albedo -> files; what `NeRFRenderer.export_mesh` calls
  write_obj        vertex-coloured OBJ (`v x y z r g b`) + the reference's `mat0` material, no texture

`mcubes` (the reference's extractor) is on no machine this project builds on: vertex positions, ordering and the case
table are this project's contract, not a pinned copy of PyMCubes.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import Mi3dError

CHUNK = 1 << 21      # field evaluations per launch group: the gather's planes cost about 1 KB per row (budget_rows)
MIN_DIM, MAX_DIM = 2, 1024


def marching_cubes(volume, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """volume: float32 [Rx, Ry, Rz] on the GPU (x slowest).  Returns (vertices float32 [nv, 3], triangles int32 [nt, 3])
    on the same device, in the deterministic order of include/mi3d.h Part 8; an empty surface gives [0, 3] tensors."""
    vol = _lib.dev_f32(volume, "volume")
    if vol.dim() != 3:
        raise Mi3dError(f"volume must be 3-D (got {tuple(vol.shape)})")
    Rx, Ry, Rz = (int(s) for s in vol.shape)
    if not all(MIN_DIM <= r <= MAX_DIM for r in (Rx, Ry, Rz)):
        raise Mi3dError(f"every volume dimension must lie in [{MIN_DIM}, {MAX_DIM}] (got {(Rx, Ry, Rz)})")
    iso = float(iso)
    if iso != iso:
        raise Mi3dError("iso must not be NaN")
    dev = vol.device
    ws_bytes = int(_lib.lib().mi3d_mc_workspace(Rx, Ry, Rz))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    org = (C.c_float * 3)(*[float(o) for o in origin])
    spc = (C.c_float * 3)(*[float(s) for s in spacing])
    _lib.launch("mi3d_mc_count", vol, _lib.ptr(vol), Rx, Ry, Rz, iso, _lib.ptr(ws), ws_bytes, _lib.ptr(counts))
    _lib.launch("mi3d_mc_scan", vol, Rx, Ry, Rz, _lib.ptr(ws), ws_bytes, _lib.ptr(counts))
    nv, nt = (int(c) for c in counts[:2].tolist())           # the one host read the extraction needs
    vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    triangles = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    if nv == 0 and nt == 0:
        return vertices, triangles
    if nv > 2 ** 31 - 1:
        raise Mi3dError(f"{nv} vertices do not fit int32 triangle indices")
    _lib.launch("mi3d_mc_emit", vol, _lib.ptr(vol), Rx, Ry, Rz, iso, org, spc, _lib.ptr(ws), ws_bytes, _lib.ptr(counts),
                _lib.ptr(vertices), nv, _lib.ptr(triangles), nt)
    lost = int(counts[2])
    if lost != 0:
        raise Mi3dError(f"marching cubes could not place {lost} elements (the volume changed between count and emit?)")
    return vertices, triangles


def _chunks(n):
    return ((s, min(s + CHUNK, n)) for s in range(0, n, CHUNK))


def extract_volume(model, resolution):
    """sigma of `model` at (X[i], Y[j], Z[k]), X = Y = Z = torch.linspace(-1, 1, R) made on the CPU as the reference makes
    them (renderer.py:170-172) and uploaded: float32 [R, R, R] on the model's device.  The box is [-1, 1]^3 whatever
    `bound` is - the reference's quirk, kept."""
    R = int(resolution)
    if not MIN_DIM <= R <= MAX_DIM:
        raise Mi3dError(f"resolution must lie in [{MIN_DIM}, {MAX_DIM}] (got {resolution})")
    dev = model.aabb_train.device
    if dev.type != "cuda":
        raise Mi3dError(f"mesh export needs the model on the GPU (it is on {dev}): there is no CPU path for the kernels")
    axis = torch.linspace(-1, 1, R).to(dev)
    vol = torch.empty(R, R, R, dtype=torch.float32, device=dev)
    flat = vol.view(-1)
    with torch.no_grad():
        for s, e in _chunks(R ** 3):
            idx = torch.arange(s, e, device=dev)
            k = idx % R
            j = torch.div(idx, R, rounding_mode="floor") % R
            i = torch.div(idx, R * R, rounding_mode="floor")
            pts = torch.stack([axis[i], axis[j], axis[k]], -1)
            flat[s:e] = model.density(pts)["sigma"].reshape(-1).float()
    return vol


def vertex_albedo(model, vertices):
    """model.density(vertices)["albedo"] as float32 [nv, 3], in chunks."""
    out = torch.empty(vertices.shape[0], 3, dtype=torch.float32, device=vertices.device)
    with torch.no_grad():
        for s, e in _chunks(vertices.shape[0]):
            out[s:e] = model.density(vertices[s:e])["albedo"].float()
    return out


MTL = ("newmtl mat0 \n"
       "Ka 1.000000 1.000000 1.000000 \n"
       "Kd 1.000000 1.000000 1.000000 \n"
       "Ks 0.000000 0.000000 0.000000 \n"
       "Tr 1.000000 \n"
       "illum 1 \n"
       "Ns 0.000000 \n")        # renderer.py:320-328 without map_Kd: the colours are per vertex


def _write_rows(fp, fmt, rows, block=1 << 16):
    """One `fmt` line per row of a 2-D array, formatted a block at a time by ONE string operation (no Python loop per
    row: a 256^3 export has 10^5 - 10^7 of them)."""
    for s in range(0, rows.shape[0], block):
        part = rows[s:s + block]
        fp.write((fmt * part.shape[0]) % tuple(part.ravel().tolist()))


def write_obj(path, vertices, triangles, colors, name="mesh"):
    """`<path>/<name>.obj` (lines `v x y z r g b`, `f a b c` one-based) and `<path>/<name>.mtl`.  NumPy arrays:
    vertices [nv, 3], triangles [nt, 3] (zero-based), colors [nv, 3] in [0, 1].  Returns the two file names."""
    vertices, colors = np.asarray(vertices, np.float32), np.asarray(colors, np.float32)
    triangles = np.asarray(triangles)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or colors.shape != vertices.shape:
        raise ValueError(f"vertices {vertices.shape} and colors {colors.shape} must both be [nv, 3]")
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f"triangles must be [nt, 3] (got {triangles.shape})")
    os.makedirs(path, exist_ok=True)
    obj, mtl = os.path.join(path, f"{name}.obj"), os.path.join(path, f"{name}.mtl")
    with open(obj, "w") as fp:
        fp.write(f"mtllib {name}.mtl\n")
        # %.9g round-trips binary32; colours need no more than six decimals
        _write_rows(fp, "v %.9g %.9g %.9g %.6f %.6f %.6f\n", np.concatenate([vertices, colors], 1).astype(np.float64))
        fp.write("usemtl mat0\n")
        _write_rows(fp, "f %d %d %d\n", triangles.astype(np.int64) + 1)
    with open(mtl, "w") as fp:
        fp.write(MTL)
    return obj, mtl


def export(model, path, resolution=None, S=128):
    """What NeRFRenderer.export_mesh does (see there).  `S` only sizes the reference's chunks and is ignored."""
    del S
    if model.aabb_train.device.type != "cuda":
        raise Mi3dError(f"export_mesh needs the model on the GPU (it is on {model.aabb_train.device}): the field and "
                        f"the marching-cubes kernels have no CPU path")
    R = model.grid_size if resolution is None else int(resolution)
    # renderer.py:159-165
    thresh = float(min(model.mean_density, model.density_thresh) if model.cuda_ray else model.density_thresh)
    with torch.no_grad():
        vol = extract_volume(model, R)
        h = 2.0 / (R - 1)  # renderer.py:184: vertices / (R - 1) * 2 - 1
        vertices, triangles = marching_cubes(vol, thresh, origin=(-1.0, -1.0, -1.0), spacing=(h, h, h))
        if vertices.shape[0] == 0 or triangles.shape[0] == 0:
            lo, hi = torch.nan_to_num(vol, nan=0.0).min().item(), torch.nan_to_num(vol, nan=0.0).max().item()
            raise Mi3dError(f"export_mesh: no surface at density threshold {thresh:g}: the {R}^3 volume spans "
                            f"[{lo:g}, {hi:g}]")
        albedo = vertex_albedo(model, vertices)
    v, f, c = vertices.cpu().numpy(), triangles.cpu().numpy(), albedo.cpu().numpy()
    write_obj(path, v, f, c)
    return v, f, c
