"""Mesh export: the trained field -> `mesh.obj` / `mesh.mtl` and, on request, `albedo.png` (the reference's
`NeRFRenderer.export_mesh`, nerf/renderer.py:157-330 of the reference tree).

  extract_volume   sigma on the reference's R^3 lattice of [-1, 1]^3, evaluated by the field kernels in chunks, kept on
                   the device
  marching_cubes   the kernels of csrc/mesh.hip (include/mi3d.h Part 8 states the conventions): device volume in,
                   welded indexed mesh out; the host reads the two counts once to size the outputs (and
                   the overflow counter once after emit)
  components       the kernels of csrc/meshclean.hip (include/mi3d.h Part 13): the connected components of an indexed
                   mesh - label, face count and bounding box of each - by a lock-free union-find on the device
  clean            drops the components below `min_faces` / `min_diagonal` (or all but the largest): stable compaction
                   on the device; the host reads the counts once to size the outputs
  simplify         the kernels of csrc/meshsimplify.hip (include/mi3d.h Part 14): vertex clustering on a uniform lattice -
                   one vertex per occupied cell, degenerate and duplicate triangles dropped; the host reads the counts
                   once to size the outputs
  smooth           the kernels of csrc/meshsmooth.hip (include/mi3d.h Part 16): Taubin's lambda | mu smoothing of the
                   vertices - the incidence built once, then passes without atomics over exact fixed-point sums
  bake_texture     the kernels of csrc/texture.hip (include/mi3d.h Part 9): a texel patch per triangle, the field's albedo
                   at every texel's surface point, packed to 8-bit RGB on the device
  atlas_plan       what atlas="adaptive" does with a mesh (csrc/atlasadaptive.hip, include/mi3d.h Part 20): patches whose
                   legs follow the triangle's edge lengths - shift, rows used, fill, class histogram, clamped legs
  render_depth     the depth maps of a mesh from V pinhole cameras (csrc/textureviews.hip, include/mi3d.h Part 15)
  bake_views       the same atlas coloured from views by projection: per sample the visibility-tested, angle-weighted
                   mean of the views that see it, the field's albedo where none does (Part 15)
  render           images of a mesh from V pinhole cameras (csrc/meshrender.hip, include/mi3d.h Part 17): a visibility buffer
                   per view, then per pixel the perspective-correct vertex colour or atlas texture, normals, depth,
                   triangle index and barycentrics; the field's shadings composed in torch
  fit_texture      a float texture or vertex colours fitted to views through render (include/mi3d.h Part 18): the adjoint of
  fit_colors       the shading pass in its colour source - exact 64-bit fixed-point sums - under torch's Adam
  fidelity         PSNR over the union and the intersection of two renders' masks and the masks' IoU, per view and overall
  export           volume -> surface -> per-vertex albedo (-> texture) -> files; what `NeRFRenderer.export_mesh` calls
  write_obj        vertex-coloured OBJ (`v x y z r g b`) + the reference's `mat0` material; with UVs `v` / `vt` /
                   `f v/vt` and `map_Kd`; with normals `vn` lines and `f v//vn` / `f v/vt/vn`
  write_png        8-bit RGB PNG with the standard library alone

`mcubes`, `xatlas` and `nvdiffrast` (the reference's extractor, unwrapper and rasteriser) are on no machine this project
builds on: vertex positions, ordering, the case table and the atlas are this project's contract, not pinned copies.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib
from ._lib import Mi3dError

CHUNK = 1 << 21      # field evaluations per launch group: the gather's planes cost about 1 KB per row (budget_rows)
MIN_DIM, MAX_DIM = 2, 1024


def _is_number(x, integer=False):
    """An int or a float, NumPy's included, never a bool; with `integer` an int."""
    kinds = (int, np.integer) if integer else (int, float, np.integer, np.floating)
    return isinstance(x, kinds) and not isinstance(x, (bool, np.bool_))


def _integer(x, name, lo, hi):
    if not _is_number(x, integer=True):
        raise Mi3dError(f"{name} must be an integer (got {x!r})")
    if not lo <= int(x) <= hi:
        raise Mi3dError(f"{name} must lie in [{lo}, {hi}] (got {x})")
    return int(x)


def _real(x, name, lo, hi, none=False):
    """A number in [lo, hi] (never NaN) as a binary64; with `none`, None passes through."""
    if x is None and none:
        return None
    if not _is_number(x):
        raise Mi3dError(f"{name} must be a number{' or None' if none else ''} (got {x!r})")
    if not lo <= float(x) <= hi:                                # false for NaN
        raise Mi3dError(f"{name} must lie in [{lo:g}, {hi:g}] (got {x!r})")
    return float(x)


def _number(x, name, lo, hi):
    return float(np.float32(_real(x, name, lo, hi)))           # as the kernels take it


def _flag(x, name):
    if not isinstance(x, (bool, np.bool_)):
        raise Mi3dError(f"{name} must be a bool (got {x!r})")
    return bool(x)


_INF = float("inf")


def _workspace(dev, query, *sizes, what=None):
    """The workspace of a *_workspace query of the library: (int64 tensor on `dev`, its bytes).  With `what`, 0 bytes for
    the mesh sizes (nv, nt) means more triangles than the unit takes."""
    ws_bytes = int(getattr(_lib.lib(), query)(*sizes))
    if ws_bytes == 0 and what is not None:
        raise Mi3dError(f"{sizes[1]} triangles are more than {what} takes (2^30)")
    return torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev), ws_bytes


def _outputs(kv, kt, nv, dev):
    """(vertices float32 [kv, 3], triangles int32 [kt, 3], vertex_map int32 [nv]) for an emit to fill."""
    return (torch.empty(kv, 3, dtype=torch.float32, device=dev), torch.empty(kt, 3, dtype=torch.int32, device=dev),
            torch.empty(nv, dtype=torch.int32, device=dev))


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
    ws, ws_bytes = _workspace(dev, "mi3d_mc_workspace", Rx, Ry, Rz)
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


MAX_COUNT = 2 ** 31 - 1


def _check_mesh(vertices, triangles):
    vertices = _lib.dev_f32(vertices, "vertices", 3)
    if not isinstance(triangles, torch.Tensor):
        raise TypeError("triangles must be a torch.Tensor")
    triangles = _lib.dev_typed(triangles, "triangles", torch.int32)
    if vertices.dim() != 2 or triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.device != vertices.device:
        raise Mi3dError(f"vertices {tuple(vertices.shape)} and triangles {tuple(triangles.shape)} must be [nv, 3] and "
                        f"[nt, 3] on one device")
    if vertices.shape[0] > MAX_COUNT or triangles.shape[0] > MAX_COUNT:
        raise Mi3dError(f"{vertices.shape[0]} vertices / {triangles.shape[0]} triangles do not fit int32 indices")
    return vertices, triangles


def _check_keep_rule(min_faces, min_diagonal, largest):
    return (_integer(min_faces, "min_faces", 0, 2 ** 32 - 1), _real(min_diagonal, "min_diagonal", 0.0, _INF),
            _flag(largest, "largest"))


def _label_components(vertices, triangles):
    """mi3d_mesh_components on the current stream: (label, faces, box_min, box_max, counts), nothing read back."""
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    label = torch.empty(nv, dtype=torch.int32, device=dev)
    faces = torch.empty(nv, dtype=torch.int32, device=dev)
    box_min = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    box_max = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    _lib.launch("mi3d_mesh_components", vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, _lib.ptr(label),
                _lib.ptr(faces), _lib.ptr(box_min), _lib.ptr(box_max), _lib.ptr(counts))
    return label, faces, box_min, box_max, counts


def _check_counts(counts, nv, nt):
    """`counts` as a host list: refuses what include/mi3d.h Part 13 counts instead of dropping silently."""
    if counts[2] != 0:
        raise Mi3dError(f"{counts[2]} of the {nt} triangles hold a vertex index outside [0, {nv})")
    if counts[3] != 0:
        raise Mi3dError(f"mesh components: {counts[3]} threads gave up after more than {nv + 1} steps on a parent chain "
                        f"(the labelling is invalid: a bug, or the buffers changed during the call)")


def components(vertices, triangles):
    """The connected components of an indexed mesh (include/mi3d.h Part 13): vertices float32 [nv, 3], triangles int32
    [nt, 3] on the GPU.  Returns (label int32 [nv], faces int32 [nv], box_min float32 [nv, 3], box_max float32 [nv, 3]) on
    the same device: label[v] is the smallest vertex index connected to v; faces and the box of a component stand in the
    row of its label vertex, every other row holds 0.  A triangle index outside [0, nv) raises Mi3dError."""
    vertices, triangles = _check_mesh(vertices, triangles)
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    label, faces, box_min, box_max, counts = _label_components(vertices, triangles)
    if nv or nt:
        _check_counts(counts.tolist(), nv, nt)
    return label, faces, box_min, box_max


def _clean(vertices, triangles, min_faces, min_diagonal, largest):
    """clean() behind its argument checks; also returns the host copy of `counts`."""
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    if nv == 0 and nt == 0:
        return _outputs(0, 0, 0, dev) + ([0] * 8,)
    label, faces, box_min, box_max, counts = _label_components(vertices, triangles)
    ws, ws_bytes = _workspace(dev, "mi3d_mesh_components_workspace", nv, nt)
    _lib.launch("mi3d_mesh_clean_count", vertices, _lib.ptr(triangles), nv, nt, _lib.ptr(label), _lib.ptr(faces),
                _lib.ptr(box_min), _lib.ptr(box_max), min_faces, min_diagonal, int(largest), _lib.ptr(ws), ws_bytes,
                _lib.ptr(counts))
    host = counts.tolist()                                   # the one host read a clean needs
    _check_counts(host, nv, nt)
    kv, kt = host[:2]
    out_v, out_t, vertex_map = _outputs(kv, kt, nv, dev)
    _lib.launch("mi3d_mesh_clean_emit", vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, _lib.ptr(label),
                _lib.ptr(ws), ws_bytes, _lib.ptr(counts), _lib.ptr(out_v), kv, _lib.ptr(out_t), kt, _lib.ptr(vertex_map))
    return out_v, out_t, vertex_map, host


def clean(vertices, triangles, min_faces=0, min_diagonal=0.0, largest=False):
    """Drops the floaters of an indexed mesh by the keep rule of include/mi3d.h Part 13: a connected component stays iff it
    has at least one face, at least `min_faces` faces and a bounding-box diagonal of at least `min_diagonal` (equality
    keeps); with `largest=True` only the component with the most faces can stay (ties: the smaller label).  vertices
    float32 [nv, 3], triangles int32 [nt, 3] on the GPU.  Returns (vertices, triangles, vertex_map int32 [nv]) on the same
    device: what is kept, in its original relative order, the triangles renumbered; vertex_map is the new index of every
    old vertex, -1 for a dropped one.  Nothing kept gives [0, 3] tensors.  A triangle index outside [0, nv) raises
    Mi3dError."""
    vertices, triangles = _check_mesh(vertices, triangles)
    min_faces, min_diagonal, largest = _check_keep_rule(min_faces, min_diagonal, largest)
    return _clean(vertices, triangles, min_faces, min_diagonal, largest)[:3]


# decimate factors (cluster cell in grid steps) export_mesh tries for `target_faces`, from the fine end; multiples of 0.5
DECIMATE_LADDER = (1.5, 2, 2.5, 3, 3.5, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64)
SIMPLIFY_COUNTS = ("vertices", "triangles", "bad_triangles", "gave_up", "non_finite_vertices", "clusters", "degenerate",
                   "duplicate")                              # counts[0 .. 7] of include/mi3d.h Part 14


def _check_positive(x, name):
    """A finite number > 0 that is still finite and > 0 as a binary32; returns it as a float."""
    if not _is_number(x):
        raise Mi3dError(f"{name} must be a number (got {x!r})")
    with np.errstate(over="ignore"):
        x32 = float(np.float32(x))
    if not (np.isfinite(x32) and x32 > 0.0):
        raise Mi3dError(f"{name} must be finite and > 0, as a float32 too (got {x!r})")
    return float(x)


def _simplify_count(vertices, triangles, origin, cell):
    """mi3d_mesh_simplify_count on the current stream and the one host read: (state for _simplify_emit, counts as a
    list).  `origin` 3 floats, `cell` a float; both are rounded to binary32 here."""
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    ws, ws_bytes = _workspace(dev, "mi3d_mesh_simplify_workspace", nv, nt, 0)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    org = (C.c_float * 3)(*[float(o) for o in origin])
    cell = float(np.float32(cell))
    _lib.launch("mi3d_mesh_simplify_count", vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, org, cell,
                _lib.ptr(ws), ws_bytes, _lib.ptr(counts))
    host = counts.tolist()                                   # the one host read a simplification needs
    if host[3] != 0:
        raise Mi3dError(f"mesh simplify: {host[3]} threads gave up after probing every slot of a table (the result is "
                        f"invalid: a bug, or the buffers changed during the call)")
    return (ws, ws_bytes, org, cell), host


def _simplify_emit(vertices, triangles, state, host):
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    ws, ws_bytes, org, cell = state
    kv, kt = host[:2]
    out_v, out_t, vertex_map = _outputs(kv, kt, nv, dev)
    lost = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.launch("mi3d_mesh_simplify_emit", vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, org, cell,
                _lib.ptr(ws), ws_bytes, _lib.ptr(out_v), kv, _lib.ptr(out_t), kt, _lib.ptr(vertex_map), _lib.ptr(lost))
    return out_v, out_t, vertex_map


def _check_simplify_counts(host, nv, nt):
    """Refuses what include/mi3d.h Part 14 counts instead of dropping silently."""
    if host[4] != 0 or host[2] != 0:
        raise Mi3dError(f"mesh simplify: {host[4]} of the {nv} vertices have a non-finite coordinate and {host[2]} of the "
                        f"{nt} triangles hold a vertex index outside [0, {nv}) or cite such a vertex")


def simplify(vertices, triangles, cell, origin=None, return_stats=False):
    """Vertex clustering by the contract of include/mi3d.h Part 14: the vertices in one cell of the lattice `origin` +
    `cell` * Z^3 become one vertex at their mean position; triangles that lose a corner (degenerate) or repeat an earlier
    one's three clusters (duplicate) are dropped.  vertices float32 [nv, 3], triangles int32 [nt, 3] on the GPU; `cell` a
    finite number > 0 (checked first, on any device); `origin` 3 numbers, None: the smallest finite coordinate per axis
    (`vertices.amin(0)`).  Returns (vertices [kv, 3], triangles [kt, 3], vertex_map int32 [nv]) on the same device - the
    clusters a surviving triangle cites in ascending order of their smallest member, the surviving triangles in their
    original order, renumbered; vertex_map is the new index of every old vertex's cluster, -1 where it was dropped - and,
    with `return_stats=True`, a dict of the counts named in SIMPLIFY_COUNTS.  Nothing surviving gives [0, 3] tensors.
    The output may have non-manifold edges and vertices; nothing repairs them.  A triangle index outside [0, nv) or a
    non-finite vertex raises Mi3dError."""
    cell = _check_positive(cell, "cell")
    vertices, triangles = _check_mesh(vertices, triangles)
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    if origin is None:
        if nv:
            inf = torch.full_like(vertices, float("inf"))
            lo = torch.where(torch.isfinite(vertices), vertices, inf).amin(0)
            origin = [o if np.isfinite(o) else 0.0 for o in lo.tolist()]
        else:
            origin = [0.0, 0.0, 0.0]
    else:
        origin = [float(o) for o in np.asarray(origin, dtype=np.float32).reshape(-1)]
        if len(origin) != 3 or not all(np.isfinite(o) for o in origin):
            raise Mi3dError(f"origin must be 3 finite numbers (got {origin!r})")
    if nv == 0 and nt == 0:
        out = _outputs(0, 0, 0, dev)
        return out + (dict(zip(SIMPLIFY_COUNTS, [0] * 8)),) if return_stats else out
    state, host = _simplify_count(vertices, triangles, origin, cell)
    _check_simplify_counts(host, nv, nt)
    out = _simplify_emit(vertices, triangles, state, host)
    return out + (dict(zip(SIMPLIFY_COUNTS, host)),) if return_stats else out


def export_lattice(R, d):
    """The lattice export_mesh clusters on for `decimate=d` at resolution R: (origin, cell) as binary32 values.  The cell
    is d grid steps h = 2 / (R - 1); the origin lies a QUARTER step below the grid's corner, so that no grid plane - where
    two of a marching-cubes vertex's three coordinates lie exactly - meets a cell boundary for any d that is a multiple
    of 0.5, and rounding noise decides no cluster."""
    h = 2.0 / (R - 1)
    o = np.float32(-1.0) - np.float32(h) / np.float32(4.0)
    return (float(o),) * 3, float(np.float32(d * h))


def _check_decimate(decimate, target_faces):
    if decimate is not None and target_faces is not None:
        raise Mi3dError("decimate and target_faces are mutually exclusive: give one of them")
    if decimate is not None:
        decimate = _check_positive(decimate, "decimate")
    if target_faces is not None:
        target_faces = _integer(target_faces, "target_faces", 1, 2 ** 63 - 1)
    return decimate, target_faces


def _decimate(vertices, triangles, R, decimate, target_faces):
    """export's simplify step: `decimate=d` clusters at d grid steps; `target_faces=N` walks DECIMATE_LADDER from the fine
    end with the count phase alone (one host read per rung) and emits the first rung with at most N faces."""
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    if target_faces is not None:
        if nt <= target_faces:
            return vertices, triangles
        left = nt
        for d in DECIMATE_LADDER:
            origin, cell = export_lattice(R, d)
            state, host = _simplify_count(vertices, triangles, origin, cell)
            _check_simplify_counts(host, nv, nt)
            if 0 < host[1] <= target_faces:
                break
            if host[1] == 0:                                    # no mesh is no answer; coarser cells leave no more
                raise Mi3dError(f"export_mesh: target_faces={target_faces} is not reached: decimate={d:g} leaves no "
                                f"triangle, and the rung before it {left} of the {nt}")
            left = host[1]
        else:
            raise Mi3dError(f"export_mesh: target_faces={target_faces} is not reached: decimate={DECIMATE_LADDER[-1]}, "
                            f"the coarsest rung, leaves {left} of the {nt} triangles")
    else:
        d = decimate
        origin, cell = export_lattice(R, d)
        state, host = _simplify_count(vertices, triangles, origin, cell)
        _check_simplify_counts(host, nv, nt)
    if host[0] == 0 or host[1] == 0:
        raise Mi3dError(f"export_mesh: nothing survives decimate={d:g}: the {nv} vertices fall into {host[5]} clusters, "
                        f"{host[6]} of the {nt} triangles are degenerate and {host[7]} duplicates")
    return _simplify_emit(vertices, triangles, state, host)[:2]


# Taubin's published pair (G. Taubin, "A signal processing approach to fair surface design", SIGGRAPH 1995: lambda = 0.5,
# mu = -0.53, a pass band just above 0.1).  Nobody has measured them against alternatives on this project's meshes.
SMOOTH_LAMBDA, SMOOTH_MU = 0.5, -0.53
SMOOTH_MAX_ITERATIONS, SMOOTH_MAX_FRACTION_BITS = 1000, 40
SMOOTH_COUNTS = ("unusable_triangles", "non_finite_vertices", "isolated_vertices", "border_vertices",
                 "over_degree_vertices", "clamped_vertices", "errors")   # counts[0 .. 6] of include/mi3d.h Part 16
SMOOTH_KEYS = ("iterations", "lam", "mu", "pin_border", "max_move")


def _check_smooth(iterations, lam=SMOOTH_LAMBDA, mu=SMOOTH_MU, pin_border=True, max_move=None):
    """The arguments of smooth() that need no tensor: (iterations, lam, mu, pin_border, max_move as a float or None)."""
    return (_integer(iterations, "iterations", 1, SMOOTH_MAX_ITERATIONS),
            _real(lam, "lam", -1.0, 1.0), _real(mu, "mu", -1.0, 1.0),     # binary64, as the kernels take them
            _flag(pin_border, "pin_border"), _real(max_move, "max_move", 0.0, _INF, none=True))


def smooth_fraction_bits(extent):
    """The fraction bits e of include/mi3d.h Part 16 for coordinates up to `extent` in magnitude: the largest e <= 40
    with extent * 2^e <= 2^38, so that a coordinate may grow fourfold before its fixed-point image saturates."""
    extent = _real(extent, "extent", 0.0, float(np.finfo(np.float64).max))      # finite
    exponent = int(np.frexp(extent)[1]) if extent > 0.0 else -SMOOTH_MAX_FRACTION_BITS   # extent <= 2^exponent
    return min(max(38 - exponent, 0), SMOOTH_MAX_FRACTION_BITS)


def smooth(vertices, triangles, iterations, lam=SMOOTH_LAMBDA, mu=SMOOTH_MU, pin_border=True, max_move=None, extent=None,
           return_stats=False):
    """Taubin smoothing by the contract of include/mi3d.h Part 16: `iterations` times a pass that moves every vertex
    towards the mean of its umbrella by `lam`, then one by `mu` (negative: the pass that undoes the shrinkage; mu=0:
    plain Laplacian smoothing, which shrinks).  vertices float32 [nv, 3], triangles int32 [nt, 3] on the GPU.
    `pin_border=True` keeps the vertices on an open edge where they are; `max_move` (a number >= 0, None: no limit) keeps
    every coordinate within that distance of its input value.  `extent` (finite, >= 0) bounds |coordinate| and fixes the
    fixed-point scale of the neighbour sums (smooth_fraction_bits); None reads `|vertices|.amax()` of the finite
    coordinates from the device - the one host read; with `extent` given nothing is read.  Returns the new vertices
    float32 [nv, 3] on the same device and, with `return_stats=True` (one more host read), a dict of the counts named in
    SMOOTH_COUNTS; a non-zero `errors` raises Mi3dError then.  Triangles with an index outside [0, nv), a repeated index
    or a non-finite vertex take no part (they are counted, not refused); vertices no usable triangle cites, and those
    with more than 1024 triangles, stay where they are.  The defaults lam=0.5, mu=-0.53 are Taubin's published pair, not
    measured on this project's meshes.  The arguments are checked first, on any device."""
    iterations, lam, mu, pin_border, max_move = _check_smooth(iterations, lam, mu, pin_border, max_move)
    e = None if extent is None else smooth_fraction_bits(extent)
    vertices, triangles = _check_mesh(vertices, triangles)
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    out = torch.empty_like(vertices)
    if nv == 0:
        return (out, dict(zip(SMOOTH_COUNTS, [0] * len(SMOOTH_COUNTS)))) if return_stats else out
    if e is None:
        mag = torch.where(torch.isfinite(vertices), vertices.abs(), torch.zeros_like(vertices)).amax()
        e = smooth_fraction_bits(float(mag))                    # the one host read
    ws, ws_bytes = _workspace(dev, "mi3d_mesh_smooth_workspace", nv, nt, what="a smoothing")
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    _lib.launch("mi3d_mesh_smooth", vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, iterations, lam, mu,
                int(pin_border), float("inf") if max_move is None else max_move, e, _lib.ptr(ws), ws_bytes, _lib.ptr(out),
                _lib.ptr(counts))
    if not return_stats:
        return out
    stats = dict(zip(SMOOTH_COUNTS, counts.tolist()))
    if stats["errors"] != 0:
        raise Mi3dError(f"mesh smooth: {stats['errors']} row slots could not be placed (the result is invalid: a bug, or "
                        f"the buffers changed during the call)")
    return out, stats


def _check_smooth_option(smooth):
    """export's `smooth`: None, an iteration count, or a dict of SMOOTH_KEYS -> the tuple _check_smooth returns."""
    if smooth is None:
        return None
    if isinstance(smooth, dict):
        unknown = sorted(set(smooth) - set(SMOOTH_KEYS))
        if unknown or "iterations" not in smooth:
            raise Mi3dError(f"smooth: unknown keys {unknown}; it takes {SMOOTH_KEYS}, and iterations is required")
        return _check_smooth(**smooth)
    return _check_smooth(smooth)


def _smooth_export(vertices, triangles, smoothing, h):
    """export's smoothing step: the vertices lie in [-1, 1]^3 (extent 1: nothing is read for the scale), `max_move` counts
    grid steps h; the counts are read once, so that an inconsistency raises."""
    iterations, lam, mu, pin_border, max_move = smoothing
    if max_move is not None:
        max_move = float(np.float32(max_move * h))
    return smooth(vertices, triangles, iterations, lam=lam, mu=mu, pin_border=pin_border, max_move=max_move, extent=1.0,
                  return_stats=True)[0]


COLLAPSE_COUNTS = ("vertices", "triangles", "unusable_triangles", "rounds", "non_finite_vertices", "collapses",
                   "locked_vertices", "errors")             # counts[0 .. 7] of include/mi3d.h Part 19
COLLAPSE_KEYS = ("target_faces", "max_error", "max_rounds")
COLLAPSE_MAX_ROUNDS, COLLAPSE_ROUNDS_PER_CALL = 1 << 20, 4096


def _check_collapse(target_faces, max_error=None, max_rounds=256, rounds_per_read=8):
    """The arguments of collapse() that need no tensor: (target_faces, max_error as a float or None, max_rounds,
    rounds_per_read)."""
    target_faces = _integer(target_faces, "target_faces", 0, 2 ** 63 - 1)
    max_rounds = _integer(max_rounds, "max_rounds", 0, COLLAPSE_MAX_ROUNDS)
    rounds_per_read = _integer(rounds_per_read, "rounds_per_read", 1, COLLAPSE_ROUNDS_PER_CALL)
    max_error = _real(max_error, "max_error", 0.0, _INF, none=True)
    if max_error is not None:
        with np.errstate(over="ignore"):
            max_error = float(np.float32(max_error))            # binary32, as the kernels take it
    return target_faces, max_error, max_rounds, rounds_per_read


def collapse(vertices, triangles, target_faces, max_error=None, max_rounds=256, rounds_per_read=8, return_stats=False):
    """Decimation to `target_faces` faces by quadric edge collapse, the contract of include/mi3d.h Part 19: rounds of
    independent collapses, each of an interior edge whose removal keeps the surface manifold and flips no triangle, the
    new vertex at the point of least quadric error among the two ends, the midpoint and (where the quadric is well
    conditioned) its optimum.  vertices float32 [nv, 3], triangles int32 [nt, 3] on the GPU.  `max_error` (a number
    >= 0, None: no limit) bounds the quadric error of a collapse; at most `max_rounds` rounds run, `rounds_per_read` of
    them between two host reads of the counts.  Vertices on an open edge and vertices of more than 64 triangles stay
    where they are.  Returns (vertices [kv, 3], triangles [kt, 3], vertex_map int32 [nv]) on the same device - the
    surviving triangles in their original order and corner order, renumbered; the vertices they cite in ascending
    original index; vertex_map the new index of the vertex every old vertex was collapsed into, -1 where that is not
    emitted - and, with `return_stats=True`, a dict of the counts named in COLLAPSE_COUNTS (`unusable_triangles` without
    the planeless ones, which stand in `planeless_triangles`) plus `rounds_launched`, `done` (the face count is at or
    below the target) and `stalled` (a round found no collapse above the target: not an error).  A closed mesh that does
    not stall ends on `target_faces` or one face less.  Triangles with an index outside [0, nv), a repeated index or a
    non-finite vertex are counted and dropped.  The arguments are checked first, on any device."""
    target, max_error, max_rounds, per_read = _check_collapse(target_faces, max_error, max_rounds, rounds_per_read)
    vertices, triangles = _check_mesh(vertices, triangles)
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    if nv == 0 and nt == 0:
        out = _outputs(0, 0, 0, dev)
        stats = dict(zip(COLLAPSE_COUNTS, [0] * 8), planeless_triangles=0, rounds_launched=0, done=True, stalled=False)
        return out + (stats,) if return_stats else out
    ws, ws_bytes = _workspace(dev, "mi3d_mesh_collapse_workspace", nv, nt, what="a collapse")
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    limit = float("inf") if max_error is None else max_error
    _lib.launch("mi3d_mesh_collapse_begin", vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, _lib.ptr(ws),
                ws_bytes, _lib.ptr(counts))
    launched, over = 0, False
    while launched < max_rounds and not over:
        n = min(per_read, max_rounds - launched)
        _lib.launch("mi3d_mesh_collapse_rounds", vertices, nv, nt, target, limit, n, _lib.ptr(ws), ws_bytes,
                    _lib.ptr(counts))
        launched += n
        host = counts.tolist()                                  # one host read per batch of rounds
        over = host[3] < launched                               # a round was a no-op or found no winner: so is every later one
    _lib.launch("mi3d_mesh_collapse_count", vertices, nv, nt, _lib.ptr(ws), ws_bytes, _lib.ptr(counts))
    host = counts.tolist()                                      # the read that sizes the output
    kv, kt = host[:2]
    out_v, out_t, vertex_map = _outputs(kv, kt, nv, dev)
    _lib.launch("mi3d_mesh_collapse_emit", vertices, nv, nt, _lib.ptr(ws), ws_bytes, _lib.ptr(out_v), kv, _lib.ptr(out_t),
                kt, _lib.ptr(vertex_map), _lib.ptr(counts))
    if not return_stats:
        return out_v, out_t, vertex_map
    host = counts.tolist()
    if host[7] != 0:
        raise Mi3dError(f"mesh collapse: {host[7]} slots could not be placed (the result is invalid: a bug, or the "
                        f"buffers changed during the call)")
    stats = dict(zip(COLLAPSE_COUNTS, host))
    stats["planeless_triangles"], stats["unusable_triangles"] = host[2] >> 32, host[2] & 0xFFFFFFFF
    stats["rounds_launched"], stats["done"] = launched, kt <= target
    stats["stalled"] = kt > target and host[3] < launched
    return out_v, out_t, vertex_map, stats


def _check_collapse_option(collapse):
    """export's `collapse`: None, a face count >= 1, or a dict of COLLAPSE_KEYS -> (target_faces, max_error, max_rounds)."""
    if collapse is None:
        return None
    if isinstance(collapse, dict):
        unknown = sorted(set(collapse) - set(COLLAPSE_KEYS))
        if unknown or "target_faces" not in collapse:
            raise Mi3dError(f"collapse: unknown keys {unknown}; it takes {COLLAPSE_KEYS}, and target_faces is required")
        checked = _check_collapse(**collapse)[:3]
    else:
        checked = _check_collapse(collapse)[:3]
    if checked[0] < 1:
        raise Mi3dError(f"collapse: target_faces must be >= 1 (got {checked[0]})")
    return checked


def _collapse_export(vertices, triangles, collapsing):
    """export's collapse step; the counts are read, so that an inconsistency raises."""
    target, max_error, max_rounds = collapsing
    out_v, out_t, _, stats = collapse(vertices, triangles, target, max_error=max_error, max_rounds=max_rounds,
                                      return_stats=True)
    if out_v.shape[0] == 0 or out_t.shape[0] == 0:
        raise Mi3dError(f"export_mesh: nothing survives collapse: {stats['unusable_triangles']} of the "
                        f"{triangles.shape[0]} triangles are unusable")
    return out_v, out_t


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


MIN_TEXTURE, MAX_TEXTURE = 64, 16384
SSAA = (1, 2, 4)


def atlas_cell(nt, texture_size):
    """The cell size c of include/mi3d.h Part 9 for `nt` triangles in a texture_size^2 atlas; 0 if they do not fit."""
    nt, T = int(nt), int(texture_size)
    if nt < 0 or not 0 <= T < 2 ** 32:
        return 0
    return int(_lib.lib().mi3d_atlas_cell(nt, T))


def _check_texture(texture_size, ssaa):
    if isinstance(texture_size, bool) or int(texture_size) != texture_size:
        raise Mi3dError(f"texture_size must be an integer (got {texture_size!r})")
    if not MIN_TEXTURE <= int(texture_size) <= MAX_TEXTURE:
        raise Mi3dError(f"texture_size must lie in [{MIN_TEXTURE}, {MAX_TEXTURE}] (got {texture_size})")
    if ssaa not in SSAA:
        raise Mi3dError(f"ssaa must be one of {SSAA} (got {ssaa!r})")
    return int(texture_size), int(ssaa)


def _fitting_cell(nt, T):
    c = atlas_cell(nt, T)
    if c == 0:
        fit = next((t for t in (1 << k for k in range(6, 15)) if atlas_cell(nt, t) > 0), None)
        hint = f"the smallest power of two that fits is {fit}" if fit else f"no size up to {MAX_TEXTURE} fits"
        raise Mi3dError(f"{nt} triangles do not fit a {T} x {T} texture atlas: {hint}")
    return c


ATLASES = ("uniform", "adaptive")
PLAN_WORDS = 3472                                    # MI3D_ATLAS_PLAN_WORDS
ATLAS_LEGS = (2, 3, 4, 6, 8, 11, 16, 23, 32, 45, 64, 91, 128, 181, 256, 362)


def _check_atlas(atlas, texture_size=0):
    if not isinstance(atlas, str) or atlas not in ATLASES:
        raise Mi3dError(f"atlas must be one of {ATLASES} (got {atlas!r})")
    if atlas == "adaptive" and texture_size is None:
        raise Mi3dError('atlas="adaptive" lays out a texture: give texture_size too')
    return atlas


def atlas_adaptive_plan(hist, texture_size):
    """The host plan of include/mi3d.h Part 20 for a 64 x 64 bin histogram (indexed [binAC, binAB]) and a texture size:
    the int32 [PLAN_WORDS] array in the header's layout, or None if no shift fits.  Host arithmetic: no GPU."""
    hist = np.ascontiguousarray(np.asarray(hist).reshape(-1))
    if hist.shape != (4096,) or hist.dtype.kind not in "iu" or (hist < 0).any() or (hist > 2 ** 32 - 1).any():
        raise Mi3dError("hist must hold 64 x 64 counts below 2^32")
    T = int(texture_size)
    if not 0 <= T < 2 ** 32:
        return None
    hist = hist.astype(np.uint32)
    words = np.empty(PLAN_WORDS, np.int32)
    ok = _lib.lib().mi3d_atlas_adaptive_plan(hist.ctypes.data, T, words.ctypes.data)
    return words if ok else None


def _plan_dict(words):
    recs = words[144:144 + 12 * int(words[5])].reshape(-1, 12)
    classes = np.zeros((16, 16), np.int64)               # [kb, ka]
    classes[recs[:, 0] // 16, recs[:, 0] % 16] = recs[:, 7]
    T = int(words[1])
    return {"shift": int(words[0]), "texture_size": T, "kmax": int(words[2]), "rows": int(words[3]),
            "fill": int(words[7]) / float(T * T), "classes": classes, "clamped_small": int(words[8]),
            "clamped_large": int(words[9])}


def _fitting_plan(hist, nt, T):
    words = atlas_adaptive_plan(hist, T)
    if words is None:
        fit = next((t for t in (1 << k for k in range(6, 15)) if atlas_adaptive_plan(hist, t) is not None), None)
        hint = f"the smallest power of two that fits is {fit}" if fit else f"no size up to {MAX_TEXTURE} fits"
        raise Mi3dError(f"{nt} triangles do not fit a {T} x {T} adaptive texture atlas: {hint}")
    return words


class _AdaptiveAtlas:
    """Steps 1 and 2 of include/mi3d.h Part 20 for a mesh: the shape words, the histogram read back (the first host read),
    the plan on the host and on the device, the bad-triangle counter (read at the end of a bake)."""

    def __init__(self, vertices, triangles, T):
        nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
        self.T, self.nt = T, nt
        self.shape = torch.empty(nt, dtype=torch.int32, device=dev)
        hist = torch.zeros(4096, dtype=torch.int32, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.launch("mi3d_atlas_adaptive_measure", vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt,
                    _lib.ptr(self.shape), _lib.ptr(hist), _lib.ptr(self.bad))
        self.hist = hist.cpu().numpy().view(np.uint32)
        self.words = _fitting_plan(self.hist, nt, T)
        self.plan = torch.from_numpy(self.words).to(dev)

    def layout(self):
        """Steps 3 and 4: (slot, triangle_of, vt)."""
        dev, nt = self.shape.device, self.nt
        ws, ws_bytes = _workspace(dev, "mi3d_atlas_adaptive_workspace", nt)
        slot = torch.empty(nt, dtype=torch.int32, device=dev)
        triangle_of = torch.empty(nt, dtype=torch.int32, device=dev)
        vt = torch.empty(3 * nt, 2, dtype=torch.float32, device=dev)
        _lib.launch("mi3d_atlas_adaptive_sort", vt, _lib.ptr(self.shape), nt, _lib.ptr(self.plan), _lib.ptr(ws), ws_bytes,
                    _lib.ptr(slot), _lib.ptr(triangle_of))
        _lib.launch("mi3d_atlas_adaptive_uv", vt, _lib.ptr(self.shape), _lib.ptr(slot), nt, _lib.ptr(self.plan), self.T,
                    _lib.ptr(vt))
        return slot, triangle_of, vt


def _atlas_state(vertices, triangles, T, atlas):
    """What _bake_bands lays the texture out by: the cell size of the uniform atlas, or the measured and planned
    adaptive one.  A mesh that does not fit raises here, before any colour is evaluated."""
    if atlas == "adaptive":
        return _AdaptiveAtlas(vertices, triangles, T)
    return _fitting_cell(int(triangles.shape[0]), T)


def atlas_plan(vertices, triangles, texture_size):
    """What atlas="adaptive" would do with this mesh at this texture size (include/mi3d.h Part 20), without baking: a
    dict with `shift` (the chosen s: every leg gets LEGS[bin - s] texel intervals), `rows` (image rows used of
    texture_size), `fill` (owned texels / texture_size^2), `classes` (int64 [16, 16], triangles per class, indexed
    [class of A'C', class of A'B']), `clamped_small` / `clamped_large` (legs whose bin - s lies below 0 / above `kmax`:
    they get more / fewer texels per unit length than the rest) and `kmax`, `texture_size`.  The shift moves in steps
    of sqrt 2 in length, so `rows` can end well short of texture_size.  A mesh that does not fit raises Mi3dError naming
    the smallest power of two that does.  One kernel (the measure) and one host read."""
    T, _ = _check_texture(texture_size, 1)
    vertices, triangles = _check_bake_mesh(vertices, triangles, "atlas_plan")
    return _plan_dict(_AdaptiveAtlas(vertices, triangles, T).words)


def bake_texture(model, vertices, triangles, texture_size, ssaa=1, atlas="uniform"):
    """The albedo of `model` baked into the per-triangle atlas of include/mi3d.h Part 9.  vertices float32 [nv, 3] and
    triangles int32 [nt, 3] on the GPU (what marching_cubes returns).  Returns (image uint8 [T, T, 3], vt float32
    [3 nt, 2], owner int32 [T, T]) on the same device; image row 0 is the top row, vt of triangle i are rows 3 i .. 3 i + 2.
    The texels are evaluated in bands of image rows of at most CHUNK points; bands below the last owned texel are not.

    atlas="adaptive" lays the patches out by include/mi3d.h Part 20 instead: a triangle's patch has legs that follow its
    two shorter edges, so that texels per unit length differ by less than a factor 1.6 over all legs that are not
    clamped (atlas_plan reports those) - the atlas for a mesh after collapse or decimation, whose triangles differ in
    size by orders of magnitude.  On a mesh of very many tiny triangles every leg ends at the smallest class and the
    uniform atlas is the better choice.  Same return value, same formats."""
    T, ssaa = _check_texture(texture_size, ssaa)
    atlas = _check_atlas(atlas)
    vertices, triangles = _check_bake_mesh(vertices, triangles, "bake_texture")
    return _bake_bands(vertices, triangles, T, ssaa, lambda xyz, owner, row0, rows: _field_albedo(model, xyz),
                       _atlas_state(vertices, triangles, T, atlas))


def _check_bake_mesh(vertices, triangles, who):
    vertices, triangles = _check_mesh(vertices, triangles)
    if vertices.shape[0] == 0 or triangles.shape[0] == 0:
        raise Mi3dError(f"{who} needs a mesh (got no vertices or no triangles)")
    return vertices, triangles


def _field_albedo(model, xyz):
    albedo = model.density(xyz)["albedo"].float().contiguous()
    if albedo.shape != xyz.shape:
        raise Mi3dError(f"model.density returned albedo {tuple(albedo.shape)} for points {tuple(xyz.shape)}")
    return albedo


def _bake_bands(vertices, triangles, T, ssaa, colour, state=None):
    """The band loop the two bakes share: mi3d_atlas_uv, then per band of image rows mi3d_atlas_positions,
    `colour(xyz, owner_band, row0, rows)` -> float32 [rows T ssaa^2, 3], and mi3d_texture_pack; the one host read (the
    bad-triangle counter) at the end.  Returns (image, vt, owner).  `state`: what _atlas_state returned (None: the
    uniform atlas); with an adaptive one the sort, mi3d_atlas_adaptive_uv and mi3d_atlas_adaptive_positions take the
    places of Part 9's two kernels."""
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    adaptive = isinstance(state, _AdaptiveAtlas)
    c = None if adaptive else _fitting_cell(nt, T) if state is None else state
    dev, ss2 = vertices.device, ssaa * ssaa
    image = torch.zeros(T, T, 3, dtype=torch.uint8, device=dev)
    owner = torch.full((T, T), -1, dtype=torch.int32, device=dev)
    if adaptive:
        bad = state.bad
        _, triangle_of, vt = state.layout()
        used = int(state.words[3])
    else:
        vt = torch.empty(3 * nt, 2, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.launch("mi3d_atlas_uv", vt, nt, T, _lib.ptr(vt))
        cols = T // (c + 1)
        used = -(-((nt + 1) // 2) // cols) * c          # image rows down to the last cell row that holds a triangle
    band = max(4, CHUNK // (T * ss2) // 4 * 4)          # a multiple of 4 rows: every band starts on a 32-bit word
    with torch.no_grad():
        for row0 in range(0, used, band):
            rows = min(band, used - row0)
            xyz = torch.empty(rows * T * ss2, 3, dtype=torch.float32, device=dev)
            if adaptive:
                _lib.launch("mi3d_atlas_adaptive_positions", xyz, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt,
                            _lib.ptr(state.shape), _lib.ptr(triangle_of), _lib.ptr(state.plan), T, ssaa, row0, rows,
                            _lib.ptr(xyz), _lib.ptr(owner[row0]))
            else:
                _lib.launch("mi3d_atlas_positions", xyz, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, T, ssaa, row0,
                            rows, _lib.ptr(xyz), _lib.ptr(owner[row0]), _lib.ptr(bad))
            albedo = colour(xyz, owner[row0:row0 + rows], row0, rows)
            _lib.launch("mi3d_texture_pack", albedo, _lib.ptr(albedo), _lib.ptr(owner[row0]), T, ssaa, rows,
                        _lib.ptr(image[row0]))
    lost = int(bad)                                     # the one host read of a bake
    if lost != 0:
        raise Mi3dError(f"{lost} of the {nt} triangles hold a vertex index outside [0, {nv})")
    return image, vt, owner


MIN_VIEW_SIDE, MAX_VIEW_SIDE, MAX_VIEWS = 2, 16384, 64
POWERS = (2, 4, 8, 16)
VIEW_KEYS = ("images", "c2w", "K", "masks", "weights", "power", "min_cos", "depth_tol")


def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else tuple(np.shape(a))


def _host64(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64)


def view_records(c2w, K):
    """The float32 [V, 24] view records of include/mi3d.h Part 15 from camera-to-world matrices [V, 4, 4] and the shared
    intrinsics [3, 3] (last row 0 0 1): per view the rows of [R | t] of the world-to-camera matrix (the NumPy float64
    inverse, as pointcloud.build takes it), K, and the camera centre, each rounded once."""
    c2w, K = _host64(c2w), _host64(K)
    if c2w.ndim != 3 or c2w.shape[1:] != (4, 4) or not 1 <= c2w.shape[0] <= MAX_VIEWS:
        raise Mi3dError(f"c2w must be [V, 4, 4] with V in [1, {MAX_VIEWS}] (got {c2w.shape})")
    if K.shape != (3, 3):
        raise Mi3dError(f"K must be [3, 3] (got {K.shape})")
    if not (np.isfinite(c2w).all() and np.isfinite(K).all()):
        raise Mi3dError("c2w and K must be finite")
    if not np.array_equal(K[2], [0.0, 0.0, 1.0]):
        raise Mi3dError(f"the last row of K must be 0 0 1 (got {K[2].tolist()})")
    rec = np.empty((c2w.shape[0], 24), np.float64)
    for v, pose in enumerate(c2w):
        try:
            w2c = np.linalg.inv(pose)
        except np.linalg.LinAlgError:
            raise Mi3dError(f"c2w[{v}] is singular") from None
        rec[v] = np.concatenate([w2c[:3, :3].ravel(), w2c[:3, 3], K.ravel(), pose[:3, 3]])
    return rec.astype(np.float32)


def _check_view_size(V, H, W):
    if not 1 <= V <= MAX_VIEWS:
        raise Mi3dError(f"the number of views must lie in [1, {MAX_VIEWS}] (got {V})")
    if not (MIN_VIEW_SIDE <= H <= MAX_VIEW_SIDE and MIN_VIEW_SIDE <= W <= MAX_VIEW_SIDE):
        raise Mi3dError(f"H and W must lie in [{MIN_VIEW_SIDE}, {MAX_VIEW_SIDE}] (got {H} x {W})")


def check_views(images, c2w, K, masks=None, weights=None, power=4, min_cos=0.2, depth_tol=0.02):
    """Every view argument of bake_views, on the host, before anything is uploaded or launched.  Returns (records float32
    [V, 24], weights float32 [V], min_cos^2 as the binary32 product, depth_tol as a binary32, (V, H, W))."""
    s = _shape(images)
    if len(s) != 4 or s[3] != 3:
        raise Mi3dError(f"images must be [V, H, W, 3] (got {s})")
    V, H, W = s[:3]
    _check_view_size(V, H, W)
    if isinstance(images, torch.Tensor) and not images.dtype.is_floating_point or \
            not isinstance(images, torch.Tensor) and np.asarray(images).dtype.kind != "f":
        raise Mi3dError("images must be floating point, in [0, 1]")
    if _shape(c2w) != (V, 4, 4):
        raise Mi3dError(f"c2w must be [{V}, 4, 4] for images {s} (got {_shape(c2w)})")
    records = view_records(c2w, K)
    if masks is not None and _shape(masks) != (V, H, W):
        raise Mi3dError(f"masks must be [{V}, {H}, {W}] for images {s} (got {_shape(masks)})")
    if weights is None:
        weights = np.ones(V, np.float32)
    else:
        if _shape(weights) != (V,):
            raise Mi3dError(f"weights must be [{V}] for images {s} (got {_shape(weights)})")
        with np.errstate(over="ignore"):
            weights = _host64(weights).astype(np.float32)
        if not (np.isfinite(weights).all() and (weights >= 0).all()):
            raise Mi3dError(f"weights must be finite and >= 0, as float32 too (got {weights.tolist()})")
    if isinstance(power, (bool, np.bool_)) or power not in POWERS:
        raise Mi3dError(f"power must be one of {POWERS} (got {power!r})")
    min_cos = np.float32(_number(min_cos, "min_cos", 0.0, 1.0))
    depth_tol = _number(depth_tol, "depth_tol", 0.0, float(np.finfo(np.float32).max))
    return records, weights, float(min_cos * min_cos), depth_tol, (V, H, W)


def _check_views_dict(views):
    if not isinstance(views, dict):
        raise Mi3dError(f"views must be a dict with the keys {VIEW_KEYS[:3]} and optionally {VIEW_KEYS[3:]} (got "
                        f"{type(views).__name__})")
    unknown = sorted(set(views) - set(VIEW_KEYS) - {"fit"})
    missing = [k for k in VIEW_KEYS[:3] if k not in views]
    if unknown or missing:
        raise Mi3dError(f"views: unknown keys {unknown}, missing keys {missing}; it takes {VIEW_KEYS + ('fit',)}")
    views = dict(views)
    fit = views.pop("fit", None)
    check_views(**views)
    if fit is not None:
        if not isinstance(fit, dict) or set(fit) - set(FIT_KEYS):
            raise Mi3dError(f"views: fit must be a dict with keys among {FIT_KEYS} (got {fit!r})")
        fit = dict(zip(FIT_KEYS, _check_fit(fit.get("iterations", 200), fit.get("lr", 0.01))))
    return views, fit


def _to_dev(a, dtype, dev):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.detach().to(device=dev, dtype=dtype).contiguous()


def _mesh_depth(vertices, triangles, records, H, W):
    """mi3d_mesh_depth on the current stream: (depth float32 [V, H, W], counts int64 [2] on the device)."""
    dev, V = vertices.device, int(records.shape[0])
    depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.launch("mi3d_mesh_depth", vertices, _lib.ptr(vertices), int(vertices.shape[0]), _lib.ptr(triangles),
                int(triangles.shape[0]), _lib.ptr(records), V, H, W, _lib.ptr(depth), _lib.ptr(counts))
    return depth, counts


def render_depth(vertices, triangles, c2w, K, H, W, return_counts=False):
    """The depth maps of an indexed mesh from V pinhole cameras (include/mi3d.h Part 15): vertices float32 [nv, 3],
    triangles int32 [nt, 3] on the GPU; c2w [V, 4, 4] and K [3, 3] as pointcloud.build takes them, pixel centres at
    half-integers.  Returns depth float32 [V, H, W] on the same device: the camera-space z of the nearest surface at
    every pixel centre (back faces included), +inf where nothing is drawn.  Nothing is clipped: a triangle with a vertex
    at z <= 0 is left out of that view.  A triangle index outside [0, nv) raises Mi3dError - unless
    `return_counts=True`, which returns (depth, {"bad": .., "skipped": ..}) instead: the triangles with such an index,
    and the (triangle, view) pairs left out."""
    records = view_records(c2w, K)
    H, W = int(H), int(W)
    _check_view_size(records.shape[0], H, W)
    vertices, triangles = _check_mesh(vertices, triangles)
    depth, counts = _mesh_depth(vertices, triangles, torch.from_numpy(records).to(vertices.device), H, W)
    bad, skipped = counts.tolist()
    if return_counts:
        return depth, {"bad": bad, "skipped": skipped}
    if bad != 0:
        raise Mi3dError(f"{bad} of the {triangles.shape[0]} triangles hold a vertex index outside [0, {vertices.shape[0]})")
    return depth


def bake_views(model_or_base, vertices, triangles, texture_size, images, c2w, K, ssaa=1, masks=None, weights=None,
               power=4, min_cos=0.2, depth_tol=0.02, atlas="uniform"):
    """The atlas of bake_texture coloured from VIEWS by projection (include/mi3d.h Part 15): every atlas sample takes the
    weighted mean of the views that see it - inside the image, not behind a nearer surface of the mesh (the depth maps
    of render_depth, made once), inside the view's mask, and facing the camera with cos >= `min_cos` - each weighted
    by weights[v] * cos^power; a sample no view sees keeps the base colour.

    images float [V, H, W, 3] in [0, 1], c2w [V, 4, 4], K [3, 3] (pointcloud.build's conventions; what
    refine.render_views returns); masks [V, H, W] (non-zero: usable) and weights [V] (finite, >= 0) optional; NumPy or
    tensors.  `model_or_base`: a model, whose density(xyz)["albedo"] is the base, or a base colour of 3 numbers, or a
    float32 tensor [T, T, ssaa^2, 3] of per-sample base colours.  vertices and triangles as bake_texture takes them.
    Returns (image uint8 [T, T, 3], vt float32 [3 nt, 2], owner int32 [T, T], hits uint8 [T, T, ssaa^2]: the number of
    views that contributed to each sample).  Every argument is checked before anything is uploaded or launched.
    atlas="adaptive": the layout of include/mi3d.h Part 20 (see bake_texture) in place of Part 9's.

    The defaults power=4, min_cos=0.2 and depth_tol=0.02 (in world units, for an object in [-1, 1]^3) are choices
    nobody has measured against alternatives."""
    T, ssaa = _check_texture(texture_size, ssaa)
    atlas = _check_atlas(atlas)
    records, weights, min_cos2, depth_tol, (V, H, W) = check_views(images, c2w, K, masks, weights, power, min_cos,
                                                                   depth_tol)
    vertices, triangles = _check_bake_mesh(vertices, triangles, "bake_views")
    dev, ss2 = vertices.device, ssaa * ssaa
    state = _atlas_state(vertices, triangles, T, atlas)
    base = None
    if not hasattr(model_or_base, "density"):
        if _shape(model_or_base) == (3,):
            base = _to_dev(model_or_base, torch.float32, dev)
        elif isinstance(model_or_base, torch.Tensor) and _shape(model_or_base) == (T, T, ss2, 3):
            base = _lib.dev_f32(model_or_base, "base", 3)
        else:
            raise Mi3dError(f"model_or_base must be a model, 3 numbers or a float32 tensor [{T}, {T}, {ss2}, 3] (got "
                            f"{_shape(model_or_base)})")
    records = torch.from_numpy(records).to(dev)
    weights = torch.from_numpy(weights).to(dev)
    images = _to_dev(images, torch.float32, dev)
    if masks is not None:
        masks = (_to_dev(masks, torch.float32, dev) != 0).to(torch.uint8).contiguous()
    depth, _ = _mesh_depth(vertices, triangles, records, H, W)     # once, before the bands; a bad index raises below
    hits = torch.zeros(T, T, ss2, dtype=torch.uint8, device=dev)
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])

    def colour(xyz, owner, row0, rows):
        if base is None:
            b = _field_albedo(model_or_base, xyz)
        elif base.dim() == 1:
            b = base.expand(xyz.shape[0], 3).contiguous()
        else:
            b = base[row0:row0 + rows].reshape(-1, 3)
        out = torch.empty_like(xyz)
        _lib.launch("mi3d_texture_project", xyz, _lib.ptr(xyz), _lib.ptr(owner), _lib.ptr(vertices), nv,
                    _lib.ptr(triangles), nt, T, ssaa, rows, _lib.ptr(records), V, H, W, _lib.ptr(depth), _lib.ptr(images),
                    _lib.ptr(masks), _lib.ptr(weights), int(power), min_cos2, depth_tol, _lib.ptr(b), _lib.ptr(out),
                    _lib.ptr(hits[row0]))
        return out

    image, vt, owner = _bake_bands(vertices, triangles, T, ssaa, colour, state)
    return image, vt, owner, hits


SHADINGS = ("albedo", "lambertian", "textureless", "normal")
PREVIEW_KEYS = ("c2w", "K", "H", "W", "shading", "ssaa", "fidelity")


def _check_shading(shading, ssaa):
    if not isinstance(shading, str) or shading not in SHADINGS:
        raise Mi3dError(f"shading must be one of {SHADINGS} (got {shading!r})")
    if not _is_number(ssaa, integer=True) or ssaa not in SSAA:
        raise Mi3dError(f"ssaa must be one of {SSAA} (got {ssaa!r})")
    return shading, int(ssaa)


def _check_render_options(ambient_ratio, bg_color, light_d, V):
    """The arguments of render() that need no tensor: (ambient, background float32 [3], light [V, 3] float32 or None)."""
    ambient = _number(ambient_ratio, "ambient_ratio", 0.0, 1.0)
    bg = np.asarray(bg_color, dtype=np.float64).reshape(-1)
    if bg.size not in (1, 3) or not np.isfinite(bg).all():
        raise Mi3dError(f"bg_color must be one finite number or three (got {bg_color!r})")
    bg = np.broadcast_to(bg, (3,)).astype(np.float32)
    if light_d is not None:
        light_d = _host64(light_d)
        if light_d.shape not in ((3,), (V, 3)) or not np.isfinite(light_d).all() or not (light_d * light_d).sum(-1).all():
            raise Mi3dError(f"light_d must be 3 finite numbers or [{V}, 3], none of them a zero vector (got {light_d.shape})")
        light_d = np.broadcast_to(light_d / np.linalg.norm(light_d, axis=-1, keepdims=True), (V, 3)).astype(np.float32)
    return ambient, bg, light_d


def _render_buffers(vertices, triangles, records, H, W, colors=None, uvs=None, texture=None, normals=None,
                    bg=(1.0, 1.0, 1.0)):
    """mi3d_mesh_visibility and mi3d_mesh_shade on the current stream, nothing read back: a dict of vis int64 [V, H, W]
    (the uint64 keys), counts int64 [2], image float32 [V, H, W, 3], alpha uint8 [V, H, W], depth, tri int32, bary and
    normal (None without `normals`).  `records` float32 [V, 24] on the mesh's device; the arguments are checked by the
    callers."""
    vis, counts = _visibility(vertices, triangles, records, H, W)
    out = _shade(vertices, triangles, records, H, W, vis, colors, uvs, texture, normals, bg)
    out.update(vis=vis, counts=counts)
    return out


def _visibility(vertices, triangles, records, H, W):
    """mi3d_mesh_visibility on the current stream: (vis int64 [V, H, W], counts int64 [2]), nothing read back."""
    dev, V = vertices.device, int(records.shape[0])
    vis = torch.empty(V, H, W, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.launch("mi3d_mesh_visibility", vertices, _lib.ptr(vertices), int(vertices.shape[0]), _lib.ptr(triangles),
                int(triangles.shape[0]), _lib.ptr(records), V, H, W, _lib.ptr(vis), _lib.ptr(counts))
    return vis, counts


def _shade(vertices, triangles, records, H, W, vis, colors=None, uvs=None, texture=None, normals=None, bg=(1.0, 1.0, 1.0),
           image_only=False):
    """mi3d_mesh_shade - mi3d_mesh_shade_f32 for a float32 texture - from the keys `vis`: _render_buffers' dict without
    vis and counts; with `image_only` the image alone is written and the other entries are None."""
    dev, V = vertices.device, int(records.shape[0])
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])

    def buffer(*shape, dtype=torch.float32, wanted=True):
        return torch.empty(V, H, W, *shape, dtype=dtype, device=dev) if wanted else None

    out = dict(image=buffer(3), alpha=buffer(dtype=torch.uint8, wanted=not image_only), depth=buffer(wanted=not image_only),
               tri=buffer(dtype=torch.int32, wanted=not image_only), bary=buffer(3, wanted=not image_only),
               normal=buffer(3, wanted=normals is not None and not image_only))
    T = 0 if texture is None else int(texture.shape[0])
    background = (C.c_float * 3)(*[float(b) for b in bg])
    entry = "mi3d_mesh_shade_f32" if texture is not None and texture.dtype == torch.float32 else "mi3d_mesh_shade"
    _lib.launch(entry, vertices, _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, _lib.ptr(records), V, H, W,
                _lib.ptr(vis), _lib.ptr(colors), _lib.ptr(uvs), _lib.ptr(texture), T,
                _lib.ptr(normals if out["normal"] is not None else None), background, _lib.ptr(out["image"]),
                _lib.ptr(out["normal"]), _lib.ptr(out["depth"]), _lib.ptr(out["tri"]), _lib.ptr(out["bary"]),
                _lib.ptr(out["alpha"]))
    return out


def _shade_backward(vertices, triangles, records, H, W, vis, dimage, uvs, shape):
    """mi3d_mesh_shade_backward on the current stream: the gradient float32 of `shape` - [nv, 3] without `uvs`, [T, T, 3]
    with them - from dimage float32 [V, H, W, 3].  The workspace comes from torch's allocator; nothing is read back."""
    dev, V = vertices.device, int(records.shape[0])
    grad = torch.empty(shape, dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace(dev, "mi3d_mesh_shade_backward_workspace", grad.numel())
    textured = uvs is not None
    _lib.launch("mi3d_mesh_shade_backward", vertices, _lib.ptr(vertices), int(vertices.shape[0]), _lib.ptr(triangles),
                int(triangles.shape[0]), _lib.ptr(records), V, H, W, _lib.ptr(vis), _lib.ptr(dimage), _lib.ptr(uvs),
                int(shape[0]) if textured else 0, _lib.ptr(None if textured else grad), _lib.ptr(grad if textured else None),
                _lib.ptr(ws), ws_bytes)
    return grad


class _ShadeColour(torch.autograd.Function):
    """The shading pass as a differentiable function of its colour source (include/mi3d.h Part 18): `source` is colors
    [nv, 3] without `uvs` and a float32 texture [T, T, 3] with them.  Visibility and geometry are constants: the keys
    `vis` are saved for backward, and only `source` receives a gradient.  `out` (a dict) takes the buffers."""

    @staticmethod
    def forward(ctx, source, vertices, triangles, records, H, W, vis, uvs, normals, bg, image_only, out):
        src = dict(colors=source) if uvs is None else dict(uvs=uvs, texture=source)
        out.update(_shade(vertices, triangles, records, H, W, vis, normals=normals, bg=bg, image_only=image_only, **src))
        ctx.save_for_backward(vertices, triangles, records, vis, *(() if uvs is None else (uvs,)))
        ctx.size = (H, W, tuple(source.shape))
        return out["image"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dimage):
        vertices, triangles, records, vis, *uvs = ctx.saved_tensors
        H, W, shape = ctx.size
        grad = _shade_backward(vertices, triangles, records, H, W, vis, dimage.contiguous().float(),
                               uvs[0] if uvs else None, shape)
        return (grad,) + (None,) * 11


def box_average(x, ssaa):
    """[V, ssaa H, ssaa W, ...] -> [V, H, W, ...]: the float32 sum of a pixel's ssaa^2 sub-pixels, rows first and columns
    within a row, times 1 / ssaa^2 (Part 9's order for a texel's samples); ssaa = 1 returns x."""
    if ssaa == 1:
        return x
    V, H, W = x.shape[0], x.shape[1] // ssaa, x.shape[2] // ssaa
    x = x.reshape(V, H, ssaa, W, ssaa, *x.shape[3:])
    s = x[:, :, 0, :, 0]
    for k in range(1, ssaa * ssaa):
        s = s + x[:, :, k // ssaa, :, k % ssaa]
    return s * (1.0 / (ssaa * ssaa))


def _scaled_K(K, ssaa):
    """K for ssaa x ssaa sub-pixels: its first two rows times ssaa (exact: a power of two); any other shape is returned
    as it is, for view_records to refuse."""
    K = _host64(K)
    return K * np.array([[ssaa], [ssaa], [1.0]]) if K.shape == (3, 3) else K


def _check_colour_source(nv, nt, dev, colors, uvs, texture):
    """One colour source of a mesh of nv vertices and nt triangles on `dev`: colors float32 [nv, 3], or uvs float32
    [3 nt, 2] with a texture uint8 or float32 [T, T, 3].  Returns (colors, uvs, texture) as the kernels take them."""
    if colors is not None:
        colors = _lib.dev_f32(colors, "colors", 3)
        if tuple(colors.shape) != (nv, 3) or colors.device != dev:
            raise Mi3dError(f"colors must be [{nv}, 3] on the mesh's device (got {tuple(colors.shape)} on {colors.device})")
        return colors, None, None
    if uvs is None or texture is None:
        raise Mi3dError("uvs and texture go together")
    uvs = _lib.dev_f32(uvs, "uvs", 2)
    if not isinstance(texture, torch.Tensor):
        raise TypeError("texture must be a torch.Tensor")
    texture = _lib.dev_typed(texture, "texture", torch.float32 if texture.dtype == torch.float32 else torch.uint8)
    if tuple(uvs.shape) != (3 * nt, 2) or uvs.device != dev:
        raise Mi3dError(f"uvs must be [{3 * nt}, 2] on the mesh's device (got {tuple(uvs.shape)} on {uvs.device})")
    if texture.dim() != 3 or texture.shape[0] != texture.shape[1] or texture.shape[2] != 3 or texture.device != dev or \
            not MIN_TEXTURE <= texture.shape[0] <= MAX_TEXTURE:
        raise Mi3dError(f"texture must be [T, T, 3] with T in [{MIN_TEXTURE}, {MAX_TEXTURE}] on the mesh's device (got "
                        f"{tuple(texture.shape)} on {texture.device})")
    return None, uvs, texture


def render(vertices, triangles, c2w, K, H, W, colors=None, uvs=None, texture=None, normals=None, shading="albedo",
           light_d=None, ambient_ratio=0.1, bg_color=1.0, ssaa=1, return_buffers=False):
    """Images of an indexed mesh from V pinhole cameras (include/mi3d.h Part 17): vertices float32 [nv, 3], triangles
    int32 [nt, 3] on the GPU; c2w [V, 4, 4], K [3, 3], H, W as render_depth takes them.  The colour comes from exactly one
    of `colors` float32 [nv, 3] (per vertex, interpolated perspective-correctly) and `uvs` float32 [3 nt, 2] with
    `texture` uint8 [T, T, 3] (what bake_texture and bake_views return: bilinear taps, row 0 the top row) or float32
    [T, T, 3] (the blend of the taps as it is, no / 255); all on the mesh's device.  When `colors` or a float32 `texture`
    requires grad, the image is differentiable in it (include/mi3d.h Part 18: visibility and geometry are constants;
    `vertices`, `uvs` or `normals` that require grad raise Mi3dError); otherwise the launches and the bits are the same
    with or without autograd.  `normals` float32 [nv, 3] are interpolated too and needed by every shading but "albedo".

    `shading` as the field's (the reference's nerf/network_tcnn.py:159-168), composed in torch from the kernel's albedo
    and normal buffers, n the normalised interpolated normal and l `light_d` (3 numbers or [V, 3], normalised here;
    None: from the origin towards each camera): "albedo" the colour as it is (bit for bit the kernel's image),
    "lambertian" the colour times ambient_ratio + (1 - ambient_ratio) clamp(n . l, min=0.1), "textureless" that factor
    alone, "normal" (n + 1) / 2.  A pixel no triangle covers is `bg_color` (a number or three).  `ssaa` in {1, 2, 4}
    renders ssaa H x ssaa W pixels with K scaled and box-averages them (box_average).

    Returns (image float32 [V, H, W, 3], alpha float32 [V, H, W]: the covered share of the pixel, 0 or 1 without
    supersampling); with `return_buffers=True` also a dict of depth float32 (+inf where nothing is drawn), tri int32
    (-1 there), bary float32 [.., 3] and normal (un-normalised; None without `normals`), at the ssaa H x ssaa W the
    kernels ran at.  Nothing is clipped: a triangle with a vertex at z <= 0 is left out of that view.  A triangle index
    outside [0, nv) raises Mi3dError.  Every argument is checked before anything is launched."""
    shading, ssaa = _check_shading(shading, ssaa)
    H, W = int(H), int(W)
    records = view_records(c2w, _scaled_K(K, ssaa))
    V = int(records.shape[0])
    _check_view_size(V, H, W)
    ambient, bg, light = _check_render_options(ambient_ratio, bg_color, light_d, V)
    _check_view_size(V, ssaa * H, ssaa * W)
    vertices, triangles = _check_mesh(vertices, triangles)
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    for name, x in (("vertices", vertices), ("uvs", uvs), ("normals", normals)):
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise Mi3dError(f"render: {name} requires grad, but visibility and geometry are constants here: only colors "
                            f"and a float32 texture are differentiable (detach {name})")
    if (colors is None) == (uvs is None and texture is None):
        raise Mi3dError("render takes exactly one colour source: colors, or uvs with texture")
    colors, uvs, texture = _check_colour_source(nv, nt, dev, colors, uvs, texture)
    if normals is not None:
        normals = _lib.dev_f32(normals, "normals", 3)
        if tuple(normals.shape) != (nv, 3) or normals.device != dev:
            raise Mi3dError(f"normals must be [{nv}, 3] on the mesh's device (got {tuple(normals.shape)} on {normals.device})")
    elif shading != "albedo":
        raise Mi3dError(f"shading={shading!r} needs normals")
    source = colors if colors is not None else texture
    if torch.is_grad_enabled() and source.requires_grad:       # Part 18: the image as a function of its colour source
        rec = torch.from_numpy(records).to(dev)
        vis, counts = _visibility(vertices, triangles, rec, ssaa * H, ssaa * W)
        buf = dict(vis=vis, counts=counts)
        image = _ShadeColour.apply(source, vertices, triangles, rec, ssaa * H, ssaa * W, vis, uvs, normals, bg, False, buf)
        buf["image"] = image
    else:
        buf = _render_buffers(vertices, triangles, torch.from_numpy(records).to(dev), ssaa * H, ssaa * W, colors, uvs,
                              texture, normals, bg)
    bad = int(buf["counts"][0])                                 # the one host read
    if bad != 0:
        raise Mi3dError(f"{bad} of the {nt} triangles hold a vertex index outside [0, {nv})")
    image, covered = buf["image"], buf["alpha"] != 0
    if shading != "albedo":
        n = buf["normal"]
        n = n / torch.sqrt(torch.clamp((n * n).sum(-1, keepdim=True), min=1e-20))
        if light is None:
            light = records[:, 21:24].astype(np.float64)
            norm = np.linalg.norm(light, axis=-1, keepdims=True)
            light = np.where(norm > 0, light / np.where(norm > 0, norm, 1.0), [0.0, 0.0, 1.0]).astype(np.float32)
        l = torch.from_numpy(np.ascontiguousarray(light)).to(dev)[:, None, None, :]
        lambertian = ambient + (1.0 - ambient) * (n * l).sum(-1, keepdim=True).clamp(min=0.1)
        shaded = {"lambertian": image * lambertian, "textureless": lambertian.expand_as(image), "normal": (n + 1.0) / 2.0}
        image = torch.where(covered[..., None], shaded[shading], torch.from_numpy(bg).to(dev))
    image, alpha = box_average(image, ssaa), box_average(covered.float(), ssaa)
    if return_buffers:
        return image, alpha, {k: buf[k] for k in ("depth", "tri", "bary", "normal")}
    return image, alpha


def fidelity(image_a, alpha_a, image_b, alpha_b):
    """How far two sets of renders from the same cameras are apart: images [V, H, W, 3] in [0, 1] and alphas [V, H, W]
    (a pixel belongs to a render's mask iff its alpha > 0.5), tensors or NumPy arrays.  Returns a dict of floats:
    `psnr_union` = 10 log10(1 / mse) with the mean over the three channels of the pixels in EITHER mask (what differs in
    silhouette counts), `psnr_intersection` the same over the pixels in BOTH (colour alone), `iou` = |both| / |either|
    of the masks; and `views`, a list of the same three per view.  The overall figures pool the pixels of all views.
    Equal images give +inf; an empty set of pixels gives nan.  Plain torch in float64."""
    def t(a):
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return a.detach().to(torch.float64)
    image_a = t(image_a)
    image_b, alpha_a, alpha_b = (t(a).to(image_a.device) for a in (image_b, alpha_a, alpha_b))
    if image_a.dim() != 4 or image_a.shape[3] != 3 or image_b.shape != image_a.shape or \
            alpha_a.shape != image_a.shape[:3] or alpha_b.shape != image_a.shape[:3]:
        raise Mi3dError(f"fidelity takes images [V, H, W, 3] and alphas [V, H, W] of one size (got {tuple(image_a.shape)}, "
                        f"{tuple(alpha_a.shape)}, {tuple(image_b.shape)}, {tuple(alpha_b.shape)})")
    ma, mb = alpha_a > 0.5, alpha_b > 0.5
    se = ((image_a - image_b) ** 2).sum(-1)                     # per pixel, the three channels summed

    def figures(se, either, both):
        def psnr(m):
            n = int(m.sum())
            if n == 0:
                return float("nan")
            mse = float(se[m].sum()) / (3 * n)
            return float("inf") if mse == 0.0 else float(10.0 * np.log10(1.0 / mse))
        ne = int(either.sum())
        return {"psnr_union": psnr(either), "psnr_intersection": psnr(both),
                "iou": float("nan") if ne == 0 else int(both.sum()) / ne}

    out = figures(se, ma | mb, ma & mb)
    out["views"] = [figures(se[v], (ma | mb)[v], (ma & mb)[v]) for v in range(image_a.shape[0])]
    return out


def quantise(image):
    """Part 9's quantisation of a float image in [0, 1] to uint8: min(255, floor(a * 255)) in float32, 0 for a negative
    value or a NaN - what write_png is given for the previews."""
    a = torch.nan_to_num(image.float() * 255.0, nan=0.0, posinf=255.0, neginf=0.0)
    return a.floor().clamp(0.0, 255.0).to(torch.uint8)


FIT_KEYS = ("iterations", "lr")
MAX_FIT_ITERATIONS = 100000


def _check_fit(iterations, lr):
    if not _is_number(lr) or not 0 < lr <= 1:                   # false for NaN
        raise Mi3dError(f"lr must be a number in (0, 1] (got {lr!r})")
    return _integer(iterations, "iterations", 1, MAX_FIT_ITERATIONS), float(lr)


def _fit(vertices, triangles, uvs, start, images, c2w, K, masks, weights, iterations, lr, ssaa, bg_color, return_history):
    """fit_texture (with uvs) and fit_colors (without): see there."""
    iterations, lr = _check_fit(iterations, lr)
    _, ssaa = _check_shading("albedo", ssaa)
    _, weights, _, _, (V, H, W) = check_views(images, c2w, K, masks, weights)
    if not weights.sum() > 0:
        raise Mi3dError("weights must not all be zero")
    records = view_records(c2w, _scaled_K(K, ssaa))
    _, bg, _ = _check_render_options(0.0, bg_color, None, V)
    _check_view_size(V, ssaa * H, ssaa * W)
    vertices, triangles = _check_mesh(vertices, triangles)
    nv, nt, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    if not isinstance(start, torch.Tensor):
        raise TypeError("the start must be a torch.Tensor")
    if uvs is None:
        start = _check_colour_source(nv, nt, dev, start, None, None)[0]
    else:
        _, uvs, start = _check_colour_source(nv, nt, dev, None, uvs, start)
        if start.dtype == torch.uint8:
            start = start.float() / 255.0                       # what mi3d_mesh_shade makes of a byte
    rec = torch.from_numpy(records).to(dev)
    target = _to_dev(images, torch.float32, dev)
    pixel = torch.from_numpy(weights).to(dev)[:, None, None].expand(V, H, W)
    if masks is not None:
        pixel = pixel * (_to_dev(masks, torch.float32, dev) != 0)
    pixel = (pixel / (3.0 * pixel.sum().clamp(min=1e-30)))[..., None]     # the weighted mean over pixels and channels
    vis, counts = _visibility(vertices, triangles, rec, ssaa * H, ssaa * W)     # once: the geometry does not move
    with torch.enable_grad():
        value = start.detach().clone().requires_grad_(True)
        optimiser = torch.optim.Adam([value], lr=lr)
        history = []
        for _ in range(iterations):
            optimiser.zero_grad(set_to_none=True)
            image = _ShadeColour.apply(value, vertices, triangles, rec, ssaa * H, ssaa * W, vis, uvs, None, bg, True, {})
            loss = (pixel * (box_average(image, ssaa) - target) ** 2).sum()
            loss.backward()
            optimiser.step()
            with torch.no_grad():
                value.clamp_(0.0, 1.0)
            history.append(loss.detach())
    bad, losses = int(counts[0]), torch.stack(history).cpu().tolist()    # the host reads: after the last launch
    if bad != 0:
        raise Mi3dError(f"{bad} of the {nt} triangles hold a vertex index outside [0, {nv})")
    value = value.detach()
    return (value, losses) if return_history else value


def fit_texture(vertices, triangles, uvs, texture, images, c2w, K, masks=None, weights=None, iterations=200, lr=0.01,
                ssaa=1, bg_color=1.0, return_history=False):
    """A texture fitted to VIEWS through the renderer that will show it (include/mi3d.h Part 18): Adam (torch's, its
    default betas and eps) on the weighted mean squared error between render(..., uvs=uvs, texture=value, ssaa=ssaa,
    bg_color=bg_color) and `images` - the mean over the three channels of the pixels whose mask is non-zero, view v's
    pixels weighted by weights[v] - starting from `texture` (float32 [T, T, 3], or uint8, read as byte / 255), the values
    clamped to [0, 1] after every step.  The gradient reaches the four bilinear taps of every drawn pixel, gutter texels
    included; a texel no pixel touches receives an exact zero gradient and keeps its value bit for bit.

    vertices, triangles, uvs as render takes them; images float [V, H, W, 3], c2w, K, masks and weights as bake_views
    takes them, checked by its rules before anything is launched.  Visibility is computed once.  Returns the fitted
    float32 [T, T, 3] on the mesh's device; with `return_history=True` also the list of the loss before each step, which
    stays on the device until the loop is over and is read once.  Pass the result through quantise() for a PNG.

    iterations=200 and lr=0.01 are choices nobody has measured on a trained object."""
    if uvs is None:
        raise Mi3dError("fit_texture needs uvs")
    return _fit(vertices, triangles, uvs, texture, images, c2w, K, masks, weights, iterations, lr, ssaa, bg_color,
                return_history)


def fit_colors(vertices, triangles, colors, images, c2w, K, masks=None, weights=None, iterations=200, lr=0.01, ssaa=1,
               bg_color=1.0, return_history=False):
    """fit_texture for vertex colours: `colors` float32 [nv, 3] is the start, render(..., colors=value) the model; a
    vertex no drawn pixel's triangle names keeps its value bit for bit.  Returns the fitted float32 [nv, 3]."""
    return _fit(vertices, triangles, None, colors, images, c2w, K, masks, weights, iterations, lr, ssaa, bg_color,
                return_history)


def camera_rays(c2w, K, H, W, device):
    """Rays through the pixel centres of pinhole cameras: a point at depth z along the ray of pixel (i, j) projects, by
    Part 15's PROJECTION with these c2w and K, to (i + 0.5, j + 0.5).  Returns (origins, unit directions) float32
    [V, H W, 3] on `device`; the directions are K^-1 (i + 0.5, j + 0.5, 1) rotated by c2w, computed in binary64 and
    rounded once."""
    c2w, K = _host64(c2w), _host64(K)
    j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    cam = np.stack([i.ravel(), j.ravel(), np.ones(H * W)], -1) @ np.linalg.inv(K).T
    d = cam @ c2w[:, :3, :3].transpose(0, 2, 1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(c2w[:, None, :3, 3], d.shape)
    return (torch.from_numpy(np.ascontiguousarray(o, dtype=np.float32)).to(device),
            torch.from_numpy(d.astype(np.float32)).to(device))


def render_field(model, c2w, K, H, W):
    """The field's own renders from the cameras render() takes: the eval route (no perturbation, all rays, albedo) over
    a white background, rays by camera_rays.  Returns (image float32 [V, H, W, 3], alpha float32 [V, H, W]: the rays'
    accumulated opacity) on the model's device."""
    dev = model.aabb_train.device
    ro, rd = camera_rays(c2w, K, H, W, dev)
    was_training = model.training
    model.eval()
    images, alphas = [], []
    try:
        with torch.no_grad():
            for v in range(ro.shape[0]):
                out = model.render(ro[v:v + 1], rd[v:v + 1], staged=True, perturb=False, force_all_rays=True,
                                   bg_color=torch.ones(3, device=dev), shading="albedo", ambient_ratio=1.0)
                images.append(out["image"].reshape(H, W, 3).float())
                alphas.append(out["weights_sum"].reshape(H, W).float())
    finally:
        model.train(was_training)
    return torch.stack(images), torch.stack(alphas)


def _check_preview(preview):
    """export's `preview`: a dict of PREVIEW_KEYS, checked on the host; returns it with the defaults filled in."""
    if not isinstance(preview, dict):
        raise Mi3dError(f"preview must be a dict with the keys {PREVIEW_KEYS[:4]} and optionally {PREVIEW_KEYS[4:]} (got "
                        f"{type(preview).__name__})")
    unknown = sorted(set(preview) - set(PREVIEW_KEYS))
    missing = [k for k in PREVIEW_KEYS[:4] if k not in preview]
    if unknown or missing:
        raise Mi3dError(f"preview: unknown keys {unknown}, missing keys {missing}; it takes {PREVIEW_KEYS}")
    p = dict(shading="albedo", ssaa=1, fidelity=False)
    p.update(preview)
    for k in ("H", "W"):
        if not _is_number(p[k], integer=True):
            raise Mi3dError(f"preview: {k} must be an integer (got {p[k]!r})")
    V = view_records(p["c2w"], p["K"]).shape[0]
    _check_view_size(V, int(p["H"]), int(p["W"]))
    p["shading"], p["ssaa"] = _check_shading(p["shading"], p["ssaa"])
    _check_view_size(V, p["ssaa"] * int(p["H"]), p["ssaa"] * int(p["W"]))
    p["fidelity"] = _flag(p["fidelity"], "preview: fidelity")
    if p["fidelity"] and p["shading"] != "albedo":
        raise Mi3dError("preview: fidelity compares albedo renders: give shading='albedo' with it")
    return p


def _json_number(x):
    return x if np.isfinite(x) else None                       # JSON has no inf and no nan


def _write_preview(path, model, p, vertices, triangles, albedo, vt, image, vn):
    """export's preview step: the final mesh rendered as it is written - with its texture, or its vertex colours -
    to `preview_000.png` ...; with fidelity also the field's renders from the same cameras and `preview.json`."""
    import json
    if p["shading"] != "albedo" and vn is None:
        vn = vertex_normals(model, vertices).contiguous()
    source = dict(colors=albedo.contiguous()) if image is None else dict(uvs=vt, texture=image)
    rendered, alpha = render(vertices, triangles, p["c2w"], p["K"], p["H"], p["W"], normals=vn, shading=p["shading"],
                             ssaa=p["ssaa"], **source)
    os.makedirs(path, exist_ok=True)
    for v, img in enumerate(quantise(rendered).cpu().numpy()):
        write_png(os.path.join(path, f"preview_{v:03d}.png"), img)
    if p["fidelity"]:
        field, field_alpha = render_field(model, p["c2w"], p["K"], int(p["H"]), int(p["W"]))
        report = fidelity(rendered, alpha, field, field_alpha)
        report = {k: [{a: _json_number(b) for a, b in r.items()} for r in x] if k == "views" else _json_number(x)
                  for k, x in report.items()}
        report.update(H=int(p["H"]), W=int(p["W"]), ssaa=int(p["ssaa"]), a="mesh", b="field")
        with open(os.path.join(path, "preview.json"), "w") as fp:
            json.dump(report, fp, indent=1)
            fp.write("\n")


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


def write_png(path, image):
    """`image` uint8 [H, W, 3] (row 0 = top) as an 8-bit RGB PNG, non-interlaced, filter 0 on every row; zlib, struct and
    the CRC of the standard library - no imaging package."""
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or 0 in image.shape:
        raise ValueError(f"image must be uint8 [H, W, 3] (got {image.dtype} {image.shape})")
    H, W = image.shape[:2]

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))

    rows_per_block = max(1, (1 << 24) // (3 * W + 1))
    z = zlib.compressobj(6)
    with open(path, "wb") as fp:
        fp.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)))
        for s in range(0, H, rows_per_block):
            part = image[s:s + rows_per_block].reshape(-1, 3 * W)
            raw = np.concatenate([np.zeros((part.shape[0], 1), np.uint8), part], 1)     # the filter byte of every row
            data = z.compress(raw.tobytes())
            if data:
                fp.write(chunk(b"IDAT", data))
        fp.write(chunk(b"IDAT", z.flush()) + chunk(b"IEND", b""))
    return path


def write_obj(path, vertices, triangles, colors, name="mesh", uvs=None, uv_faces=None, texture=None, normals=None):
    """`<path>/<name>.obj` (lines `v x y z r g b`, `f a b c` one-based) and `<path>/<name>.mtl`.  NumPy arrays:
    vertices [nv, 3], triangles [nt, 3] (zero-based), colors [nv, 3] in [0, 1].  Returns the two file names.
    With `uvs` [nuv, 2], `uv_faces` [nt, 3] (zero-based rows of uvs) and `texture` (an image file name, as the MTL is to
    cite it) - all three or none - the lines are `v x y z`, `vt u v`, `f a/ta b/tb c/tc` instead and the MTL ends with
    `map_Kd <texture>`; `colors` is not written then.
    With `normals` [nv, 3] (one per vertex) a line `vn x y z` per vertex follows the `v` / `vt` block and the faces cite
    normal a for vertex a: `f a//a b//b c//c`, textured `f a/ta/a b/tb/b c/tc/c`.  Without it the files are what they
    were before the argument existed."""
    vertices, colors = np.asarray(vertices, np.float32), np.asarray(colors, np.float32)
    triangles = np.asarray(triangles)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or colors.shape != vertices.shape:
        raise ValueError(f"vertices {vertices.shape} and colors {colors.shape} must both be [nv, 3]")
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f"triangles must be [nt, 3] (got {triangles.shape})")
    textured = uvs is not None or uv_faces is not None or texture is not None
    if textured:
        if uvs is None or uv_faces is None or texture is None:
            raise ValueError("uvs, uv_faces and texture go together")
        uvs, uv_faces = np.asarray(uvs, np.float32), np.asarray(uv_faces)
        if uvs.ndim != 2 or uvs.shape[1] != 2 or uv_faces.shape != triangles.shape:
            raise ValueError(f"uvs must be [nuv, 2] and uv_faces [nt, 3] (got {uvs.shape} and {uv_faces.shape})")
    if normals is not None:
        normals = np.asarray(normals, np.float32)
        if normals.shape != vertices.shape:
            raise ValueError(f"normals must be [nv, 3] like vertices {vertices.shape} (got {normals.shape})")
    os.makedirs(path, exist_ok=True)
    obj, mtl = os.path.join(path, f"{name}.obj"), os.path.join(path, f"{name}.mtl")
    with open(obj, "w") as fp:
        fp.write(f"mtllib {name}.mtl\n")
        # %.9g round-trips binary32; colours need no more than six decimals
        if textured:
            _write_rows(fp, "v %.9g %.9g %.9g\n", vertices.astype(np.float64))
            _write_rows(fp, "vt %.9g %.9g\n", uvs.astype(np.float64))
        else:
            _write_rows(fp, "v %.9g %.9g %.9g %.6f %.6f %.6f\n", np.concatenate([vertices, colors], 1).astype(np.float64))
        if normals is not None:
            _write_rows(fp, "vn %.9g %.9g %.9g\n", normals.astype(np.float64))
        fp.write("usemtl mat0\n")
        tri = triangles.astype(np.int64) + 1
        if textured and normals is not None:
            _write_rows(fp, "f %d/%d/%d %d/%d/%d %d/%d/%d\n", np.stack([tri, uv_faces.astype(np.int64) + 1, tri], -1).reshape(-1, 9))
        elif textured:
            both = np.stack([tri, uv_faces.astype(np.int64) + 1], -1).reshape(-1, 6)
            _write_rows(fp, "f %d/%d %d/%d %d/%d\n", both)
        elif normals is not None:
            _write_rows(fp, "f %d//%d %d//%d %d//%d\n", np.stack([tri, tri], -1).reshape(-1, 6))
        else:
            _write_rows(fp, "f %d %d %d\n", tri)
    with open(mtl, "w") as fp:
        fp.write(MTL + (f"map_Kd {texture}\n" if textured else ""))
    return obj, mtl


def vertex_normals(model, vertices):
    """model.analytic_normal(vertices): the unit normal of the density isosurface at every vertex, float32 [nv, 3] (the
    field's own chunking)."""
    return model.analytic_normal(vertices).float()


def export(model, path, resolution=None, S=128, texture_size=None, ssaa=1, normals=False, min_faces=None,
           min_diagonal=None, largest=False, decimate=None, target_faces=None, views=None, smooth=None, preview=None,
           collapse=None, atlas="uniform"):
    """What NeRFRenderer.export_mesh does (see there).  `S` only sizes the reference's chunks and is ignored."""
    del S
    atlas = _check_atlas(atlas, texture_size)                   # before any work
    collapsing = _check_collapse_option(collapse)              # before any work
    smoothing = _check_smooth_option(smooth)                    # before any work
    if preview is not None:                                     # before any work
        preview = _check_preview(preview)
    if views is not None:                                       # before any work
        if texture_size is None:
            raise Mi3dError("export_mesh: views colour the texture: give texture_size too")
        views, fit = _check_views_dict(views)
    decimate, target_faces = _check_decimate(decimate, target_faces)
    cleaning = min_faces is not None or min_diagonal is not None or largest is not False
    if cleaning:
        rule = _check_keep_rule(0 if min_faces is None else min_faces, 0.0 if min_diagonal is None else min_diagonal,
                                largest)
    if model.aabb_train.device.type != "cuda":
        raise Mi3dError(f"export_mesh needs the model on the GPU (it is on {model.aabb_train.device}): the field and "
                        f"the marching-cubes kernels have no CPU path")
    if texture_size is not None:
        texture_size, ssaa = _check_texture(texture_size, ssaa)
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
        if cleaning:                                            # before the atlas, the colours and the normals
            nv0, nt0 = vertices.shape[0], triangles.shape[0]
            vertices, triangles, _, counts = _clean(vertices, triangles, *rule)
            if vertices.shape[0] == 0 or triangles.shape[0] == 0:
                raise Mi3dError(f"export_mesh: nothing survives min_faces={rule[0]}, min_diagonal={rule[1]:g}, "
                                f"largest={rule[2]}: the surface has {counts[5]} components, the largest of "
                                f"{counts[4] >> 32} triangles ({nv0} vertices, {nt0} triangles in all)")
        if decimate is not None or target_faces is not None:    # after the floater filter, which sees the original mesh
            vertices, triangles = _decimate(vertices, triangles, R, decimate, target_faces)
        if collapsing is not None:                              # after the clustering: cluster coarsely, then collapse
            vertices, triangles = _collapse_export(vertices, triangles, collapsing)
        if smoothing is not None:                               # before the atlas check, the colours, the bakes, the normals
            vertices = _smooth_export(vertices, triangles, smoothing, h)
        if texture_size is not None:
            _atlas_state(vertices, triangles, texture_size, atlas)   # refuse before the field is evaluated anywhere
        albedo = vertex_albedo(model, vertices)
        if views is not None:                                   # after the floater filter and the decimation
            image, vt = bake_views(model, vertices, triangles, texture_size, ssaa=ssaa, atlas=atlas, **views)[:2]
            if fit is not None:                                 # the bake corrected by what the renderer reads from it
                start = image.float() / 255.0
                fitted = fit_texture(vertices, triangles, vt, start, views["images"], views["c2w"], views["K"],
                                     views.get("masks"), views.get("weights"), **fit)
                image = torch.where(fitted == start, image, quantise(fitted))     # an untouched texel keeps its byte
        elif texture_size is not None:
            image, vt, _ = bake_texture(model, vertices, triangles, texture_size, ssaa, atlas)
        vn = vertex_normals(model, vertices).cpu().numpy() if normals else None
        if preview is not None:                                 # the mesh as it is written: after the bake
            textured = texture_size is not None
            _write_preview(path, model, preview, vertices, triangles, albedo, vt if textured else None,
                           image if textured else None, None if vn is None else torch.from_numpy(vn).to(vertices.device))
    v, f, c = vertices.cpu().numpy(), triangles.cpu().numpy(), albedo.cpu().numpy()
    last = () if vn is None else (vn,)
    if texture_size is None:
        write_obj(path, v, f, c, normals=vn)
        return (v, f, c) + last
    vt, image = vt.cpu().numpy(), image.cpu().numpy()
    write_obj(path, v, f, c, uvs=vt, uv_faces=np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3), texture="albedo.png",
              normals=vn)
    write_png(os.path.join(path, "albedo.png"), image)
    return (v, f, c, vt, image) + last
