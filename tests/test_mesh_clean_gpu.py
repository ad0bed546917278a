"""GPU: mesh components and the floater filter (csrc/meshclean.hip through mi3d.mesh.components / clean, include/mi3d.h
Part 13).  Every comparison is exact with tests/mesh_components_model.py, the NumPy restatement of the contract: integer
arrays equal, float rows bit-identical.  The inputs are the smallest at which the kernels can still go wrong: surfaces of the
product's own marching cubes (two components, a component with specks, one long thin component, nothing) and hand-built
index meshes (more than one workgroup and a multiple of neither 64 nor 256, three vertex numberings of one strip, labels
past 16 bits, more elements than one pass of the statistics kernels' grid, unreferenced vertices, duplicate and degenerate
triangles, non-finite coordinates).  Three meshes lie above the sizes at which the statistics kernels' strides and both
scans of k_cl_scan go round again (section "the loops' later rounds"); one of them holds bad indices and so goes
through the entry points themselves.  Then export_mesh with the three arguments, end to end."""
import os

import numpy as np
import pytest

import mesh_components_model as M
from test_mc_tables_cpu import sphere_volume
from test_mesh_cpu import parse_obj

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the inputs

def speck_volume(R=24, r0=0.45, n=30, seed=3):
    """A sphere (value r0 - distance) plus `n` isolated one-voxel islands of value 0.5 in the free space around it: on a
    stride-3 lattice, so that no two touch, away from the sphere and from the box walls."""
    vol = sphere_volume(R, r0)
    ax = np.linspace(-1, 1, R)
    cand = [(i, j, k) for i in range(2, R - 2, 3) for j in range(2, R - 2, 3) for k in range(2, R - 2, 3)
            if np.sqrt(ax[i] ** 2 + ax[j] ** 2 + ax[k] ** 2) > r0 + 0.3]
    pick = np.random.default_rng(seed).choice(len(cand), n, replace=False)
    for q in pick:
        vol[cand[q]] = 0.5
    return vol


def helix_volume(R=32):
    """A tube of radius 0.09 around two and a half turns of a helix: one long, thin component."""
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    s = np.linspace(0, 1, 600)
    cx, cy, cz = 0.6 * np.cos(5 * np.pi * s), 0.6 * np.sin(5 * np.pi * s), -0.7 + 1.4 * s
    d = np.full(x.shape, np.inf)
    for a, b, c in zip(cx, cy, cz):
        d = np.minimum(d, (x - a) ** 2 + (y - b) ** 2 + (z - c) ** 2)
    return (0.09 - np.sqrt(d)).astype(np.float32)


VOLUMES = {
    "two_spheres": lambda: np.maximum(sphere_volume(24, 0.3, (0.5, 0, 0)), sphere_volume(24, 0.3, (-0.5, 0, 0))),
    "sphere_and_specks": speck_volume,
    "helix": helix_volume,
    "nothing": lambda: np.full((8, 8, 8), -1.0, np.float32),
}

STRIP = 4099            # triangles: more than one workgroup, a multiple of neither 64 nor 256


def strip(order):
    """A strip of STRIP triangles over STRIP + 2 vertices, vertex i of the strip stored as index order[i]."""
    i = np.arange(STRIP)
    t = order[np.stack([i, i + 1, i + 2], 1)].astype(np.int32)
    v = np.zeros((STRIP + 2, 3), np.float32)
    v[order, 0] = np.arange(STRIP + 2, dtype=np.float32) * np.float32(0.25)
    v[order, 1] = (np.arange(STRIP + 2) % 2).astype(np.float32)
    return v, t


def coords(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32)


def disjoint():
    """1 000 triangles without a common vertex; triangle 0 has the box [0, 3] x [0, 4] x [0, 0]: diag2 = 25 exactly."""
    v = coords(3000, 1)
    v[0], v[1], v[2] = (0, 0, 0), (3, 0, 0), (0, 4, 0)
    return v, np.arange(3000, dtype=np.int32).reshape(1000, 3)


def two_fans():
    """Two fans of 40 triangles around the centres 0 and 100 whose rims share vertex 41 alone: one component."""
    a = [[0, i, i + 1] for i in range(1, 41)]
    b = [[100, 41 + i, 42 + i] for i in range(0, 40)]
    return coords(101, 2), np.array(a + b, np.int32)


def past_16_bits():
    """nv = 70 001: a strip whose smallest index is 66 000, disjoint triangles on both sides of 65 536, the rest uncited."""
    nv = 70001
    i = np.arange(66000, 66300)
    t = [np.stack([i + 2, i + 1, i], 1), np.arange(65400, 65700).reshape(100, 3)[::-1], [[70000, 69999, 300]]]
    return coords(nv, 3), np.concatenate(t).astype(np.int32)


def interleaved_strips():
    """Two strips of 67 600 triangles each, one over the even and one over the odd vertices: two large components whose
    labels alternate lane by lane, and more vertices and triangles (135 200) than one pass of the statistics kernels'
    grid covers (512 workgroups of 256), so their grid-stride loops go round."""
    i = np.arange(135200)
    return coords(135300, 9), np.stack([i, i + 2, i + 4], 1).astype(np.int32)


def unreferenced():
    """Vertices no triangle cites in front (0 .. 4), in the middle (20 .. 29) and at the end (60 .. 69)."""
    t = [[5 + i, 6 + i, 7 + i] for i in range(0, 13)] + [[30 + i, 32 + i, 31 + i] for i in range(0, 28, 3)]
    return coords(70, 4), np.array(t, np.int32)


def duplicate_and_degenerate():
    t = [[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 3, 4], [5, 5, 5], [6, 7, 7], [7, 8, 8], [9, 10, 9], [4, 4, 3], [11, 12, 13]]
    return coords(15, 5), np.array(t, np.int32)


def non_finite():
    """NaN, +inf and -inf coordinates inside one component (0 .. 5); a component all of whose x are NaN and y are +inf
    (6 .. 8); a finite one with a -0 / +0 pair (9 .. 11)."""
    v = coords(12, 6)
    v[0, 0], v[1, 0], v[2, 1], v[3, 1], v[4, 2] = np.nan, np.inf, -np.inf, np.nan, np.inf
    v[6:9, 0], v[6:9, 1] = np.nan, np.inf
    v[9:12, 2] = (-0.0, 0.0, -0.0)
    return v, np.array([[0, 1, 2], [2, 3, 4], [4, 5, 0], [6, 7, 8], [9, 10, 11]], np.int32)


HAND_BUILT = {
    "strip_ascending": lambda: strip(np.arange(STRIP + 2)),
    "strip_descending": lambda: strip(np.arange(STRIP + 2)[::-1].copy()),
    "strip_permuted": lambda: strip(np.random.default_rng(7).permutation(STRIP + 2)),
    "disjoint": disjoint,
    "two_fans": two_fans,
    "past_16_bits": past_16_bits,
    "interleaved_strips": interleaved_strips,
    "one_triangle": lambda: (coords(3, 8), np.array([[2, 0, 1]], np.int32)),
    "unreferenced": unreferenced,
    "duplicate_and_degenerate": duplicate_and_degenerate,
    "non_finite": non_finite,
}
NAMES = list(VOLUMES) + list(HAND_BUILT)


@pytest.fixture(scope="module")
def inputs(cuda):
    """name -> (vertices, triangles, model components): NumPy arrays, each made and modelled once, never changed."""
    import torch
    from mi3d import mesh
    out = {}
    for name, make in VOLUMES.items():
        vol = make()
        R = vol.shape[0]
        h = 2.0 / (R - 1)
        v, t = mesh.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0, origin=(-1.0,) * 3, spacing=(h,) * 3)
        out[name] = (v.cpu().numpy(), t.cpu().numpy())
    for name, make in HAND_BUILT.items():
        out[name] = make()
    for name, (v, t) in out.items():
        comps = M.components(v, t)
        roots = np.flatnonzero(comps[0] == np.arange(len(v)))
        print(f"[clean] {name}: nv {len(v)} nt {len(t)} components {len(roots)} with faces {int((comps[1][roots] > 0).sum())}")
        out[name] = (v, t, comps)
    return out


def test_the_inputs_are_what_they_claim(inputs):
    def faced(name):
        label, faces = inputs[name][2][:2]
        return sorted(faces[faces > 0].tolist())
    assert len(faced("two_spheres")) == 2
    assert len(faced("sphere_and_specks")) == 31 and faced("sphere_and_specks")[:30] == [8] * 30
    assert len(faced("helix")) == 1 and len(inputs["helix"][1]) > 1000
    assert inputs["nothing"][0].shape == (0, 3) and inputs["nothing"][1].shape == (0, 3)
    for name in ("strip_ascending", "strip_descending", "strip_permuted"):
        assert faced(name) == [STRIP] and STRIP % 64 and STRIP % 256 and STRIP > 256
    assert faced("disjoint") == [1] * 1000 and faced("two_fans") == [80]
    assert inputs["past_16_bits"][2][0].max() > 65536
    assert faced("interleaved_strips") == [67600, 67600] and 67600 * 2 > 512 * 256
    assert M.diag2(*inputs["disjoint"][2][2:4])[0] == 25.0


def upload(cuda, v, t):
    import torch
    return torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)


# ------------------------------------------------------------------------------------------------ components

@pytest.mark.parametrize("name", NAMES)
def test_components_against_the_model(cuda, inputs, name):
    import torch
    from mi3d import mesh
    v, t, (rl, rf, rmin, rmax, bad) = inputs[name]
    assert bad == 0
    gv, gt = upload(cuda, v, t)
    label, faces, bmin, bmax = mesh.components(gv, gt)
    assert label.dtype == torch.int32 and faces.dtype == torch.int32 and bmin.dtype == bmax.dtype == torch.float32
    assert label.shape == (len(v),) and faces.shape == (len(v),) and bmin.shape == bmax.shape == (len(v), 3)
    assert all(x.device == cuda for x in (label, faces, bmin, bmax))
    assert np.array_equal(label.cpu().numpy(), rl)
    assert np.array_equal(faces.cpu().numpy(), rf)
    assert bmin.cpu().numpy().tobytes() == rmin.tobytes() and bmax.cpu().numpy().tobytes() == rmax.tobytes()
    # the counters themselves: no bad index, and no thread gave up
    counts = mesh._label_components(gv, gt)[4].tolist()
    faced = rf[rf > 0]
    assert counts[2] == 0 and counts[3] == 0 and counts[5] == len(faced)
    if len(faced):
        top = int(faced.max())
        assert counts[4] == (top << 32) | (~int(np.flatnonzero(rf == top)[0]) & 0xFFFFFFFF)
    again = mesh.components(gv, gt)                    # deterministic: a second call, the same bytes
    for a, b in zip((label, faces, bmin, bmax), again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ clean

def settings(comps):
    """The keep rules an input is cleaned under: min_faces at, just below and just above the sizes of its smallest and
    its largest component, min_diagonal at a component's diagonal and one binary32 step to either side, `largest` alone
    and with thresholds at and above the largest component."""
    label, faces, bmin, bmax, _ = comps
    out = [(0, 0.0, False), (0, 0.0, True)]
    roots = np.flatnonzero((label == np.arange(len(label))) & (faces > 0))
    if len(roots) == 0:
        return out + [(1, 0.5, False)]
    sizes = faces[roots]
    for f in sorted({int(sizes.min()), int(sizes.max())}):
        out += [(f - 1, 0.0, False), (f, 0.0, False), (f + 1, 0.0, False)]
    out += [(int(sizes.max()), 0.0, True), (int(sizes.max()) + 1, 0.0, True)]
    d2 = M.diag2(bmin[roots], bmax[roots])
    finite = d2[np.isfinite(d2) & (d2 > 0)]
    if len(finite):
        md = np.sqrt(np.float32(np.median(finite)), dtype=np.float32)
        for m in (np.nextafter(md, np.float32(0)), md, np.nextafter(md, np.float32(np.inf))):
            out += [(0, float(m), False), (2, float(m), True)]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_clean_against_the_model(cuda, inputs, name):
    import torch
    from mi3d import mesh
    v, t, comps = inputs[name]
    gv, gt = upload(cuda, v, t)
    kept_counts = set()
    for min_faces, min_diagonal, largest in settings(comps):
        rv, rt, rmap, _ = M.clean(v, t, min_faces, min_diagonal, largest, comps=comps)
        cv, ct, cmap = mesh.clean(gv, gt, min_faces, min_diagonal, largest)
        what = f"{name} min_faces={min_faces} min_diagonal={min_diagonal!r} largest={largest}"
        assert cv.dtype == torch.float32 and ct.dtype == torch.int32 and cmap.dtype == torch.int32, what
        assert cv.shape == rv.shape and ct.shape == rt.shape and cmap.shape == rmap.shape, what
        assert cv.dim() == 2 and cv.shape[1] == 3 and ct.dim() == 2 and ct.shape[1] == 3, what
        assert cv.cpu().numpy().tobytes() == rv.tobytes(), what          # bit for bit, in the original order
        assert np.array_equal(ct.cpu().numpy(), rt) and np.array_equal(cmap.cpu().numpy(), rmap), what
        cv2, ct2, cmap2 = mesh.clean(gv, gt, min_faces, min_diagonal, largest)     # twice: byte-identical
        assert cv2.cpu().numpy().tobytes() == cv.cpu().numpy().tobytes(), what
        assert torch.equal(ct2, ct) and torch.equal(cmap2, cmap), what
        kept_counts.add(len(rt))
    print(f"[clean] {name}: kept triangle counts over the settings {sorted(kept_counts)}")
    if len(t):
        assert len(kept_counts) > 1                       # the settings do tell components apart


def test_exact_diagonal_and_ties(cuda, inputs):
    from mi3d import mesh
    v, t, _ = inputs["disjoint"]                          # 1 000 one-face components: triangle 0 has diag2 == 25 == 5 * 5
    gv, gt = upload(cuda, v, t)
    up = float(np.nextafter(np.float32(5), np.float32(6)))
    at = mesh.clean(gv, gt, 0, 5.0, False)[2].cpu().numpy()
    above = mesh.clean(gv, gt, 0, up, False)[2].cpu().numpy()
    assert at[0] == 0 and above[0] == -1                  # equality keeps
    assert np.array_equal(above, M.clean(v, t, 0, up, False)[2])
    cv, ct, cmap = mesh.clean(gv, gt, largest=True)       # a thousandfold tie: the smaller label, triangle 0
    assert ct.cpu().numpy().tolist() == [[0, 1, 2]] and cv.cpu().numpy().tobytes() == v[:3].tobytes()
    assert cmap.cpu().numpy().tolist() == [0, 1, 2] + [-1] * 2997
    v, t, comps = inputs["two_spheres"]                   # mirror images: the same face count, the tie goes to the first
    faces = comps[1][comps[1] > 0]
    assert len(faces) == 2 and faces[0] == faces[1]
    cv, ct, cmap = mesh.clean(*upload(cuda, v, t), largest=True)
    assert len(ct) == faces[0] and cmap[0] == 0


def test_nothing_kept_and_empty_input(cuda, inputs):
    import torch
    from mi3d import mesh
    v, t, _ = inputs["sphere_and_specks"]
    for out in (mesh.clean(*upload(cuda, v, t), min_faces=10 ** 6),
                mesh.clean(torch.empty(0, 3, device=cuda), torch.empty(0, 3, dtype=torch.int32, device=cuda)),
                mesh.clean(torch.zeros(5, 3, device=cuda), torch.empty(0, 3, dtype=torch.int32, device=cuda))):
        cv, ct, cmap = out
        assert cv.shape == (0, 3) and ct.shape == (0, 3) and cv.dtype == torch.float32 and ct.dtype == torch.int32
        assert torch.all(cmap == -1)
    label, faces, bmin, bmax = mesh.components(torch.zeros(5, 3, device=cuda),
                                               torch.empty(0, 3, dtype=torch.int32, device=cuda))
    assert label.tolist() == [0, 1, 2, 3, 4] and faces.tolist() == [0] * 5
    assert mesh.components(torch.empty(0, 3, device=cuda), torch.empty(0, 3, dtype=torch.int32, device=cuda))[0].shape == (0,)


def test_on_a_side_stream(cuda, inputs):
    import torch
    from mi3d import mesh
    v, t, comps = inputs["helix"]
    f = int(comps[1].max())
    rv, rt, rmap, _ = M.clean(v, t, f, 0.0, True, comps=comps)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        gv, gt = upload(cuda, v, t)
        label = mesh.components(gv, gt)[0]
        cv, ct, cmap = mesh.clean(gv, gt, f, 0.0, True)
    side.synchronize()
    assert np.array_equal(label.cpu().numpy(), comps[0])
    assert cv.cpu().numpy().tobytes() == rv.tobytes() and np.array_equal(ct.cpu().numpy(), rt)
    assert np.array_equal(cmap.cpu().numpy(), rmap)


# ------------------------------------------------------------------------------------------------ the loops' later rounds

CLEAN_BLOCK = 256                       # kBlock of csrc/meshclean.hip: elements per workgroup
STAT_BLOCKS = 512                       # kStatBlocks: k_cc_faces / k_cc_boxes / k_cc_finish stride from at most this many
STAT_SLOTS = 512                        # kSlots: labels a workgroup's LDS table holds (kProbes = 4 probes each)
SCAN_ROUND = 1024                       # block sums per round of k_cl_scan: kRowThreads of scan_row in csrc/mi3d_scan.h
STAT_PASS, SCAN_PASS = STAT_BLOCKS * CLEAN_BLOCK, SCAN_ROUND * CLEAN_BLOCK       # 131 072 and 262 144 elements
SINGLES, LONG_STRIP = 150_000, 300_000


def many_singles():
    """150 000 one-triangle components, nv = 450 000: the statistics kernels go round four times over the vertices and
    twice over the triangles; a workgroup meets up to 342 labels in k_cc_boxes and 512 in k_cc_faces, which four probes
    into 512 slots cannot all place, so the path to global atomics is an everyday one here.  The sizes of the triangles
    spread over three decades: a diagonal rule keeps and drops on both sides of every round boundary."""
    rng = np.random.default_rng(21)
    scale = np.repeat(10.0 ** rng.uniform(-2, 1, SINGLES), 3)[:, None]
    v = (rng.normal(size=(3 * SINGLES, 3)) * scale).astype(np.float32)
    return v, np.arange(3 * SINGLES, dtype=np.int32).reshape(SINGLES, 3)


def long_strip():
    """One strip (i, i + 1, i + 2) of 300 000 triangles: a single label cited from every workgroup in every stride, and
    more than 262 144 vertices AND triangles, so both scans of k_cl_scan carry a base into a second round."""
    i = np.arange(LONG_STRIP)
    return coords(LONG_STRIP + 2, 22), np.stack([i, i + 1, i + 2], 1).astype(np.int32)


def both_with_dirt():
    """The two above in one mesh, the triangles of both shuffled together with 3 000 that hold an index outside [0, nv)
    (-1, nv, the int32 extremes, in any of the three places), NaN coordinates in a thousand vertices of either part and
    1 000 vertices no triangle cites behind everything."""
    rng = np.random.default_rng(23)
    (va, ta), (vb, tb) = many_singles(), long_strip()
    v = np.concatenate([va, vb, coords(1000, 24)])
    nv = len(v)
    bad = rng.integers(0, len(va) + len(vb), size=(3000, 3)).astype(np.int64)
    bad[np.arange(3000), rng.integers(0, 3, 3000)] = rng.choice([-1, nv, nv + 7, 2 ** 31 - 1, -2 ** 31], 3000)
    t = np.concatenate([ta, tb + len(va), bad.astype(np.int32)])
    t = t[rng.permutation(len(t))]
    for lo, hi in ((0, len(va)), (len(va), len(va) + len(vb))):
        rows = rng.choice(np.arange(lo, hi), 1000, replace=False)
        v[rows, rng.integers(0, 3, 1000)] = np.nan
    v[len(va) + 5] = np.nan                                # a vertex of the strip without any number
    return v, np.ascontiguousarray(t)


LARGE = {"many_singles": many_singles, "long_strip": long_strip, "both_with_dirt": both_with_dirt}
LARGE_BAD = {"many_singles": 0, "long_strip": 0, "both_with_dirt": 3000}


@pytest.fixture(scope="module")
def large(cuda):
    """name -> (vertices, triangles, model components, the two on the GPU): made and modelled once, never changed."""
    out = {}
    for name, make in LARGE.items():
        v, t = make()
        comps = M.components(v, t)
        out[name] = (v, t, comps) + upload(cuda, v, t)
    return out


def test_the_large_inputs_cross_the_thresholds(large):
    """The block counts are the library's own (mi3d_mesh_components_workspace: a uint32 per block of vertices and of
    triangles, a byte per vertex, each part padded to 8 bytes)."""
    from mi3d import _lib
    pad8 = lambda b: (b + 7) // 8 * 8                      # noqa: E731
    blocks = {}
    for name, (v, t, comps, _, _) in large.items():
        nbv, nbt = -(-len(v) // CLEAN_BLOCK), -(-len(t) // CLEAN_BLOCK)
        assert int(_lib.lib().mi3d_mesh_components_workspace(len(v), len(t))) == pad8(nbv * 4) + pad8(nbt * 4) + pad8(len(v))
        assert nbv > STAT_BLOCKS and nbt > STAT_BLOCKS and len(v) > STAT_PASS and len(t) > STAT_PASS    # every statistics loop
        assert nbv > SCAN_ROUND and nbv % 64 != 0                                                  # the vertex scan, ragged
        assert comps[4] == LARGE_BAD[name]
        blocks[name] = (nbv, nbt)
    assert blocks["long_strip"][1] > SCAN_ROUND and blocks["both_with_dirt"][1] > SCAN_ROUND        # the triangle scan
    label, faces = large["many_singles"][2][:2]
    assert np.array_equal(label, np.repeat(np.arange(0, 3 * SINGLES, 3), 3)) and int(faces.sum()) == SINGLES
    # labels one workgroup of a statistics kernel meets (its vertices / triangles over all strides) against its table
    assert -(-len(label) // STAT_PASS) * CLEAN_BLOCK // 3 > STAT_SLOTS // 2 and 2 * CLEAN_BLOCK >= STAT_SLOTS
    label, faces = large["long_strip"][2][:2]
    assert not label.any() and faces[0] == LONG_STRIP
    v, t, (label, faces, _, _, _), _, _ = large["both_with_dirt"]
    roots = np.flatnonzero((label == np.arange(len(v))) & (faces > 0))
    assert len(roots) == SINGLES + 1 and faces.max() == LONG_STRIP and np.isnan(v).any(1).sum() > 1900
    assert (faces[len(v) - 1000:] == 0).all() and (label[len(v) - 1000:] == np.arange(len(v) - 1000, len(v))).all()


@pytest.mark.parametrize("name", list(LARGE))
def test_large_components_against_the_model(cuda, large, name):
    from mi3d import mesh
    v, t, (rl, rf, rmin, rmax, bad), gv, gt = large[name]
    outs = [mesh._label_components(gv, gt) for _ in range(2)]          # the entry point itself: a bad index is counted
    label, faces, bmin, bmax, counts = outs[0]
    assert np.array_equal(label.cpu().numpy(), rl)
    assert np.array_equal(faces.cpu().numpy(), rf)
    assert bmin.cpu().numpy().tobytes() == rmin.tobytes() and bmax.cpu().numpy().tobytes() == rmax.tobytes()
    counts = counts.tolist()
    top = int(rf.max())
    assert counts[2] == bad and counts[3] == 0 and counts[5] == int((rf > 0).sum())
    assert counts[4] == (top << 32) | (~int(np.flatnonzero(rf == top)[0]) & 0xFFFFFFFF)
    for a, b in zip(outs[0], outs[1]):                                 # a second call, the same bytes
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    if bad == 0:                                                       # and the checked front door agrees
        for a, b in zip(mesh.components(gv, gt), outs[0][:4]):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    else:
        from mi3d import _lib
        with pytest.raises(_lib.Mi3dError, match=rf"\b{bad} of the {len(t)} triangles"):
            mesh.components(gv, gt)


def clean_through_the_abi(gv, gt, min_faces, min_diagonal, largest):
    """mi3d.mesh._clean without its refusal of bad indices: (vertices, triangles, vertex_map, counts after the count pass,
    counts after the emit pass)."""
    import torch
    from mi3d import _lib, mesh
    nv, nt, p = len(gv), len(gt), _lib.ptr
    label, faces, bmin, bmax, counts = mesh._label_components(gv, gt)
    need = int(_lib.lib().mi3d_mesh_components_workspace(nv, nt))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=gv.device)
    _lib.launch("mi3d_mesh_clean_count", gv, p(gt), nv, nt, p(label), p(faces), p(bmin), p(bmax), min_faces, min_diagonal,
                int(largest), p(ws), need, p(counts))
    host = counts.tolist()
    out_v = torch.empty(host[0], 3, dtype=torch.float32, device=gv.device)
    out_t = torch.empty(host[1], 3, dtype=torch.int32, device=gv.device)
    vmap = torch.empty(nv, dtype=torch.int32, device=gv.device)
    _lib.launch("mi3d_mesh_clean_emit", gv, p(gv), nv, p(gt), nt, p(label), p(ws), need, p(counts), p(out_v), host[0],
                p(out_t), host[1], p(vmap))
    return out_v, out_t, vmap, host, counts.tolist()


@pytest.mark.parametrize("name", list(LARGE))
def test_large_clean_against_the_model(cuda, large, name):
    import torch
    from mi3d import mesh
    v, t, comps, gv, gt = large[name]
    label, faces, bmin, bmax, bad = comps
    roots = np.flatnonzero((label == np.arange(len(v))) & (faces > 0))
    d2 = M.diag2(bmin[roots], bmax[roots])
    md = float(np.sqrt(np.float32(np.median(d2[np.isfinite(d2) & (d2 > 0)])), dtype=np.float32))
    both_sides = lambda keep: bool(keep[:SCAN_PASS].any() and keep[SCAN_PASS:].any())      # noqa: E731
    crossed = set()
    for min_faces, min_diagonal, largest in ((2, 0.0, False), (0, 0.0, True), (0, md, False)):
        what = f"{name} min_faces={min_faces} min_diagonal={min_diagonal!r} largest={largest}"
        rv, rt, rmap, rbad = M.clean(v, t, min_faces, min_diagonal, largest, comps=comps)
        cv, ct, cmap, counted, emitted = clean_through_the_abi(gv, gt, min_faces, min_diagonal, largest)
        assert counted[:4] == [len(rv), len(rt), rbad, 0] and rbad == bad and emitted[6] == 0, what
        assert cv.cpu().numpy().tobytes() == rv.tobytes(), what              # bit for bit, NaNs too, in the original order
        assert np.array_equal(ct.cpu().numpy(), rt) and np.array_equal(cmap.cpu().numpy(), rmap), what
        cv2, ct2, cmap2, _, _ = clean_through_the_abi(gv, gt, min_faces, min_diagonal, largest)
        assert cv2.cpu().numpy().tobytes() == cv.cpu().numpy().tobytes(), what
        assert torch.equal(ct2, ct) and torch.equal(cmap2, cmap), what
        if bad == 0:
            for a, b in zip(mesh.clean(gv, gt, min_faces, min_diagonal, largest), (cv, ct, cmap)):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), what
        # kept AND dropped elements on both sides of the first scan round's end: the base carried over is neither 0 nor
        # the round's size
        keep_v, keep_t = rmap >= 0, np.zeros(len(t), bool)
        ok = M.valid_triangles(t, len(v))
        keep_t[ok] = keep_v[t[ok, 0]]
        if both_sides(keep_v) and both_sides(~keep_v):
            crossed.add("v")
        if len(t) > SCAN_PASS and both_sides(keep_t) and both_sides(~keep_t):
            crossed.add("t")
        print(f"[clean] {what}: kept {len(rv)} of {len(v)} vertices, {len(rt)} of {len(t)} triangles")
    assert crossed == {"many_singles": {"v"}, "long_strip": set(), "both_with_dirt": {"v", "t"}}[name]
    if name == "long_strip":                                   # all or nothing: the base equals the round's size
        assert len(M.clean(v, t, 2, 0.0, False, comps=comps)[1]) == LONG_STRIP > SCAN_PASS


# ------------------------------------------------------------------------------------------------ bad indices, the C ABI

GUARD = 16


def guarded(cuda, rows, cols, dtype, fill):
    """A [rows (, cols)] view with GUARD rows of `fill` in front of it and behind it: (whole buffer, view)."""
    import torch
    shape = (rows + 2 * GUARD,) + ((cols,) if cols else ())
    whole = torch.full(shape, fill, dtype=dtype, device=cuda)
    return whole, whole[GUARD:GUARD + rows]


def test_bad_indices_are_counted_and_never_dereferenced(cuda):
    import torch
    from mi3d import _lib, mesh
    rng = np.random.default_rng(11)
    nv, nt = 300, 100
    v = coords(nv, 12)
    t = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    t[5, 1], t[40, 2] = -1, nv                            # row -1 and row nv lie in the guards below
    gv, gt = upload(cuda, v, t)
    for fn in (mesh.components, mesh.clean):
        with pytest.raises(_lib.Mi3dError, match=r"\b2 of the 100 triangles"):
            fn(gv, gt)

    # the entry points themselves, on buffers with guard rows on both sides
    rl, rf, rmin, rmax, bad = comps = M.components(v, t)
    rv, rt, rmap, _ = M.clean(v, t, 2, 0.0, False, comps=comps)
    assert bad == 2 and 0 < len(rt) < nt - 2
    p, lib = _lib.ptr, _lib.lib()
    pairs = {"label": guarded(cuda, nv, 0, torch.int32, -7), "faces": guarded(cuda, nv, 0, torch.int32, -7),
             "bmin": guarded(cuda, nv, 3, torch.float32, -7.0), "bmax": guarded(cuda, nv, 3, torch.float32, -7.0),
             "vmap": guarded(cuda, nv, 0, torch.int32, -7), "vin": guarded(cuda, nv, 3, torch.float32, -7.0),
             "out_v": guarded(cuda, len(rv), 3, torch.float32, -7.0),
             "out_t": guarded(cuda, len(rt), 3, torch.int32, -7)}
    view = {k: b for k, (a, b) in pairs.items()}
    view["vin"].copy_(gv)
    counts = torch.full((8,), 99, dtype=torch.int64, device=cuda)
    need = int(lib.mi3d_mesh_components_workspace(nv, nt))
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=cuda)
    _lib.launch("mi3d_mesh_components", gv, p(view["vin"]), nv, p(gt), nt, p(view["label"]), p(view["faces"]),
                p(view["bmin"]), p(view["bmax"]), p(counts))
    _lib.launch("mi3d_mesh_clean_count", gv, p(gt), nv, nt, p(view["label"]), p(view["faces"]), p(view["bmin"]),
                p(view["bmax"]), 2, 0.0, 0, p(ws), need, p(counts))
    host = counts.tolist()
    assert host[:4] == [len(rv), len(rt), 2, 0] and host[6:] == [0, 0]
    _lib.launch("mi3d_mesh_clean_emit", gv, p(view["vin"]), nv, p(gt), nt, p(view["label"]), p(ws), need, p(counts),
                p(view["out_v"]), len(rv), p(view["out_t"]), len(rt), p(view["vmap"]))
    assert counts.tolist()[6] == 0
    assert np.array_equal(view["label"].cpu().numpy(), rl) and np.array_equal(view["faces"].cpu().numpy(), rf)
    assert view["bmin"].cpu().numpy().tobytes() == rmin.tobytes() and view["bmax"].cpu().numpy().tobytes() == rmax.tobytes()
    assert view["out_v"].cpu().numpy().tobytes() == rv.tobytes() and np.array_equal(view["out_t"].cpu().numpy(), rt)
    assert np.array_equal(view["vmap"].cpu().numpy(), rmap)
    for name, (whole, _) in pairs.items():                # every guard row keeps its pattern
        assert torch.all(whole[:GUARD] == -7) and torch.all(whole[-GUARD:] == -7), name

    # caps below the kept counts: nothing past them is written, the overflow is counted
    out_v, out_t = torch.full((len(rv), 3), -7.0, device=cuda), torch.full((len(rt), 3), -7, dtype=torch.int32, device=cuda)
    _lib.launch("mi3d_mesh_clean_emit", gv, p(gv), nv, p(gt), nt, p(view["label"]), p(ws), need, p(counts), p(out_v),
                len(rv) - 3, p(out_t), len(rt) - 2, p(view["vmap"]))
    assert counts.tolist()[6] == 5
    assert out_v[:-3].cpu().numpy().tobytes() == rv[:-3].tobytes() and torch.all(out_v[-3:] == -7.0)
    assert np.array_equal(out_t[:-2].cpu().numpy(), rt[:-2]) and torch.all(out_t[-2:] == -7)


def test_emit_into_short_buffers_counts_what_does_not_fit(cuda):
    """A strip of 600 vertices / 598 triangles behind a one-triangle floater that min_faces=2 drops: both rows of block sums
    have three entries, and the one kept row of each kind that does not fit stands in the LAST workgroup, so only `block
    base + rank` finds it.  Caps one below the kept counts: a sentinel row behind each cap stays, the two losses are
    counted, vertex_map is complete, and every row below the caps is that of a full emit."""
    import torch
    from mi3d import _lib
    n = 600
    strip = np.stack([np.arange(n - 2), np.arange(1, n - 1), np.arange(2, n)], 1) + 3
    t = np.concatenate([[[0, 1, 2]], strip]).astype(np.int32)
    v = coords(n + 3, 23)
    nv, nt, kv, kt = n + 3, n - 1, n, n - 2
    assert -(-nv // CLEAN_BLOCK) == 3 and -(-nt // CLEAN_BLOCK) == 3
    rv, rt, rmap, _ = M.clean(v, t, 2, 0.0, False)
    assert (len(rv), len(rt)) == (kv, kt) and rmap[nv - 1] == kv - 1 and (rmap[:3] == -1).all()
    gv, gt = upload(cuda, v, t)
    full_v, full_t, full_map, counted, emitted = clean_through_the_abi(gv, gt, 2, 0.0, False)
    assert counted[:2] == [kv, kt] and emitted[6] == 0
    assert full_v.cpu().numpy().tobytes() == rv.tobytes() and np.array_equal(full_t.cpu().numpy(), rt)

    from mi3d import mesh
    p = _lib.ptr
    label, faces, bmin, bmax, counts = mesh._label_components(gv, gt)
    need = int(_lib.lib().mi3d_mesh_components_workspace(nv, nt))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=cuda)
    _lib.launch("mi3d_mesh_clean_count", gv, p(gt), nv, nt, p(label), p(faces), p(bmin), p(bmax), 2, 0.0, 0, p(ws), need,
                p(counts))
    out_v = torch.full((kv, 3), -7.0, device=cuda)             # row kv - 1: the sentinel behind the cap
    out_t = torch.full((kt, 3), -7, dtype=torch.int32, device=cuda)
    vmap = torch.full((nv,), -7, dtype=torch.int32, device=cuda)
    _lib.launch("mi3d_mesh_clean_emit", gv, p(gv), nv, p(gt), nt, p(label), p(ws), need, p(counts), p(out_v), kv - 1,
                p(out_t), kt - 1, p(vmap))
    host = counts.tolist()
    assert host[:2] == [kv, kt] and host[6] == 2
    assert torch.all(out_v[kv - 1] == -7.0) and torch.all(out_t[kt - 1] == -7)
    assert torch.equal(out_v[:kv - 1], full_v[:kv - 1]) and torch.equal(out_t[:kt - 1], full_t[:kt - 1])
    assert torch.equal(vmap, full_map) and np.array_equal(vmap.cpu().numpy(), rmap)


def test_c_abi_argument_checks_launch_nothing(cuda):
    """hipErrorInvalidValue (1) for NULL pointers, a short or misaligned workspace, sizes out of range and a bad
    min_diagonal; success (0) without a launch for an empty mesh.  Nothing refused touches its buffers."""
    import torch
    from mi3d import _lib
    lib, p = _lib.lib(), _lib.ptr
    nv, nt = 6, 2
    v = torch.zeros(nv, 3, device=cuda)
    t = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device=cuda)
    label = torch.full((nv,), -7, dtype=torch.int32, device=cuda)
    faces, vmap = label.clone(), label.clone()
    bmin, bmax = torch.full((nv, 3), -7.0, device=cuda), torch.full((nv, 3), -7.0, device=cuda)
    counts = torch.full((8,), 99, dtype=torch.int64, device=cuda)
    need = int(lib.mi3d_mesh_components_workspace(nv, nt))
    ws = torch.full((need // 8 + 2,), -7, dtype=torch.int64, device=cuda)
    out_v, out_t = torch.full((nv, 3), -7.0, device=cuda), torch.full((nt, 3), -7, dtype=torch.int32, device=cuda)
    s = _lib.stream(v)
    big = 2 ** 31
    with torch.cuda.device(cuda):
        comp = lambda **k: lib.mi3d_mesh_components(*[k.get(n, d) for n, d in (  # noqa: E731
            ("v", p(v)), ("nv", nv), ("t", p(t)), ("nt", nt), ("label", p(label)), ("faces", p(faces)), ("bmin", p(bmin)),
            ("bmax", p(bmax)), ("counts", p(counts)))], s)
        for k in ("v", "t", "label", "faces", "bmin", "bmax", "counts"):
            assert comp(**{k: None}) == 1, k
        assert comp(nv=big) == 1 and comp(nt=big) == 1
        assert comp(counts=_lib.C.c_void_p(counts.data_ptr() + 4)) == 1
        count = lambda **k: lib.mi3d_mesh_clean_count(*[k.get(n, d) for n, d in (  # noqa: E731
            ("t", p(t)), ("nv", nv), ("nt", nt), ("label", p(label)), ("faces", p(faces)), ("bmin", p(bmin)),
            ("bmax", p(bmax)), ("min_faces", 0), ("min_diagonal", 0.0), ("largest", 0), ("ws", p(ws)), ("need", need),
            ("counts", p(counts)))], s)
        for k in ("t", "label", "faces", "bmin", "bmax", "ws", "counts"):
            assert count(**{k: None}) == 1, k
        assert count(need=need - 1) == 1 and count(ws=_lib.C.c_void_p(ws.data_ptr() + 4)) == 1
        assert count(min_diagonal=-1.0) == 1 and count(min_diagonal=float("nan")) == 1 and count(nv=big) == 1
        emit = lambda **k: lib.mi3d_mesh_clean_emit(*[k.get(n, d) for n, d in (  # noqa: E731
            ("v", p(v)), ("nv", nv), ("t", p(t)), ("nt", nt), ("label", p(label)), ("ws", p(ws)), ("need", need),
            ("counts", p(counts)), ("out_v", p(out_v)), ("nv_cap", nv), ("out_t", p(out_t)), ("nt_cap", nt),
            ("vmap", p(vmap)))], s)
        for k in ("v", "t", "label", "ws", "counts", "out_v", "out_t", "vmap"):
            assert emit(**{k: None}) == 1, k
        assert emit(need=need - 1) == 1 and emit(nt=big) == 1
        # an empty mesh: success, and nothing is launched - not even the zeroing of counts
        assert comp(nv=0, nt=0, v=None, t=None, label=None, faces=None, bmin=None, bmax=None, counts=None) == 0
        assert count(nv=0, nt=0, t=None, label=None, faces=None, bmin=None, bmax=None, ws=None, need=0, counts=None) == 0
        assert emit(nv=0, nt=0, v=None, t=None, label=None, ws=None, need=0, counts=None, out_v=None, nv_cap=0,
                    out_t=None, nt_cap=0, vmap=None) == 0
    torch.cuda.synchronize(cuda)
    assert torch.all(counts == 99) and torch.all(ws == -7)
    for x in (label, faces, vmap, bmin, bmax, out_v, out_t):
        assert torch.all(x == -7)


def test_python_argument_checks_launch_nothing(cuda, monkeypatch):
    import torch
    from mi3d import _lib, mesh
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    v = torch.zeros(6, 3, device=cuda)
    t = torch.zeros(2, 3, dtype=torch.int32, device=cuda)
    bad_meshes = {
        "cpu vertices": (v.cpu(), t), "cpu triangles": (v, t.cpu()), "float64 vertices": (v.double(), t),
        "int64 triangles": (v, t.long()), "vertices [nv, 2]": (v[:, :2].contiguous(), t), "1-D vertices": (v[0], t),
        "triangles [nt, 4]": (v, torch.zeros(2, 4, dtype=torch.int32, device=cuda)), "1-D triangles": (v, t[0]),
        "non-contiguous vertices": (torch.zeros(6, 6, device=cuda)[:, ::2], t),
        "non-contiguous triangles": (v, torch.zeros(2, 6, dtype=torch.int32, device=cuda)[:, ::2]),
    }
    for what, (bv, bt) in bad_meshes.items():
        for fn in (mesh.components, mesh.clean):
            with pytest.raises(_lib.Mi3dError):
                fn(bv, bt)
            assert calls == [], what
    for kw in ({"min_faces": -1}, {"min_faces": 1.5}, {"min_diagonal": -0.1}, {"min_diagonal": float("nan")},
               {"largest": 1}):
        with pytest.raises(_lib.Mi3dError):
            mesh.clean(v, t, **kw)
        assert calls == [], kw


# ------------------------------------------------------------------------------------------------ export_mesh

R_EXPORT = 24


@pytest.fixture(scope="module")
def model(cuda):
    """The field of __graft_entry__.smoke() (what tests/test_mesh_gpu.py exports)."""
    import torch
    from mi3d import sds_step
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    m, _, _ = sds_step.build_training_state(opt, cuda, bitfield=0.5)
    with torch.no_grad():
        m.encoder.params.uniform_(-0.3, 0.3)
    return m


@pytest.fixture()
def floaters(cuda, model, monkeypatch):
    """export_mesh sees the sphere-and-specks volume instead of the random-weight field's own density, which has no
    floaters.  Yields (unfiltered vertices, unfiltered triangles) as GPU tensors: what export_mesh extracts."""
    import torch
    from mi3d import mesh
    thresh = float(min(model.mean_density, model.density_thresh) if model.cuda_ray else model.density_thresh)
    vol = torch.from_numpy(speck_volume(R_EXPORT)).to(cuda) + thresh
    monkeypatch.setattr(mesh, "extract_volume", lambda m, R: vol)
    h = 2.0 / (R_EXPORT - 1)
    return mesh.marching_cubes(vol, thresh, origin=(-1.0, -1.0, -1.0), spacing=(h, h, h))


@pytest.mark.parametrize("rule", [{"min_faces": 9}, {"largest": True}, {"min_diagonal": 0.3}])
def test_export_mesh_writes_the_cleaned_mesh(cuda, model, floaters, tmp_path, rule):
    import torch
    from mi3d import mesh
    uv, ut = floaters
    cv, ct, _ = mesh.clean(uv, ut, **rule)
    assert len(ut) - len(ct) == 30 * 8 and len(uv) - len(cv) == 30 * 6          # the thirty specks, nothing else
    v, f, c = model.export_mesh(str(tmp_path), resolution=R_EXPORT, **rule)
    assert v.dtype == np.float32 and f.dtype == np.int32 and c.dtype == np.float32
    assert v.tobytes() == cv.cpu().numpy().tobytes() and np.array_equal(f, ct.cpu().numpy())
    with torch.no_grad():
        albedo = model.density(cv)["albedo"].float()
    assert c.tobytes() == albedo.cpu().numpy().tobytes()                       # the colours of the kept vertices
    mtllib, pv, pc, pf, usemtl = parse_obj(tmp_path / "mesh.obj")
    assert np.array_equal(pv.astype(np.float32), v) and np.array_equal(pf, f.astype(np.int64) + 1)
    np.testing.assert_allclose(pc, c, atol=5e-7)                               # six decimals, as tests/test_mesh_gpu.py


def test_export_mesh_textures_and_normals_follow_the_cleaned_mesh(cuda, model, floaters, tmp_path):
    from mi3d import mesh
    uv, ut = floaters
    cv, ct, _ = mesh.clean(uv, ut, min_faces=9)
    T = 256
    cell, cell_all = mesh.atlas_cell(len(ct), T), mesh.atlas_cell(len(ut), T)
    assert cell > cell_all > 0                                                 # the specks' texels go to the object
    v, f, c, vt, image, vn = model.export_mesh(str(tmp_path), resolution=R_EXPORT, texture_size=T, normals=True,
                                               min_faces=9)
    assert np.array_equal(f, ct.cpu().numpy()) and v.tobytes() == cv.cpu().numpy().tobytes()
    assert vt.shape == (3 * len(ct), 2) and image.shape == (T, T, 3) and vn.shape == (len(cv), 3)
    # include/mi3d.h Part 9: vertices 0 and 1 of triangle 0 sit at the centres of texels (0, 0) and (c - 2, 0)
    assert round(float(vt[1, 0] - vt[0, 0]) * T) == cell - 2
    bi, bvt, _ = mesh.bake_texture(model, cv, ct, T)
    assert vt.tobytes() == bvt.cpu().numpy().tobytes() and image.tobytes() == bi.cpu().numpy().tobytes()
    assert vn.tobytes() == mesh.vertex_normals(model, cv).cpu().numpy().tobytes()
    lines = open(tmp_path / "mesh.obj").read().splitlines()
    count = lambda tag: sum(1 for ln in lines if ln.startswith(tag + " "))     # noqa: E731
    assert count("v") == len(cv) and count("vn") == len(cv) and count("vt") == 3 * len(ct) and count("f") == len(ct)


def test_export_mesh_with_nothing_left_names_the_components(cuda, model, floaters, tmp_path):
    from mi3d import _lib
    uv, ut = floaters
    sphere = len(ut) - 30 * 8
    with pytest.raises(_lib.Mi3dError, match=rf"31 components, the largest of {sphere} triangles"):
        model.export_mesh(str(tmp_path), resolution=R_EXPORT, min_faces=sphere + 1)
    with pytest.raises(_lib.Mi3dError, match="31 components"):
        model.export_mesh(str(tmp_path), resolution=R_EXPORT, min_diagonal=0.3, largest=True, min_faces=sphere + 1)
    assert not os.path.exists(tmp_path / "mesh.obj")


def test_export_mesh_defaults_do_not_touch_the_new_entry_points(cuda, model, floaters, tmp_path, monkeypatch):
    from mi3d import _lib
    uv, ut = floaters
    seen, launch = [], _lib.launch

    def spy(name, *a):
        seen.append(name)
        return launch(name, *a)
    monkeypatch.setattr(_lib, "launch", spy)
    a = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT)
    b = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, min_faces=None, min_diagonal=None, largest=False)
    assert "mi3d_mc_emit" in seen and not [n for n in seen if n.startswith("mi3d_mesh_")]
    assert len(a[1]) == len(ut) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for name in ("mesh.obj", "mesh.mtl"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    model.export_mesh(str(tmp_path / "c"), resolution=R_EXPORT, min_faces=9)
    assert [n for n in seen if n.startswith("mi3d_mesh_")] == ["mi3d_mesh_components", "mi3d_mesh_clean_count",
                                                               "mi3d_mesh_clean_emit"]
