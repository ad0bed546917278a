"""CPU: tests/mesh_smooth_model.py - the NumPy restatement of include/mi3d.h Part 16 that tests/test_mesh_smooth_gpu.py
holds the kernels to - against an independent brute-force version (an element at a time: Python integers for the sums,
dicts for the edge counts), on the very inputs the GPU tests use; that these inputs contain what their names say; the
properties that make the scheme worth having, with thresholds measured from the model here and written next to the
asserts; and the argument checks of mesh.smooth and export_mesh that need no GPU."""
import math

import numpy as np
import pytest

import mesh_smooth_model as M
from test_mc_tables_cpu import load_table, marching_cubes_ref


# ------------------------------------------------------------------------------------------------ brute force

def brute_setup(vertices, triangles, pin_border):
    """(rows: vertex -> list of neighbour indices, two per usable triangle; pinned border set; counts[0 .. 4])."""
    v = np.asarray(vertices, np.float32)
    nv = len(v)
    finite = [all(math.isfinite(float(x)) for x in v[i]) for i in range(nv)]
    rows, edges, unusable = {}, {}, 0
    for tri in np.asarray(triangles).tolist():
        a, b, c = tri
        if not all(0 <= x < nv for x in tri) or a == b or b == c or a == c or not all(finite[x] for x in tri):
            unusable += 1
            continue
        for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
            rows.setdefault(x, []).extend((y, z))
            edges[frozenset((x, y))] = edges.get(frozenset((x, y)), 0) + 1
    over = {i for i, r in rows.items() if len(r) // 2 > M.MAX_DEGREE}
    border = set()
    if pin_border:
        border = {x for e, n in edges.items() if n == 1 for x in e} - over
    counts = [unusable, nv - sum(finite), nv - len(rows), len(border), len(over)]
    return rows, border, over, counts


def brute_vertex(cur, rows, i, k, e):
    """One pass for vertex i from the positions `cur` (float32 [nv, 3]): three float32 coordinates."""
    out = []
    for a in range(3):
        S = 0
        for j in rows[i]:
            x = float(cur[j, a]) * 2.0 ** e                            # exact: a power of two
            S += 2 ** 40 if x >= 2 ** 40 else -2 ** 40 if x <= -2 ** 40 else 0 if x != x else round(x)   # ties to even
        m = float(S) / float(len(rows[i]))                             # Python floats: binary64, each operation rounded
        m = m * 2.0 ** -e
        p = float(cur[i, a])
        d = m - p
        d = k * d
        with np.errstate(over="ignore"):
            out.append(np.float32(p + d))
    return out


def brute(vertices, triangles, iterations, lam, mu, pin_border, max_move, e, only=None):
    """Part 16 once more.  `only`: the vertices to move (a sample; then `iterations` must be 1 and mu 0, because one
    pass needs no neighbour's result) - None: all."""
    v0 = np.ascontiguousarray(vertices, np.float32)
    rows, border, over, counts = brute_setup(v0, triangles, pin_border)
    movers = [i for i in (sorted(rows) if only is None else only) if i in rows and i not in border and i not in over]
    cur, held = v0.copy(), set()
    for _ in range(iterations):
        for k in (lam, mu):
            if k == 0:
                continue
            new, held = cur.copy(), set()
            for i in movers:
                p = brute_vertex(cur, rows, i, float(k), e)
                if max_move is not None:
                    for a in range(3):
                        lo, hi = v0[i, a] - np.float32(max_move), v0[i, a] + np.float32(max_move)
                        kept = lo if p[a] < lo else hi if p[a] > hi else p[a]
                        if kept != p[a]:
                            held.add(i)
                        p[a] = kept
                new[i] = p
            cur = new
    return cur, counts + [len(held), 0]


def same(a, b):
    return a[0].dtype == b[0].dtype == np.float32 and a[0].tobytes() == b[0].tobytes() and list(a[1]) == list(b[1])


@pytest.fixture(scope="module")
def surfaces():
    rows, _ = load_table()
    out = {}
    for name, (R, make) in M.VOLUMES.items():
        h = np.float32(2.0 / (R - 1))
        out[name] = (R,) + marching_cubes_ref(make(), 0.0, (-1, -1, -1), (h, h, h), rows)
    return out


# ------------------------------------------------------------------------------------------------ model vs brute force

@pytest.mark.parametrize("name", list(M.VOLUMES))
def test_model_equals_brute_force_on_the_surfaces(surfaces, name):
    """Two iterations (four passes) with the clamp; the larger spheres one, to stay within seconds."""
    R, v, t = surfaces[name]
    h = 2.0 / (R - 1)
    assert len(v) > 500 and len(t) > 1000
    its = 1 if len(v) > 5000 else 2
    got = M.smooth(v, t, its, max_move=0.1 * h, e=M.EXTENT_E)
    assert same(got, brute(v, t, its, M.LAMBDA, M.MU, True, 0.1 * h, M.EXTENT_E))
    assert got[1][:5] == [0, 0, 0, 0, 0]                                 # closed manifolds: no border, nothing unusable
    assert not np.array_equal(got[0], v)


@pytest.mark.parametrize("name", list(M.VOLUMES))
def test_the_binding_max_move_binds(surfaces, name):
    """The runs the GPU test repeats: the one with max_move holds vertices at the box, the others hold none."""
    R, v, t = surfaces[name]
    h = 2.0 / (R - 1)
    for its, lam, mu, pin, mm in M.SURFACE_RUNS:
        out, counts = M.smooth(v, t, its, lam, mu, pin, None if mm is None else mm * h, e=M.EXTENT_E)
        assert (counts[5] > 0) == (mm is not None), (name, its, counts)
        assert np.isfinite(out).all()


@pytest.mark.parametrize("name", list(M.HAND_MADE))
@pytest.mark.parametrize("run", M.HAND_RUNS)
def test_model_equals_brute_force_on_the_hand_made_cases(name, run):
    make, extent = M.HAND_MADE[name]
    v, t = make()
    its, lam, mu, pin, mm = run
    e = M.fraction_bits(extent)
    assert same(M.smooth(v, t, its, lam, mu, pin, mm, e=e), brute(v, t, its, lam, mu, pin, mm, e))


def test_model_equals_brute_force_on_a_sample_of_the_big_sheet():
    """One pass.  The brute force moves every 173rd vertex, from the triangles that cite one of them alone (a sampled
    vertex keeps its whole umbrella, so its row and its border status are those of the full sheet); the border of the
    sheet is known without either."""
    v, t = M.big_sheet()
    assert len(v) == 360_000 and len(v) > M.S.SCAN_ROUND and -(-len(v) // 256) > 1024    # a second round of the scan
    e = M.fraction_bits(1024.0)
    got, counts = M.smooth(v, t, 1, M.LAMBDA, 0.0, True, None, e=e)
    only = np.arange(0, len(v), 173)
    around = t[np.isin(t, only).any(1)]
    ref, _ = brute(v, around, 1, M.LAMBDA, 0.0, True, None, e, only=only.tolist())
    assert got[only].tobytes() == ref[only].tobytes()
    i, j = np.arange(len(v)) // 600, np.arange(len(v)) % 600
    edge = (i == 0) | (i == 599) | (j == 0) | (j == 599)
    assert counts == [0, 0, 0, 4 * 599, 0, 0, 0] and edge.sum() == 4 * 599
    moved = (got != v).any(1)
    assert np.array_equal(moved, ~edge) and 0 < edge[only].sum() < 100 and len(only) > 2000


# ------------------------------------------------------------------------------------------------ the inputs are what they claim

def test_hand_made_cases_hold_what_they_name():
    v, t = M.open_sheet()
    assert len(v) == 400 and M.smooth(v, t, 1, e=33)[1] == [0, 0, 0, 76, 0, 0, 0]
    v, t = M.fan300()
    rows, border, over, counts = brute_setup(v, t, True)
    assert len(rows[0]) == 600 and 0 not in border and len(border) == 300 and counts == [0, 0, 0, 300, 0]
    v, t = M.degree_limit_case()
    rows, border, over, counts = brute_setup(v, t, True)
    assert len(rows[0]) // 2 == M.MAX_DEGREE == 1024 and over == {1025} and len(rows[1025]) // 2 == 1025
    out, counts = M.smooth(v, t, 1, e=35)
    assert counts[4] == 1 and out[1025].tobytes() == v[1025].tobytes() and out[0].tobytes() != v[0].tobytes()
    v, t = M.fans_case()
    rows, border, over, counts = brute_setup(v, t, True)
    edges = {}
    for tri in t.tolist():
        for x, y in ((0, 1), (1, 2), (2, 0)):
            edges[frozenset((tri[x], tri[y]))] = edges.get(frozenset((tri[x], tri[y])), 0) + 1
    assert max(edges.values()) == 3 and counts[2] == 2 and not {11, 12} & set(rows)     # an edge of three triangles
    v, t = M.bad_case()
    nv = len(v)
    assert (t == -1).sum() == 1 and (t == nv).sum() == 1 and (t == 2 ** 31 - 1).sum() == 1
    assert np.isnan(v).sum() == 1 and np.isinf(v).sum() == 1 and (t[:, 0] == t[:, 2]).sum() == 1
    e = M.fraction_bits(M.HAND_MADE["bad"][1])
    assert float(v[65, 2]) * 2.0 ** e > 2 ** 40 and np.abs(M.quantise(v, e)).max() == 2 ** 40 and e == 31
    out, counts = M.smooth(v, t, 2, pin_border=False, e=e)
    assert counts[0] > 4 + 2 and counts[1] == 2 and counts[2] >= 3 and counts[:2] + counts[3:] == [counts[0], 2, 0, 0, 0, 0]
    assert out[144].tobytes() == v[144].tobytes() and out[40].tobytes() == v[40].tobytes()   # NaN bits and all
    assert np.isfinite(out[np.isfinite(v).all(1)]).all()


# ------------------------------------------------------------------------------------------------ properties

@pytest.fixture(scope="module")
def noisy(surfaces):
    R, v, t = surfaces["sphere24"]
    return M.noisy_sphere(v), t


def test_radial_rms_falls_with_every_iteration_and_the_volume_stays(noisy):
    """The marching-cubes sphere of radius 0.6 at 24^3 with 3 % radial noise.  Measured from the model: the radial rms
    falls from 0.01055 to 0.00438 (0.415 of it) over ten lambda | mu iterations, every iteration lowering it; the enclosed
    volume ends at 1.0059 of the input's.  Ten lambda-only passes end at 0.8735 of it.  Margin: 1 %."""
    v, t = noisy
    rms = [M.radial_rms(v, 0.6)]
    for n in range(1, 11):
        rms.append(M.radial_rms(M.smooth(v, t, n, e=M.EXTENT_E)[0], 0.6))
    assert all(b < a for a, b in zip(rms, rms[1:])), rms
    assert rms[0] > 0.0100 and rms[-1] < 0.45 * rms[0], rms
    vol0 = M.enclosed_volume(v, t)
    taubin = M.enclosed_volume(M.smooth(v, t, 10, e=M.EXTENT_E)[0], t) / vol0
    laplace = M.enclosed_volume(M.smooth(v, t, 10, mu=0.0, e=M.EXTENT_E)[0], t) / vol0
    assert abs(taubin - 1) < 0.01, taubin
    assert laplace < 0.90, laplace                                       # lambda alone shrinks: outside the margin


def test_pinned_border_stays_bit_for_bit():
    v, t = M.open_sheet()
    ij = np.arange(400)
    edge = (ij // 20 == 0) | (ij // 20 == 19) | (ij % 20 == 0) | (ij % 20 == 19)
    assert edge.sum() == 76
    out, counts = M.smooth(v, t, 5, pin_border=True, e=33)
    assert counts[3] == 76 and out[edge].tobytes() == v[edge].tobytes() and (out[~edge] != v[~edge]).any(1).all()
    out, counts = M.smooth(v, t, 5, pin_border=False, e=33)
    assert counts[3] == 0 and (out[edge] != v[edge]).any(1).all()


def test_max_move_bounds_every_coordinate(noisy):
    v, t = noisy
    free = M.smooth(v, t, 10, e=M.EXTENT_E)[0]
    assert np.abs(free - v).max() > 0.01
    for mm in (0.0, 0.002, 0.01):
        out, counts = M.smooth(v, t, 10, max_move=mm, e=M.EXTENT_E)
        lo, hi = v - np.float32(mm), v + np.float32(mm)
        assert np.all(out >= lo) and np.all(out <= hi) and counts[5] > 0
    assert M.smooth(v, t, 10, max_move=0.0, e=M.EXTENT_E)[0].tobytes() == v.tobytes()
    out, counts = M.smooth(v, t, 10, max_move=1.0, e=M.EXTENT_E)
    assert counts[5] == 0 and out.tobytes() == free.tobytes()


def test_permuting_the_triangles_changes_no_byte(noisy):
    v, t = noisy
    rng = np.random.default_rng(5)
    ref = M.smooth(v, t, 4, max_move=0.01, e=M.EXTENT_E)
    shuffled = np.roll(t[rng.permutation(len(t))], 1, axis=1)           # another order, another first corner
    assert same(M.smooth(v, shuffled, 4, max_move=0.01, e=M.EXTENT_E), ref)


def test_mu_zero_is_the_lambda_only_passes(noisy):
    """mu = 0 launches no second pass: n iterations are n single passes chained by hand."""
    v, t = noisy
    chained = v
    for _ in range(3):
        chained = M.smooth(chained, t, 1, M.LAMBDA, 0.0, e=M.EXTENT_E)[0]
    assert M.smooth(v, t, 3, M.LAMBDA, 0.0, e=M.EXTENT_E)[0].tobytes() == chained.tobytes()
    assert M.smooth(v, t, 3, 0.0, 0.0, e=M.EXTENT_E)[0].tobytes() == v.tobytes()
    # and (lambda, mu) is lambda then mu
    two = M.smooth(M.smooth(v, t, 1, M.LAMBDA, 0.0, e=M.EXTENT_E)[0], t, 1, M.MU, 0.0, e=M.EXTENT_E)[0]
    assert M.smooth(v, t, 1, e=M.EXTENT_E)[0].tobytes() == two.tobytes()


def test_fraction_bits_is_the_products():
    from mi3d import mesh
    for extent in (0.0, 1e-30, 0.3, 0.5, 1.0, 1.0001, 2.0, 600.0, 3e30, 3e38):
        e = mesh.smooth_fraction_bits(extent)
        assert e == M.fraction_bits(extent) and 0 <= e <= 40
        assert e == 0 or extent * 2.0 ** e <= 2.0 ** 38
    assert mesh.smooth_fraction_bits(1.0) == M.EXTENT_E == 37
    assert (mesh.SMOOTH_LAMBDA, mesh.SMOOTH_MU) == (M.LAMBDA, M.MU) == (0.5, -0.53)
    assert mesh.SMOOTH_COUNTS == M.COUNTS


# ------------------------------------------------------------------------------------------------ argument checks

BAD_ARGUMENTS = [
    ({"iterations": 0}, "iterations"), ({"iterations": 1001}, "iterations"), ({"iterations": 2.0}, "iterations"),
    ({"iterations": True}, "iterations"), ({"iterations": "3"}, "iterations"), ({"iterations": -1}, "iterations"),
    ({"iterations": 3, "lam": 1.5}, "lam"), ({"iterations": 3, "lam": float("nan")}, "lam"),
    ({"iterations": 3, "lam": "0.5"}, "lam"), ({"iterations": 3, "mu": -1.01}, "mu"),
    ({"iterations": 3, "mu": float("-inf")}, "mu"), ({"iterations": 3, "mu": None}, "mu"),
    ({"iterations": 3, "pin_border": 1}, "pin_border"), ({"iterations": 3, "max_move": -0.1}, "max_move"),
    ({"iterations": 3, "max_move": float("nan")}, "max_move"), ({"iterations": 3, "max_move": "1"}, "max_move"),
]


@pytest.mark.parametrize("kw, match", BAD_ARGUMENTS + [({"iterations": 3, "extent": -1.0}, "extent"),
                                                       ({"iterations": 3, "extent": float("inf")}, "extent")])
def test_smooth_checks_its_arguments_first_on_any_device(kw, match):
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match=match):
        mesh.smooth(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), **kw)
    with pytest.raises(_lib.Mi3dError, match=match):
        mesh.smooth("no tensor", None, **kw)                             # before the tensors are looked at


def test_smooth_refuses_cpu_tensors_after_the_arguments():
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="GPU"):
        mesh.smooth(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), 3, max_move=0.1, extent=1.0)


class _CpuModel:
    """What export looks at before it needs a GPU."""
    import torch as _torch
    aabb_train = _torch.zeros(6)
    grid_size, cuda_ray, mean_density, density_thresh = 16, False, 0.0, 10.0


@pytest.mark.parametrize("smooth, match", [(kw["iterations"] if len(kw) == 1 else kw, m) for kw, m in BAD_ARGUMENTS]
                         + [({"lam": 0.5}, "iterations is required"), ({"iterations": 3, "extent": 1.0}, "unknown keys"),
                            ({"iterations": 3, "lamda": 0.5}, "unknown keys")])
def test_export_checks_smooth_before_the_device(tmp_path, smooth, match):
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match=match):
        mesh.export(_CpuModel(), str(tmp_path), smooth=smooth)


@pytest.mark.parametrize("smooth", [None, 1, 3, np.int64(1000), {"iterations": 2},
                                    {"iterations": 2, "lam": 0.6, "mu": -0.6, "pin_border": False, "max_move": 0.5}])
def test_export_with_a_good_smooth_reaches_the_device_check(tmp_path, smooth):
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError, match="export_mesh needs the model on the GPU"):
        mesh.export(_CpuModel(), str(tmp_path), smooth=smooth)


def test_export_mesh_passes_the_argument_on():
    import inspect
    from mi3d import mesh, renderer
    assert inspect.signature(renderer.NeRFRenderer.export_mesh).parameters["smooth"].default is None
    assert inspect.signature(mesh.export).parameters["smooth"].default is None
    doc = renderer.NeRFRenderer.export_mesh.__doc__
    assert "smooth" in doc and "analytic normal" in doc


def test_binding_build_and_workspace_query():
    import importlib.util
    import os
    from conftest import PKG
    from mi3d import _lib
    assert "mi3d_mesh_smooth" in _lib._SIGNATURES and "mi3d_mesh_smooth_workspace" in _lib._LATE_SIGNATURES
    spec = importlib.util.spec_from_file_location("mi3d_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("meshsmooth.hip", ["-ffp-contract=off"]) in b.UNITS
    ws = _lib.lib().mi3d_mesh_smooth_workspace                          # host only: no GPU here
    pad8 = lambda n: (n + 7) // 8 * 8                                   # noqa: E731
    for nv, nt in ((1, 0), (3, 1), (255, 256), (256, 257), (1000, 2000), (360_000, 717_602), (2 ** 31 - 1, 2 ** 30)):
        # cursors, offsets (nv + 1), block sums per 256 vertices, flags, the second vertex buffer, 3 nt rows of 8 bytes
        assert ws(nv, nt) == (pad8(4 * nv) + pad8(4 * (nv + 1)) + pad8(4 * -(-nv // 256)) + pad8(nv) + pad8(12 * nv)
                              + 24 * nt), (nv, nt)
    assert ws(0, 0) == 0 and ws(0, 5) == 0 and ws(2 ** 31, 1) == 0 and ws(1, 2 ** 30 + 1) == 0
