"""CPU: the host side of the area-adaptive atlas (include/mi3d.h Part 20) - the library's plan against the NumPy
restatement of tests/atlas_adaptive_model.py, the geometry of the planned cells, the refusal, the ownership rule against
the bilinear footprint, the texel density the ladder promises, and the argument checks of the public interface."""
import numpy as np
import pytest

import atlas_adaptive_model as M

SIZES = (256, 512, 777)


def mc_sphere():
    from test_mc_tables_cpu import marching_cubes_ref
    from test_mesh_gpu import vol_a
    vol, iso, frame = vol_a()
    return marching_cubes_ref(vol, iso, origin=frame[0], spacing=frame[1])


@pytest.fixture(scope="module")
def histograms():
    """name -> (vertices, triangles, shape, hist) of the meshes a CPU can build, by the model's measure."""
    out = {}
    for name, (v, t) in (("plane", M.graded_plane()), ("latlong", M.latlong_sphere()), ("mc_sphere", mc_sphere())):
        shape, hist, bad = M.measure(v, t)
        assert bad == 0 and hist.sum() == len(t)
        out[name] = (v, t, shape, hist)
    assert len(out["plane"][1]) == 252 and len(out["latlong"][1]) == 3968
    return out


def random_histograms():
    rng = np.random.default_rng(20)
    for n in range(40):
        hist = np.zeros((64, 64), np.uint32)
        centre, spread, bins = rng.integers(20, 60), rng.integers(1, 12), rng.integers(1, 40)
        for _ in range(bins):
            bc, bb = np.clip(rng.normal(centre, spread, 2).round().astype(int), 0, 63)
            hist[bc, bb] += rng.integers(1, 10 ** rng.integers(1, 4))
        yield n, hist, int(rng.choice((64, 100, 256, 777, 1024, 4096)))


def check_cells(p):
    """Every cell of every class lies inside T x T and inside the rows used, and no two cells meet."""
    T = p["T"]
    taken = np.zeros((T, T), np.uint8)
    for r in p["records"]:
        X0, Y0 = M.cell_origin(r, np.arange(r["cells"]))
        w, h = r["a"] + 3, r["b"] + 3
        assert X0.min() >= 0 and (X0 + w).max() <= T and Y0.min() >= 0 and (Y0 + h).max() <= p["rows"] <= T
        for x, y in zip(X0, Y0):
            taken[y:y + h, x:x + w] += 1
    assert taken.max() == 1


def test_the_host_plan_is_the_models_plan(histograms):
    from mi3d import mesh
    cases = [(name, h[3], T) for name, h in histograms.items() for T in SIZES] + list(random_histograms())
    fits = 0
    for name, hist, T in cases:
        p, words = M.plan(hist, T), mesh.atlas_adaptive_plan(hist, T)
        assert (p is None) == (words is None), (name, T)
        if p is None:
            continue
        fits += 1
        assert words.dtype == np.int32 and words.shape == (M.PLAN_WORDS,) == (mesh.PLAN_WORDS,)
        assert np.array_equal(words, p["words"]), (name, T, np.flatnonzero(words != p["words"])[:8])
        if T <= 1024:
            check_cells(p)
        d = mesh._plan_dict(words)
        assert (d["shift"], d["rows"], d["kmax"]) == (p["shift"], p["rows"], p["kmax"])
        assert np.array_equal(d["classes"], p["classes"]) and d["fill"] == p["owned"] / (T * T) <= 1
        assert (d["clamped_small"], d["clamped_large"]) == (p["clamped_small"], p["clamped_large"])
    print(f"[atlas-adaptive] {fits} of {len(cases)} (histogram, T) pairs fit and agree word for word")
    assert fits >= 20
    for name in ("plane", "latlong"):
        assert all(M.plan(histograms[name][3], T) is not None for T in SIZES)


def test_the_shift_is_the_smallest_that_fits(histograms):
    """Scanning upward from 0 without assuming monotony: every smaller shift uses more than T rows."""
    for name, (_, _, _, hist) in histograms.items():
        for T in SIZES:
            p = M.plan(hist, T)
            if p is None:
                continue
            for s in range(p["shift"]):
                assert M.shelves(M.classes_of(hist, s, p["kmax"])[0], T)[0] > T


def test_a_mesh_that_does_not_fit_is_refused():
    """400 triangles at T = 64: class-(0, 0) cells are 5 x 5, 12 x 12 of them hold 288 triangles; 288 fit."""
    from mi3d import mesh
    for bins in ((0, 0), (30, 41), (63, 63)):
        hist = np.zeros((64, 64), np.uint32)
        hist[bins] = 400
        assert mesh.atlas_adaptive_plan(hist, 64) is None and M.plan(hist, 64) is None
        hist[bins] = 288
        words = mesh.atlas_adaptive_plan(hist, 64)
        assert words is not None and words[3] == 60 and np.array_equal(words, M.plan(hist, 64)["words"])
        hist[bins] = 289
        assert mesh.atlas_adaptive_plan(hist, 64) is None
    assert mesh.atlas_adaptive_plan(np.zeros((64, 64), np.uint32), 256) is None         # no triangles
    hist[bins] = 10
    assert mesh.atlas_adaptive_plan(hist, 63) is None and mesh.atlas_adaptive_plan(hist, 16385) is None
    with pytest.raises(mesh.Mi3dError):
        mesh.atlas_adaptive_plan(np.zeros(100, np.uint32), 256)


def test_kmax_follows_the_texture_size():
    from mi3d import mesh
    hist = np.zeros((64, 64), np.uint32)
    hist[63, 63] = 1
    for T, kmax in ((64, 9), (66, 9), (67, 10), (256, 13), (258, 13), (259, 14), (365, 15), (16384, 15)):
        assert M.kmax_of(T) == kmax
        words = mesh.atlas_adaptive_plan(hist, T)
        # the one triangle gets the largest legs that exist, at the smallest shift: both legs are clamped there
        assert words[2] == kmax and words[0] == 0 and words[9] == 2 and words[8] == 0 and words[3] == M.LEGS[kmax] + 3
    assert mesh.ATLAS_LEGS == M.LEGS == tuple(int(np.floor(2 ** (k / 2 + 1) + 0.5)) for k in range(16))


def test_ownership_is_the_bilinear_footprint_and_the_halves_are_disjoint():
    """All 144 class pairs with legs up to 91: half 0's set is what bilinear filtering touches in the UV triangle, half
    1's its point reflection, and the two never meet.  The library's rule, texel by texel, is the model's."""
    from mi3d import _lib
    rule = _lib.lib().mi3d_atlas_adaptive_owner
    pairs = 0
    for kb in range(12):
        for ka in range(12):
            a, b = M.LEGS[ka], M.LEGS[kb]
            h0, h1 = M.half0_mask(a, b), M.half1_mask(a, b)
            assert np.array_equal(h0, M.bilinear_footprint(a, b)), (a, b)
            assert not (h0 & h1).any(), (a, b)
            if a <= 23 and b <= 23 or (ka, kb) in ((11, 0), (0, 11), (11, 11), (10, 11)):
                got = np.array([[rule(ka, kb, x, y) for x in range(a + 3)] for y in range(b + 3)])
                assert np.array_equal(got, np.where(h0, 0, np.where(h1, 1, -1))), (a, b)
            pairs += 1
    assert pairs == 144
    assert rule(16, 0, 0, 0) == -2 and rule(0, 0, 5, 0) == -2 and rule(0, 0, 0, 5) == -2
    # a cell of height b + 2 would not do: with it the reflected half meets half 0 for unequal legs
    a, b = 11, 4
    short = M.half0_mask(a, b)[:b + 2]
    assert (short & short[::-1, ::-1]).any()


def test_density_over_unclamped_legs_stays_below_the_ladders_bound(histograms):
    """Texels per unit length over all legs that are not clamped differ by less than 1.6 (the ladder gives at most
    sqrt 2 * 1.061 / 0.972 = 1.543)."""
    for name in ("plane", "latlong"):
        v, t, shape, hist = histograms[name]
        for T in SIZES:
            p = M.plan(hist, T)
            d, clamped = M.densities(v, t, shape, p)
            assert (~clamped).sum() > len(t)
            ratio = d[~clamped].max() / d[~clamped].min()
            print(f"[atlas-adaptive] {name} T {T}: shift {p['shift']}, rows {p['rows']}, fill {p['owned'] / T / T:.3f}, "
                  f"clamped legs {p['clamped_small']} + {p['clamped_large']}, texels per unit length "
                  f"{d[~clamped].min():.1f} .. {d[~clamped].max():.1f}, ratio {ratio:.3f}")
            assert ratio < 1.6
            assert clamped.sum() == p["clamped_small"] + p["clamped_large"]
    assert M.plan(histograms["latlong"][3], 256)["clamped_small"] > 500              # the polar slivers


def test_the_longest_edge_faces_the_first_patch_corner(histograms):
    for name, (v, t, shape, _) in histograms.items():
        p = v[t].astype(np.float64)
        l = np.stack([np.linalg.norm(p[:, (k + 2) % 3] - p[:, (k + 1) % 3], axis=1) for k in range(3)], 1)
        rot = (shape & 3).astype(np.int64)
        assert (rot < 3).all() and (l[np.arange(len(t)), rot] >= l.max(1) * (1 - 1e-6)).all(), name


def test_arguments_are_checked_before_anything_runs():
    import torch
    from mi3d import mesh
    from mi3d._lib import Mi3dError
    v, t = M.graded_plane()
    v, t = torch.from_numpy(v), torch.from_numpy(t)
    for bad in ("Adaptive", "chart", None, 1, b"adaptive"):
        with pytest.raises(Mi3dError, match="atlas"):
            mesh.bake_texture(None, v, t, 256, atlas=bad)
        with pytest.raises(Mi3dError, match="atlas"):
            mesh.export(None, "/nonexistent", texture_size=256, atlas=bad)
        with pytest.raises(Mi3dError, match="atlas"):
            mesh.bake_views(None, v, t, 256, None, None, None, atlas=bad)
    with pytest.raises(Mi3dError, match="texture_size"):
        mesh.export(None, "/nonexistent", atlas="adaptive")
    for call in (lambda: mesh.bake_texture(None, v, t, 256, atlas="adaptive"), lambda: mesh.atlas_plan(v, t, 256)):
        with pytest.raises(Mi3dError, match="GPU"):                   # CPU tensors
            call()
    with pytest.raises(Mi3dError, match="texture_size"):
        mesh.atlas_plan(v, t, 63)


def test_the_unit_is_built_without_contraction_and_bound():
    import importlib.util
    import os
    from conftest import PKG
    from mi3d import _lib
    spec = importlib.util.spec_from_file_location("mi3d_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("atlasadaptive.hip", ["-ffp-contract=off"]) in b.UNITS and "mi3d_atlas_adaptive.h" in b.HEADERS
    for name in ("measure", "sort", "uv", "positions"):
        assert f"mi3d_atlas_adaptive_{name}" in _lib._SIGNATURES
    for name in ("workspace", "plan", "owner"):
        assert f"mi3d_atlas_adaptive_{name}" in _lib._LATE_SIGNATURES
    assert _lib.lib().mi3d_atlas_adaptive_workspace(0) == 0 and _lib.lib().mi3d_atlas_adaptive_workspace(2 ** 31) == 0
    assert _lib.lib().mi3d_atlas_adaptive_workspace(257) == 256 * 2 * 4
    assert _lib.lib().mi3d_abi_version() == 5
