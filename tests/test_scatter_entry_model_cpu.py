"""The per-entry model of the table gradient (tests/scatter_entry_model.py) on the CPU: the oracle's own backward - a
sequential binary32 sum - stays inside the model's binary32 term, and faults planted into the oracle's result do not.

What the faults show (measured here, printed by the tests): the older GPU tests judge the whole gradient by
|g - ref|.max() <= 2e-5 |ref|.max() + 1e-6, and |ref|.max() sits on level 0 where dozens of samples share an entry.  Of
100 faults planted on the FINEST level of the default grid (3000 ray-like samples x 7 stencil points), each at least 2^-16
of its element's magnitude, that tolerance sees
    unit-normal gradients:            dropped smallest contribution 97, one contribution x (1 + 2^-12) 0, x shares
                                      exchanged 95, a contribution moved to entry e ^ 1 99
    gradients over 2^-14 ... 2^14:    dropped 25, scaled 0, exchanged 30, moved 29
and the per-entry bound sees 100 of 100 of each.  On the 8-level grid with 2^12-entry tables collisions make m about 40 on
the finest level and the bound naturally looser: there the dropped SMALLEST contribution, whatever its size, is seen 70
times of 100 with unit gradients (old tolerance: 12) and 20 times with wide ones (old: 0) - the test asserts those
counts, not 100 %."""
import numpy as np
import pytest

import scatter_entry_model as M
from test_grid_points_gpu import _points, _ray_like_points
from test_hashgrid_gpu import CONFIGS

N, P = 3000, 7
GRIDS = dict(CONFIGS, log2_10=dict(n_levels=16, log2_hashmap_size=10, base_resolution=16, per_level_scale=None),
             log2_12=dict(n_levels=16, log2_hashmap_size=12, base_resolution=16, per_level_scale=None))
_CACHE = {}


def _inputs(oracle, grid, grads):
    """3000 ray-like samples x the 7-point stencil as ONE point list (so that one oracle call sums them sequentially), the
    oracle's backward, the model, the lattice of every contribution.  Built once per (grid, gradients), never written."""
    key = (grid, grads)
    if key not in _CACHE:
        from mi3d import grid_ops
        cfg = oracle.GridConfig(n_features_per_level=2, **GRIDS[grid])
        rng = np.random.default_rng(14)
        x = _ray_like_points(rng, N, 1.0)
        x[:8] = 1.0
        offs, P0 = grid_ops.stencil_offsets(center=True, second=False)
        assert offs.shape[0] == P
        x01 = np.concatenate([((q + np.float32(1.0)) / np.float32(2.0)).astype(np.float32) for q in _points(x, x, offs, P0, 1.0)])
        d = rng.normal(size=(N * P, cfg.n_levels, 2)).astype(np.float32)
        if grads == "wide":
            # the shape of GradScaler-scaled binary16 gradients: exact powers of two, 2^-14 ... 2^14 within every level,
            # one per (stretch of 50 consecutive samples, level) - the magnitude of a real gradient varies along a ray, not
            # from one stencil point to the next.  (Independent exponents per contribution would put most faults below
            # what a binary32 sum can hold beside its largest term: nothing any result could show.)
            ex = rng.integers(-14, 15, size=(N // 50, cfg.n_levels))
            ex = np.tile(np.repeat(ex, 50, axis=0), (P, 1))                       # rows are point-major: p * N + s
            d = (d * np.exp2(ex).astype(np.float32)[:, :, None]).astype(np.float32)
        d[100:140] = 0
        d[:, 2] = 0
        g = oracle.hashgrid_backward(x01, d.reshape(N * P, -1), cfg)
        mdl = M.entry_model(oracle, cfg, [x01], [d])
        idx, w = oracle.hashgrid_indices(x01, cfg)
        for a in (x01, d, g, idx, w):
            a.setflags(write=False)
        _CACHE[key] = (cfg, x01, d, g, mdl, idx, w)
    return _CACHE[key]


@pytest.mark.parametrize("grads", ["unit", "wide"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_oracle_backward_is_inside_the_binary32_term(oracle, grid, grads):
    """The "atomic" route's bound is the binary32 term alone with c = 1 - w d rounded once, any order of additions - and the
    oracle's backward is exactly such a sum: it must fit, on every element, and where nothing contributes it is 0.0."""
    cfg, _, _, g, mdl, _, _ = _inputs(oracle, grid, grads)
    bound = M.entry_bound(mdl, ["atomic"] * cfg.n_levels)
    assert all(np.array_equal(bound[t], np.zeros_like(bound[t])) for t in ("reduce", "gather", "rec16"))
    report = M.assert_entries(g, mdl, bound, f"oracle {grid} {grads}")
    assert max(r["worst_ratio"] for r in report) > 0.05          # (a bound the result never comes near would test nothing)


def _plant(cfg, mdl, d, idx, w, kind, rng, count=100, least=2.0 ** -16):
    """`count` faults of one kind on the finest level, each on an element (and partner element) of its own.  Returns the
    changes [(element, delta), ...] per fault.  `least`: only faults that change an element by at least that share of its A
    - its leading 16 bits; the finest level of the default grid has m + c <= 2^6, so such a fault is 2^2 above the bound
    whatever the gradients, while one far below 2^-24 A is nothing a binary32 result could show (wide gradients put two
    contributions 2^28 apart into one element now and then).  None: every fault counts."""
    l = cfg.n_levels - 1
    base = int(cfg.offsets[l])
    flat = (idx[:, l, :].astype(np.int64) + base) * 2                               # [rows, 8]: feature-0 elements
    v = w[:, l, :].astype(np.float64) * d[:, l, 0].astype(np.float64)[:, None]       # [rows, 8]
    rows, ks = np.nonzero(v != 0)
    order = rng.permutation(rows.size)
    used, faults = set(), []
    for j in order:
        r, k = int(rows[j]), int(ks[j])
        el = int(flat[r, k])
        if kind == "drop":       # the SMALLEST non-zero contribution of the element goes missing
            sel = (flat == el) & (v != 0)
            cand = np.abs(np.where(sel, v, np.inf))
            r, k = np.unravel_index(int(np.argmin(cand)), cand.shape)
            change = [(el, -v[r, k])]
        elif kind == "scale":    # a weight off by 2^-12
            change = [(el, v[r, k] * 2.0 ** -12)]
        elif kind == "swap":     # the x-pair's two shares exchanged: fx <-> 1 - fx on both entries
            el1 = int(flat[r, k ^ 1])
            dv = v[r, k ^ 1] - v[r, k]
            if el1 == el or abs(dv) < 2.0 ** -12 * max(abs(v[r, k]), abs(v[r, k ^ 1])):
                continue         # (a pair on one entry, or shares equal to within the 2^-12 the scaled fault has)
            change = [(el, dv), (el1, -dv)]
        else:                    # "move": the contribution lands on entry e ^ 1
            el1 = ((el // 2 - base) ^ 1) * 2 + base * 2
            change = [(el, -v[r, k]), (el1, v[r, k])]
        if any(e in used for e, _ in change):
            continue
        if least is not None and not any(abs(dv) >= least * mdl.A[e] for e, dv in change):
            continue
        used.update(e for e, _ in change)
        faults.append(change)
        if len(faults) == count:
            break
    assert len(faults) == count
    return faults


def _seen(g, faults, mdl, total):
    """Of the planted faults, how many the per-entry bound flags and how many the old global tolerance flags."""
    mut = g.astype(np.float64)
    for change in faults:
        for e, dv in change:
            mut[e] += dv
    mut = mut.astype(np.float32).astype(np.float64)          # what a kernel would hand back: binary32
    err = np.abs(mut - mdl.ref)
    new_flags = (err > total) | ((total == 0) & (mut != 0))
    old_flags = M.old_tolerance_misses(mut, mdl.ref)
    new = sum(any(new_flags[e] for e, _ in ch) for ch in faults)
    old = sum(any(old_flags[e] for e, _ in ch) for ch in faults)
    touched = np.zeros(mut.size, bool)
    for ch in faults:
        for e, _ in ch:
            touched[e] = True
    assert not new_flags[~touched].any()                      # nothing but the planted faults is flagged
    return new, old


# the widest binary32 term a GPU route is held to: pair records with the extra pair summed first, c = 6 + 1
def _widest(mdl, cfg):
    b = M.entry_bound(mdl, ["atomic"] * cfg.n_levels)
    total = (mdl.m + (M.ROUTE_C["pair"] + 1)) * M.U * mdl.A
    total[mdl.m == 0] = 0.0
    assert (total >= b["total"]).all()
    return total


@pytest.mark.parametrize("grads", ["unit", "wide"])
@pytest.mark.parametrize("kind", ["drop", "scale", "swap", "move"])
def test_planted_faults_miss_the_bound(oracle, kind, grads):
    """100 faults of each kind on the finest level of the default grid: the per-entry bound flags every one, the old
    tolerance does not (the counts are in the module docstring)."""
    cfg, _, d, g, mdl, idx, w = _inputs(oracle, "default16", grads)
    faults = _plant(cfg, mdl, d, idx, w, kind, np.random.default_rng(5))
    new, old = _seen(g, faults, mdl, _widest(mdl, cfg))
    print(f"default16 {grads} {kind}: per-entry bound sees {new} of 100, old global tolerance {old} of 100")
    assert int(mdl.m[mdl.level_slice(cfg.n_levels - 1)].max()) + M.ROUTE_C["pair"] + 1 <= 64    # (what `least` rests on)
    assert new == 100
    assert old < 100 or kind == "move"     # (unit gradients: a whole contribution on the wrong entry is coarse enough for both)


@pytest.mark.parametrize("grads", ["unit", "wide"])
def test_dropped_contribution_on_the_small_hash_grid(oracle, grads):
    """small_hash: 2^12-entry tables, about 40 contributions per element of the finest level, from unrelated places.  The
    smallest of m contributions carries a share of A that shrinks faster than 1 / m while the bound grows like m, so some
    of these faults are below what a binary32 sum of the element resolves - legitimately invisible.  Unit gradients: the
    measured rate is 70 of 100; wide gradients mix magnitudes 2^28 apart in one element, where the
    smallest contribution is seldom resolvable.  The measured counts are asserted as they are."""
    cfg, _, d, g, mdl, idx, w = _inputs(oracle, "small_hash", grads)
    faults = _plant(cfg, mdl, d, idx, w, "drop", np.random.default_rng(5), least=None)
    new, old = _seen(g, faults, mdl, _widest(mdl, cfg))
    print(f"small_hash {grads} drop: per-entry bound sees {new} of 100, old global tolerance {old} of 100")
    # what was measured (inputs and faults are seeded): a weaker bound or model moves these counts
    assert (new, old) == ((70, 12) if grads == "unit" else (20, 0))


def test_a_nan_or_inf_is_a_miss(oracle):
    """A non-finite value on an element WITH contributions (|nan - ref| > bound is False) and on one that owes 0.0: both
    must fail, on their level and nowhere else."""
    cfg, _, _, g, mdl, _, _ = _inputs(oracle, "small_hash", "unit")
    bound = M.entry_bound(mdl, ["pair"] * cfg.n_levels)
    assert M.check_entries(g, mdl, bound)[1] == []
    busy = int(np.flatnonzero(mdl.m > 0)[-1])
    idle = int(np.flatnonzero(mdl.m == 0)[0])
    for at, bad in ((busy, np.nan), (busy, np.inf), (busy, -np.inf), (idle, np.nan), (idle, np.inf)):
        mut = g.copy()
        mut[at] = bad
        report, failures = M.check_entries(mut, mdl, bound)
        assert len(failures) == 1 and failures[0]["misses"] == 1, (at, bad, failures)
        assert mdl.level_slice(failures[0]["level"]).start <= at < mdl.level_slice(failures[0]["level"]).stop
        with pytest.raises(AssertionError):
            M.assert_entries(mut, mdl, bound)


def test_bound_terms_follow_the_routes(oracle):
    """The terms a route carries and the ones it does not; m == 0 means bound 0."""
    cfg, x01, d, _, mdl, _, _ = _inputs(oracle, "small_hash", "unit")
    L = cfg.n_levels
    for route, half, want in (("atomic", False, {"binary32"}), ("pair", False, {"binary32", "reduce"}),
                              ("pair", True, {"binary32", "reduce", "rec16"}), ("single", True, {"binary32", "reduce"}),
                              ("coarse", True, {"binary32", "reduce", "gather"})):
        b = M.entry_bound(mdl, [route] * L, half=half)
        assert {t for t in M.TERMS if b[t].any()} == want, (route, half)
        assert (b["total"][mdl.m == 0] == 0).all() and (b["total"][mdl.m > 0] > 0).all()
        assert b["c"] == [M.ROUTE_C[route]] * L
    # the extra pair: one more rounding where it is summed first, none for binary16 pair records and the atomic routes
    mdl2 = M.entry_model(oracle, cfg, [x01[:N]], [d[:N]], extra0=d[N:2 * N])
    assert M.entry_bound(mdl2, ["pair"] * L, extra_summed=True)["c"] == [7] * L
    assert M.entry_bound(mdl2, ["pair"] * L, half=True, extra_summed=True)["c"] == [6] * L
    assert M.entry_bound(mdl2, ["coarse"] * L, half=True, extra_summed=True)["c"] == [4] * L
    assert M.entry_bound(mdl2, ["atomic"] * L, extra_summed=True)["c"] == [1] * L
    # the extra pair is one more point set to the model: w (a + b) = w a + w b
    both = M.entry_model(oracle, cfg, [x01[:N], x01[:N]], [d[:N], d[N:2 * N]])
    assert np.array_equal(both.ref, mdl2.ref) and np.array_equal(both.m, mdl2.m)
