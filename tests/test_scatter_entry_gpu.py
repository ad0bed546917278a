"""GPU parity, PER TABLE ELEMENT: every route of the table-gradient scatter (csrc/hashgrid.hip: k_scatter, k_scatter_runs,
k_bin_emit's fine and coarse roles, k_bin_reduce's three record types, k_replica_reduce) against the binary64 model of
tests/scatter_entry_model.py under the route's derived error bound - every element of every level, and exactly 0.0 where
nothing contributes.  Each case also asserts, through the workspace spy and the host-side plan queries, that the route it
names is the one that ran.  What the MI355X measured is in profiles/scatter_entry_parity.json (written at the end of
this module when MI3D_SCATTER_PARITY_JSON names a file; otherwise nothing is written)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import scatter_entry_model as M
from conftest import record_scatter_workspaces
from test_grid_points_gpu import T, _points, _ray_like_points
from test_hashgrid_gpu import CONFIGS
from test_hashgrid_gpu import _points as _unit_points

pytestmark = pytest.mark.gpu

N = 3000
STEP = 0.0034
_CACHE = {}


_ROWS = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    """The inputs and models of the cases live as long as this module runs (a model of the default grid is four arrays
    of 12 M numbers); the figures every case measured are written ONCE, at the end, one line per case."""
    yield
    _CACHE.clear()
    path = os.environ.get("MI3D_SCATTER_PARITY_JSON")
    if path and _ROWS:
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(_ROWS[k], sort_keys=True)}" for k in sorted(_ROWS))
                    + "\n}\n")
    _ROWS.clear()


def _check(case, g, mdl, bound, facts=None):
    """Every element of `g` against the model; the figures are printed and recorded BEFORE the assertion.  Recorded per
    case: lists over the levels - route, c, worst err / bound, the element it occurred on, its m, the dominant term."""
    report, failures = M.check_entries(g, mdl, bound)
    for row in report:
        print(case, row)
    row = {"route": [r["route"] for r in report], "c": [r["c"] for r in report],
           "worst_ratio": [float(f"{r['worst_ratio']:.3g}") for r in report], "element": [r["element"] for r in report],
           "m": [r["m"] for r in report], "dominant_term": [r["dominant_term"] for r in report]}
    row.update(facts or {})
    _ROWS[case] = row
    assert not failures, f"{case}: per-entry bound missed on {len(failures)} level(s): {failures}"


def _kcfg(cfg):
    return dict(n_levels=cfg.n_levels, base_resolution=cfg.base_resolution, per_level_scale=cfg.per_level_scale,
                log2_hashmap_size=cfg.log2_hashmap_size)


def _x01(pts, bound):
    return [((q + np.float32(bound)) / np.float32(2 * bound)).astype(np.float32) for q in pts]


def _plan(n, P, bound, step, cfg, workspace):
    from mi3d import _lib
    out = (ctypes.c_ulonglong * (6 + 7 * cfg.n_levels))()
    _lib.call("mi3d_grid_scatter_plan", n, P, float(bound), float(step), cfg.n_levels, cfg.base_resolution,
              float(cfg.per_level_scale), cfg.log2_hashmap_size, ctypes.c_size_t(int(workspace)), out)
    return list(out)


def _record_routes(plan, cfg):
    """The route of every level on the record path, from the plan: coarse below merge_levels, pair records where the
    level can pair (the plan's flag), single records elsewhere."""
    return ["coarse" if l < plan[2] else ("pair" if plan[6 + 7 * l + 3] else "single") for l in range(cfg.n_levels)]


def _merging_levels(cfg, step, bound):
    """Levels that run-merge on the atomic routes: cells at least 1.05 marching steps long (include/mi3d.h: `step` only
    selects them), a prefix of the levels."""
    s01 = np.float32(step) / np.float32(2 * bound)
    return int(sum(np.float32(1.0) / np.float32(r) >= np.float32(1.05) * s01 for r in cfg.resolutions))


# ---------------------------------------------------------------------------------------------------------------- inputs
def _stencil_case(oracle, key, second=True, bound=1.0, log2=19, grads="unit", n=N, extra=False, n_levels=16):
    """Ray-like samples with rows on +bound, zeroed rows and a zeroed level, the 7- or 13-point stencil, gradient pairs that
    binary16 holds exactly (so fp32 and binary16 planes share one model), the model.  Built once per key, never written."""
    if key in _CACHE:
        return _CACHE[key]
    from mi3d import grid_ops
    rng = np.random.default_rng(14)
    cfg = oracle.GridConfig(bound=bound, log2_hashmap_size=log2, n_levels=n_levels)
    L = n_levels
    x = _ray_like_points(rng, n, bound)
    x[:8] = bound
    x[8:16, 1] = -bound
    if log2 < 13:   # cells whose x index ends in many ones on the finest levels: the pair flip must stay inside the level
        for i, cx in enumerate((1023, 511, 1535, 255, 767)):
            x[200 * i + 300:200 * i + 400, 0] = np.float32((cx + 0.3) / 2048.0 * 2.0 - 1.0)
    x2 = (x + rng.normal(size=x.shape).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    offs, P0 = grid_ops.stencil_offsets(center=True, second=second)
    P = offs.shape[0]
    if grads == "unit":
        dout = rng.normal(size=(n, P, L, 2)).astype(np.float16)
    else:
        # magnitudes over 2^-14 ... 2^14 within every level (one exponent per stretch of 50 samples and level: a real
        # gradient's magnitude varies along a ray), binary16 subnormals on some rows
        mant = (rng.uniform(1.0, 2.0, size=(n, P, L, 2)) * rng.choice([-1.0, 1.0], size=(n, P, L, 2)))
        ex = np.repeat(rng.integers(-14, 14, size=(n // 50, 1, L, 1)), 50, axis=0)
        dout = (mant * np.exp2(ex)).astype(np.float16)
        dout[1000:1100:3] = (rng.integers(1, 64, size=dout[1000:1100:3].shape) * 2.0 ** -24).astype(np.float16)  # subnormals
    dout[100:140] = 0
    dout[:, 2, 2] = 0
    if grads != "unit":   # one 6e4 per level, next to the subnormals on other elements of the same level (after the zeroing,
        for l in range(L):   # and never on the zeroed (point 2, level 2))
            dout[1500 + 7 * l, (l + 1) % P, l, l & 1] = np.float16(6e4)
        assert all(np.abs(dout[:, :, l].astype(np.float32)).max() > 5.9e4 for l in range(L))
    assert np.isfinite(dout.astype(np.float32)).all()
    e0 = None
    if extra:
        e0 = rng.normal(size=(n, L, 2)).astype(np.float16)
        e0[50:120] = 0
        e0[200:260, L - 2] = -dout[200:260, 0, L - 2]    # the two point-0 pairs cancel exactly on one fine level
    pts = _points(x, x2, offs, P0, bound)
    mdl = M.entry_model(oracle, cfg, _x01(pts, bound), [dout[:, p] for p in range(P)], extra0=e0)
    for a in (x, x2, dout) + ((e0,) if extra else ()):
        a.setflags(write=False)
    _CACHE[key] = dict(cfg=cfg, x=x, x2=x2, offs=offs, P0=P0, P=P, dout=dout, extra=e0, mdl=mdl, bound=bound, n=n)
    return _CACHE[key]


def _planes(case, half):
    dt = np.float16 if half else np.float32
    n, P, L = case["n"], case["P"], case["cfg"].n_levels
    planes = np.ascontiguousarray(case["dout"].astype(dt).transpose(2, 1, 0, 3).reshape(L, P * n, 2))   # [L][p*n + s][2]
    eplanes = None if case["extra"] is None else np.ascontiguousarray(case["extra"].astype(dt).transpose(1, 0, 2))
    return planes, eplanes


def _run_binned(cuda, case, half, workspace, step=STEP):
    """field_ops.scatter_binned on a case; returns (gradient, routes, facts about the route that ran)."""
    from mi3d import _lib, field_ops
    cfg, n, P, bound = case["cfg"], case["n"], case["P"], case["bound"]
    planes, eplanes = _planes(case, half)
    need = int(_lib.lib().mi3d_grid_scatter_binned_workspace(n, P, float(bound), step, cfg.n_levels, cfg.base_resolution, cfg.per_level_scale,
                                                             cfg.log2_hashmap_size))
    ws = {"auto": None, "none": 0}.get(workspace)
    if workspace == "tiny":   # room for about a third of the samples per slice
        ws = int(_lib.lib().mi3d_grid_scatter_binned_workspace(n // 3, P, float(bound), step, cfg.n_levels, cfg.base_resolution, cfg.per_level_scale,
                                                               cfg.log2_hashmap_size))
    second = case["P0"] < P
    with record_scatter_workspaces() as arenas:
        g = field_ops.scatter_binned(T(case["x"], cuda), T(case["x2"], cuda) if second else None, case["offs"], case["P0"],
                                     bound, T(planes, cuda), _kcfg(cfg), step, cfg.n_params, workspace_bytes=ws,
                                     extra0=None if eplanes is None else T(eplanes, cuda)).cpu().numpy()
    facts = {"arena_bytes": arenas[0] if arenas else 0}
    if workspace == "none":
        assert arenas == []                                   # the all-atomic path was asked for
        return g, ["atomic"] * cfg.n_levels, facts
    assert len(arenas) == 1 and arenas[0] > 0, arenas         # the record path really ran
    plan = _plan(n, P, bound, step, cfg, arenas[0])
    assert plan[1] <= arenas[0]                               # (the fp32 plan fits, so the lighter binary16 one does)
    facts["samples_per_slice_fp32_plan"] = plan[0]
    if workspace == "tiny":
        # several slices: the fp32 plan says so; binary16 pair records are 12 bytes for 16 and everything else in the
        # arena is the same size, so one binary16 slice needs at least 3/4 of `need` - more than this arena has
        assert plan[0] < n and arenas[0] * 4 < need * 3, (plan[0], arenas[0], need)
    else:
        assert plan[0] == n
    return g, _record_routes(plan, cfg), facts


# ---------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("name", list(CONFIGS))
def test_dropin_encoding_backward(cuda, oracle, name):
    """tinycudann.Encoding backward (mi3d_hashgrid_backward: raw positions, the general index route 0; the call knows no
    marching step and lets EVERY level sum equal-cell runs first, so all of it goes through k_scatter_runs' float atomics -
    c = 1 like k_scatter), points on 0.0 and 1.0 included."""
    import tinycudann as tcnn
    from mi3d import _lib
    cfg = oracle.GridConfig(n_features_per_level=2, **CONFIGS[name])
    kinds = (ctypes.c_int32 * cfg.n_levels)()
    _lib.call("mi3d_grid_level_routes", cfg.n_levels, cfg.base_resolution, float(cfg.per_level_scale), cfg.log2_hashmap_size,
              0, kinds)
    assert list(kinds) == [0] * cfg.n_levels
    rng = np.random.default_rng(8)
    x = _unit_points(rng, N)
    dout = rng.normal(size=(N, cfg.n_levels, 2)).astype(np.float32)
    dout[100:164] = 0
    dout[:, cfg.n_levels // 2] = 0
    mdl = M.entry_model(oracle, cfg, [x], [dout])
    enc = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": cfg.n_levels, "n_features_per_level": 2,
                            "log2_hashmap_size": cfg.log2_hashmap_size, "base_resolution": cfg.base_resolution,
                            "per_level_scale": cfg.per_level_scale}).to(cuda)
    enc(T(x, cuda)).backward(T(dout.reshape(N, -1), cuda))
    g = enc.params.grad.cpu().numpy()
    _check(f"dropin_backward[{name}]", g, mdl, M.entry_bound(mdl, ["atomic"] * cfg.n_levels))


@pytest.mark.parametrize("step", [0.0034, 100.0, 1e-7])
@pytest.mark.parametrize("second", [False, True])
def test_encode_points_backward(cuda, oracle, second, step):
    """grid_ops.encode_points backward (mi3d_grid_scatter_points): `step` makes no level (100), the coarser levels (0.0034) or all
    16 (1e-7) sum equal-cell runs in k_scatter_runs before their atomics; the others go through k_scatter."""
    from mi3d import grid_ops
    case = _stencil_case(oracle, ("stencil", second), second=second)
    cfg, n, P = case["cfg"], case["n"], case["P"]
    merging = _merging_levels(cfg, step, 1.0)
    assert (merging == 0) if step == 100.0 else (merging == 16) if step == 1e-7 else (0 < merging < 16)
    params = torch.zeros(cfg.n_params, device=cuda, requires_grad=True)
    feats = grid_ops.encode_points(params, T(case["x"], cuda), case["offs"], _kcfg(cfg), 1.0,
                                   T(case["x2"], cuda) if second else None, case["P0"], step=step)
    dout = case["dout"].astype(np.float32).reshape(n, P, 32)
    feats.backward(T(dout.transpose(1, 0, 2).reshape(P * n, 32), cuda))   # point-major rows
    g = params.grad.cpu().numpy()
    _check(f"encode_points_backward[second={second},step={step}]", g, case["mdl"],
           M.entry_bound(case["mdl"], ["atomic"] * 16), {"run_merging_levels": merging})


def test_encode_points_backward_with_a_device_side_count(cuda, oracle):
    """A device-side `count` cuts the rows: samples beyond it contribute nothing, the row stride between points stays n
    (k_scatter alone: the runs kernel has no count)."""
    from mi3d import grid_ops
    case = _stencil_case(oracle, ("stencil", True), second=True)
    cfg, n, P, keep = case["cfg"], case["n"], case["P"], 1877
    key = ("stencil-count", keep)
    if key not in _CACHE:
        pts = _points(case["x"][:keep], case["x2"][:keep], case["offs"], case["P0"], 1.0)
        _CACHE[key] = M.entry_model(oracle, cfg, _x01(pts, 1.0), [case["dout"][:keep, p] for p in range(P)])
    mdl = _CACHE[key]
    params = torch.zeros(cfg.n_params, device=cuda, requires_grad=True)
    count = torch.tensor([keep], dtype=torch.int32, device=cuda)
    feats = grid_ops.encode_points(params, T(case["x"], cuda), case["offs"], _kcfg(cfg), 1.0, T(case["x2"], cuda),
                                   case["P0"], step=STEP, count=count)
    dout = case["dout"].astype(np.float32).reshape(n, P, 32)
    feats.backward(T(dout.transpose(1, 0, 2).reshape(P * n, 32), cuda))
    g = params.grad.cpu().numpy()
    _check("encode_points_backward[count]", g, mdl, M.entry_bound(mdl, ["atomic"] * 16))


@pytest.mark.parametrize("workspace", ["auto", "tiny", "none"])
@pytest.mark.parametrize("half", [False, True])
def test_scatter_binned(cuda, oracle, half, workspace):
    """field_ops.scatter_binned, 13 points: one slice, three slices, the all-atomic fallback; fp32 planes (16-byte pair
    records) and binary16 planes (12-byte records, the rec16 term)."""
    case = _stencil_case(oracle, ("stencil", True), second=True)
    g, routes, facts = _run_binned(cuda, case, half, workspace)
    if workspace != "none":
        assert routes[:7] == ["coarse"] * 7 and routes[7:] == ["pair"] * 9      # levels 0-6 gathered, 7-15 pair records
    _check(f"scatter_binned[half={half},workspace={workspace}]", g, case["mdl"],
           M.entry_bound(case["mdl"], routes, half=half), facts)


@pytest.mark.parametrize("workspace", ["auto", "tiny", "none"])
@pytest.mark.parametrize("half", [False, True])
def test_scatter_binned_with_the_extra_point0_pair(cuda, oracle, half, workspace):
    """... plus `extra0`: summed with point 0's pair in binary32 first (fp32 planes, and the coarse role for both types), a
    record of its own (binary16 pair records), a pass of its own (atomic fallback) - with rows where the two pairs cancel
    exactly on a fine level."""
    case = _stencil_case(oracle, ("stencil-extra",), second=True, extra=True)
    g, routes, facts = _run_binned(cuda, case, half, workspace)
    bound = M.entry_bound(case["mdl"], routes, half=half, extra_summed=True)
    _check(f"scatter_binned_extra0[half={half},workspace={workspace}]", g, case["mdl"], bound, facts)


@pytest.mark.parametrize("log2", [10, 12])
@pytest.mark.parametrize("half", [False, True])
def test_scatter_binned_with_tables_smaller_than_a_bin(cuda, oracle, half, log2):
    """log2_hashmap_size below 13: a hashed level is smaller than one reduce bin, the pair flip must be masked with the
    level's size - a misplaced partner is a contribution on an element that owes 0.0 or a miss on its own element."""
    case = _stencil_case(oracle, ("stencil-log2", log2), second=False, log2=log2)
    g, routes, facts = _run_binned(cuda, case, half, "auto")
    assert "pair" in routes
    _check(f"scatter_binned_small_tables[half={half},log2={log2}]", g, case["mdl"],
           M.entry_bound(case["mdl"], routes, half=half), facts)


@pytest.mark.parametrize("half", [False, True])
def test_scatter_binned_in_a_box_of_bound_2(cuda, oracle, half):
    case = _stencil_case(oracle, ("stencil-bound2",), second=True, bound=2.0)
    g, routes, facts = _run_binned(cuda, case, half, "auto")
    _check(f"scatter_binned_bound2[half={half}]", g, case["mdl"], M.entry_bound(case["mdl"], routes, half=half), facts)


@pytest.mark.parametrize("half", [False, True])
def test_scatter_binned_on_levels_that_cannot_pair(cuda, oracle, half):
    """log2_hashmap_size 20: a hashed level holds 2^20 entries, more than a pair record's 19 entry bits address, so the fine
    levels leave as one 12-byte record per contribution, whatever the planes' type (the "single" route: wk d, the reduce's
    term, no rec16 term) - with the extra pair, which this route adds to point 0's in binary32.  Ten levels keep the table
    at 5 M entries."""
    case = _stencil_case(oracle, ("stencil-log2-20",), second=True, log2=20, n_levels=10, extra=True)
    g, routes, facts = _run_binned(cuda, case, half, "auto")
    assert routes[7:] == ["single"] * 3 and "pair" not in routes, routes
    bound = M.entry_bound(case["mdl"], routes, half=half, extra_summed=True)
    assert bound["c"][7:] == [3] * 3 and not bound["rec16"].any()
    _check(f"scatter_binned_single_records[half={half}]", g, case["mdl"], bound, facts)


@pytest.mark.parametrize("workspace", ["auto", "tiny"])
@pytest.mark.parametrize("half", [False, True])
def test_scatter_binned_dynamic_range(cuda, oracle, half, workspace):
    """Gradient magnitudes over 2^-14 ... 2^14 within every level, one 6e4 per level next to binary16 subnormals on other
    elements of the same level - the regime of a GradScaler-scaled step, where the reduce's 2^-38 Lmax term is what bounds
    the small elements."""
    case = _stencil_case(oracle, ("stencil-wide",), second=True, grads="wide")
    g, routes, facts = _run_binned(cuda, case, half, workspace)
    bound = M.entry_bound(case["mdl"], routes, half=half)
    live = case["mdl"].m > 0
    facts["elements_where_the_reduce_term_dominates"] = int(np.count_nonzero(
        live & (bound["reduce"] > bound["binary32"]) & (bound["reduce"] > bound["rec16"])))
    assert facts["elements_where_the_reduce_term_dominates"] > 100000
    _check(f"scatter_binned_dynamic_range[half={half},workspace={workspace}]", g, case["mdl"], bound, facts)


@pytest.mark.parametrize("half", [False, True])
def test_scatter_binned_when_the_regions_overflow(cuda, oracle, half):
    """30 000 samples inside one cell of the finest level, all 13 stencil offsets zero: every contribution of a level lands
    on the same 8 entries (m = 390 000 each, the bound is wide there by construction), the regions overflow into float
    atomics - and every other element of the table is exactly 0.0."""
    from mi3d import field_ops
    key = ("overflow",)
    n, P = 30000, 13
    if key not in _CACHE:
        rng = np.random.default_rng(23)
        cfg = oracle.GridConfig()
        x = (np.array([0.31, -0.22, 0.47], np.float32) + rng.uniform(-1e-4, 1e-4, (n, 3)).astype(np.float32)).astype(np.float32)
        dout = rng.normal(size=(n, P, 16, 2)).astype(np.float16)
        mdl = M.EntryModel(cfg).add(oracle, _x01([x], 1.0)[0], np.ascontiguousarray(dout.transpose(1, 0, 2, 3))).finish()
        _CACHE[key] = dict(cfg=cfg, x=x, x2=None, offs=np.zeros((P, 3), np.float32), P0=P, P=P, dout=dout, extra=None, mdl=mdl,
                           bound=1.0, n=n)
    case = _CACHE[key]
    mdl, cfg = case["mdl"], case["cfg"]
    # (the 2e-4 wide cloud straddles a cell face on some fine levels: a few cells per level, 8 entries x 2 features each)
    assert int(np.count_nonzero(mdl.m)) <= 16 * 8 * 2 * 8 and int(mdl.m.max()) == n * P
    planes, _ = _planes(case, half)
    with record_scatter_workspaces() as arenas:
        g = field_ops.scatter_binned(T(case["x"], cuda), None, case["offs"], P, 1.0, T(planes, cuda), _kcfg(cfg), STEP,
                                     cfg.n_params).cpu().numpy()
    assert len(arenas) == 1 and arenas[0] > 0
    plan = _plan(n, P, 1.0, STEP, cfg, arenas[0])
    assert plan[0] == n
    # a (wave, bin) region against what it receives: the n P points of a level leave 4 pair records each, into at most 4 bins
    # (one cell: the four (y, z) corner pairs), from at most `waves` waves - several times the capacity
    fine = [l for l in range(16) if l >= plan[2]]
    assert all(n * P * 4 / 4 / plan[6 + 7 * l + 2] > 3 * plan[6 + 7 * l + 1] for l in fine)
    _check(f"scatter_binned_overflow[half={half}]", g, mdl, M.entry_bound(mdl, _record_routes(plan, cfg), half=half),
           {"arena_bytes": arenas[0]})


REPLICA_GRID = dict(n_levels=4, log2_hashmap_size=6, base_resolution=2, per_level_scale=2.0)   # 8 + 64 + 64 + 64 entries


@pytest.mark.parametrize("n", [3000, 100])
@pytest.mark.parametrize("step", [100.0, 0.5])
def test_replica_fallback(cuda, oracle, step, n):
    """A workspace that holds the 64 private table copies but not the smallest slice's records: k_scatter (and, with step
    0.5, k_scatter_runs on level 0) with n_rep = 64, then k_replica_reduce.  Reached with a table of 200 entries - 64 copies
    are 102 400 bytes - and the 13-point stencil with no level gathered, whose 64-sample slice plans 370 832 bytes: the plan
    query says so, the C ABI is called with a buffer of a size in between.  3000 samples put thousands of contributions on
    each of the 200 entries, where the worst-case bound is far above a float sum's error; 100 samples keep m in the
    hundreds (and use few of the copies: the others must add exactly nothing)."""
    from mi3d import _lib, grid_ops
    key = ("replica", n)
    if key not in _CACHE:
        rng = np.random.default_rng(37)
        cfg = oracle.GridConfig(n_features_per_level=2, **REPLICA_GRID)
        x = _ray_like_points(rng, n, 1.0)
        x[:8] = 1.0
        x2 = (x + rng.normal(size=x.shape).astype(np.float32) * np.float32(0.01)).astype(np.float32)
        offs, P0 = grid_ops.stencil_offsets(center=True, second=True)
        P = offs.shape[0]
        dout = rng.normal(size=(n, P, cfg.n_levels, 2)).astype(np.float32)
        dout[n // 30:n // 30 + 40] = 0
        dout[:, 2, 2] = 0
        mdl = M.entry_model(oracle, cfg, _x01(_points(x, x2, offs, P0, 1.0), 1.0), [dout[:, p] for p in range(P)])
        _CACHE[key] = dict(cfg=cfg, x=x, x2=x2, offs=offs, P0=P0, P=P, dout=dout, mdl=mdl)
    case = _CACHE[key]
    cfg, P, mdl = case["cfg"], case["P"], case["mdl"]
    L = cfg.n_levels
    rep_bytes = 64 * cfg.n_entries * 2 * 4
    ws_bytes = rep_bytes + 4096
    plan = _plan(n, P, 1.0, step, cfg, ws_bytes)
    # the planner cut the slice down to its floor of 64 samples and the plan still does not fit: the fallback; the buffer
    # holds the 64 copies: the replica form of it
    assert plan[0] <= 64 and plan[0] < n and plan[1] > ws_bytes >= rep_bytes and plan[2] == 0, plan[:6]
    assert _merging_levels(cfg, step, 1.0) == {100.0: 0, 0.5: 1}[step]
    planes = np.ascontiguousarray(case["dout"].transpose(2, 1, 0, 3).reshape(L, P * n, 2))
    xd, x2d, pd = T(case["x"], cuda), T(case["x2"], cuda), T(planes, cuda)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
    grad = torch.zeros(cfg.n_params, device=cuda)
    _, offs_p = grid_ops._offs_arg(case["offs"])
    with _lib.on(xd):
        _lib.call("mi3d_grid_scatter_binned", _lib.ptr(xd), _lib.ptr(x2d), n, offs_p, int(case["P0"]), P, 1.0, _lib.ptr(pd),
                  0, L, cfg.base_resolution, float(cfg.per_level_scale), cfg.log2_hashmap_size, float(step), _lib.ptr(ws),
                  ctypes.c_size_t(ws_bytes), _lib.ptr(grad), _lib.stream(xd))
    torch.cuda.synchronize(cuda)
    g = grad.cpu().numpy()
    _check(f"replica_fallback[step={step},n={n}]", g, mdl, M.entry_bound(mdl, ["atomic"] * L),
           {"workspace_bytes": ws_bytes, "replica_bytes": rep_bytes, "smallest_plan_bytes": plan[1]})
