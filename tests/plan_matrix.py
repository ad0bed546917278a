"""The matrix over which the hash grid's host-side plans are pinned (tests/golden/grid_plans.npz, tests/test_plan_cpu.py):
raw integer outputs of the five planning queries of the C ABI - mi3d_grid_encode_plan, mi3d_grid_scatter_plan,
mi3d_grid_scatter_binned_workspace, mi3d_grid_level_routes, mi3d_hashgrid_levels - and the return codes of their
invalid-argument cases.  Shared by the generator (tests/golden/make_golden_plans.py), the golden test and the test that
runs the same planners from a g++ build of csrc/mi3d_grid_plan.h (tests/host_math/host_math.cpp)."""
import ctypes as C

import numpy as np

PLS = 1.3819128274917603          # 16 levels from 16 to 2048
STEP = 2 * 3 ** 0.5 / 1024        # C2's marching step

# (levels, base resolution, log2 table size, per-level scale); in the last one every level fits LDS
GRIDS = [(16, 16, 19, PLS), (4, 16, 19, PLS), (6, 8, 12, 1.5), (8, 16, 10, 2.0), (2, 16, 19, PLS)]
NS = [1, 64, 65, 4096, 1_000_003, 10_878_464]
POINTS = [1, 13, 16]
STEPS = [0.0, STEP, 4 * STEP]
BOUNDS = [1.0, 2.0]
# the slice counts on both sides of each k at C2, the switch from k + 1 to doubling at 64, and "nothing fits"
WORKSPACES = [1 << 20, 12 << 30, 24 << 30, 31 << 30, 40 << 30, 56 << 30, 100 << 30, 1 << 50]

u32, i32, f32, vp = C.c_uint32, C.c_int32, C.c_float, C.c_void_p
ENCODE_ARGS = [u32, f32, f32, u32, u32, f32, u32, vp, vp]
SCATTER_ARGS = [u32, u32, f32, f32, u32, u32, f32, u32, C.c_size_t, vp]
SCATTER_WORDS = 6 + 7 * 16


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def encode_plans(fn):
    """fn: mi3d_grid_encode_plan or a function of its signature -> return codes, segment counts and segments."""
    fn.argtypes, fn.restype = ENCODE_ARGS, C.c_int
    shape = (len(GRIDS), len(NS), len(STEPS), len(BOUNDS))
    rc = np.zeros(shape, np.int32)
    nseg = np.zeros(shape + (8,), np.uint32)
    seg = np.zeros(shape + (8, 16, 3), np.uint32)
    for g, (L, base, log2, pls) in enumerate(GRIDS):
        for i, n in enumerate(NS):
            for s, step in enumerate(STEPS):
                for b, bound in enumerate(BOUNDS):
                    a, q = np.zeros(8, np.uint32), np.zeros((8, 16, 3), np.uint32)
                    rc[g, i, s, b] = fn(n, bound, step, L, base, pls, log2, _p(a), _p(q))
                    nseg[g, i, s, b], seg[g, i, s, b] = a, q
    return dict(encode_rc=rc, encode_nseg=nseg, encode_seg=seg)


def scatter_plans(fn):
    """fn: mi3d_grid_scatter_plan or a function of its signature -> return codes and the raw output words."""
    fn.argtypes, fn.restype = SCATTER_ARGS, C.c_int
    shape = (len(GRIDS), len(NS), len(POINTS), len(STEPS), len(BOUNDS), len(WORKSPACES))
    rc = np.zeros(shape, np.int32)
    out = np.zeros(shape + (SCATTER_WORDS,), np.uint64)
    for g, (L, base, log2, pls) in enumerate(GRIDS):
        for i, n in enumerate(NS):
            for p, P in enumerate(POINTS):
                for s, step in enumerate(STEPS):
                    for b, bound in enumerate(BOUNDS):
                        for w, ws in enumerate(WORKSPACES):
                            o = np.zeros(SCATTER_WORDS, np.uint64)
                            rc[g, i, p, s, b, w] = fn(n, P, bound, step, L, base, pls, log2, ws, _p(o))
                            out[g, i, p, s, b, w] = o
    return dict(scatter_rc=rc, scatter_out=out)


def record(lib):
    """Everything the golden file holds, from a loaded libmi3d.so (a ctypes.CDLL)."""
    rec = {}
    rec.update(encode_plans(lib.mi3d_grid_encode_plan))
    rec.update(scatter_plans(lib.mi3d_grid_scatter_plan))
    ws = lib.mi3d_grid_scatter_binned_workspace
    ws.argtypes, ws.restype = [u32, u32, f32, f32, u32, u32, f32, u32], C.c_size_t
    routes = lib.mi3d_grid_level_routes
    routes.argtypes, routes.restype = [u32, u32, f32, u32, i32, vp], C.c_int
    levels = lib.mi3d_hashgrid_levels
    levels.argtypes, levels.restype = [u32, u32, f32, u32, vp, vp, vp], u32
    enc, sca = lib.mi3d_grid_encode_plan, lib.mi3d_grid_scatter_plan

    need = np.zeros((len(GRIDS), len(NS), len(POINTS), len(STEPS), len(BOUNDS)), np.uint64)
    kinds = np.full((len(GRIDS), 2, 16), -1, np.int32)
    total = np.zeros(len(GRIDS), np.uint32)
    offsets, res = np.zeros((len(GRIDS), 17), np.uint32), np.zeros((len(GRIDS), 16), np.uint32)
    scale_bits = np.zeros((len(GRIDS), 16), np.uint32)
    for g, (L, base, log2, pls) in enumerate(GRIDS):
        for i, n in enumerate(NS):
            for p, P in enumerate(POINTS):
                for s, step in enumerate(STEPS):
                    for b, bound in enumerate(BOUNDS):
                        need[g, i, p, s, b] = ws(n, P, bound, step, L, base, pls, log2)
        for mode in (0, 1):
            k = np.full(16, -1, np.int32)
            assert routes(L, base, pls, log2, mode, _p(k)) == 0
            kinds[g, mode] = k
        o, r, sc = np.zeros(17, np.uint32), np.zeros(16, np.uint32), np.zeros(16, np.float32)
        total[g] = levels(L, base, pls, log2, _p(o), _p(r), _p(sc))
        offsets[g], res[g], scale_bits[g] = o, r, sc.view(np.uint32)
    rec.update(workspace=need, routes=kinds, levels_total=total, levels_offsets=offsets, levels_res=res,
               levels_scale_bits=scale_bits)

    # invalid arguments: the return codes (the workspace query and mi3d_hashgrid_levels return a size: 0)
    a8, q, o118, k16 = np.zeros(8, np.uint32), np.zeros(8 * 16 * 3, np.uint32), np.zeros(SCATTER_WORDS, np.uint64), np.zeros(17, np.int32)
    o18 = np.zeros(18, np.uint32)
    g = (16, 16, PLS, 19)
    cases = []
    for L in (0, 17):
        cases += [(f"encode_plan levels={L}", enc(4096, 1.0, STEP, L, 16, PLS, 19, _p(a8), _p(q))),
                  (f"scatter_plan levels={L}", sca(4096, 13, 1.0, STEP, L, 16, PLS, 19, 1 << 30, _p(o118))),
                  (f"workspace levels={L}", ws(4096, 13, 1.0, STEP, L, 16, PLS, 19)),
                  (f"level_routes levels={L}", routes(L, 16, PLS, 19, 1, _p(k16))),
                  (f"hashgrid_levels levels={L}", levels(L, 16, PLS, 19, _p(o18), None, None))]
    for P in (0, 17):
        cases += [(f"scatter_plan P={P}", sca(4096, P, 1.0, STEP, *g, 1 << 30, _p(o118))),
                  (f"workspace P={P}", ws(4096, P, 1.0, STEP, *g))]
    cases += [("encode_plan n=0", enc(0, 1.0, STEP, *g, _p(a8), _p(q))),
              ("scatter_plan n=0", sca(0, 13, 1.0, STEP, *g, 1 << 30, _p(o118))),
              ("workspace n=0", ws(0, 13, 1.0, STEP, *g)),
              ("encode_plan n_segments=null", enc(4096, 1.0, STEP, *g, None, _p(q))),
              ("encode_plan segments=null", enc(4096, 1.0, STEP, *g, _p(a8), None)),
              ("scatter_plan out=null", sca(4096, 13, 1.0, STEP, *g, 1 << 30, None)),
              ("level_routes kinds=null", routes(*g[:2], PLS, 19, 1, None)),
              ("hashgrid_levels outputs=null", levels(16, 16, PLS, 19, None, None, None))]
    rec["invalid_case"] = np.array([c[0] for c in cases])
    rec["invalid_rc"] = np.array([int(c[1]) for c in cases], np.int64)
    return rec
