"""CPU: the product's own scalar math (make-it-3d_amd/csrc/mi3d_common.h - the DDA step, Morton codes and hash-grid
indexing the HIP kernels execute) compiled for the HOST and compared bit-for-bit with the oracle, so that index-exactness
is established before a GPU is involved.  tests/host_math/host_math.cpp is the thin extern-C shim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, make_rays, random_bitfield, sphere_bitfield

HERE = os.path.join(ROOT, "tests", "host_math")


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(HERE, "libhostmath.so")
    src = os.path.join(HERE, "host_math.cpp")
    hdrs = [os.path.join(PKG, "csrc", h) for h in ("mi3d_common.h", "mi3d_grid_plan.h", "mi3d_dev.h")]
    if not os.path.exists(so) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math",
                               "-fPIC", "-shared",
                               "-I", os.path.join(PKG, "csrc"), src, "-o", so])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("C_,bound,kind,dt_gamma,max_steps,perturb", [
    (1, 1.0, "ones", 0.0, 256, False), (1, 1.0, "sphere", 0.0, 512, True), (1, 1.0, "random", 1 / 128, 256, True),
    (2, 2.0, "sphere", 0.0, 256, True), (3, 4.0, "random", 1 / 128, 128, False)])
def test_march_bit_exact_with_oracle(hm, oracle, C_, bound, kind, dt_gamma, max_steps, perturb):
    rng = np.random.default_rng(11)
    N, H = 500, 128
    o, d = make_rays(rng, N, bound)
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb)
    bits = {"ones": lambda: np.full(C_ * H ** 3 // 8, 255, np.uint8), "sphere": lambda: sphere_bitfield(oracle, C_, H, 0.45 * bound),
            "random": lambda: random_bitfield(rng, C_, H)}[kind]()
    noises = rng.uniform(0, 1, N).astype(np.float32) if perturb else None
    xr, dr, lr, rr, cr = oracle.march_rays_train(o, d, bound, bits, C_, H, nears, fars, noises, align=-1,
                                                 dt_gamma=dt_gamma, max_steps=max_steps, return_counter=True)
    M = N * max_steps
    xyzs, dirs, deltas = np.zeros((M, 3), np.float32), np.zeros((M, 3), np.float32), np.zeros((M, 2), np.float32)
    rays, counter = np.zeros((N, 3), np.int32), np.zeros(2, np.int32)
    nz = np.zeros(N, np.float32) if noises is None else noises
    hm.hm_march_train(_p(o), _p(d), _p(bits), C.c_float(bound), C.c_float(dt_gamma), C.c_uint32(max_steps),
                      C.c_uint32(N), C.c_uint32(C_), C.c_uint32(H), C.c_uint32(M), _p(nears), _p(fars), _p(xyzs),
                      _p(dirs), _p(deltas), _p(rays), _p(counter), _p(nz))
    assert np.array_equal(counter, cr)
    # the oracle lays rays out in ray order too (sequential host loop): everything must agree bit for bit
    assert np.array_equal(rays, rr)
    m = int(counter[0])
    assert np.array_equal(xyzs[:m].view(np.uint32), xr[:m].view(np.uint32))
    assert np.array_equal(deltas[:m].view(np.uint32), lr[:m].view(np.uint32))
    assert np.array_equal(dirs[:m].view(np.uint32), dr[:m].view(np.uint32))


def test_morton_bit_exact_with_oracle(hm, oracle):
    rng = np.random.default_rng(2)
    co = rng.integers(0, 1024, (20000, 3)).astype(np.int32)
    out = np.empty(20000, np.int32)
    hm.hm_morton(_p(co), C.c_uint32(20000), _p(out))
    assert np.array_equal(out, oracle.morton3D(co))
    back = np.empty((20000, 3), np.int32)
    hm.hm_morton_invert(_p(out), C.c_uint32(20000), _p(back))
    assert np.array_equal(back, co)


@pytest.mark.parametrize("kw", [{}, dict(n_levels=4, per_level_scale=128 ** (1 / 3)),
                                dict(n_levels=6, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.7)])
def test_grid_corner_indices_bit_exact_with_oracle(hm, oracle, kw):
    import tinycudann as tcnn
    cfg = oracle.GridConfig(**kw)
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    x[0] = 0.0; x[1] = 1.0; x[2] = [1.0, 0.0, 0.999999]
    idx_ref, w_ref = oracle.hashgrid_indices(x, cfg)
    total, offs, res, scl = tcnn.grid_levels(cfg.n_levels, cfg.base_resolution, cfg.per_level_scale,
                                             cfg.log2_hashmap_size)
    assert total == cfg.n_entries
    for l in range(cfg.n_levels):
        size = int(offs[l + 1] - offs[l])
        stride, dims = 1, 0
        while dims < 3 and stride <= size:
            stride *= int(res[l]); dims += 1
        hashed = 1 if size < stride else 0
        idx, w = np.empty((3000, 8), np.uint32), np.empty((3000, 8), np.float32)
        hm.hm_grid_corners(_p(x), C.c_uint32(3000), C.c_float(float(scl[l])), C.c_uint32(int(res[l])),
                           C.c_uint32(int(offs[l])), C.c_uint32(size), C.c_uint32(hashed), C.c_uint32(dims), _p(idx),
                           _p(w))
        ref_local = idx_ref[:, l, :] - (0 if idx_ref[:, l, :].max() < size else offs[l])
        assert np.array_equal(idx, ref_local.astype(np.uint32)), l
        assert np.array_equal(w.view(np.uint32), w_ref[:, l, :].view(np.uint32)), l


def test_row12_record_packing_and_the_x_pair_rule(hm):
    """The scatter's 12-byte pair record under autocast (csrc/mi3d_common.h: pack_row12 / unpack_row12_fields, used by
    k_bin_emit / k_bin_reduce): the entry's 13 bits, the flip count and the raw binary16 pair survive exactly, the weight and
    the x fraction come back within 2^-24 (2^-23 at exactly 1, the clamp) - and the rule the record relies on: on a hashed
    power-of-two level the entry of the x + 1 corner is the x corner's with its t low bits flipped, t = 1 + trailing ones of
    cx (x enters the hash with prime 1)."""
    rng = np.random.default_rng(3)
    n = 200_000
    e = rng.integers(0, 8192, n).astype(np.uint32)
    t = rng.integers(0, 14, n).astype(np.uint32)
    w = rng.uniform(0, 1, n).astype(np.float32)
    fx = rng.uniform(0, 1, n).astype(np.float32)
    w[:6] = [0.0, 1.0, 2.0 ** -24, 1 - 2.0 ** -24, 0.5, 2.0 ** -23]
    fx[:6] = [0.0, 2.0 ** -25, 1 - 2.0 ** -24, 0.25, 2.0 ** -23, 0.75]
    raw = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    words = np.empty((n, 3), np.uint32)
    e2, t2 = np.empty(n, np.uint32), np.empty(n, np.uint32)
    w2, fx2 = np.empty(n, np.float32), np.empty(n, np.float32)
    hm.hm_row12_roundtrip(_p(e), _p(t), _p(w), _p(fx), _p(raw), C.c_uint32(n), _p(words), _p(e2), _p(t2), _p(w2), _p(fx2))
    assert np.array_equal(e2, e) and np.array_equal(t2, t) and np.array_equal(words[:, 1], raw)
    assert np.abs(w2.astype(np.float64) - w).max() <= 2.0 ** -23 and np.abs(w2.astype(np.float64) - w)[w < 1].max() <= 2.0 ** -24 + 1e-12
    assert np.abs(fx2.astype(np.float64) - fx).max() <= 2.0 ** -24 + 1e-12
    assert w2[0] == 0.0 and fx2[0] == 0.0 and fx2[1] == 0.0          # fx_q == 0 marks a single: 2^-25 rounds to it
    assert (w2 < 1.0).all() and (fx2 < 1.0).all()
    # the x-pair rule, for cells of every trailing-ones pattern, on the levels the reference hashes into 2^19 (and a 2^12)
    cells = rng.integers(0, 2048, (100_000, 3)).astype(np.uint32)
    cells[:4096, 0] = np.arange(4096)            # every low-bit pattern of cx
    for size in (1 << 19, 1 << 12):
        e0, e1, rule = (np.empty(100_000, np.uint32) for _ in range(3))
        hm.hm_pair_rule(_p(cells), C.c_uint32(100_000), C.c_uint32(size), _p(e0), _p(e1), _p(rule))
        assert np.array_equal(e1, rule), size
        same_bin = (e0 >> 13) == (e1 >> 13)      # what the emit sends as ONE record (the others leave as two singles)
        assert 0.99 < same_bin.mean() <= 1.0


def test_fixed_point_rounds_like_rint(hm):
    """fixed_point (csrc/mi3d_common.h: the 1.5 * 2^52 trick both scatter passes use for their 64-bit sums) is
    round-to-nearest-even of a float as a two's complement integer, for |x| < 2^51."""
    rng = np.random.default_rng(7)
    big = np.float32(2.0 ** 51 - 2.0 ** 27)          # the largest float below 2^51: what 2^51 - 1 is closest to from below
    assert float(big) < 2.0 ** 51 - 1 < float(np.nextafter(big, np.float32(np.inf)))
    tiny = np.float32(2.0 ** -149)
    special = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 4194304.5, -4194303.5, 8388607.5, 0.49999997, -0.49999997,
                        0.0, -0.0, tiny, -tiny, 2.0 ** -127, -2.0 ** -127, 1.17549435e-38, big, -big, 1.0, -1.0,
                        -7.0, 123456.75], np.float32)
    x = np.concatenate([special, (rng.standard_normal(60_000) * 100).astype(np.float32),
                        (rng.uniform(-1, 1, 40_000) * 2.0 ** rng.integers(-30, 51, 40_000)).astype(np.float32)])
    assert len(x) >= 100_000 and np.abs(x).max() <= big
    out = np.empty(len(x), np.int64)
    hm.hm_fixed_point(_p(x), C.c_uint32(len(x)), _p(out))
    assert np.array_equal(out, np.rint(x.astype(np.float64)).astype(np.int64))


def test_gather_scale_is_a_power_of_two_that_fits(hm):
    """The gather table's scale for a tile whose largest gradient is tmax, in every binade from the smallest subnormal
    to FLT_MAX (low end, middle and top of each): a power of two with tmax * scale < 2^40 - and >= 2^39 wherever the
    +-126 clamp of the exponent is not hit; unscale is its exact inverse."""
    lo = 2.0 ** np.arange(-149, 128, dtype=np.float64)
    hi = np.minimum(2 * lo * (1 - 2.0 ** -24), 3.4028234663852886e38)   # the binade's last float (normal binades)
    tmax = np.unique(np.concatenate([lo, 1.5 * lo, hi]).astype(np.float32))
    tmax = tmax[(tmax > 0) & np.isfinite(tmax)]
    assert tmax.min() == np.float32(2.0 ** -149) and tmax.max() == np.finfo(np.float32).max
    scale, unscale = np.empty(len(tmax), np.float32), np.empty(len(tmax), np.float64)
    hm.hm_gather_scale(_p(tmax), C.c_uint32(len(tmax)), _p(scale), _p(unscale))
    m, k = np.frexp(scale.astype(np.float64))
    assert (m == 0.5).all()                                   # a power of two: 2^(k - 1)
    k2 = k - 1
    assert (np.abs(k2) <= 126).all() and np.array_equal(unscale, np.ldexp(1.0, -k2))
    prod = tmax.astype(np.float64) * scale.astype(np.float64)  # exact
    assert (prod < 2.0 ** 40).all()
    want = 40 - np.frexp(tmax.astype(np.float64))[1]          # the exponent before the clamp (tmax < 2^ex)
    free = np.abs(want) <= 126                                # the clamp is not hit (40 - ex == 126 included)
    assert np.array_equal(k2[free], want[free])
    assert free.sum() > 200 and (want[free] == 126).any() and (prod[free] >= 2.0 ** 39).all()
    # at the clamp: the product still fits (tiny tmax) - a tmax large enough for -126 (> 2^166) does not exist
    assert (want[~free] > 126).all() and (k2[~free] == 126).all()


def test_merge_slot_stays_in_the_table(hm):
    rng = np.random.default_rng(9)
    e = np.concatenate([np.arange(1 << 16, dtype=np.uint32), rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 2 ** 19 - 1, 2 ** 32 - 1], np.uint32)])
    slot = np.empty(len(e), np.uint32)
    hm.hm_merge_slot(_p(e), C.c_uint32(len(e)), _p(slot))
    assert slot.max() < 512
    assert np.array_equal(slot, ((e.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> 23)


def test_corner_weights_are_the_forward_products(hm):
    """corner_weights (one routine for forward, scatter and emit) gives ((wx * wy) * wz) per corner, bit for bit."""
    rng = np.random.default_rng(4)
    f = rng.uniform(0, 1, (5000, 3)).astype(np.float32)
    f[0] = 0.0; f[1] = [1.0, 0.0, 0.5]
    w = np.empty((5000, 8), np.float32)
    hm.hm_corner_weights(_p(f), C.c_uint32(5000), _p(w))
    g = np.float32(1.0) - f
    for k in range(8):
        wx, wy, wz = ((f if (k >> d) & 1 else g)[:, d] for d in range(3))
        assert np.array_equal(w[:, k].view(np.uint32), ((wx * wy) * wz).view(np.uint32)), k


def test_face_maps_against_the_neighbouring_cells_corners(hm):
    """The coarse role's shared-face pass (face_k1 / face_k0 / face_far_coord): for each axis and direction, enumerate the
    8 corners of the neighbouring cell by brute force; the four that are NOT corners of the base cell are the far face,
    and far corner j (the other two axes' bits in x < y < z order) must be corner k1 (+) / k0 (-) of the neighbour's cell
    at the coordinates the maps give; the other four are corner k ^ axis-bit of the base cell (the near face)."""
    base = np.array([10, 20, 30], np.uint32)
    k1, k0 = np.empty(12, np.uint32), np.empty(12, np.uint32)
    far_plus, far_minus = np.empty((12, 3), np.uint32), np.empty((12, 3), np.uint32)
    hm.hm_face_maps(_p(base), _p(k1), _p(k0), _p(far_plus), _p(far_minus))
    base_corners = {tuple(int(base[d]) + ((k >> d) & 1) for d in range(3)) for k in range(8)}
    for axis in range(3):
        others = [d for d in range(3) if d != axis]
        for sign, ks, far in ((+1, k1, far_plus), (-1, k0, far_minus)):
            cell = [int(v) for v in base]
            cell[axis] += sign
            far_face = {}
            for k in range(8):
                c = tuple(cell[d] + ((k >> d) & 1) for d in range(3))
                if c in base_corners:          # the near face: the base cell's corner with the axis bit flipped
                    assert c == tuple(int(base[d]) + (((k ^ (1 << axis)) >> d) & 1) for d in range(3))
                else:
                    j = ((k >> others[0]) & 1) | (((k >> others[1]) & 1) << 1)
                    far_face[j] = (k, c)
            assert sorted(far_face) == [0, 1, 2, 3]
            for j in range(4):
                assert int(ks[axis * 4 + j]) == far_face[j][0], (axis, sign, j)
                assert tuple(int(v) for v in far[axis * 4 + j]) == far_face[j][1], (axis, sign, j)


def test_grid_planners_built_for_the_host_plan_what_the_library_plans(hm):
    """csrc/mi3d_grid_plan.h is host code: built with plain g++ (no HIP header, -Wall -Wextra -Werror), its encode and
    scatter planners return the very integers libmi3d.so's plan queries - and so its launches - return, over the whole
    matrix of tests/plan_matrix.py."""
    import plan_matrix
    from mi3d import _lib
    lib = _lib.lib()
    for name, plans in (("encode", plan_matrix.encode_plans), ("scatter", plan_matrix.scatter_plans)):
        host, product = plans(getattr(hm, f"hm_grid_{name}_plan")), plans(getattr(lib, f"mi3d_grid_{name}_plan"))
        assert sorted(host) == sorted(product)
        for k in host:
            assert np.array_equal(host[k], product[k]), k
        assert (host[f"{name}_rc"] == 0).all()


def test_lds_tile_transposition_offsets(hm):
    """The MLP backward turns its 32 x 32 binary16 tiles round through LDS (csrc/lds_transpose.h, offsets in
    csrc/mi3d_common.h).  Played through on the host: every lane writes its four 8-byte chunks at its write offset, the
    transposing read's exchange (lane t of a 16-lane group, value j <- value t & 3 of what lane 4 j + (t >> 2) of the group
    loaded; tools/tr_probe.hip checks that pattern on the chip) is applied to what every lane loads at its read offset, and
    lane = feature must end up with value q = sample rowmap(q, h') - for both value orders; a half-wave's writes spread over
    all 32 LDS banks (two lanes per bank pair: the rate of a 256-byte-per-instruction write anyway)."""
    wr_d, wr_x, rd = (np.empty(64, np.uint32) for _ in range(3))
    row = C.c_int32(0)
    hm.hm_tr_offsets(_p(wr_d), _p(wr_x), _p(rd), C.byref(row))
    row = row.value
    assert row % 8 == 0 and row >= 64           # 8-byte aligned chunks (the read returns wrong data off alignment)
    rowmap = lambda q, h: (q & 3) + 8 * (q >> 2) + 4 * h
    for kind, wr, step in (("D", wr_d, 16), ("X", wr_x, 8)):
        img = np.full(32 * row // 2, -1, np.int64)  # halfwords; the value = 100 sample + feature
        for lane in range(64):
            s, h = lane & 31, lane >> 5
            for c in range(4):
                at = int(wr[lane]) + step * c
                assert at % 8 == 0
                for e in range(4):
                    q = 4 * c + e
                    assert img[at // 2 + e] == -1   # nobody else's chunk
                    img[at // 2 + e] = 100 * s + (rowmap(q, h) if kind == "D" else 16 * h + q)
        for c in range(4):
            loaded = np.stack([img[(int(rd[lane]) + 8 * row * c) // 2:][:4] for lane in range(64)])   # [lane][4]
            for lane in range(64):
                g, t, f, hp = lane >> 4, lane & 15, lane & 31, lane >> 5
                for j in range(4):
                    got = loaded[16 * g + 4 * j + (t >> 2)][t & 3]
                    assert got == 100 * rowmap(4 * c + j, hp) + f, (kind, lane, c, j)
        # bank spread of one write instruction (32 banks of 4 bytes, a half-wave at a time)
        for half in (0, 1):
            banks = np.concatenate([((wr[32 * half:32 * half + 32].astype(np.int64) // 4) + d) % 32 for d in (0, 1)])
            assert np.bincount(banks, minlength=32).max() == 2
