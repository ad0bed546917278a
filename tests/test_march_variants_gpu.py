"""GPU: every launch shape of the training march (csrc/raymarching.hip k_march_train) against the CPU oracle, sample by
sample, and against the 16-rays-per-wave variant of itself.

mi3d_march_rays_train picks the rays per wave from the ray count alone (march_train_plan: 64 for one wave's worth, then
16, 32 from 32 737 rays, 64 from 65 473) and launches at most 4096 single-wave workgroups, so beyond 262 144 rays a wave
takes a second batch and re-uses its LDS staging.  What depends on the variant - the `live` mask, the ray count added to
counter[1], the cooperative flush of up to 64 x 8 staged samples, the re-use of the staging by the next batch - can put
a ray's rows into a neighbour's slab without changing a count or a tiling invariant, so every case here compares the
CONTENTS of xyzs / dirs / deltas per ray id.  Each case first asserts, through mi3d_march_train_plan (the function the
launch itself calls), that its N runs the variant it is meant for; tests/test_march_plan_cpu.py pins that table.

Bounds: none.  Both sides spell the walk with the same operations and contraction sites (tests/test_raymarching_gpu.py
test_march_rays_train_bit_exact holds that bar on 7 x 3001 rays), and the second leg compares the kernel with itself:
equality of the bit patterns is asserted, as uint32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import make_rays, random_bitfield

pytestmark = pytest.mark.gpu

H = 128
SENTINEL = 7.0
ALIGN = 128
SLICE = 8192            # rays per call of the second leg: 512 batches of 16 (asserted from the plan)
RESIDENT = 4096         # workgroups of one launch at the most
SPARE = 2 * ALIGN       # rows past N * max_steps, so that padding rows AND untouched rows exist whatever the total


def plan(N):
    from mi3d import _lib as L
    out = (C.c_uint32 * 3)()
    L.call("mi3d_march_train_plan", N, out)
    return tuple(out)


# ---------------------------------------------------------------------------- inputs and the oracle's samples


@functools.lru_cache(maxsize=2)
def scene(kind, max_steps, n_base):
    """n_base rays (make_rays(default_rng(0), n_base)), their noises, the occupancy, and the oracle's march of ALL of them
    with an uncapped M.  The oracle hands out slabs in ray order, so its rows ARE the (ray, step) order, and - rays being
    independent - the march of the first N rays is the first cum[N] rows: a case of N <= n_base rays takes a prefix."""
    from oracle import oracle as O
    O.lib()
    o, d = make_rays(np.random.default_rng(0), n_base)
    bits = np.full(H ** 3 // 8, 255, np.uint8) if kind == "ones" else random_bitfield(np.random.default_rng(1), 1, H)
    noises = np.random.default_rng(2).random(n_base).astype(np.float32)
    nears, fars = O.near_far_from_aabb(o, d, np.array([-1, -1, -1, 1, 1, 1], np.float32))
    x, dr, dl, rays, counter = O.march_rays_train(o, d, 1.0, bits, 1, H, nears, fars, noises=noises, align=-1,
                                                  max_steps=max_steps, return_counter=True)
    count = rays[:, 2].astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(count)])
    assert np.array_equal(rays[:, 0], np.arange(n_base)) and np.array_equal(rays[:, 1], cum[:-1])
    assert int(counter[0]) == cum[-1] == x.shape[0] and int(counter[1]) == n_base
    return dict(o=o, d=d, bits=bits, noises=noises, nears=nears, fars=fars, count=count, cum=cum, x=x, dirs=dr, dl=dl,
                max_steps=max_steps)


_DEVICE_INPUTS = {}


def device_inputs(dev, key, s):
    """The scene's inputs on the GPU, uploaded once per scene (one entry kept)."""
    if _DEVICE_INPUTS.get("key") != (key, str(dev)):
        _DEVICE_INPUTS.clear()
        _DEVICE_INPUTS.update(key=(key, str(dev)), t={k: torch.from_numpy(s[k]).to(dev)
                                                      for k in ("o", "d", "bits", "nears", "fars", "noises")})
    return _DEVICE_INPUTS["t"]


def march(dev, t, first, N, max_steps, M, zero_tail=True):
    """mi3d_march_rays_train on rays [first, first + N) of the uploaded set, into buffers of M rows full of the sentinel."""
    from mi3d import _lib as L
    xyzs = torch.full((M, 3), SENTINEL, device=dev)
    dirs = torch.full((M, 3), SENTINEL, device=dev)
    deltas = torch.full((M, 2), SENTINEL, device=dev)
    rays = torch.full((N, 3), -1, dtype=torch.int32, device=dev)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    L.call("mi3d_march_rays_train", L.ptr(t["o"][first:]), L.ptr(t["d"][first:]), L.ptr(t["bits"]), 1.0, 0.0, max_steps,
           N, 1, H, M, L.ptr(t["nears"][first:]), L.ptr(t["fars"][first:]), L.ptr(xyzs), L.ptr(dirs), L.ptr(deltas),
           L.ptr(rays), L.ptr(counter), L.ptr(t["noises"][first:]), L.stream())
    if zero_tail:
        L.call("mi3d_march_zero_tail", L.ptr(counter), ALIGN, M, L.ptr(xyzs), L.ptr(dirs), L.ptr(deltas), L.stream())
    return xyzs, dirs, deltas, rays.cpu().numpy(), counter.cpu().numpy()


def rows_in_ray_order(offset, count):
    """Row indices listing the slabs (offset[i], count[i]) one after another: (ray, step) order."""
    offset, count = np.asarray(offset, np.int64), np.asarray(count, np.int64)
    m = int(count.sum())
    return np.repeat(offset, count) + (np.arange(m, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count))


def assert_same_bits(got, want, count, what, rpw):
    """Rows in (ray, step) order, compared as bit patterns; a failure names the rays, their batch and lane."""
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if np.array_equal(g, w):
        return
    bad = np.nonzero((g != w).any(1))[0]
    rid = np.unique(np.repeat(np.arange(len(count)), count)[bad])
    raise AssertionError(f"{what}: {len(bad)} rows of {len(rid)} rays differ; first rays (id, batch, lane) "
                         f"{[(int(r), int(r) // rpw, int(r) % rpw) for r in rid[:8]]}")


@functools.lru_cache(maxsize=2)
def sliced_samples(dev, kind, max_steps, n_base):
    """The same rays marched in calls of about SLICE rays, each ray with its own noise; every call is asserted to run 16
    rays per wave in one round.  Returns the per-ray counts and the samples in (ray, step) order."""
    s = scene(kind, max_steps, n_base)
    t = device_inputs(dev, (kind, max_steps, n_base), s)
    cuts = list(range(0, n_base, SLICE)) + [n_base]
    if len(cuts) > 2 and cuts[-1] - cuts[-2] <= 64:      # a last call of one wave's worth would run 64 rays per wave
        del cuts[-2]
    counts, xs, ds, ls = [], [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        n = b - a
        assert plan(n) == (16, -(-n // 16), -(-n // 16)) and -(-n // 16) <= RESIDENT, (n, plan(n))
        xyzs, dirs, deltas, rays, counter = march(dev, t, a, n, max_steps, n * max_steps, zero_tail=False)
        assert np.array_equal(rays[:, 0], np.arange(n)) and counter[1] == n
        assert (rays[:, 1] >= 0).all() and (rays[:, 1] + rays[:, 2] <= counter[0]).all()
        m = int(counter[0])
        idx = torch.from_numpy(rows_in_ray_order(rays[:, 1], rays[:, 2])).to(dev)
        counts.append(rays[:, 2].astype(np.int64))
        xs.append(xyzs[:m][idx].cpu().numpy()), ds.append(dirs[:m][idx].cpu().numpy()), ls.append(deltas[:m][idx].cpu().numpy())
    return np.concatenate(counts), np.concatenate(xs), np.concatenate(ds), np.concatenate(ls)


# ---------------------------------------------------------------------------- the check of one call


def check_variant(dev, kind, max_steps, N, n_base, want_plan):
    assert plan(N) == want_plan, (N, plan(N), want_plan)          # the library places N in the variant under test
    rpw = want_plan[0]
    s = scene(kind, max_steps, n_base)
    t = device_inputs(dev, (kind, max_steps, n_base), s)
    count_r, m_r = s["count"][:N], int(s["cum"][N])
    M = N * max_steps + SPARE
    xyzs, dirs, deltas, rays, counter = march(dev, t, 0, N, max_steps, M)
    print(f"N {N} max_steps {max_steps} {kind}: plan {want_plan}, {m_r} samples, "
          f"{int((count_r == max_steps).sum())} rays of max_steps samples, {int((count_r == 0).sum())} empty")

    assert counter.tolist() == [m_r, N], (counter.tolist(), m_r, N)          # the ragged batch adds its own ray count
    assert np.array_equal(rays[:, 0], np.arange(N))
    assert np.array_equal(rays[:, 2], count_r)
    hit = rays[rays[:, 2] > 0]                 # empty rays own no rows (their offset may coincide with a neighbour's)
    order = np.argsort(hit[:, 1], kind="stable")
    offs, cnts = hit[order, 1].astype(np.int64), hit[order, 2].astype(np.int64)
    if len(hit):
        assert offs[0] == 0 and np.array_equal(offs[1:], np.cumsum(cnts)[:-1]) and offs[-1] + cnts[-1] == m_r
    else:
        assert m_r == 0

    # contents against the oracle, per ray id
    idx = torch.from_numpy(rows_in_ray_order(rays[:, 1], rays[:, 2])).to(dev)
    got = [a[:m_r][idx].cpu().numpy() for a in (xyzs, dirs, deltas)]
    for g, name in zip(got, ("x", "dirs", "dl")):
        assert_same_bits(g, s[name][:m_r], count_r, f"{name} against the oracle", rpw)

    # padding rows are zero, the rows past them were never touched
    pad = ALIGN - m_r % ALIGN
    assert m_r + pad < M
    for a in (xyzs, dirs, deltas):
        assert bool((a[m_r:m_r + pad] == 0).all()) and bool((a[m_r + pad:] == SENTINEL).all())

    # variant against variant: the same rays, 16 per wave.  No leeway.
    count_s, *ref = sliced_samples(dev, kind, max_steps, n_base)
    assert np.array_equal(count_s[:N], count_r)
    for g, r, name in zip(got, ref, ("xyzs", "dirs", "deltas")):
        assert_same_bits(g, r[:m_r], count_r, f"{name} against the 16-rays-per-wave calls", rpw)
    return s, rays


# ---------------------------------------------------------------------------- the cases


@pytest.mark.parametrize("kind", ["ones", "random"])
@pytest.mark.parametrize("N", [1, 37, 64])
def test_one_wave(cuda, kind, N):
    """One batch of up to 64 rays, 64 rays per wave, rays of hundreds of samples: many flushes per ray.  The rays are the
    first N of 128, so that the second leg can march them 16 per wave among the other 128."""
    s, _ = check_variant(cuda, kind, 1024, N, 128, (64, 1, 1))
    assert s["count"][:N].max() >= (24 if kind == "ones" else 3) * 8        # ring-fulls flushed by one ray


@pytest.mark.parametrize("kind", ["ones", "random"])
def test_64_wide(cuda, kind):
    """65 573 rays: 1025 batches of 64, the last of 37 rays.  On `ones` nearly every ray takes exactly max_steps = 32 = 4
    rings: all 64 rings fill in lockstep (the 512-entry flush) and a ray ends exactly on a full ring."""
    s, _ = check_variant(cuda, kind, 32, 65_573, 65_573, (64, 1025, 1025))
    if kind == "ones":
        assert (s["count"] == 32).mean() > 0.9


@pytest.mark.parametrize("kind", ["ones", "random"])
def test_32_wide(cuda, kind):
    """40 003 rays: 1251 batches of 32, the last of 3 rays."""
    check_variant(cuda, kind, 64, 40_003, 40_003, (32, 1251, 1251))


@pytest.mark.parametrize("N,want_plan", [(32_736, (16, 2046, 2046)), (32_737, (32, 1024, 1024)),
                                         (65_472, (32, 2046, 2046)), (65_473, (64, 1024, 1024))])
def test_boundaries(cuda, N, want_plan):
    """The same rays on both sides of each switch: every set is a prefix of one set of 65 473."""
    check_variant(cuda, "random", 16, N, 65_473, want_plan)


@pytest.mark.parametrize("kind,max_steps", [("ones", 24), ("random", 40)])
def test_later_rounds(cuda, kind, max_steps):
    """262 353 = 262 144 + 3 x 64 + 17 rays: 4100 batches on 4096 waves.  Batches 4096..4099 are the second round of waves
    0..3, on the LDS staging their first batch used; the last batch has 17 rays."""
    N = 262_353
    s, rays = check_variant(cuda, kind, max_steps, N, N, (64, 4100, RESIDENT))
    second = s["count"][RESIDENT * 64:]
    assert len(second) == 209 and (second > 0).all()            # every ray of the second round writes samples
    assert (rays[RESIDENT * 64:, 2] > 0).all()


@pytest.mark.parametrize("N,want_plan", [(65_573, (64, 1025, 1025)), (262_353, (64, 4100, RESIDENT))])
def test_dropped_slabs(cuda, N, want_plan):
    """M below the sample total: a ray whose slab does not fit writes nothing, every other ray writes exactly its samples.

    M is HALF the oracle's sample total, moved to the middle of a 24-row slab so that (nearly every ray having 24 rows) a
    dropped ray's rows lie below M and must keep the sentinel.  The kernel hands out slabs in the order its waves arrive (one atomic per batch),
    not in ray order, so which rays fit differs from run to run and from the oracle; the assertions are made on the
    offsets the kernel reports.  That a second-round ray is among the dropped ones follows from the order of arrival: a
    wave reserves the slab of its second batch after it has walked its first batch twice, and every wave that started
    with it (13 per CU, a wave's LDS staging being 12 032 B of a CU's 160 KB: 3328 of the 4100 batches) has by then
    finished the one walk that precedes its own reservation.  On `ones` every batch asks for the same 64 x 24 rows, so more than
    half of the total is handed out before the slabs of rays 262 144.. are asked for."""
    assert plan(N) == want_plan
    max_steps = 24
    s = scene("ones", max_steps, N)
    t = device_inputs(cuda, ("ones", max_steps, N), s)
    count_r, cum, total = s["count"], s["cum"], int(s["cum"][N])
    M = total // 2 // max_steps * max_steps + max_steps // 2    # ... and ends inside a slab where all before it are full ones
    xyzs, dirs, deltas, rays, counter = march(cuda, t, 0, N, max_steps, M, zero_tail=False)
    assert counter.tolist() == [total, N]                       # the full total, dropped rays included
    assert np.array_equal(rays[:, 0], np.arange(N)) and np.array_equal(rays[:, 2], count_r)
    off, cnt = rays[:, 1].astype(np.int64), rays[:, 2].astype(np.int64)
    kept = (cnt > 0) & (off + cnt <= M)
    dropped = (cnt > 0) & ~kept
    print(f"N {N}: M {M} of {total} samples, {int(kept.sum())} rays kept, {int(dropped.sum())} dropped, "
          f"{int(dropped[RESIDENT * 64:].sum())} of them in the second round")
    assert dropped[:RESIDENT * 64].any() and kept.any()
    if N > RESIDENT * 64:
        assert dropped[RESIDENT * 64:].any()

    # every kept ray holds exactly the oracle's samples
    got_rows = torch.from_numpy(rows_in_ray_order(off[kept], cnt[kept])).to(cuda)
    ref_rows = rows_in_ray_order(cum[:N][kept], cnt[kept])
    kept_count = np.where(kept, cnt, 0)
    for a, name in zip((xyzs, dirs, deltas), ("x", "dirs", "dl")):
        assert_same_bits(a[got_rows].cpu().numpy(), s[name][ref_rows], kept_count, f"{name} of the kept rays", 64)

    # every row of [0, M) outside the kept slabs still holds the sentinel
    edge = np.zeros(M + 1, np.int64)
    np.add.at(edge, off[kept], 1)
    np.add.at(edge, off[kept] + cnt[kept], -1)
    cover = np.cumsum(edge[:M])
    assert cover.max() <= 1                                     # kept slabs do not overlap
    free = torch.from_numpy(cover == 0).to(cuda)
    assert int(free.sum()) == M - int(cnt[kept].sum())
    print(f"{int(free.sum())} rows of [0, M) belong to no kept slab")
    for a in (xyzs, dirs, deltas):
        assert bool((a[free] == SENTINEL).all())
