"""GPU parity: the HIP raymarching operators (through the `raymarching` drop-in package -> C ABI) against the
CPU oracle on identical seeded inputs.  Integer outputs and everything derived from the DDA walk are bit-exact;
composited floats are compared at the tolerance BASELINE.json states (1e-4 relative)."""
import numpy as np
import pytest
import torch

import infer_march_cases as IM
from conftest import make_rays, random_bitfield, sphere_bitfield

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # north_star: "within 1e-4 relative fp32"


def T(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)   # (shared case arrays are read-only)


def test_loads_native_library(cuda):
    from mi3d import _lib
    assert _lib.lib().mi3d_abi_version() == 5


def test_near_far_bit_exact(cuda, oracle):
    import raymarching
    rng = np.random.default_rng(1)
    o, d = make_rays(rng, 5000)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    for min_near in (0.2, 0.05):
        n_ref, f_ref = oracle.near_far_from_aabb(o, d, aabb, min_near)
        n, f = raymarching.near_far_from_aabb(T(o, cuda), T(d, cuda), T(aabb, cuda), min_near)
        assert np.array_equal(n.cpu().numpy(), n_ref) and np.array_equal(f.cpu().numpy(), f_ref)
    assert (n_ref == np.finfo(np.float32).max).any()  # the miss path was exercised


def test_sph_from_ray(cuda, oracle):
    import raymarching
    rng = np.random.default_rng(2)
    o = rng.uniform(-0.5, 0.5, (1000, 3)).astype(np.float32)
    d = rng.normal(size=(1000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ref = oracle.sph_from_ray(o, d, 2.0)
    out = raymarching.sph_from_ray(T(o, cuda), T(d, cuda), 2.0).cpu().numpy()
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=2e-5)


def test_morton_all_coords_bit_exact(cuda, oracle):
    import raymarching
    co = np.stack(np.meshgrid(*[np.arange(128)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    ref = oracle.morton3D(co)
    idx = raymarching.morton3D(T(co, cuda))
    assert np.array_equal(idx.cpu().numpy(), ref)
    back = raymarching.morton3D_invert(idx)
    assert np.array_equal(back.cpu().numpy(), co)
    # 10-bit range
    big = np.array([[1023, 0, 0], [0, 1023, 0], [0, 0, 1023], [1023, 1023, 1023]], np.int32)
    assert np.array_equal(raymarching.morton3D(T(big, cuda)).cpu().numpy(), oracle.morton3D(big))
    assert raymarching.morton3D(torch.zeros(0, 3, dtype=torch.int32, device=cuda)).numel() == 0


def test_packbits_bit_exact(cuda, oracle):
    import raymarching
    rng = np.random.default_rng(3)
    grid = rng.exponential(1.0, (2, 128 ** 3)).astype(np.float32)
    grid[0, :64] = -1.0
    for thresh in (0.0, 0.7, 10.0):
        grid[1, 100:108] = thresh  # strict '>' at equality
        ref = oracle.packbits(grid, thresh)
        out = raymarching.packbits(T(grid, cuda), thresh)
        assert np.array_equal(out.cpu().numpy(), ref)


MARCH_CASES = [
    # C, bound, bitfield, dt_gamma, max_steps, perturb
    (1, 1.0, "ones", 0.0, 1024, True),
    (1, 1.0, "ones", 0.0, 64, False),
    (1, 1.0, "sphere", 0.0, 512, True),
    (1, 1.0, "random", 1 / 128, 256, True),
    (3, 4.0, "random", 1 / 128, 1024, True),
    (2, 2.0, "sphere", 0.0, 1024, False),
    (1, 1.0, "empty", 0.0, 128, False),
]


def _bits(kind, rng, oracle, C, H, bound):
    if kind == "ones":
        return np.full(C * H ** 3 // 8, 255, np.uint8)
    if kind == "empty":
        return np.zeros(C * H ** 3 // 8, np.uint8)
    if kind == "sphere":
        return sphere_bitfield(oracle, C, H, 0.3 * bound)
    return random_bitfield(rng, C, H)


def _per_ray(rays, *arrays):
    """Re-key slab-ordered outputs by ray id so two legal slab orders compare equal."""
    out = {}
    for rid, off, cnt in rays:
        out[int(rid)] = tuple(a[off:off + cnt] for a in arrays)
    return out


@pytest.mark.parametrize("C,bound,kind,dt_gamma,max_steps,perturb", MARCH_CASES)
def test_march_rays_train_bit_exact(cuda, oracle, C, bound, kind, dt_gamma, max_steps, perturb):
    import raymarching
    from mi3d import _lib as L
    H, N = 128, 3001  # ragged: not a multiple of the wave size
    rng = np.random.default_rng(10 + C)
    o, d = make_rays(rng, N, bound)
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb)
    bits = _bits(kind, rng, oracle, C, H, bound)
    noises = rng.random(N).astype(np.float32) if perturb else np.zeros(N, np.float32)
    xr, dr, lr, rr, cr = oracle.march_rays_train(o, d, bound, bits, C, H, nears, fars, noises=noises, align=128,
                                                 dt_gamma=dt_gamma, max_steps=max_steps, return_counter=True)
    # call the C ABI directly so the test controls `noises` (the wrapper draws them with torch.rand)
    M = N * max_steps
    dev = cuda
    xyzs = torch.full((M, 3), 7.0, device=dev)
    dirs = torch.full((M, 3), 7.0, device=dev)
    deltas = torch.full((M, 2), 7.0, device=dev)
    rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    args = [T(o, dev), T(d, dev), T(bits, dev), T(nears, dev), T(fars, dev), T(noises, dev)]
    L.call("mi3d_march_rays_train", L.ptr(args[0]), L.ptr(args[1]), L.ptr(args[2]), float(bound), float(dt_gamma),
           max_steps, N, C, H, M, L.ptr(args[3]), L.ptr(args[4]), L.ptr(xyzs), L.ptr(dirs), L.ptr(deltas),
           L.ptr(rays), L.ptr(counter), L.ptr(args[5]), L.stream())
    L.call("mi3d_march_zero_tail", L.ptr(counter), 128, M, L.ptr(xyzs), L.ptr(dirs), L.ptr(deltas), L.stream())
    cnt = counter.cpu().numpy()
    assert np.array_equal(cnt, cr), (cnt, cr)
    m = int(cnt[0])
    rays_h = rays.cpu().numpy()
    # integer side: every ray's step count is bit-exact; slabs tile [0, m) without overlap
    assert np.array_equal(rays_h[:, 0], np.arange(N))
    assert np.array_equal(rays_h[:, 2], rr[:, 2])
    hit = rays_h[rays_h[:, 2] > 0]  # empty rays own no rows (their offset may coincide with a neighbour's)
    if len(hit):
        order = np.argsort(hit[:, 1], kind="stable")
        offs, cnts = hit[order, 1], hit[order, 2]
        assert offs[0] == 0 and np.array_equal(offs[1:], np.cumsum(cnts)[:-1]) and offs[-1] + cnts[-1] == m
    # float side: identical fused-multiply-add sites => identical bits, compared per ray id
    got = _per_ray(rays_h, xyzs[:m].cpu().numpy(), dirs[:m].cpu().numpy(), deltas[:m].cpu().numpy())
    ref = _per_ray(rr, xr, dr, lr)
    for rid in range(N):
        for a, b in zip(got[rid], ref[rid]):
            assert np.array_equal(a, b), rid
    # padding rows are zero, as the reference's zero-filled buffers leave them
    pad = 128 - m % 128
    assert float(xyzs[m:m + pad].abs().max()) == 0 and float(deltas[m:m + pad].abs().max()) == 0
    if kind == "empty":
        assert m == 0


def test_march_wrapper_contract(cuda, oracle):
    """The drop-in op: padding rule, dtypes, step_counter side effects, perturb RNG, overflow drop."""
    import raymarching
    rng = np.random.default_rng(5)
    N, H = 777, 128
    o, d = make_rays(rng, N)
    aabb = T(np.array([-1, -1, -1, 1, 1, 1], np.float32), cuda)
    bits = T(sphere_bitfield(oracle, 1, H, 0.4), cuda)
    nears, fars = raymarching.near_far_from_aabb(T(o, cuda), T(d, cuda), aabb)
    counter = torch.zeros(2, dtype=torch.int32, device=cuda)
    xyzs, dirs, deltas, rays = raymarching.march_rays_train(T(o, cuda), T(d, cuda), 1.0, bits, 1, H, nears, fars,
                                                            counter, -1, False, 128, True, 0, 512)
    m = int(counter[0])
    assert int(counter[1]) == N
    assert xyzs.shape[0] == m + (128 - m % 128) and xyzs.shape[0] % 128 == 0
    assert dirs.shape == xyzs.shape and deltas.shape == (xyzs.shape[0], 2) and rays.shape == (N, 3)
    ref = oracle.march_rays_train(o, d, 1.0, bits.cpu().numpy(), 1, H, nears.cpu().numpy(), fars.cpu().numpy(),
                                  align=128, max_steps=512)
    # slabs are reserved in wave-arrival order: compare per ray id
    got = _per_ray(rays.cpu().numpy(), xyzs.cpu().numpy(), deltas.cpu().numpy())
    want = _per_ray(ref[3], ref[0], ref[2])
    for rid in range(N):
        assert np.array_equal(got[rid][0], want[rid][0]) and np.array_equal(got[rid][1], want[rid][1])
    assert float(xyzs[m:].abs().max()) == 0 and float(deltas[m:].abs().max()) == 0
    # mean_count mode: M is capped, overflowing rays are dropped silently and composite zeroes them
    mc = max(128, m // 2)
    x2, d2, l2, r2 = raymarching.march_rays_train(T(o, cuda), T(d, cuda), 1.0, bits, 1, H, nears, fars, None, mc,
                                                  False, 128, False, 0, 512)
    assert x2.shape[0] == mc + (128 - mc % 128)
    sig = torch.ones(x2.shape[0], device=cuda)
    rgb = torch.ones(x2.shape[0], 3, device=cuda)
    ws, dep, img = raymarching.composite_rays_train(sig, rgb, l2, r2)
    r2h = r2.cpu().numpy()
    dropped = (r2h[:, 1] + r2h[:, 2] > x2.shape[0]) & (r2h[:, 2] > 0)
    assert dropped.any() and float(ws[torch.from_numpy(r2h[dropped, 0]).long()].abs().max()) == 0


def _composite_inputs(rng, oracle, N=1500, max_steps=256, kind="sphere"):
    o, d = make_rays(rng, N)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb)
    bits = sphere_bitfield(oracle, 1, 128, 0.45) if kind == "sphere" else np.full(128 ** 3 // 8, 255, np.uint8)
    xyzs, dirs, deltas, rays = oracle.march_rays_train(o, d, 1.0, bits, 1, 128, nears, fars,
                                                       noises=rng.random(N).astype(np.float32), align=128,
                                                       max_steps=max_steps)
    m = xyzs.shape[0]
    sig = rng.exponential(1.0, m).astype(np.float32)
    return sig, rng.random((m, 3)).astype(np.float32), deltas, rays


@pytest.mark.parametrize("density,T_thresh", [(3.0, 1e-4), (60.0, 1e-4), (400.0, 1e-2), (0.0, 1e-4)])
@pytest.mark.parametrize("sdf", [False, True])
def test_composite_train_forward_backward(cuda, oracle, density, T_thresh, sdf):
    import raymarching
    rng = np.random.default_rng(20)
    sig, rgb, deltas, rays = _composite_inputs(rng, oracle, kind="ones" if density < 100 else "sphere")
    sig = sig * density
    if sdf:
        sig = np.clip(sig * 0.01, 0, 0.95).astype(np.float32)  # alpha = sigma must stay in [0,1)
    rays = rays.copy()
    rays[5, 1] = sig.shape[0] - 1  # a ray whose slab overflows M: must come out as zeros
    rays[5, 2] = 64
    ws_r, dep_r, img_r = oracle.composite_rays_train(sig, rgb, deltas, rays, T_thresh, sdf=sdf)
    fn = raymarching.composite_sdf_rays_train if sdf else raymarching.composite_rays_train
    s_t = T(sig, cuda).requires_grad_(True)
    c_t = T(rgb, cuda).requires_grad_(True)
    ws, dep, img = fn(s_t, c_t, T(deltas, cuda), T(rays, cuda), T_thresh)
    np.testing.assert_allclose(ws.detach().cpu().numpy(), ws_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(img.detach().cpu().numpy(), img_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(dep.detach().cpu().numpy(), dep_r, rtol=RTOL, atol=1e-5)
    assert ws_r[rays[5, 0]] == 0 and float(ws.detach()[rays[5, 0]]) == 0

    g_ws = rng.normal(size=ws_r.shape).astype(np.float32)
    g_img = rng.normal(size=img_r.shape).astype(np.float32)
    g_dep = rng.normal(size=ws_r.shape).astype(np.float32)  # must be ignored
    torch.autograd.backward([ws, dep, img], [T(g_ws, cuda), T(g_dep, cuda), T(g_img, cuda)])
    gs_r, gc_r = oracle.composite_rays_train_backward(g_ws, g_img, sig, rgb, deltas, rays, ws_r, img_r, T_thresh,
                                                      sdf=sdf)
    gs, gc = s_t.grad.cpu().numpy(), c_t.grad.cpu().numpy()
    np.testing.assert_allclose(gc, gc_r, rtol=RTOL, atol=1e-6)
    # d sigma sums terms of mixed sign: tolerance relative to the per-ray gradient scale
    scale = np.abs(gs_r).max() + 1e-12
    assert np.abs(gs - gs_r).max() <= 2e-4 * scale
    # samples behind an early-terminated ray keep exactly zero gradient
    # (the sample where T crosses T_thresh can differ by one when the two transmittances differ by an ulp)
    assert np.mean((gs_r == 0) != (gs == 0)) < 2e-3


def test_composite_empty_and_single(cuda, oracle):
    import raymarching
    rays = np.array([[0, 0, 0], [1, 0, 1], [2, 1, 3]], np.int32)
    sig = np.array([2.0, 0.5, 100.0, 3.0], np.float32)
    rgb = np.arange(12, dtype=np.float32).reshape(4, 3) / 12
    deltas = np.full((4, 2), 0.1, np.float32)
    ref = oracle.composite_rays_train(sig, rgb, deltas, rays)
    out = raymarching.composite_rays_train(T(sig, cuda), T(rgb, cuda), T(deltas, cuda), T(rays, cuda))
    for a, b in zip(out, ref):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=RTOL, atol=1e-7)
    e = raymarching.composite_rays_train(torch.zeros(0, device=cuda), torch.zeros(0, 3, device=cuda),
                                         torch.zeros(0, 2, device=cuda), torch.zeros(0, 3, dtype=torch.int32,
                                                                                    device=cuda))
    assert e[0].numel() == 0


def test_inference_march_composite_loop(cuda, oracle):
    """The reference's test-time loop (nerf/renderer.py:526-551) driven through both implementations."""
    import raymarching
    rng = np.random.default_rng(30)
    N, H = 600, 128
    o, d = make_rays(rng, N)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb)
    bits = sphere_bitfield(oracle, 1, H, 0.5)

    def field(x):  # deterministic toy field evaluated on the host for both sides
        s = (40 * np.exp(-np.sum(x * x, 1) / 0.05)).astype(np.float32)
        c = (0.5 + 0.5 * np.sin(x * 7)).astype(np.float32)
        nrm = (x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-6)).astype(np.float32)
        return s, c, nrm

    # oracle
    ws_r, dep_r = np.zeros(N, np.float32), np.zeros(N, np.float32)
    img_r, nrm_r = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    alive_r, t_r = np.arange(N, dtype=np.int32), nears.copy()
    # device
    ws, dep = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda)
    img, nrm = torch.zeros(N, 3, device=cuda), torch.zeros(N, 3, device=cuda)
    alive, t = torch.arange(N, dtype=torch.int32, device=cuda), T(nears, cuda).clone()
    step = 0
    while step < 256:
        n_alive = alive_r.shape[0]
        assert alive.shape[0] == n_alive
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xr, dr, lr = oracle.march_rays(n_alive, n_step, alive_r, t_r, o, d, 1.0, bits, 1, H, nears, fars, align=128,
                                       max_steps=256)
        x, dd, l = raymarching.march_rays(n_alive, n_step, alive, t, T(o, cuda), T(d, cuda), 1.0, T(bits, cuda), 1,
                                          H, T(nears, cuda), T(fars, cuda), 128, False, 0, 256)
        assert np.array_equal(x.cpu().numpy(), xr) and np.array_equal(l.cpu().numpy(), lr)
        s, c, nm = field(xr)
        oracle.composite_rays(n_alive, n_step, alive_r, t_r, s, c, nm, lr, ws_r, dep_r, img_r, nrm_r, 1e-2)
        raymarching.composite_rays(n_alive, n_step, alive, t, T(s, cuda), T(c, cuda), T(nm, cuda), l, ws, dep, img,
                                   nrm, 1e-2)
        assert np.array_equal(alive.cpu().numpy() >= 0, alive_r >= 0)
        alive_r = alive_r[alive_r >= 0]
        alive = alive[alive >= 0]
        step += n_step
    np.testing.assert_allclose(ws.cpu().numpy(), ws_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(img.cpu().numpy(), img_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(nrm.cpu().numpy(), nrm_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(dep.cpu().numpy(), dep_r, rtol=RTOL, atol=1e-5)


def test_inference_march_composite_sdf_loop(cuda, oracle):
    """The same loop through composite_sdf_rays (C ABI mi3d_composite_sdf_rays: alpha = sigma, no normals), round after
    round until nobody is alive.  The three ways a ray leaves a round are told apart from the oracle's data and each must
    occur: stopped by T < T_thresh (it died although none of its rows has a zero delta), stopped on the zero-delta
    sentinel (it died with weights_sum < 1 - T_thresh, so no step of it ever saw T < T_thresh), survived (rays_t written
    back).  The alive flags and rays_t are exact: alpha is an input, and t only ever adds deltas in the same order."""
    import raymarching
    rng = np.random.default_rng(30)
    N, H, T_thresh = 600, 128, 1e-2
    o, d = make_rays(rng, N)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb)
    bits = sphere_bitfield(oracle, 1, H, 0.5)

    def field(x):  # the toy field of the density loop, its sigma in [0, 40] mapped into [0, 0.95] as alpha
        a = (40 * np.exp(-np.sum(x * x, 1) / 0.05) * (0.95 / 40)).astype(np.float32)
        c = (0.5 + 0.5 * np.sin(x * 7)).astype(np.float32)
        return a, c

    ws_r, dep_r, img_r = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
    alive_r, t_r = np.arange(N, dtype=np.int32), nears.copy()
    ws, dep, img = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda), torch.zeros(N, 3, device=cuda)
    alive, t = torch.arange(N, dtype=torch.int32, device=cuda), T(nears, cuda).clone()
    by_thresh = by_thresh_multi = by_sentinel = survived = rounds = 0
    while True:
        n_alive = alive_r.shape[0]
        assert alive.shape[0] == n_alive
        if n_alive == 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xr, dr, lr = oracle.march_rays(n_alive, n_step, alive_r, t_r, o, d, 1.0, bits, 1, H, nears, fars, align=128,
                                       max_steps=256)
        x, dd, l = raymarching.march_rays(n_alive, n_step, alive, t, T(o, cuda), T(d, cuda), 1.0, T(bits, cuda), 1,
                                          H, T(nears, cuda), T(fars, cuda), 128, False, 0, 256)
        assert np.array_equal(x.cpu().numpy(), xr) and np.array_equal(l.cpu().numpy(), lr)
        a, c = field(xr)
        assert 0 <= a.min() and a.max() <= 0.95
        ids, t_before = alive_r.copy(), t_r.copy()
        oracle.composite_sdf_rays(n_alive, n_step, alive_r, t_r, a, c, lr, ws_r, dep_r, img_r, T_thresh)
        raymarching.composite_sdf_rays(n_alive, n_step, alive, t, T(a, cuda), T(c, cuda), l, ws, dep, img, T_thresh)
        assert np.array_equal(alive.cpu().numpy() >= 0, alive_r >= 0)
        assert np.array_equal(t.cpu().numpy(), t_r)
        died = alive_r < 0
        full = (lr[:n_alive * n_step, 0].reshape(n_alive, n_step) != 0).all(1)
        by_thresh += int((died & full).sum())
        by_thresh_multi += int((died & full).sum()) if n_step > 1 else 0
        by_sentinel += int((died & ~full & (ws_r[ids] < 1 - T_thresh)).sum())
        survived += int((~died).sum())
        assert (~died <= full).all() and (t_r[ids[~died]] > t_before[ids[~died]]).all()   # a survivor took n_step steps
        assert np.array_equal(t_r[ids[died]], t_before[ids[died]])                       # rays_t of a dead ray stays
        alive_r = alive_r[alive_r >= 0]
        alive = alive[alive >= 0]
        rounds += 1
        assert rounds < 300
    print(f"{rounds} rounds: {by_thresh} rays stopped by T < T_thresh ({by_thresh_multi} in rounds of several steps), "
          f"{by_sentinel} on the zero-delta sentinel, {survived} survivals")
    assert by_thresh > 0 and by_thresh_multi > 0 and by_sentinel > 0 and survived > 0
    assert by_thresh + by_sentinel <= N
    np.testing.assert_allclose(ws.cpu().numpy(), ws_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(img.cpu().numpy(), img_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(dep.cpu().numpy(), dep_r, rtol=RTOL, atol=1e-5)
    assert float(ws_r.max()) > 1 - T_thresh and float(ws_r.min()) == 0


# ---- the inference march away from C = 1, bound = 1, dt_gamma = 0: the cases of tests/infer_march_cases.py ----------------


def _case_on_device(c, dev):
    import types
    return types.SimpleNamespace(o=T(c.o, dev), d=T(c.d, dev), bits=T(c.bits, dev), nears=T(c.nears, dev),
                                 fars=T(c.fars, dev), noises=T(c.noises, dev))


def _march_rays_abi(c, g, n_alive, n_step, alive, t, noises):
    """mi3d_march_rays called directly, so that the test supplies `noises` (the wrapper draws them with torch.rand)."""
    from mi3d import _lib as L
    M = n_alive * n_step
    M += IM.ALIGN - M % IM.ALIGN
    xyzs, dirs = torch.zeros(M, 3, device=alive.device), torch.zeros(M, 3, device=alive.device)
    deltas = torch.zeros(M, 2, device=alive.device)
    assert alive.shape[0] >= n_alive and noises.shape[0] >= n_alive and t.shape[0] == c.N
    L.call("mi3d_march_rays", n_alive, n_step, L.ptr(alive), L.ptr(t), L.ptr(g.o), L.ptr(g.d), float(c.bound),
           float(c.dt_gamma), c.max_steps, c.C, c.H, L.ptr(g.bits), L.ptr(g.nears), L.ptr(g.fars), L.ptr(xyzs), L.ptr(dirs),
           L.ptr(deltas), L.ptr(noises), L.stream())
    return xyzs, dirs, deltas


def _assert_accumulators(final, ws, dep, img, nrm):
    np.testing.assert_allclose(ws.cpu().numpy(), final.weights_sum, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(img.cpu().numpy(), final.image, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(nrm.cpu().numpy(), final.normal, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(dep.cpu().numpy(), final.depth, rtol=RTOL, atol=1e-5)


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("name", IM.NAMES)
def test_inference_march_cases_loop(cuda, oracle, name, perturb):
    """k_march_infer + composite_rays through the reference's loop at cone steps, two and three cascades and bound > 1,
    with the round-0 jitter supplied by the test: every round's xyzs / dirs / deltas bit-equal to the oracle's (the same
    fused-multiply-add sites, as at C = 1), the same rays die, rays_t moves alike, the final accumulators at 1e-4."""
    import raymarching
    c, g = IM.case(name), _case_on_device(IM.case(name), cuda)
    rounds, final = IM.reference_loop(name, perturb)
    N = c.N
    ws, dep = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda)
    img, nrm = torch.zeros(N, 3, device=cuda), torch.zeros(N, 3, device=cuda)
    alive, t = torch.arange(N, dtype=torch.int32, device=cuda), g.nears.clone()
    zeros = torch.zeros(N, device=cuda)
    for k, r in enumerate(rounds):
        assert np.array_equal(alive.cpu().numpy(), r.alive)
        noises = g.noises if perturb and k == 0 else zeros
        x, dd, l = _march_rays_abi(c, g, r.n_alive, r.n_step, alive, t, noises)
        assert np.array_equal(x.cpu().numpy(), r.xyzs), (name, k)
        assert np.array_equal(dd.cpu().numpy(), r.dirs), (name, k)
        assert np.array_equal(l.cpu().numpy(), r.deltas), (name, k)
        s, col, nm = c.field(r.xyzs)
        raymarching.composite_rays(r.n_alive, r.n_step, alive, t, T(s, cuda), T(col, cuda), T(nm, cuda), l, ws, dep, img,
                                   nrm, c.T_thresh)
        assert np.array_equal(alive.cpu().numpy() >= 0, r.alive_after >= 0), (name, k)
        assert np.array_equal(t.cpu().numpy(), r.t_after), (name, k)     # t only ever adds deltas[:, 1], in the same order
        alive = alive[alive >= 0]
    assert alive.numel() == 0
    _assert_accumulators(final, ws, dep, img, nrm)


@pytest.mark.parametrize("name", IM.NAMES)
def test_march_rays_wrapper_draws_one_rand_per_alive_slot(cuda, oracle, name):
    """raymarching.march_rays(perturb=True) draws exactly one torch.rand(n_alive) and hands noises[n] to alive SLOT n: after
    the same seed its rows equal the oracle's on that draw - in round 0, and on the alive list of a later round (fewer
    rays than N, slot != ray id, n_step > 1), where a jitter looked up by ray id or a draw of another shape would show."""
    import raymarching
    c, g = IM.case(name), _case_on_device(IM.case(name), cuda)
    rounds, _ = IM.reference_loop(name, False)
    later = next(r for r in rounds if r.n_step > 1 and r.n_alive > 32)
    assert not np.array_equal(later.alive, np.arange(later.n_alive))
    for seed, r in ((5, rounds[0]), (6, later)):
        torch.manual_seed(seed)
        noises = torch.rand(r.n_alive, dtype=torch.float32, device=cuda).cpu().numpy()
        xr, dr, lr = oracle.march_rays(r.n_alive, r.n_step, r.alive, r.t, c.o, c.d, c.bound, c.bits, c.C, c.H, c.nears,
                                       c.fars, align=IM.ALIGN, noises=noises, dt_gamma=c.dt_gamma, max_steps=c.max_steps)
        assert not np.array_equal(xr, r.xyzs)                                    # the draw moves the rows
        torch.manual_seed(seed)
        x, dd, l = raymarching.march_rays(r.n_alive, r.n_step, T(r.alive, cuda), T(r.t, cuda), g.o, g.d, c.bound, g.bits,
                                          c.C, c.H, g.nears, g.fars, IM.ALIGN, True, c.dt_gamma, c.max_steps)
        assert np.array_equal(x.cpu().numpy(), xr) and np.array_equal(dd.cpu().numpy(), dr)
        assert np.array_equal(l.cpu().numpy(), lr)
        after = torch.rand(3, device=cuda)
        torch.manual_seed(seed)
        torch.rand(r.n_alive, dtype=torch.float32, device=cuda)
        assert torch.equal(after, torch.rand(3, device=cuda))                    # and nothing else was drawn


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("name", IM.NAMES)
def test_inference_ctl_loop_cases(cuda, oracle, name, perturb):
    """infer_begin / march_rays_ctl / composite_rays_ctl / compact_alive_ctl (k_march_infer_ctl) through the same loop with
    `noises` a device tensor of N values handed to EVERY round, as the renderer does: the kernel applies them while
    ctl[4] == 0 only.  Per round: the plan in ctl, the rows [0, n_alive n_step) bit-equal to the oracle's (re-used buffers:
    the rows a finished ray leaves are zeroed), the alignment rows up to ctl[2] zero, nothing written behind the largest round, the
    compacted alive list and rays_t equal.  With perturb, round 1 matches the correct loop and so differs from the loop
    that jitters every round; and one round 0 runs on the alive list in reverse order, where a jitter looked up by ray id
    instead of alive slot lands on the wrong rays."""
    import raymarching
    c, g = IM.case(name), _case_on_device(IM.case(name), cuda)
    rounds, final = IM.reference_loop(name, perturb)
    N, FILL = c.N, 7.0
    noises = g.noises if perturb else None
    cap = N + 2 * IM.ALIGN                      # >= N + align rows, as march_rays_ctl asks
    xyzs, dirs = torch.full((cap, 3), FILL, device=cuda), torch.full((cap, 3), FILL, device=cuda)
    deltas = torch.full((cap, 2), FILL, device=cuda)

    def march(ctl, alive, t):
        raymarching.march_rays_ctl(ctl, N, alive, t, g.o, g.d, c.bound, g.bits, c.C, c.H, g.fars, xyzs, dirs, deltas,
                                   noises, c.dt_gamma, c.max_steps)

    high = [0]       # the most rows any round so far has had: the buffers are re-used, nothing is written behind that

    def rows_equal(rows, xr, dr, lr, what):
        assert rows == xr.shape[0] <= cap - 1, what
        assert np.array_equal(xyzs[:rows].cpu().numpy(), xr), what
        assert np.array_equal(dirs[:rows].cpu().numpy(), dr), what
        assert np.array_equal(deltas[:rows].cpu().numpy(), lr), what
        high[0] = max(high[0], rows)
        assert bool((xyzs[high[0]:] == FILL).all()) and bool((dirs[high[0]:] == FILL).all()), what
        assert bool((deltas[high[0]:] == FILL).all()), what

    ws, dep = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda)
    img, nrm = torch.zeros(N, 3, device=cuda), torch.zeros(N, 3, device=cuda)
    t = g.nears.clone()
    ctl, alive = raymarching.infer_begin(N, cuda, IM.ALIGN)
    spare = torch.full_like(alive, -7)
    assert ctl.numel() == 8
    for k, r in enumerate(rounds):
        st = ctl.tolist()
        assert (st[0], st[1], st[3], st[4]) == (r.n_alive, r.n_step, r.step, k), (st, k)
        m = r.n_alive * r.n_step
        assert st[2] == r.xyzs.shape[0] and not r.xyzs[m:].any() and not r.deltas[m:].any()   # the alignment rows: zero
        assert np.array_equal(alive[:r.n_alive].cpu().numpy(), r.alive)
        march(ctl, alive, t)
        rows_equal(st[2], r.xyzs, r.dirs, r.deltas, (name, k))
        if perturb and k == 1:
            wrong = IM.reference_loop(name, True, jitter_every_round=True)[0][1]
            assert wrong.n_alive == r.n_alive and not np.array_equal(xyzs[:m].cpu().numpy(), wrong.xyzs[:m])
        s, col, nm = c.field(r.xyzs)
        raymarching.composite_rays_ctl(ctl, N, alive, t, T(s, cuda), T(col, cuda), T(nm, cuda), deltas, ws, dep, img, nrm,
                                       c.T_thresh)
        assert np.array_equal(alive[:r.n_alive].cpu().numpy() >= 0, r.alive_after >= 0), (name, k)
        assert np.array_equal(t.cpu().numpy(), r.t_after), (name, k)
        raymarching.compact_alive_ctl(ctl, alive, spare, N, IM.ALIGN, c.max_steps)
        alive, spare = spare, alive
        left = r.alive_after[r.alive_after >= 0]
        assert np.array_equal(alive[:left.shape[0]].cpu().numpy(), left), (name, k)
    st = ctl.tolist()
    assert (st[0], st[1], st[2], st[3], st[4]) == (0, 0, 0, final.step, len(rounds)), st
    _assert_accumulators(final, ws, dep, img, nrm)

    if perturb:   # a fresh loop's round 0 on the alive list in reverse order: noises[n] belongs to slot n
        ctl, alive = raymarching.infer_begin(N, cuda, IM.ALIGN)
        alive.copy_(torch.arange(N - 1, -1, -1, dtype=torch.int32, device=cuda))
        rev = np.arange(N - 1, -1, -1, dtype=np.int32)
        xr, dr, lr = oracle.march_rays(N, 1, rev, c.nears, c.o, c.d, c.bound, c.bits, c.C, c.H, c.nears, c.fars,
                                       align=IM.ALIGN, noises=c.noises, dt_gamma=c.dt_gamma, max_steps=c.max_steps)
        by_ray = oracle.march_rays(N, 1, rev, c.nears, c.o, c.d, c.bound, c.bits, c.C, c.H, c.nears, c.fars,
                                   align=IM.ALIGN, noises=c.noises[::-1], dt_gamma=c.dt_gamma, max_steps=c.max_steps)[0]
        assert not np.array_equal(xr, by_ray)
        march(ctl, alive, g.nears.clone())
        rows_equal(int(ctl[2]), xr, dr, lr, (name, "reversed"))


# the chunk-edge ladder of tests/test_depth_grad_gpu.py on the SDF compositor: one slab per (length, scale) pair ...
SDF_STEPS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 200, 256)
SDF_SCALES = (3.0, 60.0, 400.0, 0.0)
# ... five rays of 256 samples and one constant alpha each, chosen so that the ray stops AT this sample (the last lane of
# the first chunk, the first lane and the inside and the last lane of the second, the first lane of the third) ...
SDF_STOPS = (63, 64, 100, 127, 128)
# ... and a ray whose slab overflows M.  (T_thresh, seed): seeds chosen on the CPU so that no transmittance of the input
# lies within 3.5 % and 1.7 % of T_thresh (the placed stop at sample 128 is itself 1.8 % from 1e-2; 1 % is asserted
# below): both sides then stop every ray at the same sample
SDF_LADDER_CASES = [(1e-4, 2), (1e-2, 0)]
SDF_MARGIN = 1e-2


def sdf_ladder_case(seed, T_thresh):
    rng = np.random.default_rng(seed)
    ladder = [(k, n, sc) for k, (sc, n) in enumerate((sc, n) for sc in SDF_SCALES for n in SDF_STEPS)]
    placed = [(len(ladder) + j, 256, ("stop", s)) for j, s in enumerate(SDF_STOPS)]
    # slabs: the scale-400 block last, so that the in-bounds rows of the overflowing ray are rows past the stop sample of
    # the last ray (256 samples that stop within the first few): they keep a zero gradient only if that ray is skipped
    layout = [r for r in ladder if r[2] != 400.0] + placed + [r for r in ladder if r[2] == 400.0]
    n_rays = len(ladder) + len(placed) + 1
    M = sum(n for _, n, _ in layout)
    alpha, first, rows, off = np.zeros(M, np.float32), [], np.zeros((n_rays, 3), np.int32), 0
    for k, n, sc in layout:
        rows[k] = (k, off, n)
        if isinstance(sc, tuple):      # (1 - alpha)^(s + 1) < T_thresh < (1 - alpha)^s, T_thresh half a sample from both
            alpha[off:off + n] = 1 - T_thresh ** (1 / (sc[1] + 0.5))
        else:                          # sigma mapped to alpha as test_composite_train_forward_backward does
            alpha[off:off + n] = np.clip(rng.exponential(1.0, n) * sc * 0.01, 0, 0.95)
        if n:
            first.append(off)
        off += n
    rows[n_rays - 1] = (n_rays - 1, M - 32, 64)
    d0 = rng.uniform(0.003, 0.02, M).astype(np.float32)
    d1 = d0.copy()
    d1[first] = 0
    rgb = rng.random((M, 3)).astype(np.float32)
    rays = rows[rng.permutation(n_rays)]
    assert (rays[:, 0] != np.arange(n_rays)).any()
    g = dict(ws=rng.normal(size=n_rays).astype(np.float32), d=rng.normal(size=n_rays).astype(np.float32),
             img=rng.normal(size=(n_rays, 3)).astype(np.float32))
    return alpha, rgb, np.stack([d0, d1], 1), rays, g


def sdf_ladder_stops(alpha, rays, T_thresh):
    """From the transmittances T_i = prod_{j <= i} (1 - alpha_j) in binary64, per ray that fits: the stop sample (the
    first with T_i < T_thresh, which is still accumulated; the last sample otherwise), whether it stopped early, the rows
    up to the stop sample, and the smallest |T_i / T_thresh - 1|."""
    M = alpha.shape[0]
    stops, live, margin = {}, np.zeros(M, bool), np.inf
    for index, offset, count in rays.tolist():
        if count == 0 or offset + count > M:
            continue
        T_incl = np.cumprod(1 - alpha[offset:offset + count].astype(np.float64))
        below = np.nonzero(T_incl < T_thresh)[0]
        stop = int(below[0]) if len(below) else count - 1
        stops[index] = (stop, bool(len(below)) and stop < count - 1)
        live[offset:offset + stop + 1] = True
        margin = min(margin, float(np.abs(T_incl / T_thresh - 1).min()))
    return stops, live, margin


@pytest.mark.parametrize("T_thresh,seed", SDF_LADDER_CASES)
def test_composite_sdf_train_chunk_edges(cuda, oracle, T_thresh, seed):
    """composite_sdf_rays_train forward and backward against the oracle on ray lengths at every chunk edge of the
    wave-per-ray kernels (64 samples per trip), with stops in the first lane, the last lane and the second chunk."""
    import raymarching
    alpha, rgb, deltas, rays, g = sdf_ladder_case(seed, T_thresh)
    n_rays, M = rays.shape[0], alpha.shape[0]
    over = n_rays - 1
    stops, live, margin = sdf_ladder_stops(alpha, rays, T_thresh)
    early = sorted(s for s, e in stops.values() if e)
    print(f"T_thresh {T_thresh}: {len(early)} early-stopped rays at samples {early}, margin {margin:.3g}")
    assert margin >= SDF_MARGIN and 0 <= alpha.min() and alpha.max() <= 0.95
    base = len(SDF_STEPS) * len(SDF_SCALES)
    assert [stops[base + j] for j in range(len(SDF_STOPS))] == [(s, True) for s in SDF_STOPS]     # placed where meant
    assert any(s > 0 and s % 64 == 0 for s in early) and any(s % 64 == 63 for s in early)         # first lane, last lane
    assert any(64 <= s < 128 for s in early) and any(s < 63 for s in early)                       # second chunk, first
    assert over not in stops and not live[M - 32:].any()

    ws_r, dep_r, img_r = oracle.composite_rays_train(alpha, rgb, deltas, rays, T_thresh, sdf=True)
    s_t, c_t = T(alpha, cuda).requires_grad_(True), T(rgb, cuda).requires_grad_(True)
    ws, dep, img = raymarching.composite_sdf_rays_train(s_t, c_t, T(deltas, cuda), T(rays, cuda), T_thresh)
    np.testing.assert_allclose(ws.detach().cpu().numpy(), ws_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(img.detach().cpu().numpy(), img_r, rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(dep.detach().cpu().numpy(), dep_r, rtol=RTOL, atol=1e-5)
    assert ws_r[over] == 0 and float(ws.detach()[over]) == 0 and float(img.detach()[over].abs().max()) == 0

    torch.autograd.backward([ws, dep, img], [T(g["ws"], cuda), T(g["d"], cuda), T(g["img"], cuda)])   # g["d"]: ignored
    gs_r, gc_r = oracle.composite_rays_train_backward(g["ws"], g["img"], alpha, rgb, deltas, rays, ws_r, img_r, T_thresh,
                                                      sdf=True)
    gs, gc = s_t.grad.cpu().numpy(), c_t.grad.cpu().numpy()
    np.testing.assert_allclose(gc, gc_r, rtol=RTOL, atol=1e-6)
    scale = np.abs(gs_r).max() + 1e-12
    print(f"grad_sigmas err {np.abs(gs - gs_r).max() / scale:.3g} x scale, grad_rgbs max abs err {np.abs(gc - gc_r).max():.3g}")
    assert np.abs(gs - gs_r).max() <= 2e-4 * scale
    assert np.mean((gs_r == 0) != (gs == 0)) < 2e-3
    # rows past a ray's stop sample, and the in-bounds rows of the overflowing ray, keep exactly zero gradient
    assert (gs[~live] == 0).all() and (gc[~live] == 0).all() and (gs_r[~live] == 0).all() and (gc_r[~live] == 0).all()
    assert (gs_r[live] != 0).mean() > 0.5


COMPACT_ROUND = 1024     # rays per round of k_compact_alive_ctl's single workgroup (its `i0 += 1024`, launch_bounds 1024)


@pytest.mark.parametrize("N,case", [pytest.param(600, None, id="600"), pytest.param(2600, None, id="2600")]
                         + [pytest.param(IM.CASES[name][0], name, id=f"{IM.CASES[name][0]}-{name}") for name in IM.NAMES])
def test_compact_budget_rounds_kernels_against_oracle(cuda, oracle, N, case):
    """The four entry points of the budget loop (C ABI Part 1b, second half: mi3d_infer_begin2, mi3d_march_rays_compact_ctl,
    mi3d_composite_rays_compact_ctl, mi3d_compact_alive_ctl2) driven directly, round by round, against the CPU oracle's
    march_rays / composite_rays (raymarching.cu:906-1115 restated): the plan in the control block, the slab packing (one
    slab per ray, slabs tile [0, rows) exactly), every slab row bit-exact, the accumulators, the death rule, the
    order-preserving compaction, the restart point (t_next = the march's own t, which the reference's running sum of
    deltas[:, 1] reproduces to float rounding) and the step cap (the only coverage used to be the
    end-to-end render comparison).  N = 2600 (the budget scaled with it): the compaction's workgroup goes round three
    times, the last round ragged, and carries the count of the survivors so far from round to round.
    case: the same at the cases of infer_march_cases (cone steps, two and three cascades, bound > 1) with budget = 4 N, and
    one jittered round 0 on an alive list in another order (the renderer never runs this schedule with perturb: after a
    jittered start the two restarts differ by design, so only that round is compared)."""
    import raymarching
    rng = np.random.default_rng(31)
    if case is None:
        H, max_steps, budget, C, bound, dt_gamma = 128, 96, 2500 * N // 600, 1, 1.0, 0.0
        o, d = make_rays(rng, N)
        aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
        nears, fars = oracle.near_far_from_aabb(o, d, aabb)
        bits = sphere_bitfield(oracle, 1, H, 0.6)

        def field(x):
            s = (6 * np.exp(-np.sum(x * x, 1) / 0.08)).astype(np.float32)
            c = (0.5 + 0.5 * np.sin(x * 7)).astype(np.float32)
            nrm = (x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-6)).astype(np.float32)
            return s, c, nrm
    else:
        cs = IM.case(case)
        assert cs.N == N
        H, max_steps, budget, C, bound, dt_gamma = cs.H, cs.max_steps, 4 * N, cs.C, cs.bound, cs.dt_gamma
        o, d, nears, fars, bits, field = cs.o, cs.d, cs.nears, cs.fars, cs.bits, cs.field
    carried = False          # a compaction of more than two rounds with rays dropped in the first and kept in the third

    ws_r, dep_r = np.zeros(N, np.float32), np.zeros(N, np.float32)
    img_r, nrm_r = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    alive_r, t_r = np.arange(N, dtype=np.int32), nears.copy()
    ws, dep = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda)
    img, nrm = torch.zeros(N, 3, device=cuda), torch.zeros(N, 3, device=cuda)
    t = T(nears, cuda).clone()
    rows_cap = max(budget, N)
    xyzs, dirs = torch.zeros(rows_cap, 3, device=cuda), torch.zeros(rows_cap, 3, device=cuda)
    deltas = torch.zeros(rows_cap, 2, device=cuda)
    slab, t_next = torch.zeros(N, 2, dtype=torch.int32, device=cuda), torch.zeros(N, device=cuda)
    ctl, alive = raymarching.infer_begin2(N, cuda, budget, 1, max_steps)
    spare = torch.empty_like(alive)
    assert ctl.numel() == 16
    od, dd, bd, fd = T(o, cuda), T(d, cuda), T(bits, cuda), T(fars, cuda)
    done, rounds = 0, 0
    while True:
        st = ctl.tolist()
        n_alive, n_step = st[0], st[1]
        assert n_alive == alive_r.shape[0] and st[3] == done and st[4] == rounds and st[8] == 0
        if n_alive == 0:
            break
        assert n_step == max(1, min(budget // n_alive, max_steps, max_steps - done)), (st, done)   # the plan, capped
        raymarching.march_rays_compact_ctl(ctl, N, alive, t, od, dd, bound, bd, C, H, fd, xyzs, dirs, deltas, slab, t_next,
                                           None, dt_gamma, max_steps)
        rows = int(ctl[2])
        xr, dr, lr = oracle.march_rays(n_alive, n_step, alive_r, t_r, o, d, bound, bits, C, H, nears, fars, align=-1,
                                       dt_gamma=dt_gamma, max_steps=max_steps)
        cnt_r = (lr[:, 0].reshape(n_alive, n_step) != 0).sum(1)
        sl = slab[:n_alive].cpu().numpy()
        assert np.array_equal(sl[:, 1], cnt_r) and rows == int(cnt_r.sum())
        order = np.argsort(sl[:, 0], kind="stable")
        nz = order[sl[order, 1] > 0]
        assert np.array_equal(sl[nz, 0], np.concatenate([[0], np.cumsum(sl[nz, 1])[:-1]]))      # slabs tile [0, rows)
        xg, dg, lg = xyzs[:rows].cpu().numpy(), dirs[:rows].cpu().numpy(), deltas[:rows].cpu().numpy()
        gather = np.concatenate([np.arange(i * n_step, i * n_step + c) for i, c in enumerate(cnt_r)]).astype(np.int64) \
            if rows else np.zeros(0, np.int64)
        place = np.concatenate([np.arange(sl[i, 0], sl[i, 0] + c) for i, c in enumerate(cnt_r)]).astype(np.int64) \
            if rows else np.zeros(0, np.int64)
        assert np.array_equal(xg[place], xr[gather]) and np.array_equal(dg[place], dr[gather])   # every slab row, bit-exact
        assert np.array_equal(lg[place], lr[gather])
        s_r, c_r, n_r = field(xr)
        s_g, c_g, n_g = field(xg)
        oracle.composite_rays(n_alive, n_step, alive_r, t_r, s_r, c_r, n_r, lr, ws_r, dep_r, img_r, nrm_r, 1e-2)
        pad = lambda a, w: T(np.concatenate([a, np.zeros((rows_cap - rows,) + a.shape[1:], np.float32)]), cuda)  # noqa: E731
        raymarching.composite_rays_compact_ctl(ctl, N, alive, t, slab, t_next, pad(s_g, 1), pad(c_g, 3), pad(n_g, 3), deltas,
                                               ws, dep, img, nrm, 1e-2)
        a_g = alive[:n_alive].cpu().numpy()
        assert np.array_equal(a_g >= 0, alive_r >= 0)                                            # the death rule
        np.testing.assert_allclose(ws.cpu().numpy(), ws_r, rtol=RTOL, atol=1e-6)     # (__expf on the device, expf in the oracle)
        np.testing.assert_allclose(img.cpu().numpy(), img_r, rtol=RTOL, atol=1e-6)
        np.testing.assert_allclose(nrm.cpu().numpy(), nrm_r, rtol=RTOL, atol=1e-6)
        np.testing.assert_allclose(dep.cpu().numpy(), dep_r, rtol=RTOL, atol=1e-5)
        keep = alive_r >= 0
        # the restart: the march's own t for a survivor; the reference's running sum agrees to float rounding - each of a
        # ray's steps so far rounds at most twice (the march's t += dt, the sum's t += (t - last_t)) at the magnitude of t
        t_g = t.cpu().numpy()
        if keep.any():
            bound_t = (done + n_step) * 2.0 ** -23 * float(fars[alive_r[keep]].max())
            np.testing.assert_allclose(t_g[alive_r[keep]], t_r[alive_r[keep]], rtol=0, atol=bound_t)
        assert np.array_equal(t_g[alive_r[keep]], t_next[:n_alive].cpu().numpy()[keep])
        t_r[alive_r[keep]] = t_g[alive_r[keep]]     # (both sides start the next round from the same t)
        raymarching.compact_alive_ctl2(ctl, alive, spare, N, max_steps)
        carried |= bool(n_alive > 2 * COMPACT_ROUND and not keep[:COMPACT_ROUND].all() and keep[2 * COMPACT_ROUND:].any())
        alive, spare = spare, alive
        alive_r = alive_r[keep]
        done += n_step
        rounds += 1
        if done >= max_steps:
            alive_r = alive_r[:0]
        assert np.array_equal(alive[:alive_r.shape[0]].cpu().numpy(), alive_r)                   # compaction keeps the order
    assert rounds >= 3 and done <= max_steps + 0 or alive_r.shape[0] == 0
    assert float(ws_r.max()) > 0.5
    assert carried == (N > 2 * COMPACT_ROUND)

    # a sample buffer smaller than the round needs: the rows are COUNTED in ctl[8], not dropped silently
    ctl, alive = raymarching.infer_begin2(N, cuda, budget, 1, max_steps)
    small = 64
    raymarching.march_rays_compact_ctl(ctl, N, alive, T(nears, cuda).clone(), od, dd, bound, bd, C, H, fd, xyzs[:small],
                                       dirs[:small], deltas[:small], slab, t_next, None, dt_gamma, max_steps)
    st = ctl.tolist()
    assert st[8] > 0 and st[8] + int(slab[:, 1].sum()) == st[2]

    if case is None:
        return
    # round 0 with a jitter, on the alive list in reverse order: noises[n] belongs to alive SLOT n, whichever ray sits there
    ctl, alive = raymarching.infer_begin2(N, cuda, budget, 1, max_steps)
    alive.copy_(torch.arange(N - 1, -1, -1, dtype=torch.int32, device=cuda))
    alive_r = np.arange(N - 1, -1, -1, dtype=np.int32)
    n_step = int(ctl[1])
    assert n_step == 4 and int(ctl[4]) == 0
    raymarching.march_rays_compact_ctl(ctl, N, alive, T(nears, cuda).clone(), od, dd, bound, bd, C, H, fd, xyzs, dirs, deltas,
                                       slab, t_next, T(cs.noises, cuda), dt_gamma, max_steps)
    xr, dr, lr = oracle.march_rays(N, n_step, alive_r, nears, o, d, bound, bits, C, H, nears, fars, align=-1,
                                   noises=cs.noises, dt_gamma=dt_gamma, max_steps=max_steps)
    x0, _, l0 = oracle.march_rays(N, n_step, alive_r, nears, o, d, bound, bits, C, H, nears, fars, align=-1,
                                  dt_gamma=dt_gamma, max_steps=max_steps)
    assert not np.array_equal(xr, x0)                                                        # the jitter moves the rows
    cnt_r = (lr[:, 0].reshape(N, n_step) != 0).sum(1)
    sl, rows = slab[:N].cpu().numpy(), int(ctl[2])
    assert np.array_equal(sl[:, 1], cnt_r) and rows == int(cnt_r.sum()) > 0 and int(ctl[8]) == 0
    gather = np.concatenate([np.arange(i * n_step, i * n_step + c) for i, c in enumerate(cnt_r)]).astype(np.int64)
    place = np.concatenate([np.arange(sl[i, 0], sl[i, 0] + c) for i, c in enumerate(cnt_r)]).astype(np.int64)
    assert np.array_equal(np.sort(place), np.arange(rows))
    assert np.array_equal(xyzs[:rows].cpu().numpy()[place], xr[gather])
    assert np.array_equal(dirs[:rows].cpu().numpy()[place], dr[gather])
    assert np.array_equal(deltas[:rows].cpu().numpy()[place], lr[gather])


def test_rejects_bad_inputs(cuda):
    import raymarching
    from mi3d._lib import Mi3dError
    with pytest.raises(Mi3dError):
        raymarching.composite_rays_train(torch.ones(4, device=cuda), torch.ones(5, 3, device=cuda),
                                         torch.ones(4, 2, device=cuda), torch.zeros(1, 3, dtype=torch.int32,
                                                                                   device=cuda))
    with pytest.raises(Mi3dError):
        raymarching.march_rays_train(torch.zeros(4, 3, device=cuda), torch.ones(4, 3, device=cuda), 1.0,
                                     torch.zeros(16, dtype=torch.uint8, device=cuda), 1, 128,
                                     torch.zeros(4, device=cuda), torch.ones(4, device=cuda))
