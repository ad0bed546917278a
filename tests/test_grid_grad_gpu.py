"""GPU: the hash grid's input gradient (k_grid_backward_input behind mi3d_hashgrid_backward_input and
mi3d_grid_points_backward_input) against the binary64 model of tests/grid_grad_model.py, its autograd surface
(tinycudann.Encoding, grid_ops.encode_points), NeRFNetwork.density_gradient against the chained model, and
export_mesh(normals=True).

THE BOUND.  |gpu - model| <= k 2^-24 B elementwise, B the model's rounding magnitude.  k counts the roundings on the path of
one term of the kernel's sum (csrc/hashgrid.hip, comment above k_grid_backward_input): the two (1 - f) (2), their product
(1), the corner difference (1), weight x difference (1), the three additions of the four (j, k) terms (3), x scale (1),
x dout (1), the two features added (1) = 11; ceil(n_levels / 4) additions into the wave's register sum (mode 0: one point
per level), 3 additions across the four waves: 14 + ceil(n_levels / 4).  Fused multiply-adds only remove roundings.  That
is below the 2 n_levels + 12 the mapping was specified with for every n_levels >= 2 (and at n_levels = 1 three waves add
exact zeros), so mode 0 asserts with k = 2 n_levels + 12; the slack covers the second-order terms of (1 + u)^k.  Mode 1
adds the factor 1 / (2 bound) (1) and sums P points per level in the wave: k1 = 15 + P ceil(n_levels / 4), asserted as
gamma_k1 = k1 u / (1 - k1 u), against the model's B / (2 bound) summed over the points that pass the clamp.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import grid_grad_model as M

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INVALID = 1          # hipErrorInvalidValue
N_MAX = 4099


def _grid(levels):
    c = levels.cfg
    return (c["n_levels"], c["base_resolution"], c["per_level_scale"], c["log2_hashmap_size"])


def c_backward_input(x, dout, table, levels):
    from mi3d import _lib as L
    g = torch.full((x.shape[0], 3), float("nan"), device=x.device)
    L.launch("mi3d_hashgrid_backward_input", x, L.ptr(x), x.shape[0], L.ptr(dout), L.ptr(table), *_grid(levels), L.ptr(g))
    return g


def c_points_backward_input(x, x2, offs, P0, bound, dout, table, levels, g2=None):
    from mi3d import _lib as L
    offs = np.ascontiguousarray(offs, np.float32).reshape(-1, 3)
    g = torch.full((x.shape[0], 3), float("nan"), device=x.device)
    if g2 is None and x2 is not None:
        g2 = torch.full((x.shape[0], 3), float("nan"), device=x.device)
    L.launch("mi3d_grid_points_backward_input", x, L.ptr(x), L.ptr(x2), x.shape[0], offs.ctypes.data_as(C.c_void_p), int(P0),
             offs.shape[0], float(bound), L.ptr(dout), L.ptr(table), *_grid(levels), L.ptr(g), L.ptr(g2))
    return g, g2


# ------------------------------------------------------------------------------------------------ C ABI, mode 0

@pytest.fixture(scope="module")
def mode0(cuda):
    """name -> (levels, x, dout, table on the GPU, model gradient, B), made once at N_MAX; a case of n rows is a prefix."""
    cache = {}

    def get(name):
        if name not in cache:
            levels = M.Levels(**M.CONFIGS[name])
            x = M.points01(levels, N_MAX, seed=21)
            table = M.table_uniform(levels, seed=22)
            dout = torch.randn(N_MAX, levels.n_levels * 2, generator=torch.Generator().manual_seed(23))
            g, B = M.grad_q(x, dout, table, levels)
            cache[name] = (levels, x.to(cuda), dout.to(cuda), table.to(cuda), g, B)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(M.CONFIGS))
@pytest.mark.parametrize("n", [1, 63, 64, N_MAX])
def test_c_abi_mode0_against_the_model(cuda, mode0, name, n):
    levels, x, dout, table, g, B = mode0(name)
    x, dout = x[:n].contiguous(), dout[:n].contiguous()
    got = c_backward_input(x, dout, table, levels)
    again = c_backward_input(x, dout, table, levels)
    err = (got.cpu().double() - g[:n]).abs()
    k = 2 * levels.n_levels + 12
    print(f"[grid-grad] mode 0 {name} n={n}: worst |gpu - model| / (2^-24 B) = {float((err / (U * B[:n])).max()):.2f} (k = {k})")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= k * U * B[:n]).all())
    assert torch.equal(got, again)                         # plain stores, one order of additions: the same bits


def test_c_abi_mode0_empty_and_bad_arguments(cuda, mode0):
    from mi3d import _lib as L
    levels, x, dout, table, _, _ = mode0("small_hash")
    fn = L.lib().mi3d_hashgrid_backward_input
    g = torch.full((64, 3), 7.0, device=cuda)
    st = L.stream(x)
    ok = (L.ptr(x), 64, L.ptr(dout), L.ptr(table), *_grid(levels), L.ptr(g), st)
    assert fn(L.ptr(x), 0, L.ptr(dout), L.ptr(table), *_grid(levels), L.ptr(g), st) == 0          # n == 0: nothing, success
    assert fn(None, 0, None, None, *_grid(levels), None, st) == 0
    for i in (0, 2, 3, 8):                                                                       # a null pointer
        bad = list(ok)
        bad[i] = None
        assert fn(*bad) == INVALID
    bad = list(ok)
    bad[4] = 17                                                                                   # n_levels > MI3D_MAX_LEVELS
    assert fn(*bad) == INVALID
    bad[4] = 0
    assert fn(*bad) == INVALID
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())                                                                 # nothing was launched


# ------------------------------------------------------------------------------------------------ C ABI, mode 1

def _stencil_inputs(levels, offs, P0, bound, n, seed):
    """n samples (x, x2) in and around the box whose every stencil point passes the face filter; the first candidates sit
    exactly on +bound, on -bound, outside the box in one coordinate and on a corner of the box (12 candidates each, random
    in the other coordinates or in x2).  Returns x, x2 and how many of each survived."""
    g = torch.Generator().manual_seed(seed)
    m = 8 * n
    b = float(np.float32(bound))
    x = (torch.rand(m, 3, generator=g) * 2 - 1) * (1.1 * b)
    x[0:12, 0], x[12:24, 1], x[24:36, 2] = b, -b, 1.3 * b
    x[36:48] = torch.tensor([b, -b, b])
    x2 = x + 0.01 * torch.randn(m, 3, generator=g)
    ok = M.keep_points(x, offs[:P0], bound, levels)
    if P0 < len(offs):
        ok &= M.keep_points(x2, offs[P0:], bound, levels)
    idx = torch.nonzero(ok)[:n, 0]
    assert idx.numel() == n, "the face filter left too few samples"
    census = [int(((idx >= lo) & (idx < lo + 12)).sum()) for lo in (0, 12, 24, 36)]
    return x[idx].contiguous(), x2[idx].contiguous(), census


@pytest.mark.parametrize("bound", [1.0, 1.5])
@pytest.mark.parametrize("second", [False, True])
def test_c_abi_mode1_against_the_model(cuda, bound, second):
    """The 7-point stencil around x and the 13-point stencil around x and x2 (grid_ops.stencil_offsets); 2 bound a power of
    two (the reciprocal) and not (the division); samples on +-bound and outside the box."""
    from mi3d import grid_ops
    levels = M.Levels(**M.CONFIGS["default16"])
    offs, P0 = grid_ops.stencil_offsets(center=True, second=second)
    P, n = offs.shape[0], 193
    assert (P, P0) == ((13, 7) if second else (7, 7)) and M.pow2b(bound) == (bound == 1.0)
    x, x2, census = _stencil_inputs(levels, offs, P0, bound, n, seed=31)
    print(f"[grid-grad] mode 1 bound={bound} P={P}: samples on +bound / -bound / outside / corner = {census}")
    assert min(census[:3]) >= 1
    table = M.table_uniform(levels, seed=32)
    dout = torch.randn(P * n, levels.n_levels * 2, generator=torch.Generator().manual_seed(33))
    gx, gx2, Bx, Bx2 = M.points_grad(x, x2 if second else None, offs, P0, bound, dout, table, levels)
    dx, dx2, dd, dt = x.to(cuda), (x2.to(cuda) if second else None), dout.to(cuda), table.to(cuda)
    sentinel = torch.full((n, 3), 7.0, device=cuda)
    got, got2 = c_points_backward_input(dx, dx2, offs, P0, bound, dd, dt, levels, g2=None if second else sentinel)
    again, again2 = c_points_backward_input(dx, dx2, offs, P0, bound, dd, dt, levels, g2=None if second else sentinel)
    k1 = 15 + P * -(-levels.n_levels // 4)
    gamma = k1 * U / (1 - k1 * U)
    pairs = [(got, gx, Bx)] + ([(got2, gx2, Bx2)] if second else [])
    for which, (a, ref, B) in enumerate(pairs):
        err = (a.cpu().double() - ref).abs()
        ratio = torch.where(B > 0, err / (U * B), err)
        print(f"[grid-grad] mode 1 bound={bound} P={P} base {which}: worst |gpu - model| / (2^-24 B) = {float(ratio.max()):.2f}"
              f" (k1 = {k1})")
        assert bool(torch.isfinite(a).all()) and bool((err <= gamma * B).all())     # (B == 0: nothing passed, exactly 0)
    assert torch.equal(got, again) and (not second or torch.equal(got2, again2))
    if not second:
        assert bool((sentinel == 7.0).all())                                        # x2 NULL: grad_x2 is untouched memory
    # the clamp rule is the inclusive one: on the bound the strict rule drops the centre point's share, far outside the bound
    strict, _, _, _ = M.points_grad(x, x2 if second else None, offs, P0, bound, dout, table, levels, inclusive=False)
    on = (x.abs() == float(np.float32(bound)))
    assert bool(on.any())
    differs = (strict - gx).abs() > 2 * gamma * Bx      # (twice the bound: a result within it of one is outside it of the other)
    assert bool(differs[on].any())                        # the case tells the rules apart ...
    assert not bool(((got.cpu().double() - strict).abs() <= gamma * Bx)[differs].any())   # ... and the kernel is not the strict one


def test_c_abi_mode1_bad_arguments(cuda):
    from mi3d import _lib as L
    from mi3d import grid_ops
    levels = M.Levels(**M.CONFIGS["small_hash"])
    offs, P0 = grid_ops.stencil_offsets(center=True, second=True)
    big = np.zeros((17, 3), np.float32)
    n = 64
    x = torch.rand(n, 3, device=cuda)
    x2 = torch.rand(n, 3, device=cuda)
    dout = torch.randn(17 * n, levels.n_levels * 2, device=cuda)
    table = M.table_uniform(levels, seed=4).to(cuda)
    g, g2 = torch.full((n, 3), 7.0, device=cuda), torch.full((n, 3), 7.0, device=cuda)
    fn, st = L.lib().mi3d_grid_points_backward_input, L.stream(x)
    op = offs.ctypes.data_as(C.c_void_p)

    def args(**kw):
        a = dict(x=L.ptr(x), x2=L.ptr(x2), n=n, offs=op, P0=int(P0), P=13, bound=1.0, dout=L.ptr(dout), table=L.ptr(table),
                 grid=_grid(levels), g=L.ptr(g), g2=L.ptr(g2))
        a.update(kw)
        return (a["x"], a["x2"], a["n"], a["offs"], a["P0"], a["P"], a["bound"], a["dout"], a["table"], *a["grid"], a["g"],
                a["g2"], st)
    assert fn(*args(n=0)) == 0
    for kw in (dict(x=None), dict(offs=None), dict(dout=None), dict(table=None), dict(g=None), dict(g2=None),
               dict(x2=None), dict(P=17, offs=big.ctypes.data_as(C.c_void_p)), dict(P=0), dict(P0=14),
               dict(grid=(17,) + _grid(levels)[1:])):
        assert fn(*args(**kw)) == INVALID, kw
    torch.cuda.synchronize()
    assert bool((g == 7.0).all()) and bool((g2 == 7.0).all())                       # nothing was launched


# ------------------------------------------------------------------------------------------------ autograd

def _encoding(cuda, name, table):
    import tinycudann as tcnn
    c = M.CONFIGS[name]
    enc = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": c["n_levels"], "n_features_per_level": 2,
                            "log2_hashmap_size": c["log2_hashmap_size"], "base_resolution": c["base_resolution"],
                            "per_level_scale": c["per_level_scale"]}, dtype=torch.float32).to(cuda)
    with torch.no_grad():
        enc.params.copy_(table)
    return enc


# (the parameter scatter adds with float atomics: its sum is the same bits from run to run only where one wave owns an
#  address - 64 samples are ONE workgroup, whose wave w walks levels w, w + 4, ...)
N_SCATTER = 64


@pytest.mark.parametrize("name", ["default16", "small_hash"])
def test_encoding_differentiates_x(cuda, mode0, name):
    levels, x, dout, table, _, _ = mode0(name)
    enc = _encoding(cuda, name, table)
    xg = x.clone().requires_grad_()
    enc(xg).backward(dout)
    assert xg.grad is not None                             # (None on the parent: the positions were silently ignored)
    assert torch.equal(xg.grad, c_backward_input(x, dout, table, levels))
    # the parameter gradient is what it is without the input gradient
    grads = []
    for wants in (True, False):
        enc.params.grad = None
        xs = x[:N_SCATTER].clone().requires_grad_(wants)
        enc(xs).backward(dout[:N_SCATTER])
        grads.append(enc.params.grad.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().sum()) > 0
    # frozen table: no scatter, no params.grad
    enc.params.grad = None
    enc.params.requires_grad_(False)
    xg = x.clone().requires_grad_()
    enc(xg).backward(dout)
    assert enc.params.grad is None and torch.equal(xg.grad, c_backward_input(x, dout, table, levels))
    enc.params.requires_grad_(True)
    # first order only: a second derivative raises torch's error, it is not a silent zero
    xg = x[:64].clone().requires_grad_()
    (g1,) = torch.autograd.grad(enc(xg), xg, dout[:64], create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g1.sum(), xg)


def test_encode_points_differentiates_x_and_x2(cuda):
    from mi3d import _lib as L
    from mi3d import grid_ops
    levels = M.Levels(**M.CONFIGS["default16"])
    offs, P0 = grid_ops.stencil_offsets(center=True, second=True)
    n, bound, cfg = 1000, 1.0, levels.cfg
    g = torch.Generator().manual_seed(41)
    x = ((torch.rand(n, 3, generator=g) * 2 - 1) * 1.05).to(cuda)
    x2 = (x + 0.01 * torch.randn(n, 3, generator=g).to(cuda)).contiguous()
    table = M.table_uniform(levels, seed=42).to(cuda)
    dout = torch.randn(13 * n, levels.n_levels * 2, generator=g).to(cuda)
    want, want2 = c_points_backward_input(x, x2, offs, P0, bound, dout, table, levels)

    params = table.clone().requires_grad_()
    xg, x2g = x.clone().requires_grad_(), x2.clone().requires_grad_()
    grid_ops.encode_points(params, xg, offs, cfg, bound, x2g, P0).backward(dout)
    assert torch.equal(xg.grad, want) and torch.equal(x2g.grad, want2) and params.grad is not None
    # x2 alone
    xg, x2g = x.clone(), x2.clone().requires_grad_()
    grid_ops.encode_points(table, xg, offs, cfg, bound, x2g, P0).backward(dout)
    assert torch.equal(x2g.grad, want2) and xg.grad is None and table.grad is None      # (a frozen table: no scatter)
    # the parameter gradient with and without the input gradient (N_SCATTER samples: see above), and a frozen table
    grads = []
    for wants in (True, False):
        params = table.clone().requires_grad_()
        xs = x[:N_SCATTER].clone().requires_grad_(wants)
        d = dout.view(13, n, -1)[:, :N_SCATTER].reshape(13 * N_SCATTER, -1).contiguous()
        grid_ops.encode_points(params, xs, offs, cfg, bound, x2[:N_SCATTER].contiguous(), P0).backward(d)
        grads.append(params.grad.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().sum()) > 0
    # first order only
    xg = x[:64].clone().requires_grad_()
    y = grid_ops.encode_points(table, xg, offs[:7], cfg, bound)
    (g1,) = torch.autograd.grad(y, xg, torch.ones_like(y), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g1.sum(), xg)
    # the counted rows belong to the inference loop
    count = torch.tensor([10], dtype=torch.int32, device=cuda)
    with pytest.raises(L.Mi3dError, match="count"):
        grid_ops.encode_points(table, x.clone().requires_grad_(), offs[:7], cfg, bound, count=count)
    assert grid_ops.encode_points(table, x, offs[:7], cfg, bound, count=count).shape == (7 * n, 32)


# ------------------------------------------------------------------------------------------------ density_gradient

def _chain(x32, q32, table, levels, W, b, bound, blob_density, blob_radius, dtype):
    """sigma and d sigma / dx of common_forward's chain in `dtype` on the CPU, by torch autograd: encode (the model's
    forward, cell and fraction the kernel's) -> Linear / ReLU -> exp(h0 + blob).  Also every hidden pre-activation and the
    magnitude |row of W| . |input| + |b| it is rounded against."""
    x = x32.to(dtype).requires_grad_()
    q = (x + bound) / (2 * bound)
    h = M.forward(q32, table, levels, dtype, dq=q - q.detach())
    pre = []
    for l, (Wl, bl) in enumerate(zip(W, b)):
        Wl, bl = Wl.to(dtype), bl.to(dtype)
        z = h @ Wl.T + bl
        if l < len(W) - 1:
            pre.append((z.detach(), h.detach().abs() @ Wl.abs().T + bl.abs()))
            h = torch.relu(z)
    z0 = z[:, 0] + blob_density * torch.exp(-(x ** 2).sum(-1) / (2 * blob_radius ** 2))
    sigma = torch.exp(z0)
    (g,) = torch.autograd.grad(sigma.sum(), x)
    return sigma.detach(), g, pre, float(z0.detach().max())


@pytest.fixture(scope="module")
def field(cuda):
    from mi3d import network, sds_step
    torch.manual_seed(0)
    model = network.NeRFNetwork(sds_step.make_opt(fp16=False)).to(cuda)
    levels = M.Levels(**M.CONFIGS["default16"])
    assert model.encoder.cfg == levels.cfg and float(model.bound) == 1.0
    table = M.table_uniform(levels, seed=51, scale=0.1)
    with torch.no_grad():
        model.encoder.params.copy_(table)
    g = torch.Generator().manual_seed(52)
    cand = torch.rand(3 * N_MAX, 3, generator=g) * 2 - 1
    q32 = M.point_q(cand, torch.zeros(3), 1.0)[0]
    ok = M.keep(q32, levels)
    x, q32 = cand[ok][:N_MAX].contiguous(), q32[ok][:N_MAX].contiguous()
    assert x.shape[0] == N_MAX
    return model, levels, table, x, q32


def test_density_gradient_against_the_chained_model(cuda, field):
    """|gpu - A| <= 4 max |B - A|: A the chain in binary64, B the same chain in binary32, both on the CPU; the 4 covers the
    matrix-core kernels' accumulation order.  Samples where a hidden pre-activation of A lies within 1e-5 of its rounding
    magnitude of zero are left out (a ReLU may flip between precisions): at most 2 % of them."""
    model, levels, table, x, q32 = field
    W = [l.weight.detach().cpu() for l in model.sigma_net.net]
    b = [l.bias.detach().cpu() for l in model.sigma_net.net]
    args = (x, q32, table, levels, W, b, 1.0, float(model.opt.blob_density), float(model.opt.blob_radius))
    sA, gA, pre, z_max = _chain(*args, torch.float64)
    sB, gB, _, _ = _chain(*args, torch.float32)
    assert z_max < 15                                      # trunc_exp's clamped derivative is exp's own here
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    for z, mag in pre:
        near |= (z.abs() <= 1e-5 * mag).any(-1)
    share = float(near.float().mean())
    print(f"[grid-grad] density_gradient: {int(near.sum())} of {x.shape[0]} samples near a ReLU kink ({100 * share:.2f} %)")
    assert share <= 0.02
    use = ~near
    sigma, grad = model.density_gradient(x.to(cuda))
    assert sigma.shape == (N_MAX,) and grad.shape == (N_MAX, 3) and sigma.dtype == grad.dtype == torch.float32
    tol_g = 4 * float((gB.double() - gA)[use].abs().max())
    tol_s = 4 * float((sB.double() - sA)[use].abs().max())
    err_g = float((grad.cpu().double() - gA)[use].abs().max())
    err_s = float((sigma.cpu().double() - sA)[use].abs().max())
    print(f"[grid-grad] density_gradient: |gpu - A| grad {err_g:.3e} (bound {tol_g:.3e}, max |A| {float(gA.abs().max()):.3e}),"
          f" sigma {err_s:.3e} (bound {tol_s:.3e})")
    assert err_g <= tol_g and err_s <= tol_s
    assert all(p.grad is None for p in model.parameters())
    # under no_grad and under autocast: the same bits
    with torch.no_grad():
        s1, g1 = model.density_gradient(x.to(cuda))
    with torch.autocast("cuda", torch.float16):
        s2, g2 = model.density_gradient(x.to(cuda))
    assert torch.equal(s1, sigma) and torch.equal(g1, grad) and torch.equal(s2, sigma) and torch.equal(g2, grad)
    assert all(p.grad is None for p in model.parameters())
    # analytic_normal: the sign and the clean-up of normal()
    from mi3d.renderer import safe_normalize
    assert torch.equal(model.analytic_normal(x.to(cuda)), torch.nan_to_num(safe_normalize(-grad)))


# ------------------------------------------------------------------------------------------------ export_mesh

@pytest.fixture(scope="module")
def blob(cuda, tmp_path_factory):
    """The `model` fixture's recipe of tests/test_mesh_gpu.py (the field of smoke(): make_opt, build_training_state) with
    the table left at its initial U(-1e-4, 1e-4) instead of redrawn in +-0.3: the BLOB field, radially symmetric up to
    1e-4-sized features - the redrawn table is noise no normal points outwards of, and its median surface has 6e5
    triangles whose OBJ files take seconds to write.  sigma = exp(h + 5 exp(-r^2 / 0.02)) with h within ~1e-3 of a constant
    and |grad h| well below 1 (finest scale 2047 x table differences 2e-4 x the MLP's gain), against the blob's radial slope
    5 exp(-r^2 / 0.02) r / 0.01 = 24 at r = 0.15, where the surface is cut.  Exported once with normals, at 64^3."""
    from mi3d import sds_step
    torch.manual_seed(0)
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    model, _, _ = sds_step.build_training_state(opt, cuda, bitfield=0.5)
    with torch.no_grad():
        thresh = float(model.density(torch.tensor([[0.15, 0.0, 0.0]], device=cuda))["sigma"][0])
    model.mean_density = model.density_thresh = thresh
    out = tmp_path_factory.mktemp("blob")
    v, f, c, n = model.export_mesh(str(out / "n"), resolution=64, normals=True)
    print(f"[grid-grad] blob mesh at sigma = {thresh:.4g}: nv {len(v)} nt {len(f)}")
    return model, out, v, f, c, n


def _obj(path):
    out = {"v": [], "vt": [], "vn": [], "f": []}
    for line in open(path):
        tok = line.split()
        if tok and tok[0] in out:
            out[tok[0]].append(tok[1:])
    return out


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_export_mesh_writes_the_normals_it_returns(cuda, blob):
    model, out, v, f, c, n = blob
    assert n.dtype == np.float32 and n.shape == v.shape and len(v) > 100 and len(f) > 100
    p = _obj(out / "n" / "mesh.obj")
    assert len(p["vn"]) == len(v) and np.array_equal(np.array(p["vn"], np.float64).astype(np.float32), n)
    assert np.array_equal(np.array([t[:3] for t in p["v"]], np.float64).astype(np.float32), v)
    idx = np.array([[t.split("//") for t in face] for face in p["f"]], np.int64)
    assert np.array_equal(idx[..., 0] - 1, f) and np.array_equal(idx[..., 1], idx[..., 0])
    with torch.no_grad():
        assert np.array_equal(model.analytic_normal(torch.from_numpy(v).to(cuda)).cpu().numpy(), n)
    # unit length (binary32: the sum of squares, the root and the division leave a few 2^-24) or exactly zero
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert bool(np.all((np.abs(length - 1) <= 1e-6) | (length == 0)))
    # the blob is radially symmetric: every normal -grad sigma / |grad sigma| points away from the centre
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    dots = (n.astype(np.float64) * v / r[:, None]).sum(1)
    print(f"[grid-grad] blob mesh: radius in [{r.min():.4f}, {r.max():.4f}], normal . v/|v| in [{dots.min():.4f}, {dots.max():.4f}]")
    assert r.min() > 0.1 and r.max() < 0.2
    assert bool((dots > 0).all())


def test_export_mesh_without_normals_is_what_it_was(cuda, blob):
    model, out, v, f, c, _ = blob
    plain = model.export_mesh(str(out / "a"), resolution=64)
    off = model.export_mesh(str(out / "b"), resolution=64, normals=False)
    assert len(plain) == len(off) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, off))
    assert _files(out / "a") == _files(out / "b") and sorted(_files(out / "a")) == ["mesh.mtl", "mesh.obj"]
    obj = _files(out / "a")["mesh.obj"]
    assert b"vn " not in obj and b"//" not in obj
    assert plain[0].tobytes() == v.tobytes() and plain[1].tobytes() == f.tobytes() and plain[2].tobytes() == c.tobytes()


def test_export_mesh_textured_with_normals(cuda, blob):
    model, out, v, f, c, n = blob
    res = model.export_mesh(str(out / "t"), resolution=64, texture_size=256, normals=True)
    assert len(res) == 6 and res[5].tobytes() == n.tobytes() and res[0].tobytes() == v.tobytes()
    p = _obj(out / "t" / "mesh.obj")
    idx = np.array([[t.split("/") for t in face] for face in p["f"]], np.int64)                 # a/ta/a b/tb/b c/tc/c
    assert idx.shape == (len(f), 3, 3) and np.array_equal(idx[..., 0] - 1, f) and np.array_equal(idx[..., 2], idx[..., 0])
    assert np.array_equal(idx[..., 1] - 1, np.arange(3 * len(f)).reshape(-1, 3))
    assert len(p["vn"]) == len(v) and len(p["vt"]) == 3 * len(f)
    assert np.array_equal(np.array(p["vn"], np.float64).astype(np.float32), n)
    plain = model.export_mesh(str(out / "u"), resolution=64, texture_size=256)
    off = model.export_mesh(str(out / "w"), resolution=64, texture_size=256, normals=False)
    assert len(plain) == len(off) == 5 and _files(out / "u") == _files(out / "w")
    assert b"vn " not in _files(out / "u")["mesh.obj"]
