"""GPU: the hash grid's second-order pass (k_grid_backward_input_backward_rows and k_grid_backward_input_backward_table behind
mi3d_hashgrid_backward_input_backward and mi3d_grid_points_backward_input_backward) against the binary64 model of
tests/grid_grad2_model.py, and its autograd surface (tinycudann.Encoding(second_order=True),
grid_ops.encode_points(second_order=True)).

THE BOUND.  |gpu - model| <= k 2^-24 B elementwise, B the model's rounding magnitude of that output.  k counts the roundings
on the path of one term, from the comments above the two kernels in csrc/hashgrid.hip (a fused multiply-add only removes
one), with C = ceil(n_levels / 4):

  grad_dout    the first-order sum T - two (1 - f) (2), their product (1), the corner difference (1), weight x difference
               (1), three additions of the four (j, k) terms (3): 8 - rho = r x scale (1), rho x T (1), two additions of the
               three dimensions (2): 12.  Mode 1: rho is r x 1 / (2 bound) first (1): 13.
  grad_x       the mixed derivative M - (1 - f) (1), the corner difference (1), the difference of two differences (1),
               weight x that (1), the two terms added (1): 5 - rho (1), rho x M (1), the two other dimensions added (1),
               x dout (1), the two features added (1), x scale (1): 11; C additions into the wave's sum (mode 0: one point
               per level) and 3 across the waves: 14 + C.  Mode 1: rho (2) and x 1 / (2 bound) at the end (1): 13; P C
               additions in the wave, 3 across: 16 + P C.
  grad_params  one contribution: (1 - f) (1), the product of the two weights (1), rho (1), rho x weights (1), two additions
               of the three terms (2), x dout (1): 7, mode 1: 8; the atomic additions of an entry's N_e contributions come in
               any order, at most N_e of them on one path: 7 + N_e, mode 1: 8 + N_e, N_e the model's count per entry.
  first-order scatter (for the sum of the two parameter gradients): (1 - f) (1), the two products of the weight (2), x dout
               (1): 4, + N_e additions in the run sums and the atomics.

Every assertion uses k + 1: the one more covers the second-order terms of (1 + u)^k - 1 = k u + k^2 u^2 / 2 + ..., below u
for every k < 5000, and N_e stays below 600 here.  Where two gradients are added into params.grad that addition is one more
rounding of either.  The derived k are not tuned: a printed worst ratio above k means the kernel or the count is wrong.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import grid_grad2_model as M2
import grid_grad_model as M

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INVALID = 1          # hipErrorInvalidValue
N_MAX = 4099
SENTINEL = 7.0


def _grid(levels):
    c = levels.cfg
    return (c["n_levels"], c["base_resolution"], c["per_level_scale"], c["log2_hashmap_size"])


def k_dout(mode):
    return 12 + mode


def k_x(levels, mode, P=1):
    c = -(-levels.n_levels // 4)
    return 14 + c if mode == 0 else 16 + P * c


def k_table(mode, N):
    return (7 + mode) + N.double()


def check(name, got, ref, B, k):
    """|got - ref| <= (k + 1) 2^-24 B elementwise (k a number or a tensor that broadcasts); prints the worst ratio."""
    got = got.detach().cpu().double().reshape(ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(B > 0, err / (U * B), err)
    kk = k if isinstance(k, torch.Tensor) else torch.tensor(float(k), dtype=torch.float64)
    kk = kk.expand_as(ratio) if kk.dim() == ratio.dim() or kk.dim() == 0 else kk[:, None].expand_as(ratio)
    i = int(torch.argmax(ratio / kk))
    print(f"[grid-grad2] {name}: worst |gpu - model| / (2^-24 B) = {float(ratio.reshape(-1)[i]):.2f} (k = {float(kk.reshape(-1)[i]):.0f})")
    assert bool(torch.isfinite(got).all()), name
    assert bool((err <= (kk + 1) * U * B).all()), name


def c_second(x, dout, r, table, levels, want=(True, True, True), x2=None, r2=None, offs=None, P0=None, bound=None):
    """The C ABI's second-order call (mode 0 without offs, mode 1 with): every wanted output in a buffer of its own,
    sentinel-filled (grad_params: zeroed), NULL for the others.  Returns grad_dout, grad_x, grad_x2, grad_params."""
    from mi3d import _lib as L
    n = x.shape[0]
    P = 1 if offs is None else np.asarray(offs).reshape(-1, 3).shape[0]
    gd = torch.full((P * n, 2 * levels.n_levels), SENTINEL, device=x.device) if want[0] else None
    gx = torch.full((n, 3), SENTINEL, device=x.device) if want[1] else None
    gx2 = torch.full((n, 3), SENTINEL, device=x.device) if want[1] and x2 is not None else None
    gp = torch.zeros(levels.n_entries * 2, device=x.device) if want[2] else None
    if offs is None:
        L.launch("mi3d_hashgrid_backward_input_backward", x, L.ptr(x), n, L.ptr(dout), L.ptr(table), L.ptr(r), *_grid(levels),
                 L.ptr(gd), L.ptr(gx), L.ptr(gp))
    else:
        offs = np.ascontiguousarray(offs, np.float32).reshape(-1, 3)
        L.launch("mi3d_grid_points_backward_input_backward", x, L.ptr(x), L.ptr(x2), n, offs.ctypes.data_as(C.c_void_p),
                 int(P0), P, float(bound), L.ptr(dout), L.ptr(table), L.ptr(r), L.ptr(r2), *_grid(levels), L.ptr(gd), L.ptr(gx),
                 L.ptr(gx2), L.ptr(gp))
    return gd, gx, gx2, gp


def check_all(tag, outs, want, levels, mode, P=1):
    gd, gx, gx2, gp = outs
    if gd is not None:
        check(f"{tag} grad_dout", gd, want["grad_dout"], want["B_dout"], k_dout(mode))
    if gx is not None:
        check(f"{tag} grad_x", gx, want["grad_x"], want["B_x"], k_x(levels, mode, P))
    if gx2 is not None:
        check(f"{tag} grad_x2", gx2, want["grad_x2"], want["B_x2"], k_x(levels, mode, P))
    if gp is not None:
        check(f"{tag} grad_params", gp, want["table"].grad, want["table"].B, k_table(mode, want["table"].N))


# ------------------------------------------------------------------------------------------------ shared cases

@pytest.fixture(scope="module")
def mode0(cuda):
    """(name, n) -> dict(levels, x, dout, r, table on the GPU, cpu = the same on the CPU, want = the model's outputs).  The
    inputs are made once per configuration at N_MAX; a case of n rows is a prefix (the table's sum depends on n, so the
    model runs per case; the N_MAX case is kept for the tests that share it)."""
    inputs, cache = {}, {}

    def get(name, n=N_MAX):
        if name not in inputs:
            levels = M.Levels(**M.CONFIGS[name])
            g = torch.Generator().manual_seed(83)
            inputs[name] = (levels, M.points01(levels, N_MAX, seed=81), torch.randn(N_MAX, levels.n_levels * 2, generator=g),
                            torch.randn(N_MAX, 3, generator=g), M.table_uniform(levels, seed=82))
        if (name, n) in cache:
            return cache[(name, n)]
        levels, x, dout, r, table = inputs[name]
        x, dout, r = x[:n].contiguous(), dout[:n].contiguous(), r[:n].contiguous()
        case = dict(levels=levels, x=x.to(cuda), dout=dout.to(cuda), r=r.to(cuda), table=table.to(cuda),
                    cpu=(x, dout, r, table), want=M2.second_order(x, dout, r, table, levels))
        if n == N_MAX:                                      # the case several tests share (the model's table sums are large)
            cache[(name, n)] = case
        return case
    return get


@pytest.fixture(scope="module")
def mode1(cuda):
    """(bound, second) -> the stencil case at n = 1000 on default16: P = 7 around x, or P = 13 around x and x2."""
    cache = {}

    def get(bound, second):
        if (bound, second) not in cache:
            from mi3d import grid_ops
            levels = M.Levels(**M.CONFIGS["default16"])
            offs, P0 = grid_ops.stencil_offsets(center=True, second=second)
            P, n = offs.shape[0], 1000
            x, x2, census = M2.stencil_inputs(levels, offs, P0, bound, n, seed=91)
            g = torch.Generator().manual_seed(93)
            table = M.table_uniform(levels, seed=92)
            dout = torch.randn(P * n, levels.n_levels * 2, generator=g)
            r, r2 = torch.randn(n, 3, generator=g), (torch.randn(n, 3, generator=g) if second else None)
            if not second:
                x2 = None
            want = M2.points_second_order(x, x2, offs, P0, bound, dout, r, r2, table, levels)
            dev = lambda t: None if t is None else t.to(cuda)      # noqa: E731
            cache[(bound, second)] = dict(levels=levels, offs=offs, P0=P0, P=P, n=n, bound=bound, census=census, want=want,
                                          x=dev(x), x2=dev(x2), dout=dev(dout), r=dev(r), r2=dev(r2), table=dev(table),
                                          cpu=(x, x2, dout, r, r2, table))
        return cache[(bound, second)]
    return get


def _second1(c, want=(True, True, True)):
    return c_second(c["x"], c["dout"], c["r"], c["table"], c["levels"], want, x2=c["x2"], r2=c["r2"], offs=c["offs"],
                    P0=c["P0"], bound=c["bound"])


# ------------------------------------------------------------------------------------------------ C ABI, mode 0

@pytest.mark.parametrize("name", list(M.CONFIGS))
@pytest.mark.parametrize("n", [1, 63, 64, N_MAX])
def test_c_abi_mode0_against_the_model(cuda, mode0, name, n):
    c = mode0(name, n)
    outs = c_second(c["x"], c["dout"], c["r"], c["table"], c["levels"])
    again = c_second(c["x"], c["dout"], c["r"], c["table"], c["levels"])
    check_all(f"mode 0 {name} n={n}", outs, c["want"], c["levels"], 0)
    assert torch.equal(outs[0], again[0]) and torch.equal(outs[1], again[1])      # the rows: the same bits
    assert float(outs[1].abs().max()) > 0 and float(outs[3].abs().max()) > 0


def test_c_abi_mode0_empty_and_bad_arguments(cuda, mode0):
    from mi3d import _lib as L
    c = mode0("small_hash", 64)
    levels, x, dout, r, table = c["levels"], c["x"], c["dout"], c["r"], c["table"]
    fn = L.lib().mi3d_hashgrid_backward_input_backward
    gd = torch.full((64, 2 * levels.n_levels), SENTINEL, device=cuda)
    gx = torch.full((64, 3), SENTINEL, device=cuda)
    gp = torch.full((levels.n_entries * 2,), SENTINEL, device=cuda)
    st = L.stream(x)
    ok = [L.ptr(x), 64, L.ptr(dout), L.ptr(table), L.ptr(r), *_grid(levels), L.ptr(gd), L.ptr(gx), L.ptr(gp), st]
    zero = list(ok)
    zero[1] = 0
    assert fn(*zero) == 0                                                          # n == 0: nothing, success
    assert fn(None, 0, None, None, None, *_grid(levels), None, None, None, st) == 0
    for i in (0, 2, 3, 4):                                                         # a null input
        bad = list(ok)
        bad[i] = None
        assert fn(*bad) == INVALID, i
    bad = list(ok)
    bad[9] = bad[10] = bad[11] = None                                              # all outputs null
    assert fn(*bad) == INVALID
    for levels_bad in (17, 0):                                                     # n_levels > MI3D_MAX_LEVELS, no level
        bad = list(ok)
        bad[5] = levels_bad
        assert fn(*bad) == INVALID
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (gd, gx, gp))                  # nothing was launched


# ------------------------------------------------------------------------------------------------ C ABI, mode 1

@pytest.mark.parametrize("bound", [1.0, 1.5])
@pytest.mark.parametrize("second", [False, True])
def test_c_abi_mode1_against_the_model(cuda, mode1, bound, second):
    """The 7-point stencil around x and the 13-point stencil around x and x2; 2 bound a power of two (the reciprocal) and
    not (the division); samples exactly on +-bound, outside the box in one coordinate and on a corner: the inclusive clamp
    rule enters twice, in rho and on grad_q's way to the base."""
    c = mode1(bound, second)
    assert (c["P"], c["P0"]) == ((13, 7) if second else (7, 7)) and M.pow2b(bound) == (bound == 1.0)
    print(f"[grid-grad2] mode 1 bound={bound} P={c['P']}: samples on +bound / -bound / outside / corner = {c['census']}")
    assert min(c["census"]) > 0
    outs, again = _second1(c), _second1(c)
    check_all(f"mode 1 bound={bound} P={c['P']}", outs, c["want"], c["levels"], 1, c["P"])
    assert torch.equal(outs[0], again[0]) and torch.equal(outs[1], again[1])
    assert (outs[2] is None) == (not second) and (not second or torch.equal(outs[2], again[2]))
    # on the bound the inclusive rule passes the centre point's share: not zero where the sample's other coordinates lie in
    # the box (a coordinate outside stops its rho, and a sample with both others outside has nothing to pass)
    x = c["cpu"][0]
    b = float(np.float32(bound))
    on = (x.abs() == b) & (x.abs() <= b).all(-1, keepdim=True)
    assert bool(on.any()) and float(c["want"]["grad_x"][on].abs().min()) > 0
    # a coordinate outside the box receives exactly nothing
    out = x[:, 2].abs() > float(np.float32(bound)) + 0.02
    assert bool(out.any()) and bool((outs[1][out.to(cuda), 2] == 0).all())


def test_c_abi_mode1_bad_arguments(cuda, mode1):
    from mi3d import _lib as L
    c = mode1(1.0, True)
    levels, n = c["levels"], c["n"]
    big = np.zeros((17, 3), np.float32)
    gd = torch.full((13 * n, 2 * levels.n_levels), SENTINEL, device=cuda)
    gx, gx2 = torch.full((n, 3), SENTINEL, device=cuda), torch.full((n, 3), SENTINEL, device=cuda)
    gp = torch.full((levels.n_entries * 2,), SENTINEL, device=cuda)
    fn, st = L.lib().mi3d_grid_points_backward_input_backward, L.stream(c["x"])
    op = c["offs"].ctypes.data_as(C.c_void_p)

    def args(**kw):
        a = dict(x=L.ptr(c["x"]), x2=L.ptr(c["x2"]), n=n, offs=op, P0=int(c["P0"]), P=13, bound=1.0, dout=L.ptr(c["dout"]),
                 table=L.ptr(c["table"]), r=L.ptr(c["r"]), r2=L.ptr(c["r2"]), grid=_grid(levels), gd=L.ptr(gd), gx=L.ptr(gx),
                 gx2=L.ptr(gx2), gp=L.ptr(gp))
        a.update(kw)
        return (a["x"], a["x2"], a["n"], a["offs"], a["P0"], a["P"], a["bound"], a["dout"], a["table"], a["r"], a["r2"],
                *a["grid"], a["gd"], a["gx"], a["gx2"], a["gp"], st)
    assert fn(*args(n=0)) == 0
    for kw in (dict(x=None), dict(offs=None), dict(dout=None), dict(table=None), dict(r=None),          # a null input
               dict(gd=None, gx=None, gx2=None, gp=None),                                               # all outputs null
               dict(r2=None), dict(gx2=None), dict(gx=None),                      # x2 without r2 / grad_x2; grad_x2 without grad_x
               dict(x2=None), dict(x2=None, P0=13, gx2=None), dict(x2=None, P0=13, r2=None),            # r2 / grad_x2 without x2
               dict(P=17, offs=big.ctypes.data_as(C.c_void_p)), dict(P=0), dict(P0=14),                 # a bad stencil
               dict(grid=(17,) + _grid(levels)[1:])):
        assert fn(*args(**kw)) == INVALID, kw
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (gd, gx, gx2, gp))                                  # nothing was launched


# ------------------------------------------------------------------------------------------------ selective outputs

WANTS = [(False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, False),
         (False, False, True)]


@pytest.mark.parametrize("mode", [0, 1])
def test_each_output_alone_and_without_each_other(cuda, mode0, mode1, mode):
    """An output that is not asked for is not computed and does not change the others: the rows keep their bits, the table
    stays within its bound, and a buffer that was not passed is untouched."""
    if mode == 0:
        c = mode0("small_hash")
        call = lambda want: c_second(c["x"], c["dout"], c["r"], c["table"], c["levels"], want)     # noqa: E731
        P = 1
    else:
        c = mode1(1.5, True)
        call = lambda want: _second1(c, want)                                                        # noqa: E731
        P = c["P"]
    full = call((True, True, True))
    spare = [torch.full_like(t, SENTINEL) for t in full if t is not None]   # buffers nobody passes, beside the live ones
    for want in WANTS:
        outs = call(want)
        assert [o is not None for o in outs] == [want[0], want[1], want[1] and mode == 1, want[2]]
        check_all(f"mode {mode} outputs {want}", outs, c["want"], c["levels"], mode, P)
        for o, f in zip(outs[:3], full[:3]):
            assert o is None or torch.equal(o, f)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in spare)
    # grad_params is ACCUMULATED: a second call adds the same again on top of what is there
    twice = full[3].clone()
    from mi3d import _lib as L
    if mode == 0:
        L.launch("mi3d_hashgrid_backward_input_backward", c["x"], L.ptr(c["x"]), c["x"].shape[0], L.ptr(c["dout"]),
                 L.ptr(c["table"]), L.ptr(c["r"]), *_grid(c["levels"]), None, None, L.ptr(twice))
        t = c["want"]["table"]
        check("mode 0 accumulated twice", twice, 2 * t.grad, 2 * t.B, k_table(0, 2 * t.N))


# ------------------------------------------------------------------------------------------------ zero rows

def test_zero_rows_add_nothing_to_the_table(cuda):
    """Rows whose dout is zero, whose r is zero, or whose dout pair is zero at some levels issue nothing: entries only they
    touch stay exactly zero, and the table is the model's (whose N counts the issued contributions alone)."""
    levels = M.Levels(**M.CONFIGS["default16"])
    n = 300
    g = torch.Generator().manual_seed(103)
    x = M.points01(levels, n, seed=101, hand=False)
    table = M.table_uniform(levels, seed=102)
    dout, r = torch.randn(n, 2 * levels.n_levels, generator=g), torch.randn(n, 3, generator=g)
    dout[0:100] = 0
    r[100:200] = 0
    dout[200:250, 10:20] = 0                                         # levels 5..9 of these rows
    want = M2.second_order(x, dout, r, table, levels)
    touched = M2.second_order(x, torch.ones_like(dout), torch.ones_like(r), table, levels)["table"].N
    only_zero = (touched > 0) & (want["table"].N == 0)
    print(f"[grid-grad2] zero rows: {int(only_zero.sum())} entries are touched by zero rows alone")
    assert int(only_zero.sum()) > 1000
    _, _, _, gp = c_second(x.to(cuda), dout.to(cuda), r.to(cuda), table.to(cuda), levels, (False, False, True))
    check("zero rows grad_params", gp, want["table"].grad, want["table"].B, k_table(0, want["table"].N))
    assert bool((gp.view(-1, 2).cpu()[only_zero] == 0).all())
    assert bool((want["table"].grad[only_zero] == 0).all())


# ------------------------------------------------------------------------------------------------ autograd, Encoding

def _encoding(cuda, name, table, **kw):
    import tinycudann as tcnn
    c = M.CONFIGS[name]
    enc = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": c["n_levels"], "n_features_per_level": 2,
                            "log2_hashmap_size": c["log2_hashmap_size"], "base_resolution": c["base_resolution"],
                            "per_level_scale": c["per_level_scale"]}, dtype=torch.float32, **kw).to(cuda)
    with torch.no_grad():
        enc.params.copy_(table)
    return enc


N_SCATTER = 64   # one workgroup: the atomic scatter gives the same bits from run to run (tests/test_grid_grad_gpu.py)


@pytest.fixture()
def profile():
    from mi3d import grid_ops
    grid_ops.PROFILE = {}
    yield grid_ops.PROFILE
    grid_ops.PROFILE = None


@pytest.mark.parametrize("name", ["default16", "small_hash"])
def test_encoding_second_order(cuda, mode0, name):
    c = mode0(name)
    levels, x, dout, r, table, want = c["levels"], c["x"], c["dout"], c["r"], c["table"], c["want"]
    off, on = _encoding(cuda, name, table), _encoding(cuda, name, table, second_order=True)
    # the first order: the same bits as with the flag off
    firsts = []
    for enc in (off, on):
        xg = x.clone().requires_grad_()
        y = enc(xg)
        y.backward(dout)
        xs = x[:N_SCATTER].clone().requires_grad_()
        enc.params.grad = None
        enc(xs).backward(dout[:N_SCATTER])
        firsts.append((y.detach(), xg.grad, enc.params.grad.clone()))
        enc.params.grad = None
    assert all(torch.equal(a, b) for a, b in zip(*firsts)) and float(firsts[0][2].abs().sum()) > 0
    # the second order: the C ABI's rows bit for bit, the table against the model
    gd_c, gx_c, _, _ = c_second(x, dout, r, table, levels, (True, True, False))
    xg, dl = x.clone().requires_grad_(), dout.clone().requires_grad_()
    (g1,) = torch.autograd.grad(on(xg), xg, dl, create_graph=True)
    assert torch.equal(g1, firsts[0][1]) and g1.requires_grad
    gd, gx, gp = torch.autograd.grad((g1 * r).sum(), [dl, xg, on.params])
    assert torch.equal(gd, gd_c) and torch.equal(gx, gx_c)
    check(f"Encoding {name} grad_params", gp, want["table"].grad, want["table"].B, k_table(0, want["table"].N))
    # with the flag off the same request raises torch's error
    xg = x[:64].clone().requires_grad_()
    (g1,) = torch.autograd.grad(off(xg), xg, dout[:64], create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g1.sum(), xg)


def test_encoding_first_and_second_order_meet_in_params_grad(cuda, mode0):
    """L = <y, a> + <g1, r>: params.grad is the first-order scatter of a plus the second-order table term; both bounds are
    added, each with the one more rounding of the addition that joins them."""
    c = mode0("small_hash")
    levels, x, dout, r, table, want = c["levels"], c["x"], c["dout"], c["r"], c["table"], c["want"]
    a_cpu = torch.randn(N_MAX, 2 * levels.n_levels, generator=torch.Generator().manual_seed(111))
    first = M2.first_order_table(c["cpu"][0], a_cpu, levels)
    on = _encoding(cuda, "small_hash", table, second_order=True)
    xg = x.clone().requires_grad_()
    y = on(xg)
    (g1,) = torch.autograd.grad(y, xg, dout, create_graph=True)
    ((y * a_cpu.to(cuda)).sum() + (g1 * r).sum()).backward()
    t = want["table"]
    ref, bound = first.grad + t.grad, ((4 + first.N.double())[:, None] + 2) * U * first.B + (k_table(0, t.N)[:, None] + 2) * U * t.B
    err = (on.params.grad.view(-1, 2).cpu().double() - ref).abs()
    print(f"[grid-grad2] scatter(a) + table term: worst |gpu - model| / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()) and float(first.grad.abs().max()) > 0
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())


def test_encoding_frozen_table_and_what_raises(cuda, mode0, profile):
    c = mode0("small_hash")
    levels, x, dout, r, table = c["levels"], c["x"], c["dout"], c["r"], c["table"]
    gd_c, gx_c, _, _ = c_second(x, dout, r, table, levels, (True, True, False))
    on = _encoding(cuda, "small_hash", table, second_order=True)
    # a frozen table: no params.grad, and the table kernel is not launched
    on.params.requires_grad_(False)
    xg, dl = x.clone().requires_grad_(), dout.clone().requires_grad_()
    (g1,) = torch.autograd.grad(on(xg), xg, dl, create_graph=True)
    (g1 * r).sum().backward()
    assert on.params.grad is None and torch.equal(xg.grad, gx_c) and torch.equal(dl.grad, gd_c)
    assert len(profile.get("second_order_rows", [])) == 1 and "second_order_table" not in profile
    on.params.requires_grad_(True)
    profile.clear()
    xg = x.clone().requires_grad_()
    (g1,) = torch.autograd.grad(on(xg), xg, dout, create_graph=True)
    (g1 * r).sum().backward()
    assert len(profile.get("second_order_table", [])) == 1 and on.params.grad is not None
    # a third derivative raises
    xg = x[:64].clone().requires_grad_()
    (g1,) = torch.autograd.grad(on(xg), xg, dout[:64], create_graph=True)
    (g2,) = torch.autograd.grad((g1 * g1).sum(), xg, create_graph=True)
    assert g2.requires_grad                                 # (marked, so that differentiating it raises instead of giving 0)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g2.sum().backward()
    # the parameter gradient stays once differentiable: differentiating it again raises, it is not a silent zero
    xg = x[:64].clone().requires_grad_()
    (gp,) = torch.autograd.grad(on(xg), on.params, dout[:64], create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gp.sum(), xg)
    # an x that does not require grad goes through the first-order node, flag or no flag
    assert type(on(x).grad_fn).__name__ == "_hashgridBackward"
    # under autocast the nodes compute in fp32 as the first-order ones do
    xg = x[:64].clone().requires_grad_()
    with torch.autocast("cuda", torch.float16):
        y = on(xg)
        (g1,) = torch.autograd.grad(y, xg, dout[:64], create_graph=True)
    assert y.dtype == g1.dtype == torch.float32
    (gx,) = torch.autograd.grad((g1 * r[:64]).sum(), xg)
    assert torch.equal(gx, gx_c[:64])


# ------------------------------------------------------------------------------------------------ autograd, encode_points

def test_encode_points_second_order(cuda, mode1, profile):
    from mi3d import _lib as L
    from mi3d import grid_ops
    c = mode1(1.0, True)
    levels, offs, P0, bound, want = c["levels"], c["offs"], c["P0"], c["bound"], c["want"]
    x, x2, dout, r, r2, table, cfg = c["x"], c["x2"], c["dout"], c["r"], c["r2"], c["table"], c["levels"].cfg
    # the first order: the same bits as with the flag off
    firsts = []
    for flag in (False, True):
        xg, x2g = x.clone().requires_grad_(), x2.clone().requires_grad_()
        y = grid_ops.encode_points(table, xg, offs, cfg, bound, x2g, P0, second_order=flag)
        y.backward(dout)
        firsts.append((y.detach(), xg.grad, x2g.grad))
    assert all(torch.equal(a, b) for a, b in zip(*firsts))
    # the second order: the C ABI's rows bit for bit, the table against the model
    gd_c, gx_c, gx2_c, _ = _second1(c, (True, True, False))
    params = table.clone().requires_grad_()
    xg, x2g, dl = x.clone().requires_grad_(), x2.clone().requires_grad_(), dout.clone().requires_grad_()
    y = grid_ops.encode_points(params, xg, offs, cfg, bound, x2g, P0, second_order=True)
    g1, g2 = torch.autograd.grad(y, [xg, x2g], dl, create_graph=True)
    assert torch.equal(g1, firsts[0][1]) and torch.equal(g2, firsts[0][2])
    profile.clear()
    gd, gx, gx2, gp = torch.autograd.grad((g1 * r).sum() + (g2 * r2).sum(), [dl, xg, x2g, params])
    assert torch.equal(gd, gd_c) and torch.equal(gx, gx_c) and torch.equal(gx2, gx2_c)
    check("encode_points grad_params", gp, want["table"].grad, want["table"].B, k_table(1, want["table"].N))
    assert len(profile["second_order_rows"]) == 1 and len(profile["second_order_table"]) == 1
    # x2 alone requires grad, the table is frozen: no table launch, and r = 0 for the points around x
    profile.clear()
    x2g = x2.clone().requires_grad_()
    y = grid_ops.encode_points(table, x, offs, cfg, bound, x2g, P0, second_order=True)
    (g2,) = torch.autograd.grad(y, x2g, dout, create_graph=True)
    assert torch.equal(g2, firsts[0][2])
    (g2 * r2).sum().backward()
    _, _, gx2_only, _ = c_second(x, dout, torch.zeros_like(r), table, levels, (False, True, False), x2=x2, r2=r2, offs=offs,
                                 P0=P0, bound=bound)
    assert torch.equal(x2g.grad, gx2_only) and table.grad is None
    assert len(profile["second_order_rows"]) == 1 and "second_order_table" not in profile
    # a third derivative raises, and so does differentiating the parameter gradient
    xg = x[:64].clone().requires_grad_()
    y = grid_ops.encode_points(params, xg, offs[:7], cfg, bound, second_order=True)
    (g1,) = torch.autograd.grad(y, xg, torch.ones_like(y), create_graph=True)
    (g2,) = torch.autograd.grad((g1 * g1).sum(), xg, create_graph=True)
    assert g2.requires_grad                                 # (marked, so that differentiating it raises instead of giving 0)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g2.sum().backward()
    (gp,) = torch.autograd.grad(y, params, torch.ones_like(y), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gp.sum(), xg)
    # with the flag off the second derivative still raises
    xg = x[:64].clone().requires_grad_()
    y = grid_ops.encode_points(table, xg, offs[:7], cfg, bound)
    (g1,) = torch.autograd.grad(y, xg, torch.ones_like(y), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g1.sum(), xg)
    # the counted rows belong to the inference loop, with the flag as without
    count = torch.tensor([10], dtype=torch.int32, device=cuda)
    with pytest.raises(L.Mi3dError, match="count"):
        grid_ops.encode_points(table, x.clone().requires_grad_(), offs[:7], cfg, bound, count=count, second_order=True)
    assert grid_ops.encode_points(table, x, offs[:7], cfg, bound, count=count, second_order=True).shape == (7 * c["n"], 32)


# ------------------------------------------------------------------------------------------------ a use

def _eikonal(cuda, second_order):
    import tinycudann as tcnn
    torch.manual_seed(0)
    cfg = M.CONFIGS["default16"]
    enc = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19,
                            "base_resolution": 16, "per_level_scale": cfg["per_level_scale"]}, dtype=torch.float32,
                        second_order=second_order).to(cuda)
    mlp = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.Softplus(), torch.nn.Linear(16, 1)).to(cuda)
    x = torch.rand(4096, 3, generator=torch.Generator().manual_seed(121)).to(cuda).requires_grad_()
    f = mlp(enc(x))
    (g,) = torch.autograd.grad(f.sum(), x, create_graph=True)
    loss = ((g.norm(dim=-1) - 1) ** 2).mean()
    return enc, mlp, loss


def test_an_eikonal_loss_trains_the_table(cuda):
    """mean((|df/dx| - 1)^2), f a small torch MLP on Encoding(second_order=True): forward and backward run and reach the
    table and the weights.  With the flag off the same code raises."""
    enc, mlp, loss = _eikonal(cuda, True)
    loss.backward()
    grads = [enc.params.grad] + [p.grad for p in list(mlp.parameters())[:3]]     # (df/dx does not contain the last bias)
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    assert math.isfinite(float(loss)) and float(loss) > 0
    enc, mlp, loss = _eikonal(cuda, False)
    with pytest.raises(RuntimeError):
        loss.backward()
