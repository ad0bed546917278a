"""GPU: the fused MLP's second-order pass (k_mlp_bwd2_g behind mi3d_mlp_backward_backward, include/mi3d.h Part 4) against
the binary64 model of tests/mlp_grad2_model.py, its autograd surface (mlp_ops.fused_mlp(second_order=True)) and the field
on top (NeRFNetwork.density_gradient / analytic_normal with create_graph=True).

THE BOUNDS are the model's running error bounds (tests/mlp_grad2_model.py: c 2^-24 sum |terms| per sum of c terms rounded
once each, nested down the chain; the weight gradients' depth from the kernel's launch geometry); every element must use
at most 1.0 of its bound.  The field is held to DESIGN.md 13's rule: four times the error the same chain has in binary32
on the CPU against binary64.

MEASURED on the MI355X (profiles/mlp_second_order_parity.json): largest share of a bound used 0.12 by grad_dout (2 -> 32 -> 4
at 196 645 rows).  Weight gradients: at most 0.27, but for two shapes at 196 645 rows where a hidden unit that is open in a
few hundred rows has an undecided mask in some of them - the model puts that unit's whole term into the bound, it is
0.97 - 0.999 of the bound of the unit's elements, and the kernel's mask fell the other way: 0.996 and 0.956 used in
8 -> 32 x 2 -> 4 (gW2, gW3), 0.62 and 0.33 in 16 -> 64 x 2 -> 4.  At most 0.46 % of a case's rows left out; the field's table
and weight gradients at 0.19 - 0.37 of four times the binary32 chain's error.

Every case appends its figures to mlp_second_order_parity.json BEFORE it asserts - in the directory MI3D_REPORT_DIR names,
or in test_reports/ at the root of the repository (git-ignored).
"""
import json
import os

import pytest
import torch

import grid_grad_model as G
import mlp_grad2_model as M2
import mlp_model as Mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_PATH = os.path.join(os.environ.get("MI3D_REPORT_DIR") or os.path.join(ROOT, "test_reports"),
                           "mlp_second_order_parity.json")
_REPORT = []

INVALID = 1            # hipErrorInvalidValue
SENTINEL = 7.0
N_LOOPS = 3 * M2.BWD2_LOOPS_ABOVE + 37     # every wave of the persistent grid walks at least three tiles
SIZES = (1, 19, 32, 33, 4099)


def _report(entry):
    _REPORT.append(entry)
    os.makedirs(os.path.dirname(REPORT_PATH), exist_ok=True)
    with open(REPORT_PATH, "w") as f:
        json.dump(_REPORT, f, indent=0)


def _wargs(ws):
    """(W1, b1, W2, b2, W3, b3), the middle pair None for two layers."""
    if len(ws) == 3:
        return [ws[0][0], ws[0][1], ws[1][0], ws[1][1], ws[2][0], ws[2][1]]
    return [ws[0][0], ws[0][1], None, None, ws[1][0], ws[1][1]]


def c_bwd2(x, ws, dout, r, n, rows=True, weights=True, fill=0.0, rc=False):
    """The C ABI's second-order call on the first n rows.  grad_dout lands in a sentinel-filled buffer as tall as x; the
    weight buffers are pre-filled with `fill`.  -> dict(grad_dout (the whole buffer), gW [L]) or, rc=True, the return code
    and the buffers."""
    from mi3d import _lib as L
    wa = _wargs(ws)
    din, hid = wa[0].shape[1], wa[0].shape[0]
    gd = torch.full((x.shape[0], 4), SENTINEL, device=x.device) if rows else None
    gW = [None if (w is None or not weights) else torch.full_like(w, fill) for w in (wa[0], wa[2], wa[4])]
    with L.on(x):
        err = L.lib().mi3d_mlp_backward_backward(L.ptr(x), L.ptr(dout), L.ptr(r), n, *[L.ptr(t) for t in wa], din, hid, 4,
                                                 L.ptr(gd), *[L.ptr(g) for g in gW], L.stream(x))
    out = dict(grad_dout=gd, gW=[g for g in gW if g is not None] if weights else None)
    if rc:
        return err, out
    assert err == 0, err
    return out


_cache = {}


def case(shape, n, cuda, extra_rows=0):
    """Inputs on the GPU and the model's result (computed once per case, on the CPU, and left unchanged)."""
    key = (shape, n, extra_rows)
    if key not in _cache:
        x, ws, dout, r = M2.make_case(*shape, n, extra_rows=extra_rows)
        ref = M2.second_order(x[:n], ws, dout[:n], r[:n])
        dev = (x.to(cuda), [(w.to(cuda), b.to(cuda)) for w, b in ws], dout.to(cuda), r.to(cuda))
        if n > 5000:
            return dev, ref            # (the large case is used once)
        _cache[key] = (dev, ref)
    return _cache[key]


def _cpu(out, n):
    return dict(grad_dout=None if out["grad_dout"] is None else out["grad_dout"][:n].cpu(),
                gW=None if out["gW"] is None else [g.cpu() for g in out["gW"]])


def _check(tag, shape, n, out, ref):
    fig, fails = M2.check(_cpu(out, n), ref)
    print(f"[mlp-grad2] {tag} {shape} n={n}: {fig}")
    _report(dict(case=tag, shape=list(shape), n=n, **fig))
    assert fails == [], (tag, shape, n, fails, fig)


# ------------------------------------------------------------------------------------------------ C ABI against the model

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", Mm.SHAPES)
def test_c_abi_against_the_model(cuda, shape, n):
    (x, ws, dout, r), ref = case(shape, n, cuda)
    _check("c_abi", shape, n, c_bwd2(x, ws, dout, r, n), ref)


@pytest.mark.parametrize("shape", Mm.SHAPES)
def test_persistent_grid_carries_its_accumulators(cuda, shape):
    """3 x (rows at which the grid becomes persistent) + 37 rows: every wave walks at least three tiles, so every instance
    carries its accumulators from tile to tile, prefetches inside the loop and launders its lane offsets again."""
    assert M2.grid_for2(N_LOOPS) == M2.grid_for2(M2.BWD2_LOOPS_ABOVE) == 512
    (x, ws, dout, r), ref = case(shape, N_LOOPS, cuda)
    _check("persistent", shape, N_LOOPS, c_bwd2(x, ws, dout, r, N_LOOPS), ref)


@pytest.mark.parametrize("shape", [(32, 64, 3), (30, 64, 2), (8, 32, 3), (2, 32, 2)])
def test_rows_past_n_and_buffers(cuda, shape):
    """POISON rows past n in x, dout and r leave no trace; nothing beyond [n, 4] is written; the weight gradients are
    accumulated into what the buffers held; grad_dout is the same bits call after call and with or without the weight
    outputs; the weight gradients with and without grad_dout differ by no more than two runs of the same call do."""
    n, extra = 4099, 70
    (x, ws, dout, r), ref = case(shape, n, cuda, extra_rows=extra)
    assert float(x[n:].min()) == Mm.POISON == float(r[n:].min()) == float(dout[n:].min())
    both = c_bwd2(x, ws, dout, r, n)
    _check("poison_rows", shape, n, both, ref)
    assert bool((both["grad_dout"][n:] == SENTINEL).all())
    # the same rows without anything behind them: the same bits
    clean = c_bwd2(x[:n].contiguous(), ws, dout[:n].contiguous(), r[:n].contiguous(), n)
    assert torch.equal(clean["grad_dout"], both["grad_dout"][:n])
    again = c_bwd2(x, ws, dout, r, n)
    rows_only = c_bwd2(x, ws, dout, r, n, weights=False)
    assert torch.equal(again["grad_dout"], both["grad_dout"]) and torch.equal(rows_only["grad_dout"], both["grad_dout"])
    w_only = c_bwd2(x, ws, dout, r, n, rows=False)
    _check("weights_only", shape, n, w_only, ref)
    # The three calls add the same per-workgroup sums (the chains are the same code with and without the row store) in
    # whatever order the float atomics land: the weight gradients with and without grad_dout may differ by what two runs
    # of the same call differ by - or, where those two happened to land in the same order, by what reordering the sum of
    # the W workgroups' partial sums can move it, 2 W 2^-24 sum |terms|.
    wgs = M2.grid_for2(n)
    for l, (g1, g2, g3) in enumerate(zip(both["gW"], again["gW"], w_only["gW"])):
        terms = Mm._finite(ref["d"][l + 1]).abs().t() @ Mm._finite(ref["u"][l]).abs()
        allowed = torch.maximum((g1 - g2).abs().cpu().double(), 2 * wgs * Mm.U32 * terms)
        assert bool(((g1 - g3).abs().cpu().double() <= allowed).all()), l
    # accumulation: pre-filled buffers come back as fill + gradient
    filled = c_bwd2(x, ws, dout, r, n, fill=3.0)
    depth = M2.wgrad2_depth(n)          # every addition on the way now also rounds against the 3.0 in the buffer
    for l, f in enumerate(filled["gW"]):
        e = ref["gW_err"][l] + Mm.U32 * ref["gW"][l].abs() + depth * Mm.U32 * 3.0
        assert bool(((f.cpu().double() - 3.0 - ref["gW"][l]).abs() <= e).all()), l


@pytest.mark.parametrize("shape", [(32, 64, 3), (16, 64, 3), (32, 32, 2)])
@pytest.mark.parametrize("n", [19, 32])
def test_one_tile_has_no_order_to_differ_by(cuda, shape, n):
    """One tile: one wave's registers hold every sum and the other waves add zeros.  Two runs of the same call are the same
    bits, and so are the weight gradients with and without grad_dout (and grad_dout with and without them)."""
    (x, ws, dout, r), _ = case(shape, n, cuda)
    both, again = c_bwd2(x, ws, dout, r, n), c_bwd2(x, ws, dout, r, n)
    w_only, rows_only = c_bwd2(x, ws, dout, r, n, rows=False), c_bwd2(x, ws, dout, r, n, weights=False)
    assert torch.equal(both["grad_dout"], again["grad_dout"]) and torch.equal(both["grad_dout"], rows_only["grad_dout"])
    for g1, g2, g3 in zip(both["gW"], again["gW"], w_only["gW"]):
        assert torch.equal(g1, g2) and torch.equal(g1, g3)


def test_zero_edge(cuda):
    x, ws, dout, r = M2.zero_edge_case(cuda)
    n = x.shape[0]
    out = c_bwd2(x, ws, dout, r, n)
    assert M2.check_zero_edge(_cpu(out, n)) == []
    assert M2.check_zero_edge(M2.as_got(M2.second_order(*M2.zero_edge_case()))) == []


def test_argument_errors(cuda):
    (x, ws, dout, r), _ = case((32, 64, 3), 33, cuda)
    from mi3d import _lib as L
    wa = _wargs(ws)
    gd = torch.full((33, 4), SENTINEL, device=cuda)
    gW = [torch.full_like(w, SENTINEL) for w in (wa[0], wa[2], wa[4])]

    def call(din, hid, dout_w, gd_, g1, g2, g3, n=33):
        with L.on(x):
            return L.lib().mi3d_mlp_backward_backward(L.ptr(x), L.ptr(dout), L.ptr(r), n, *[L.ptr(t) for t in wa], din, hid,
                                                      dout_w, L.ptr(gd_), L.ptr(g1), L.ptr(g2), L.ptr(g3), L.stream(x))
    assert call(31, 64, 4, gd, *gW) == INVALID and call(34, 64, 4, gd, *gW) == INVALID        # unsupported dims
    assert call(32, 48, 4, gd, *gW) == INVALID and call(32, 64, 3, gd, *gW) == INVALID
    assert call(32, 64, 4, None, None, None, None) == INVALID                                 # every output null
    assert call(32, 64, 4, gd, gW[0], None, gW[2]) == INVALID                                 # gW2 missing, three layers
    assert call(32, 64, 4, None, gW[0], None, gW[2]) == INVALID
    assert call(32, 64, 4, gd, *gW, n=0) == 0                                                 # n == 0: nothing to do
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (gd, *gW))                                # nothing was launched


# ------------------------------------------------------------------------------------------------ autograd

class _Lin:
    def __init__(self, w, b):
        self.weight, self.bias = w, b


def _layers(ws, grad=True):
    return [_Lin(w.clone().requires_grad_(grad), b.clone().requires_grad_(grad)) for w, b in ws]


@pytest.mark.parametrize("shape", [(32, 64, 3), (8, 32, 2)])
def test_autograd_second_order(cuda, shape):
    from mi3d import _lib as L
    from mi3d import mlp_ops
    n = 4099
    (x, ws, dout, r), ref = case(shape, n, cuda)
    want = c_bwd2(x, ws, dout, r, n)
    layers = _layers(ws)
    xg, dg = x.clone().requires_grad_(), dout.clone().requires_grad_()
    y = mlp_ops.fused_mlp(xg, layers, second_order=True)
    (dx,) = torch.autograd.grad(y, xg, dg, create_graph=True)
    # dx is the flag-off route's, bit for bit
    x0 = x.clone().requires_grad_()
    y0 = mlp_ops.fused_mlp(x0, _layers(ws))
    (dx0,) = torch.autograd.grad(y0, x0, dout)
    assert torch.equal(y, y0) and torch.equal(dx, dx0)
    params = [l.weight for l in layers] + [l.bias for l in layers]
    g = torch.autograd.grad((dx * r).sum(), [dg, xg, *params], allow_unused=True, retain_graph=True)
    L_ = len(layers)
    assert torch.equal(g[0], want["grad_dout"])
    got = dict(grad_dout=g[0], gW=list(g[2:2 + L_]))
    _check("autograd", shape, n, got, ref)
    for t in (g[1], *g[2 + L_:]):                                   # x and the biases
        assert t is None or float(t.abs().max()) == 0.0
    # only the upstream gradient asked for: the rows-only launch, the same bits
    (g_only,) = torch.autograd.grad((dx * r).sum(), [dg], retain_graph=True)
    assert torch.equal(g_only, want["grad_dout"])
    # a third derivative raises torch's own error
    rg = r.clone().requires_grad_()
    (dx2,) = torch.autograd.grad(y, xg, dg, create_graph=True)
    (gd2,) = torch.autograd.grad((dx2 * rg).sum(), [dg], create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gd2.sum(), [layers[0].weight])
    # a gradient sent into a parameter gradient raises: it is never a silent zero
    dW1 = torch.autograd.grad(y, layers[0].weight, dg, create_graph=True)[0]
    with pytest.raises(L.Mi3dError, match="once differentiable"):
        torch.autograd.grad(dW1.sum(), [dg])
    # float16 autocast: the error names the remedy
    with torch.autocast("cuda", torch.float16):
        with pytest.raises(L.Mi3dError, match="enabled=False"):
            mlp_ops.fused_mlp(xg, layers, second_order=True)
    with pytest.raises(L.Mi3dError, match="enabled=False"):
        mlp_ops.fused_mlp(xg, layers, half_mode=True, second_order=True)


def test_flag_off_is_the_node_it_was(cuda):
    from mi3d import grid_ops, mlp_ops
    (x, ws, dout, r), _ = case((32, 64, 3), 4099, cuda)
    layers = _layers(ws)
    xg = x.clone().requires_grad_()
    assert grid_ops.PROFILE is None
    grid_ops.PROFILE = {}
    try:
        y = mlp_ops.fused_mlp(xg, layers)
        assert type(y.grad_fn).__name__ == "_FusedMLPBackward"
        saved = y.grad_fn.saved_tensors
        assert len(saved) == 7 and saved[0].data_ptr() == xg.data_ptr()
        assert [s.data_ptr() for s in saved[1:]] == [t.data_ptr() for l in layers for t in (l.weight, l.bias)]
        y.backward(dout)
        names = sorted(k for k in grid_ops.PROFILE if not k.endswith("_evals"))
        assert names == ["mlp_bwd", "mlp_fwd"] and [len(grid_ops.PROFILE[k]) for k in names] == [1, 1]
        # the flag without anything to differentiate, or without grad mode, is the same node too
        grid_ops.PROFILE.clear()
        with torch.no_grad():
            y1 = mlp_ops.fused_mlp(xg, layers, second_order=True)
        y2 = mlp_ops.fused_mlp(x, _layers(ws, grad=False), second_order=True)
        assert y1.grad_fn is None and y2.grad_fn is None and torch.equal(y1, y) and torch.equal(y2, y)
        # flag on: the same two launches first, then the second-order one
        grid_ops.PROFILE.clear()
        xg2, dg = x.clone().requires_grad_(), dout.clone().requires_grad_()
        y3 = mlp_ops.fused_mlp(xg2, layers, second_order=True)
        (dx,) = torch.autograd.grad(y3, xg2, dg, create_graph=True)
        assert sorted(k for k in grid_ops.PROFILE if not k.endswith("_evals")) == ["mlp_bwd", "mlp_fwd"]
        torch.autograd.grad((dx * r).sum(), [dg])
        assert sorted(k for k in grid_ops.PROFILE if not k.endswith("_evals")) == ["mlp_bwd", "mlp_bwd2", "mlp_fwd"]
    finally:
        grid_ops.PROFILE = None


# ------------------------------------------------------------------------------------------------ the field

N_FIELD = 1000


def _chain_loss(x32, q32, a, table, levels, W, b, bound, blob_density, blob_radius, dtype):
    """L = mean((|d sigma / dx| - 1)^2) + <analytic normal, a> of common_forward's chain in `dtype` on the CPU by torch
    autograd (tests/grid_grad_model.forward: the kernel's binary32 cell and fraction -> Linear / ReLU -> exp(h0 + blob)),
    and its gradients with respect to the table and the three weights.  Also the hidden pre-activations with the magnitude
    they are rounded against, and the largest exponent."""
    x = x32.to(dtype).requires_grad_()
    table = table.to(dtype).requires_grad_()
    W = [w.to(dtype).requires_grad_() for w in W]
    b = [bb.to(dtype) for bb in b]
    q = (x + bound) / (2 * bound)
    h = G.forward(q32, table, levels, dtype, dq=q - q.detach())
    pre = []
    for l in range(len(W)):
        z = h @ W[l].T + b[l]
        if l < len(W) - 1:
            pre.append((z.detach(), h.detach().abs() @ W[l].detach().abs().T + b[l].abs()))
            h = torch.relu(z)
    z0 = z[:, 0] + blob_density * torch.exp(-(x ** 2).sum(-1) / (2 * blob_radius ** 2))
    sigma = torch.exp(z0)
    (g,) = torch.autograd.grad(sigma.sum(), x, create_graph=True)
    nrm = -g / torch.sqrt(torch.clamp((g * g).sum(-1, keepdim=True), min=1e-20, max=1e32))
    loss = ((g.norm(dim=-1) - 1) ** 2).mean() + (torch.nan_to_num(nrm) * a.to(dtype)).sum()
    grads = torch.autograd.grad(loss, [table, *W])
    return loss.detach(), [t.detach() for t in grads], pre, float(z0.detach().max())


@pytest.fixture(scope="module")
def field(cuda):
    """A small blob field - 16 levels of at most 2^14 entries, 64 x 3, the table at its initial U(-1e-4, 1e-4) - and 1000
    points kept 2^-10 of a cell from every face, none of them within 1e-5 of a ReLU kink in binary64."""
    from mi3d import network, sds_step
    torch.manual_seed(0)
    model = network.NeRFNetwork(sds_step.make_opt(fp16=False), log2_hashmap_size=14).to(cuda)
    levels = G.Levels(**model.encoder.cfg)
    assert levels.n_levels == 16 and float(model.bound) == 1.0 and model.sigma_net.dim_hidden == 64
    gen = torch.Generator().manual_seed(61)
    cand = torch.rand(4 * N_FIELD, 3, generator=gen) * 2 - 1
    cand[::2] *= 0.3                                            # half of them inside the blob, where sigma has a slope
    q32 = G.point_q(cand, torch.zeros(3), 1.0)[0]
    ok = G.keep(q32, levels)
    x, q32 = cand[ok][:2 * N_FIELD].contiguous(), q32[ok][:2 * N_FIELD].contiguous()
    a = torch.randn(x.shape[0], 3, generator=gen)
    table = model.encoder.params.detach().cpu().clone()
    W = [l.weight.detach().cpu() for l in model.sigma_net.net]
    b = [l.bias.detach().cpu() for l in model.sigma_net.net]
    args = (table, levels, W, b, 1.0, float(model.opt.blob_density), float(model.opt.blob_radius))
    _, _, pre, _ = _chain_loss(x, q32, a, *args, torch.float64)
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    for z, mag in pre:
        near |= (z.abs() <= 1e-5 * mag).any(-1)
    x, q32, a = x[~near][:N_FIELD].contiguous(), q32[~near][:N_FIELD].contiguous(), a[~near][:N_FIELD].contiguous()
    assert x.shape[0] == N_FIELD
    return model, x, q32, a, args


@pytest.fixture(scope="module")
def chain_ref(field):
    """The loss and its gradients by the CPU chain: A in binary64, B in binary32 (computed once, shared, left unchanged)."""
    model, x, q32, a, args = field
    lA, gA, _, z_max = _chain_loss(x, q32, a, *args, torch.float64)
    lB, gB, _, _ = _chain_loss(x, q32, a, *args, torch.float32)
    assert z_max < 15                                           # trunc_exp's clamped derivative is exp's own here
    return lA, gA, lB, gB


def _field_loss_backward(model, xg, ag):
    model.zero_grad(set_to_none=True)
    sigma, grad = model.density_gradient(xg, create_graph=True)
    nrm = model.analytic_normal(xg, create_graph=True)
    assert sigma.requires_grad and grad.requires_grad and nrm.requires_grad and grad.shape == (xg.shape[0], 3)
    loss = ((grad.norm(dim=-1) - 1) ** 2).mean() + (nrm * ag).sum()
    loss.backward()
    got = [model.encoder.params.grad] + [l.weight.grad for l in model.sigma_net.net]
    assert all(g is not None for g in got)
    got = [g.detach().clone() for g in got]
    model.zero_grad(set_to_none=True)
    return sigma.detach(), grad.detach(), loss.detach(), got


def test_field_in_several_chunks(cuda, field, chain_ref, monkeypatch):
    """mesh.CHUNK = 300: the 1000 points go through four chunks, the last one partial, and are concatenated.  The rows are
    the one-chunk call's bit for bit (a row does not know its chunk); the parameter gradients, now sums of four launches,
    are held to the same tolerance against the binary64 chain as the one-chunk call."""
    from mi3d import mesh
    model, x, q32, a, args = field
    _, gA, _, gB = chain_ref
    xg, ag = x.to(cuda), a.to(cuda)
    s1, g1, _, _ = _field_loss_backward(model, xg, ag)
    assert mesh.CHUNK >= N_FIELD
    monkeypatch.setattr(mesh, "CHUNK", 300)
    s4, g4, _, got = _field_loss_backward(model, xg, ag)
    assert torch.equal(s4, s1) and torch.equal(g4, g1)
    for name, g, A, B in zip(("table", "W1", "W2", "W3"), got, gA, gB):
        err = float((g.cpu().double().reshape(A.shape) - A).abs().max())
        tol = 4 * float((B.double() - A).abs().max())
        print(f"[mlp-grad2] field in 4 chunks {name}: |gpu - A| {err:.3e}, bound {tol:.3e}")
        assert err <= tol, name
    # the create_graph=False route in chunks: the same bits too
    s0, g0 = model.density_gradient(xg)
    assert torch.equal(s0, s1) and torch.equal(g0, g1)
    # no points: empty results, attached
    se, ge = model.density_gradient(xg[:0], create_graph=True)
    assert se.shape == (0,) and ge.shape == (0, 3) and se.requires_grad and ge.requires_grad
    (se.sum() + ge.sum()).backward()
    assert float(model.encoder.params.grad.abs().max()) == 0.0
    model.zero_grad(set_to_none=True)


def test_field_loss_on_the_density_gradient_trains(cuda, field, chain_ref):
    """|gpu - A| <= 4 max |B - A| per gradient tensor: A the chain in binary64, B the same chain in binary32, both on the
    CPU (DESIGN.md 13's rule; the 4 covers the matrix core's unknown summation order)."""
    from mi3d.renderer import safe_normalize
    model, x, q32, a, args = field
    lA, gA, lB, gB = chain_ref
    xg, ag = x.to(cuda), a.to(cuda)
    sigma, grad, loss, got = _field_loss_backward(model, xg, ag)
    figs = {}
    for name, g, A, B in zip(("table", "W1", "W2", "W3"), got, gA, gB):
        tol = 4 * float((B.double() - A).abs().max())
        err = float((g.detach().cpu().double().reshape(A.shape) - A).abs().max())
        figs[name] = dict(err_gpu=err, err_binary32_cpu=tol / 4, max_abs=float(A.abs().max()))
        print(f"[mlp-grad2] field {name}: |gpu - A| {err:.3e}, binary32 chain |B - A| {tol / 4:.3e}, max |A| {float(A.abs().max()):.3e}")
    err_l = abs(float(loss) - float(lA))
    figs["loss"] = dict(err_gpu=err_l, err_binary32_cpu=abs(float(lB) - float(lA)), value=float(lA))
    _report(dict(case="field", n=N_FIELD, **figs))
    for name, f in figs.items():
        if name != "loss":
            assert f["max_abs"] > 0 and f["err_gpu"] <= 4 * f["err_binary32_cpu"], (name, f)
    model.zero_grad(set_to_none=True)
    # grad mode is needed
    from mi3d import _lib as L
    with torch.no_grad():
        with pytest.raises(L.Mi3dError, match="grad mode"):
            model.density_gradient(xg, create_graph=True)
    # create_graph=False: yesterday's launches and bits, and no .grad anywhere
    from mi3d import grid_ops, mlp_ops, network
    s0, g0 = model.density_gradient(xg)
    assert not s0.requires_grad and not g0.requires_grad
    assert all(p.grad is None for p in model.parameters())
    weights = tuple(t.detach() for t in mlp_ops.layer_args(model.sigma_net.net))
    with torch.enable_grad(), torch.autocast("cuda", enabled=False):
        xc = xg.detach().requires_grad_()
        feat = grid_ops.encode_points(model.encoder.params.detach(), xc, model._CENTER, model.encoder.cfg, 1.0)
        h = mlp_ops._FusedMLP.apply(feat, *weights, False)
        sig = network.trunc_exp(h[..., 0] + model.gaussian(xc))
        (gp,) = torch.autograd.grad(sig.sum(), xc)
    assert torch.equal(s0, sig.detach()) and torch.equal(g0, gp)
    assert torch.equal(model.analytic_normal(xg), torch.nan_to_num(safe_normalize(-g0)))
    # the attached route computes the same values
    assert torch.equal(sigma, s0) and torch.equal(grad, g0)
    assert all(p.grad is None for p in model.parameters())
