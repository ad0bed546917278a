"""Reference model of the fused MLP's SECOND-ORDER pass (mi3d_mlp_backward_backward, include/mi3d.h Part 4) in plain torch,
written from the header's contract - not from the kernel.  It runs on CPU or GPU tensors.

  a1 = W1 x + b1, M1 = [a1 > 0];  a2 = W2 relu(a1) + b2, M2 = [a2 > 0];  y = W3 relu(a2) + b3     (two layers: no a2)
  first order, upstream dy:     d2 = M2 (W3^T dy),  d1 = M1 (W2^T d2),  dx = W1^T d1
  second order, r = dL/d(dx):   u1 = M1 (W1 r),     u2 = M2 (W2 u1),    u3 = W3 u2
  grad_dout = u3,  grad_W3 = sum_rows dy u2^T,  grad_W2 = sum_rows d2 u1^T,  grad_W1 = sum_rows d1 r^T
  grad_x = 0, grad_b = 0 exactly (dx depends on x and the biases through the piecewise constant masks only)

Every product is written out per layer; every sum is binary64.  The masks are tests/mlp_model.py's (`pre`: open iff not
(pre-activation <= 0)), and so are the undecided units: those whose binary64 pre-activation lies within its running bound
`pre_err` of zero.  With the result comes a RUNNING ERROR BOUND per element, by mlp_model's own rule - a sum of c terms, each
rounded once, is off by at most c 2^-24 times the sum of the absolute values of its terms, nested down the chain:

  grad_dout   the tangent chain's contraction lengths dim_in, hid, (hid); rows with an undecided unit are left out
              (`uncertain_rows`)
  grad_W      sums over the n rows.  Their depth is the launch geometry of the SECOND-ORDER kernel (k_mlp_bwd2_g, grid_for2
              below): 32 rows per tile on the matrix core, the tiles of a persistent wave added into the same registers, 4
              waves per workgroup added in LDS, the workgroups added with float atomics, + 1 for the accumulation into the
              caller's buffer - with at most 256 x BWD2_WGS_PER_CU workgroups.  On top come the two factors' own bounds;
              where a unit is undecided its factor's whole value is in the bound, not out of the sum.
  Each element gets + 2^-24 |result| (the result itself is an fp32 number).

`acc` = torch.float32 evaluates the same model with fp32 products (how far two correct evaluations may differ); `faults`
seeds one of FAULTS (tests/test_mlp_grad2_cpu.py: each must break the assertion FAULT_BREAKS names).
"""
import torch

import mlp_model as Mm

U32 = Mm.U32
BWD2_WGS_PER_CU = 2        # kBwd2WgsPerCU in csrc/field.hip
BWD2_LOOPS_ABOVE = Mm.CUS * BWD2_WGS_PER_CU * Mm.WAVES_PER_WG * Mm.ROWS_PER_TILE     # 65 536 rows

FAULTS = ("tangent_unmasked", "mask_from_tangent", "wgrad_pairs_swapped", "bias_in_tangent", "last_row_twice",
          "poison_row")
FAULT_BREAKS = {"tangent_unmasked": "grad_dout_bound", "mask_from_tangent": "grad_dout_bound",
                "bias_in_tangent": "grad_dout_bound", "wgrad_pairs_swapped": "wgrad_bound",
                "last_row_twice": "wgrad_bound", "poison_row": "wgrad_bound"}


def grid_for2(n):
    """The second-order kernel's grid: mlp_model.grid_for's rule at BWD2_WGS_PER_CU workgroups per CU."""
    return Mm.grid_for(n, BWD2_WGS_PER_CU)


def wgrad2_depth(n):
    """Terms one weight-gradient element passes through on its way to memory (see the module docstring)."""
    wgs = grid_for2(n)
    tiles = (n + Mm.ROWS_PER_TILE - 1) // Mm.ROWS_PER_TILE
    tiles_per_wave = (tiles + wgs * Mm.WAVES_PER_WG - 1) // (wgs * Mm.WAVES_PER_WG)
    return Mm.ROWS_PER_TILE + tiles_per_wave + Mm.WAVES_PER_WG + wgs + 1


def second_order(x, layers, dout, r, acc=torch.float64, faults=()):
    """layers: [(W_1, b_1), ..., (W_L, b_L)], L = 2 or 3.  Returns grad_dout [n, 4], gW[l], grad_x, gb[l] (binary64), the
    bounds grad_dout_err and gW_err[l], `uncertain_rows`, and the factors d[l], u[l] with their bounds."""
    faults = set(faults)
    assert faults <= set(FAULTS), faults
    fwd = Mm.model_fp32(x, layers, dout, acc=acc)
    L, n = len(layers), x.shape[0]
    W = [w.double() for w, _ in layers]
    b = [bb.double() for _, bb in layers]
    fin = Mm._finite

    def gate(t, t_err, m, und):
        """A masked factor and its bound: an undecided unit's whole value is in the bound."""
        v = torch.where(m, t, torch.zeros_like(t))
        e = torch.where(und, fin(t).abs() + t_err, torch.where(m, t_err, torch.zeros_like(t_err)))
        return v, e

    mask, und = [], []
    for l in range(L - 1):
        s, e = fwd["pre"][l], fwd["pre_err"][l]
        mask.append(~(s <= 0))                          # open iff not (activation <= 0): a NaN passes
        und.append(((s + e) > 0) != ((s - e) > 0))

    # ---- the tangent chain: u[0] = r, u[l + 1] = M_(l+1) (W_(l+1) u[l]), no bias
    u, u_err = [r.double()], [torch.zeros_like(r.double())]
    for l in range(L - 1):
        fan = W[l].shape[1]
        t = Mm._mm(u[l], W[l].t(), acc)
        t_err = fan * U32 * (fin(u[l]).abs() @ W[l].abs().t()) + u_err[l] @ W[l].abs().t()
        if "bias_in_tangent" in faults:
            t = t + b[l]
        m = mask[l]
        if "mask_from_tangent" in faults and l == 0:
            m = ~(t <= 0)
        if "tangent_unmasked" in faults:
            m = torch.ones_like(m)
        v, e = gate(t, t_err, m, und[l])
        u.append(v); u_err.append(e)
    fan = W[L - 1].shape[1]
    u3 = Mm._mm(u[L - 1], W[L - 1].t(), acc)
    u3_err = fan * U32 * (fin(u[L - 1]).abs() @ W[L - 1].abs().t()) + u_err[L - 1] @ W[L - 1].abs().t()

    # ---- the first-order chain: d[L] = dy, d[l] = M_l (W_(l+1)^T d[l + 1]); d[0] = dx
    d, d_err = [None] * (L + 1), [None] * (L + 1)
    d[L], d_err[L] = dout.double(), torch.zeros_like(dout.double())
    for l in reversed(range(L)):
        c = W[l].shape[0]
        t = Mm._mm(d[l + 1], W[l], acc)
        t_err = c * U32 * (fin(d[l + 1]).abs() @ W[l].abs()) + d_err[l + 1] @ W[l].abs()
        if l > 0:
            d[l], d_err[l] = gate(t, t_err, mask[l - 1], und[l - 1])
        else:
            d[0], d_err[0] = t, t_err

    # ---- the weight gradients: grad_W_(l+1) = sum_rows d[l + 1] u[l]^T
    depth = wgrad2_depth(n)
    gW, gW_err = [], []
    for l in range(L):
        if "wgrad_pairs_swapped" in faults:       # the tangent of the output side with the gradient of the input side
            uo = u3 if l == L - 1 else u[l + 1]
            g = Mm._mm(uo.t(), d[l], acc)
        else:
            g = Mm._mm(d[l + 1].t(), u[l], acc)
        da, ua = fin(d[l + 1]).abs(), fin(u[l]).abs()
        e = depth * U32 * (da.t() @ ua) + d_err[l + 1].t() @ ua + da.t() @ u_err[l] + d_err[l + 1].t() @ u_err[l]
        if "last_row_twice" in faults:
            g = g + d[l + 1][n - 1:n].t() @ u[l][n - 1:n]
        if "poison_row" in faults:                # a row past n whose factors were not zeroed
            g = g + torch.full_like(d[l + 1][:1], Mm.POISON).t() @ torch.full_like(u[l][:1], Mm.POISON)
        gW.append(g); gW_err.append(e)
    return dict(grad_dout=u3, grad_dout_err=u3_err, gW=gW, gW_err=gW_err, grad_x=torch.zeros_like(x.double()),
                gb=[torch.zeros_like(bb) for bb in b], uncertain_rows=fwd["uncertain_rows"], d=d, d_err=d_err, u=u,
                u_err=u_err, n=n)


# ------------------------------------------------------------------------------------------------ inputs

def make_case(din, hid, layers, n, seed=0, device="cpu", extra_rows=0):
    """mlp_model.make_case's x, weights and dout, plus r ~ N(0, 1) [n, din] from the same generator family; the
    `extra_rows` rows past n of r hold POISON like those of x and dout."""
    x, ws, dout = Mm.make_case(din, hid, layers, n, seed=seed, device=device, extra_rows=extra_rows)
    gen = torch.Generator().manual_seed(1000 * seed + 7 * din + hid + layers + 500)
    r = torch.full((n + extra_rows, din), Mm.POISON)
    r[:n] = torch.randn(n, din, generator=gen)
    return x, ws, dout, r.to(device)


def zero_edge_case(device="cpu", n=5):
    """After mlp_model.zero_edge_case, in fp32.  2 -> 32 -> 4, two layers, x = (1, 1): unit 0 has the pre-activation 1 - 1 =
    +0 exactly, unit 1 has -0.5, unit 2 is open (1); every other unit has zero weights (+0, closed).  W3 = 1, dy = 1,
    r = (3, 2).  Nothing passes the closed units: u1 = (0, 0, 2, 0...) so grad_dout = 2 everywhere (an open unit 0 would add
    3 - 2 = 1 - and W1 r is positive there, so a mask taken from the tangent opens it - an open unit 1 -3 + 1 = -2);
    d1 = 4 at unit 2 only, so grad_W1 is zero but for row 2 = 4 n (3, 2), and grad_W3 is zero but for column 2 = 2 n."""
    x = torch.ones(n, 2)
    W1 = torch.zeros(32, 2); W1[0] = torch.tensor([1.0, -1.0]); W1[1] = torch.tensor([-1.0, 0.5]); W1[2, 1] = 1.0
    b1 = torch.zeros(32)
    W3 = torch.ones(4, 32); b3 = torch.zeros(4)
    dout = torch.ones(n, 4)
    r = torch.tensor([3.0, 2.0]).repeat(n, 1)
    return x.to(device), [(W1.to(device), b1.to(device)), (W3.to(device), b3.to(device))], dout.to(device), r.to(device)


def check_zero_edge(got, base=0.0):
    """Named assertions `zero_unit_gradient` and `zero_edge_control`; `base`: what the weight buffers held before."""
    fails = []
    n = got["grad_dout"].shape[0]
    gW1, gW3 = got["gW"][0].double() - base, got["gW"][1].double() - base
    if float(gW1[:2].abs().max()) != 0.0 or float(gW1[3:].abs().max()) != 0.0 or float(gW3[:, :2].abs().max()) != 0.0 or \
            float(gW3[:, 3:].abs().max()) != 0.0:
        fails.append("zero_unit_gradient")
    want1 = torch.tensor([12.0 * n, 8.0 * n], dtype=torch.float64, device=gW1.device)
    if not bool((got["grad_dout"] == 2.0).all()) or not bool((gW1[2] == want1).all()) or \
            not bool((gW3[:, 2] == 2.0 * n).all()):
        fails.append("zero_edge_control")
    return fails


# ------------------------------------------------------------------------------------------------ the assertions

def check(got, ref):
    """got: dict of grad_dout [n, 4] and / or gW [L] (either may be absent).  -> (figures, names of the failed assertions)"""
    fig, fails = {}, []
    keep = ~ref["uncertain_rows"]
    fig["rows_left_out"] = float((~keep).sum()) / ref["n"]
    if fig["rows_left_out"] > Mm.MAX_ROWS_LEFT_OUT:
        fails.append("rows_left_out")
    if got.get("grad_dout") is not None:
        a, w = got["grad_dout"].double(), ref["grad_dout"]
        if not Mm._nonfinite_same(a, w):
            fails.append("nonfinite_pattern")
        ok = keep.unsqueeze(1) & torch.isfinite(w)
        e = ref["grad_dout_err"] + U32 * w.abs()
        fig["grad_dout_bound_used"] = Mm._used((a - w).abs()[ok], e[ok])
        if fig["grad_dout_bound_used"] > 1.0:
            fails.append("grad_dout_bound")
    if got.get("gW") is not None:
        worst = 0.0
        for l in range(len(ref["gW"])):
            a, w = got["gW"][l].double(), ref["gW"][l]
            if not Mm._nonfinite_same(a, w):
                fails.append("nonfinite_pattern")
            ok = torch.isfinite(w)
            e = ref["gW_err"][l] + U32 * w.abs()
            used = Mm._used((a - w).abs()[ok], e[ok])
            fig[f"gW{l + 1}_bound_used"] = used
            worst = max(worst, used)
        fig["wgrad_bound_used"] = worst
        if worst > 1.0:
            fails.append("wgrad_bound")
    return fig, fails


def as_got(m):
    """A model result standing in for the kernel's (fp32 outputs)."""
    f = (lambda t: t.float().double())
    return dict(grad_dout=f(m["grad_dout"]), gW=[f(t) for t in m["gW"]])
