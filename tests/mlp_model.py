"""Reference models of the field's MLP (include/mi3d.h Part 4) in plain torch, written from the header's contract and
from torch.autocast's semantics for an nn.Linear / ReLU stack - not from the kernels.  They run on CPU or GPU tensors.

  y = W_L relu(... relu(W_1 x + b_1) ...) + b_L,   W_l [out_l, in_l] (nn.Linear layout), 2 or 3 layers

model_fp32   every sum in fp64; with it a RUNNING ERROR BOUND per element for a kernel that evaluates the same sums in
             fp32 in any order: a sum of c terms, each rounded once, is off by at most c 2^-24 times the sum of the
             absolute values of its terms (first order), and nested sums nest the absolute values:
               forward   c 2^-24 (|W_L|(...(|W_1||x| + |b_1|)...) + |b_L|),  c = din + hid (+ hid) + layers
               dx        the same rule down the transposed chain (contraction lengths 4, hid, (hid))
               dW, db    sums over the n rows.  Their depth is the launch geometry of the backward (grid_for in
                         csrc/field.hip: 32 rows per tile on the matrix core, the tiles of a persistent wave added into
                         the same registers, 4 waves per workgroup added in LDS, the workgroups added with float
                         atomics): 32 + tiles per wave + 4 + workgroups (+ 1 for the accumulation into the caller's
                         buffer), with at most 256 x 2 workgroups.  On top of that come the errors of the two factors
                         (the activation's and the hidden gradient's own bounds).
             A ReLU mask may legitimately differ where the fp64 pre-activation lies within its bound of zero: such rows
             are reported (`uncertain_rows`), and in the weight gradients their terms go into the bound (the whole
             upstream gradient of that unit), not out of the sum.
model_half   half_mode: x, W_l, b_l, every layer output, dout and every hidden gradient are rounded to binary16 (round
             to nearest even, directly from fp64); ReLU masks are `activation > 0` on the ROUNDED activations; dx is
             rounded to binary16 when the planes are binary16 (planes_half), otherwise it is the fp64 sum (the kernel
             stores its fp32 accumulator); weight and bias gradients are fp64 sums of products of the rounded factors,
             never rounded.  A NaN activation stays NaN and passes its gradient, as torch.relu does.  The result is determined up to the order of the fp32 accumulation, which can move a sum
             across a rounding boundary: the same interval rule as above, pushed through the roundings, says where.

`acc` = torch.float32 evaluates the SAME model with fp32 matrix products (the reference-alone figures: how far two
correct evaluations may differ).  `faults` seeds one of FAULTS into the model (tests/test_mlp_model_cpu.py: each must
break a named assertion below).

check_fp32 / check_half are the assertions tests/test_mlp_exact_gpu.py makes, as functions of (got, model): they return
the measured figures and the list of assertions that failed, by name.
"""
import math

import torch

U32 = 2.0 ** -24          # unit roundoff of an fp32 sum
ULP16 = 2.0 ** -10        # one binary16 ulp relative to the top of its binade
HALF_MAX = 65504.0

ROWS_PER_TILE, WAVES_PER_WG, CUS = 32, 4, 256
BWD_WGS_PER_CU, FWD_WGS_PER_CU = 2, 5
BWD_LOOPS_ABOVE = CUS * BWD_WGS_PER_CU * WAVES_PER_WG * ROWS_PER_TILE     # 65 536 rows
FWD_LOOPS_ABOVE = CUS * FWD_WGS_PER_CU * WAVES_PER_WG * ROWS_PER_TILE     # 163 840 rows

# the shares the issue sets
MIN_IDENTICAL = 0.98      # half mode: elements of y / dx bit-identical to model_half
MAX_ROWS_LEFT_OUT = 0.01  # rows whose ReLU mask is undecided at the accumulation bound

FAULTS = ("dout_unrounded", "bias_unrounded", "hidden_grad_unrounded", "mask_pre_rounding", "last_row_twice",
          "poison_row", "swap_pairs")


def grid_for(n, wgs_per_cu):
    """csrc/field.hip grid_for: one wave per 32-row tile, 4 waves per workgroup, at most 256 x wgs_per_cu workgroups."""
    tiles = (n + ROWS_PER_TILE - 1) // ROWS_PER_TILE
    wgs = (tiles + WAVES_PER_WG - 1) // WAVES_PER_WG
    return max(1, min(wgs, CUS * wgs_per_cu))


def wgrad_depth(n):
    """Terms one weight-gradient element passes through on its way to memory (see the module docstring)."""
    wgs = grid_for(n, BWD_WGS_PER_CU)
    tiles = (n + ROWS_PER_TILE - 1) // ROWS_PER_TILE
    tiles_per_wave = (tiles + wgs * WAVES_PER_WG - 1) // (wgs * WAVES_PER_WG)
    return ROWS_PER_TILE + tiles_per_wave + WAVES_PER_WG + wgs + 1


def round_half(t):
    """fp64 -> nearest binary16 (ties to even, subnormals, overflow to inf, the sign of zero kept) -> fp64."""
    t = t.double()
    _, e = torch.frexp(t)
    # 2^(e - 11), at least the subnormal quantum 2^-24, built from its bits: torch.ldexp goes through pow(), which is not
    # exact on every device
    q = ((torch.clamp(e - 11, min=-24, max=1000).to(torch.int64) + 1023) << 52).view(torch.float64)
    r = torch.round(t / q) * q
    r = torch.where(r.abs() > HALF_MAX, torch.copysign(torch.full_like(t, math.inf), t), r)
    return torch.where(torch.isfinite(t), r, t)


def _mm(a, b, acc):
    if acc == torch.float64:
        return a @ b
    a, b = a.to(acc), b.to(acc)
    if a.shape[1] > 64:        # a sum over the rows: whatever order torch takes
        return (a @ b).double()
    s = torch.zeros(a.shape[0], b.shape[1], dtype=acc, device=a.device)
    for k in range(a.shape[1]):   # a layer's sum, term by term in index order: the same figures on every machine
        s += a[:, k:k + 1] * b[k]
    return s.double()


def _model(x, layers, dout, half, planes_half, acc, faults):
    faults = set(faults)
    assert faults <= set(FAULTS), faults
    rnd = round_half if half else (lambda t: t)
    L, n = len(layers), x.shape[0]
    x64, g_out = x.double(), dout.double()
    W = [rnd(w.double()) for w, _ in layers]
    b = [(bb.double() if "bias_unrounded" in faults else rnd(bb.double())) for _, bb in layers]

    def spread(s, e):   # how far apart the two ends of [s - e, s + e] land once rounded
        return (rnd(s + e) - rnd(s - e)) if half else e

    # ---- forward
    acts, act_err, mask, undecided, pre, pre_err, nested = [rnd(x64)], [torch.zeros_like(x64)], [], [], [], [], []
    absnet, depth = acts[0].abs(), 0
    for l in range(L):
        fan = W[l].shape[1]
        s = _mm(acts[l], W[l].t(), acc) + b[l]
        depth += fan + 1
        # the running bound: this layer's own fp32 sum over the values it actually adds + what the errors (fp32) or the
        # undecided roundings (half) of the layer below can move.  It decides which ReLU masks are undecided.
        e = (fan + 1) * U32 * (_finite(acts[l]).abs() @ W[l].abs().t() + b[l].abs()) + act_err[l] @ W[l].abs().t()
        absnet = absnet @ W[l].abs().t() + b[l].abs()
        nested.append(depth * U32 * absnet)      # the nested rule of the docstring (never smaller than e in fp32 mode)
        pre.append(s); pre_err.append(e)
        r = rnd(s)
        if l < L - 1:
            # open <=> not (activation <= 0), which is `activation > 0` but for a NaN activation: torch.relu's backward
            # (threshold_backward) passes the gradient there
            m = ~(s <= 0) if "mask_pre_rounding" in faults else ~(r <= 0)
            mask.append(m)
            undecided.append((rnd(s + e) > 0) != (rnd(s - e) > 0))
            r = torch.where((r > 0) | torch.isnan(r), r, torch.zeros_like(r))   # torch.relu: NaN stays NaN
        acts.append(r); act_err.append(spread(s, e))
    y, y_err = acts[L], act_err[L] if half else nested[L - 1]

    # ---- backward
    g = g_out if "dout_unrounded" in faults else rnd(g_out)
    g_err = torch.zeros_like(g)
    sum_depth = wgrad_depth(n)
    dW, db, dW_err, db_err = [None] * L, [None] * L, [None] * L, [None] * L
    dx = dx_err = dx_exact = None
    for l in reversed(range(L)):
        a, a_err = acts[l], act_err[l]
        dW[l] = _mm(g.t(), a, acc)
        db[l] = g.sum(0) if acc == torch.float64 else g.to(acc).sum(0).double()
        ga, aa = _finite(g).abs(), _finite(a).abs()
        dW_err[l] = sum_depth * U32 * (ga.t() @ aa) + g_err.t() @ aa + ga.t() @ a_err + g_err.t() @ a_err
        db_err[l] = sum_depth * U32 * ga.sum(0) + g_err.sum(0)
        if "last_row_twice" in faults:
            dW[l] = dW[l] + g[n - 1:n].t() @ a[n - 1:n]
        if "poison_row" in faults:   # a row past n whose upstream gradient was not zeroed
            dW[l] = dW[l] + torch.full_like(g[:1], 3e4).t() @ torch.full_like(a[:1], 3e4)
        t = _mm(g, W[l], acc)
        c = W[l].shape[0]
        t_err = c * U32 * (ga @ W[l].abs()) + g_err @ W[l].abs()
        if l > 0:
            tr = t if (l == 1 and "hidden_grad_unrounded" in faults) else rnd(t)
            m, und = mask[l - 1], undecided[l - 1]
            sp = spread(t, t_err)
            g = torch.where(m, tr, torch.zeros_like(tr))
            g_err = torch.where(und, _finite(tr).abs() + sp, torch.where(m, sp, torch.zeros_like(sp)))
        else:
            dx_exact, dx_err = t, t_err
            dx = rnd(t) if (half and planes_half) else t
    if "swap_pairs" in faults:
        dx = dx.view(n, -1, 2).flip(-1).reshape(n, -1)
    und_rows = torch.zeros(n, dtype=torch.bool, device=x.device)
    for u in undecided:
        und_rows |= u.any(1)
    return dict(y=y, y_err=y_err, dx=dx, dx_err=dx_err, dx_exact=dx_exact, dW=dW, db=db, dW_err=dW_err, db_err=db_err,
                pre=pre, pre_err=pre_err, uncertain_rows=und_rows, half=half, planes_half=bool(planes_half), n=n)


def _finite(t):
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)


def model_fp32(x, layers, dout, acc=torch.float64, faults=()):
    """layers: [(W_1, b_1), ..., (W_L, b_L)].  Returns a dict: y, dx, dW[l], db[l] (fp64), the pre-activations `pre`,
    the running bounds y_err, dx_err, dW_err[l], db_err[l], pre_err[l], and `uncertain_rows` (see the module docstring)."""
    return _model(x, layers, dout, False, False, acc, faults)


def model_half(x, layers, dout, planes_half, acc=torch.float64, faults=()):
    return _model(x, layers, dout, True, planes_half, acc, faults)


# ------------------------------------------------------------------------------------------------ inputs

SHAPES = [(32, 64, 3), (16, 64, 3), (32, 64, 2), (30, 64, 2), (32, 32, 3), (8, 32, 3), (32, 32, 2), (8, 32, 2), (2, 32, 2)]
DOUT_SIGMA, LAST_ROW_FACTOR, POISON = 16.0, 1000.0, 3e4

# Largest distance, in binary16 ulps of the row's largest model element, at which a non-identical element of y / dx was
# seen between the fp32- and the fp64-accumulating evaluation of model_half on make_case()'s inputs (70 003 rows):
# 0.86 - 1.02 for every shape but 2 -> 32 -> 4, whose two-element dx rows cancel (4.14).  tests/test_mlp_model_cpu.py
# re-measures it and fails if it grows.  The GPU test allows 4 x that: nobody knows the matrix core's internal order.
K_MEASURED = {sh: 1.05 for sh in SHAPES}
K_MEASURED[(2, 32, 2)] = 4.2


def k_cap(din, hid, layers):
    return 4.0 * K_MEASURED[(din, hid, layers)]


def make_case(din, hid, layers, n, seed=0, device="cpu", extra_rows=0):
    """The inputs of the exactness tests: x ~ 0.5 N(0,1), nn.Linear's default initialisation for weights and biases,
    dout ~ 16 N(0,1) cut at 3 sigma - with row n - 1 carrying LAST_ROW_FACTOR times that, so that counting it twice
    would dominate its weight-gradient terms (16 x 3 x 1000 = 48 000 stays finite in binary16; at the issue's 64 sigma
    that row would overflow and the case would test the overflow path instead).
    x and dout get `extra_rows` rows past n filled with POISON, finite and large: whatever leaks from them shows."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * din + hid + layers)
    x = torch.full((n + extra_rows, din), POISON)
    dout = torch.full((n + extra_rows, 4), POISON)
    x[:n] = 0.5 * torch.randn(n, din, generator=gen)
    dout[:n] = (DOUT_SIGMA * torch.randn(n, 4, generator=gen)).clamp(-3 * DOUT_SIGMA, 3 * DOUT_SIGMA)
    dout[n - 1] *= LAST_ROW_FACTOR
    ws = []
    dims = [din] + [hid] * (layers - 1) + [4]
    for l in range(layers):
        k = 1.0 / math.sqrt(dims[l])
        ws.append(((torch.rand(dims[l + 1], dims[l], generator=gen) * 2 - 1) * k,
                   (torch.rand(dims[l + 1], generator=gen) * 2 - 1) * k))
    return x.to(device), [(w.to(device), b.to(device)) for w, b in ws], dout.to(device)


def zero_edge_case(device="cpu", n=5):
    """Hidden units whose pre-activation rounds to zero in binary16: unit 0 to NEGATIVE zero (weight -2^-14, input
    2^-14, zero bias), unit 1 to positive zero from above (weight +2^-14: a mask taken before the rounding would open),
    unit 2 an ordinary open unit on the other input feature.  2 -> 32 -> 4, two layers, every other weight of layer 1
    zero.  torch.relu's backward passes nothing through units 0 and 1: their rows of dW1 and db1 stay zero, dx[:, 0] is
    exactly zero and dx[:, 1] is the control (4 per row)."""
    x = torch.zeros(n, 2); x[:, 0] = 2.0 ** -14; x[:, 1] = 1.0
    W1 = torch.zeros(32, 2); W1[0, 0] = -2.0 ** -14; W1[1, 0] = 2.0 ** -14; W1[2, 1] = 1.0
    b1 = torch.zeros(32)
    W3 = torch.ones(4, 32); b3 = torch.zeros(4)
    dout = torch.ones(n, 4)
    return x.to(device), [(W1.to(device), b1.to(device)), (W3.to(device), b3.to(device))], dout.to(device)


def check_zero_edge(got):
    """Named assertion `zero_unit_gradient`: nothing passes through the two units that rounded to zero."""
    fails = []
    if float(got["dW"][0][:2].abs().max()) != 0.0 or float(got["db"][0][:2].abs().max()) != 0.0 or \
            float(got["dx"][:, 0].abs().max()) != 0.0:
        fails.append("zero_unit_gradient")
    n = got["dx"].shape[0]   # (the control unit; its bias gradient may have been added to a pre-filled buffer in fp32)
    if not bool((got["dx"][:, 1] == 4.0).all()) or abs(float(got["db"][0][2]) - 4.0 * n) > 1e-4 * n:
        fails.append("zero_edge_control")
    return fails


# ------------------------------------------------------------------------------------------------ the assertions

def _used(diff, bound):
    """Largest share of the bound used; an element beyond a zero bound counts as infinite."""
    if diff.numel() == 0:
        return 0.0
    r = torch.where(diff <= bound, diff / torch.clamp(bound, min=1e-300), torch.full_like(diff, math.inf))
    r = torch.where(diff == 0, torch.zeros_like(r), r)
    return float(r.max())


def _nonfinite_same(a, b):
    a, b = a.double(), b.double()
    return bool(((torch.isnan(a) == torch.isnan(b)) & (torch.isposinf(a) == torch.isposinf(b)) &
                 (torch.isneginf(a) == torch.isneginf(b))).all())


def _check_wgrads(got, ref, fig, fails):
    worst = 0.0
    if "dW" not in got:
        return
    for l in range(len(ref["dW"])):
        for nm in ("dW", "db"):
            a, w, e = got[nm][l].double(), ref[nm][l], ref[nm + "_err"][l]
            if not _nonfinite_same(a, w):
                fails.append("nonfinite_pattern")
            ok = torch.isfinite(w)
            e = e + U32 * w.abs()   # the result itself is an fp32 number
            worst = max(worst, _used((a - w).abs()[ok], e[ok]))
    fig["wgrad_bound_used"] = worst
    if worst > 1.0:
        fails.append("wgrad_bound")


def check_fp32(got, ref, forward=True, backward=True):
    """got: dict of y, dx [n, din], dW[l], db[l] (any of the two halves may be absent).  -> (figures, failed names)"""
    fig, fails = {}, []
    n = ref["n"]
    if forward:
        e = ref["y_err"] + U32 * ref["y"].abs()
        fig["y_bound_used"] = _used((got["y"].double() - ref["y"]).abs(), e)
        if fig["y_bound_used"] > 1.0:
            fails.append("y_bound")
    if backward:
        keep = ~ref["uncertain_rows"]
        fig["rows_left_out"] = float((~keep).sum()) / n
        if fig["rows_left_out"] > MAX_ROWS_LEFT_OUT:
            fails.append("rows_left_out")
        e = ref["dx_err"] + U32 * ref["dx"].abs()
        fig["dx_bound_used"] = _used((got["dx"].double() - ref["dx"]).abs()[keep], e[keep])
        if fig["dx_bound_used"] > 1.0:
            fails.append("dx_bound")
        _check_wgrads(got, ref, fig, fails)
    return fig, fails


def _check_half_tensor(name, a, w, keep_rows, k_cap, fig, fails):
    a, w = a.double(), w.double()
    if not _nonfinite_same(a, w):
        fails.append("nonfinite_pattern")
    same = (a == w) | (torch.isnan(a) & torch.isnan(w))     # (+0 == -0: both are "no value", as torch.equal has it)
    fig[name + "_identical"] = float(same.double().mean())
    if fig[name + "_identical"] < MIN_IDENTICAL:
        fails.append(name + "_identical")
    row_max = _finite(w).abs().max(1, keepdim=True).values
    d = _finite(a - w).abs() / torch.clamp(row_max * ULP16, min=2.0 ** -24)   # in ulps of the row's largest element
    d = torch.where(same, torch.zeros_like(d), d)[keep_rows]
    fig[name + "_k"] = float(d.max()) if d.numel() else 0.0
    if fig[name + "_k"] > k_cap:
        fails.append(name + "_k")


def check_half(got, ref, k_cap, forward=True, backward=True):
    """The half-mode assertions.  got["dx"] is what the kernel stored, as numbers: binary16 planes are compared as they
    are (equal numbers = equal bit patterns, but for the sign of zero); an fp32 dx (rows, fp32 planes) is the kernel's
    unrounded accumulator - its binary16 rounding is held to the same count, and the fp32 value itself to the running
    bound of the fp64 sum."""
    fig, fails = {}, []
    n = ref["n"]
    keep = ~ref["uncertain_rows"]
    fig["rows_left_out"] = float((~keep).sum()) / n
    if fig["rows_left_out"] > MAX_ROWS_LEFT_OUT:
        fails.append("rows_left_out")
    if forward:
        _check_half_tensor("y", got["y"], ref["y"], keep, k_cap, fig, fails)
    if backward:
        dx = got["dx"].double()
        if not ref["planes_half"]:
            ok = keep.unsqueeze(1) & torch.isfinite(ref["dx_exact"])
            e = ref["dx_err"] + U32 * ref["dx_exact"].abs()
            fig["dx_bound_used"] = _used((dx - ref["dx_exact"]).abs()[ok], e[ok])
            if fig["dx_bound_used"] > 1.0:
                fails.append("dx_bound")
            dx = round_half(dx)
        _check_half_tensor("dx", dx, round_half(ref["dx_exact"]), keep, k_cap, fig, fails)
        _check_wgrads(got, ref, fig, fails)
    return fig, fails


def as_got(m):
    """A model result standing in for a kernel's (fp32 outputs)."""
    f = (lambda t: t.float().double())
    return dict(y=f(m["y"]), dx=f(m["dx"]), dW=[f(t) for t in m["dW"]], db=[f(t) for t in m["db"]])


def check_nonfinite(got, ref, forward=True, backward=True):
    """Named assertions `nonfinite_pattern:<tensor>`: NaN, +inf and -inf sit exactly where the model has them."""
    pairs = []
    if forward:
        pairs.append(("y", got["y"], ref["y"]))
    if backward:
        pairs.append(("dx", got["dx"], ref["dx"]))
        for l in range(len(ref["dW"])):
            pairs += [(f"dW{l + 1}", got["dW"][l], ref["dW"][l]), (f"db{l + 1}", got["db"][l], ref["db"][l])]
    return [f"nonfinite_pattern:{nm}" for nm, a, w in pairs if not _nonfinite_same(a, w)]


def nonfinite_case(kind, din, hid, layers, device="cpu", n=100):
    """Ordinary data that leaves binary16's range.  "x": one input above 65 504 (inf once rounded, as autocast's cast
    makes it); "dout": one upstream row that overflows binary16 (the step GradScaler's overflow check then skips)."""
    x, ws, dout = make_case(din, hid, layers, n, seed=9, device=device)
    if kind == "x":
        x[5, 1] = 7e4
    else:
        dout[7] = torch.tensor([1e5, -2e5, 3e5, 1.0], device=dout.device)
    return x, ws, dout
