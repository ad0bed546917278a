"""Reference model of the field head (mi3d_field_head_forward / _backward, include/mi3d.h Part 5) in plain torch, written
from the header's contract and the reference's three functions - trunc_exp (exp forward, its derivative evaluated at
min(u, 15)), safe_normalize (v / sqrt(clamp(|v|^2, 1e-20, 1e32))) and torch.nan_to_num over the finite-difference normal -
not from the kernel.  It runs on CPU tensors.

  u_p     = h_p[0] + blob_density exp(-|clamp(base_p + offsets_p, -bound, bound)|^2 / two_r2)     base: x (p < 7), x2 (p >= 7)
  sigma   = exp(u_0)                     albedo = 1 / (1 + exp(-h_0[1..3]))
  v_d     = -(exp(u_+d) - exp(u_-d)) inv_2eps,   c = clamp(|v|^2, 1e-20, 1e32),   y = v / sqrt(c),   normal = nan_to_num(y)
  dh      [P_active n, 4], point-major: row 0 = (dsigma exp(min(u_0, 15)), dalbedo a (1 - a)), rows 1.. = (du_p, 0, 0, 0)

THE CONSTANTS are the floats the ABI computes on the host: two_r2 = float(2 r r) evaluated in binary64 and rounded once,
inv_2eps = 0.5f / epsilon.  They carry no error of their own.  The clamp's two edges are the decimal numbers of the
contract; a binary32 evaluation holds them rounded, so each carries 2^-24 relative.

THE VALUES are binary64.  The backward is written operation by operation as torch's graph of the composition evaluates it
(nan_to_num: grad * isfinite(y); division: grad / d and -grad (y / d); sqrt: grad / (2 d); clamp: where(inside, grad, 0);
v * v: grad v + grad v), because in the overflow regime the order decides which 0 * inf become NaN: that pattern is the
contract ("pass gradients exactly where torch's do").  To have binary32's pattern and not binary64's, every exponential and
the difference quotient are rounded to the binary32 RANGE (beyond FLT_MAX: +-inf); nothing else can overflow or the clamp
hides it (|v|^2 = inf and |v|^2 = 1e60 both give c = 1e32 and the same closed gate).

THE BOUNDS are running error bounds by tests/mlp_model.py's rule - every binary32 operation is rounded once, 2^-24 of its
result, and the bounds are nested down the chain - kept per element by a small error arithmetic (class V):
  a + b      e_a + e_b + min(2^-24 |a + b|, |a|, |b|)       (the nearest float is no further than either operand)
  a b, a / b first-order propagation + 2^-24 |result| + 2^-149 (a product or quotient can underflow)
  sqrt       correctly rounded, as the division: 2^-24
  exp        |result| expm1(e_a) + 2^-23 |result| + 2^-149: one ulp, the documented accuracy of the HIP math API's expf
  clamp, min 1-Lipschitz: the bound of the argument; decidedly outside, the edge's own 2^-24
A fused multiply-add removes one rounding of a product-and-sum, so the count covers the contracted and the plain code.  The
quotient v / sqrt(c) is counted as reciprocal and product (one rounding more than the division), and the backward as
  dv = r dn - k v,   k = [1e-20 <= |v|^2 <= 1e32] (dn . v) (r / c),   r = 1 / sqrt(c)
which is the graph above with its sums collected; where dn is parallel to the normal the two terms cancel and the bound
stays at the terms' size.  No constant here comes from what a kernel was seen to do.

UNDECIDED ROWS.  The forward is continuous in every decision it takes, so no forward element is ever left out.  The
backward has one discontinuous decision per normal, the clamp's gate.  A normal whose binary64 |v|^2 lies within its own
bound (plus the edge's rounding) of 1e-20 or 1e32 is undecided; its six rows of dh, and only those, may be left out.

`acc` = torch.float32 evaluates the same model with binary32 operations (how far two correct evaluations may differ);
`faults` seeds one of FAULTS (tests/test_head_model_cpu.py: each must break the assertion FAULT_BREAKS names).
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
SUB32 = 2.0 ** -149
FLT_MAX = 3.4028234663852886e38
LO, HI = 1e-20, 1e32
DERIV_CLAMP = 15.0
SENTINEL = 7.0
PAD_ROWS = 3                  # sentinel rows behind dh
MAX_UNDECIDED = 0.02          # share of the samples whose clamp gate may be undecided (the straddling block only)

# (bound, epsilon, blob_density, blob_radius)
PARAMS = ((1.0, 1e-2, 5.0, 0.1), (2.0, 5e-3, 0.0, 0.1), (1.5, 1e-2, 10.0, 0.5))
SIGNS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)

FAULTS = ("dexp_unclamped", "blob_unclamped", "blob2_around_x", "inv_eps", "axis_pair_swapped", "mask_on_c", "k_over_c",
          "nan_to_num_mask_dropped", "sigmoid_deriv_a", "neighbour_cols_nonzero", "last_row_skipped", "last_row_twice")
# mask_on_c is the clamp's gate applied to c instead of |v|^2 (the strict gate differs only where |v|^2 equals an edge to the
# bit - an undecided row by definition - so it cannot be seeded observably).
# nan_to_num_mask_dropped breaks NOTHING, and cannot: y_d is non-finite only where v_d or r is.  A non-finite r (c = NaN)
# makes every component NaN with or without the mask; a non-finite v_d makes |v|^2 non-finite, the clamp's gate closed, so
# no other component sees dn_d, and its own gradient is r dn_d - 0 v_d = NaN whatever finite dn_d is.  (v r cannot overflow
# from finite factors either: r <= 1e10 only while |v| < 1e-10.)  With finite upstream gradients the mask is unobservable
# in dh; tests/test_head_model_cpu.py asserts exactly that - the seeded model returns the same bits - rather than drop it.
FAULT_BREAKS = {"dexp_unclamped": "dh_bound", "blob_unclamped": "sigma_bound", "blob2_around_x": "normal2_bound",
                "inv_eps": "normal_bound", "axis_pair_swapped": "normal_bound", "mask_on_c": "dh_bound",
                "k_over_c": "dh_bound", "nan_to_num_mask_dropped": None, "sigmoid_deriv_a": "dh_bound",
                "neighbour_cols_nonzero": "neighbour_cols_zero", "last_row_skipped": "dh_bound",
                "last_row_twice": "sentinel_rows"}

# named blocks of head_cases and their share of the rows
BLOCKS = (("well", 0.20), ("near", 0.20), ("zero", 0.04), ("empty", 0.20), ("straddle", 0.02), ("above", 0.06),
          ("around15", 0.06), ("overflow1", 0.03), ("overflow2", 0.03), ("box", 0.08), ("blob", 0.08))
NONFINITE_BLOCKS = ("overflow1", "overflow2")


def host_constants(blob_radius, epsilon):
    """(two_r2, inv_2eps) as the ABI computes them from its float arguments."""
    r = float(np.float32(blob_radius))
    return float(np.float32(2.0 * r * r)), float(np.float32(0.5) / np.float32(epsilon))


def stencil(P, epsilon):
    """[P, 3] float32 offsets: the sample, its six +-epsilon neighbours (+x, -x, +y, -y, +z, -z), the same six again."""
    six = SIGNS * np.float32(epsilon)
    return np.concatenate([np.zeros((1, 3), np.float32), six] + ([six] if P == 13 else []), 0)


# ------------------------------------------------------------------------------------------------ the error arithmetic

def _abs(t):
    t = t.double().abs()
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


class V:
    """A value (dtype `acc`) and the running bound (binary64) of a binary32 evaluation's distance from its binary64 value.
    A non-finite value has no bound: it is compared as a pattern."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        e = torch.zeros(v.shape, dtype=torch.float64) if e is None else e
        e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)       # 0 * inf: no bound
        self.e = torch.where(torch.isfinite(v.double()), e, torch.zeros_like(e))

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])


def const(c, acc):
    return V(torch.tensor(c, dtype=acc))


def add(a, b, sign=1.0):
    v = a.v + b.v if sign > 0 else a.v - b.v
    e = a.e + b.e
    rnd = torch.minimum(U32 * (_abs(v) + e), torch.minimum(_abs(a.v) + a.e, _abs(b.v) + b.e))
    return V(v, e + rnd)


def sub(a, b):
    return add(a, b, -1.0)


def neg(a):
    return V(-a.v, a.e)


def mul(a, b):
    v = a.v * b.v
    e = _abs(a.v) * b.e + _abs(b.v) * a.e + a.e * b.e
    return V(v, e + U32 * (_abs(v) + e) + SUB32)


def div(a, b):
    v = a.v / b.v
    low = _abs(b.v) - b.e
    e = (a.e + _abs(v) * b.e) / low
    e = torch.where(low > 0, e, torch.full_like(e, math.inf))
    return V(v, e + U32 * (_abs(v) + e) + SUB32)


def sqrt_(a):
    v = torch.sqrt(a.v)
    e = _abs(v) - torch.sqrt(torch.clamp(_abs(a.v) - a.e, min=0.0))
    return V(v, e + U32 * (_abs(v) + e))


def to_range(a):
    """Round to the binary32 RANGE: beyond FLT_MAX the value is +-inf (a no-op on binary32 values)."""
    v = torch.where(a.v.abs() > FLT_MAX, torch.copysign(torch.full_like(a.v, math.inf), a.v), a.v)
    return V(v, a.e)


def exp_(a, ranged=True):
    v = torch.exp(a.v)
    e = _abs(v) * torch.expm1(a.e)
    out = V(v, e + 2 * U32 * (_abs(v) + e) + SUB32)
    return to_range(out) if ranged else out


def sum3(t, dim):
    """A sum of three terms in any order: two additions, each 2^-24 of at most the sum of the absolute values."""
    e = t.e.sum(dim)
    return V(t.v.sum(dim), e + 2 * U32 * (_abs(t.v).sum(dim) + e))


def fmin_(a, c):
    return V(torch.clamp(a.v, max=c), a.e)


# ------------------------------------------------------------------------------------------------ the model

def _pre(h0, x, x2, offs, bound, density, two_r2, acc, faults):
    """u [P, n] = h_p[0] + blob at the clamped stencil point (header Part 5)."""
    P, n = h0.shape
    base = x.to(acc).unsqueeze(0).expand(P, n, 3)
    if P == 13:
        b2 = x if "blob2_around_x" in faults else x2
        base = torch.cat([base[:7], b2.to(acc).unsqueeze(0).expand(6, n, 3)], 0)
    q = add(V(base), V(torch.from_numpy(np.ascontiguousarray(offs)).to(acc).unsqueeze(1).expand(P, n, 3)))
    if "blob_unclamped" not in faults:
        q = V(torch.clamp(q.v, -bound, bound), q.e)
    d2 = sum3(mul(q, q), -1)
    g = mul(const(density, acc), exp_(div(neg(d2), const(two_r2, acc))))
    # neighbours p, p + 1 of one axis with the same h and the same |coordinates| (an offset pair around 0) pass through the
    # same operations on the same numbers: whatever the evaluation, their sigmas are the same float
    twin = torch.zeros(P, n, dtype=torch.bool)
    for p in range(1, P, 2):
        twin[p] = twin[p + 1] = (h0[p] == h0[p + 1]) & (q.v[p].abs() == q.v[p + 1].abs()).all(-1)
    return add(V(h0.to(acc)), g), twin


def _normal_forward(s, twin, inv, acc, faults):
    sp, sm = s[0::2], s[1::2]                       # [3, n]: the + and the - neighbour of each axis
    if "axis_pair_swapped" in faults:
        pv, mv, pe, me = sp.v.clone(), sm.v.clone(), sp.e.clone(), sm.e.clone()
        pv[1], mv[1], pe[1], me[1] = sm.v[1], sp.v[1], sm.e[1], sp.e[1]
        sp, sm = V(pv, pe), V(mv, me)
    diff = sub(sp, sm)
    diff = V(diff.v, torch.where(twin[0::2] & (diff.v == 0), torch.zeros_like(diff.e), diff.e))
    v = to_range(neg(mul(diff, const(inv, acc))))
    ss = sum3(mul(v, v), 0)
    cv = torch.clamp(ss.v, LO, HI)                  # torch.clamp hands a NaN on
    below = ss.v.double() + ss.e < LO * (1 - U32)
    above = ss.v.double() - ss.e > HI * (1 + U32)
    c = V(cv, torch.where(below, torch.full_like(ss.e, U32 * LO),
                          torch.where(above, torch.full_like(ss.e, U32 * HI), ss.e + U32 * _abs(cv))))
    undecided = torch.isfinite(ss.v.double()) & (((ss.v.double() - LO).abs() <= ss.e + U32 * LO) |
                                                 ((ss.v.double() - HI).abs() <= ss.e + U32 * HI))
    d = sqrt_(c)
    r = div(const(1.0, acc), d)
    y = to_range(mul(v, r))
    nv = torch.nan_to_num(y.v, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)
    return dict(v=v, ss=ss, c=c, d=d, r=r, y=y, n=V(nv, y.e), undecided=undecided)


def _normal_backward(f, u, dn, inv, acc, faults):
    """du [6, n] and its bound from the upstream gradient dn [3, n] of the nan_to_num'ed normal."""
    v, ss, c, d, r, y = f["v"], f["ss"], f["c"], f["d"], f["r"], f["y"]
    fin = torch.isfinite(y.v)
    inside = (ss.v >= LO) & (ss.v <= HI)
    if "mask_on_c" in faults:
        inside = (c.v >= LO) & (c.v <= HI)
    # ---- the values: torch's graph, operation by operation
    gy = dn if "nan_to_num_mask_dropped" in faults else dn * fin
    gd = (-gy * ((v.v / d.v) / d.v)).sum(0)
    gc = gd / 2 if "k_over_c" in faults else gd / (2 * d.v)
    gss = torch.where(inside, gc, torch.zeros_like(gc))
    gv = gy / d.v + (gss * v.v + gss * v.v)
    E = exp_(fmin_(u, math.inf if "dexp_unclamped" in faults else DERIV_CLAMP))
    gdiff = -gv * inv
    du = torch.stack([gdiff, -gdiff], 1).reshape(6, -1) * E.v
    # ---- the bound: dv = r dn - k v down the same chain
    dnm = V(torch.where(fin, dn, torch.zeros_like(dn)))
    dot = sum3(mul(dnm, v), 0)
    k = mul(dot, div(r, c))
    k = V(torch.where(inside, k.v, torch.zeros_like(k.v)), torch.where(inside, k.e, torch.zeros_like(k.e)))
    dg = mul(sub(mul(r, dnm), mul(k, v)), const(inv, acc))
    e = torch.stack([dg.e, dg.e], 1).reshape(6, -1)
    dgv = torch.stack([dg.v, dg.v], 1).reshape(6, -1)
    return du, mul(V(dgv, e), E).e


def head(h, x, x2, offsets, bound, blob_density, blob_radius, epsilon, dsigma=None, dalbedo=None, dnormal=None,
         dnormal2=None, P_active=None, acc=torch.float64, faults=()):
    """h [P n, 4] point-major, x / x2 [n, 3], offsets [P, 3] (numpy float32); the upstream gradients may be None (= zeros).
    -> dict of sigma [n], albedo / normal / normal2 [n, 3], dh [P_active n, 4] (binary64) with `<name>_err` beside each,
    `undecided` [K, n] per normal, `undecided_rows` [P_active n] and |v|^2 with its bound (`ss`, `ss_err`: [K, n])."""
    faults = set(faults)
    assert faults <= set(FAULTS), faults
    offs = np.asarray(offsets, np.float32).reshape(-1, 3)
    P, n = offs.shape[0], x.shape[0]
    assert P in (7, 13) and h.shape == (P * n, 4) and (P == 7 or x2 is not None)
    P_active = P if P_active is None else P_active
    assert P_active in (1, 7, 13) and P_active <= P
    two_r2, inv = host_constants(blob_radius, epsilon)
    if "inv_eps" in faults:
        inv = 2 * inv
    bound, density = float(np.float32(bound)), float(np.float32(blob_density))
    hv = h.view(P, n, 4)
    u, twin = _pre(hv[..., 0], x, x2, offs, bound, density, two_r2, acc, faults)
    sig = exp_(u)
    one = const(1.0, acc)
    # the sigmoid is continuous where exp(-h) leaves the binary32 range: the quotient is an exact zero there and the number
    # it stands for lies below 1 / FLT_MAX - a bound, not a pattern
    ex = exp_(neg(V(hv[0, :, 1:].to(acc))), ranged=False)
    a = div(one, add(one, ex))
    a = V(a.v, a.e + torch.where(ex.v.double() > FLT_MAX, 1.0 / FLT_MAX, 0.0))
    out = dict(n=n, P=P, P_active=P_active, sigma=sig.v[0].double(), sigma_err=sig.e[0], albedo=a.v.double(),
               albedo_err=a.e)
    K = 2 if P == 13 else 1
    fwd = [_normal_forward(sig[1 + 6 * k:7 + 6 * k], twin[1 + 6 * k:7 + 6 * k], inv, acc, faults) for k in range(K)]
    for k, name in enumerate(("normal", "normal2")[:K]):
        out[name], out[name + "_err"] = fwd[k]["n"].v.t().double(), fwd[k]["n"].e.t()
    out["ss"] = torch.stack([f["ss"].v.double() for f in fwd])
    out["ss_err"] = torch.stack([f["ss"].e for f in fwd])
    out["undecided"] = torch.stack([f["undecided"] for f in fwd])

    # ---- backward
    def up(t, shape):
        return torch.zeros(shape, dtype=acc) if t is None else t.to(acc)
    dh = torch.zeros(P_active, n, 4, dtype=torch.float64)
    dh_err = torch.zeros(P_active, n, 4, dtype=torch.float64)
    g0 = mul(V(up(dsigma, (n,))), exp_(fmin_(u[0], math.inf if "dexp_unclamped" in faults else DERIV_CLAMP)))
    da = V(up(dalbedo, (n, 3)))
    ga = mul(da, a) if "sigmoid_deriv_a" in faults else mul(mul(da, a), sub(one, a))
    dh[0, :, 0], dh_err[0, :, 0] = g0.v.double(), g0.e
    dh[0, :, 1:], dh_err[0, :, 1:] = ga.v.double(), ga.e
    und_rows = torch.zeros(P_active, n, dtype=torch.bool)
    for k, dn in enumerate((dnormal, dnormal2)[:K]):
        if P_active < 7 + 6 * k:
            break
        du, du_err = _normal_backward(fwd[k], u[1 + 6 * k:7 + 6 * k], up(dn, (n, 3)).t(), inv, acc, faults)
        dh[1 + 6 * k:7 + 6 * k, :, 0], dh_err[1 + 6 * k:7 + 6 * k, :, 0] = du.double(), du_err
        und_rows[1 + 6 * k:7 + 6 * k] = fwd[k]["undecided"]
        if "neighbour_cols_nonzero" in faults:
            dh[1 + 6 * k:7 + 6 * k, :, 1] = du.double()
    dh_err = torch.where(torch.isfinite(dh), dh_err, torch.zeros_like(dh_err))
    out["overrun"] = None
    if "last_row_skipped" in faults:                 # sample n - 1 keeps whatever the buffers held
        for name in ("sigma", "albedo", "normal", "normal2")[:2 + K]:
            out[name] = out[name].clone()
            out[name][n - 1] = SENTINEL
        dh[:, n - 1] = SENTINEL
    if "last_row_twice" in faults:                   # a thread for sample n: point-major, it lands on the next point's row 0
        out["overrun"] = dh[:, n - 1].clone()
    out.update(dh=dh.view(P_active * n, 4), dh_err=dh_err.view(P_active * n, 4), undecided_rows=und_rows.view(-1))
    return out


# ------------------------------------------------------------------------------------------------ inputs

def block_rows(n):
    """{name: (lo, hi)}: the named blocks' rows; a block too small for n holds none."""
    edges, acc_f = [0], 0.0
    for _, f in BLOCKS:
        acc_f += f
        edges.append(int(math.floor(acc_f * n + 1e-9)))
    edges[-1] = n
    return {name: (edges[i], edges[i + 1]) for i, (name, _) in enumerate(BLOCKS)}


def _blob64(x, x2, offs, bound, density, two_r2):
    """The blob term of every stencil point in binary64 [P, n] (the model's own forward, without its bounds)."""
    P, n = offs.shape[0], x.shape[0]
    return _pre(torch.zeros(P, n), x, x2, offs, bound, density, two_r2, torch.float64, ())[0].v


def _ss64(h6, g6, inv):
    """|v|^2 in binary64 of six neighbour rows h6 [6, m] with their blob terms g6."""
    s = torch.exp(h6.double() + g6)
    v = (s[0::2] - s[1::2]) * inv
    return (v * v).sum(0)


def _tune(h6, g6, inv, row, target, below):
    """Move h6[row] (float32) so that |v|^2 is the nearest it can be to `target` from below (or from above): bisection on
    the real line, then the neighbouring float on the side asked for."""
    lo = h6[row ^ 1].double() + g6[row ^ 1] - g6[row]       # the partner's pre-activation: this axis adds nothing
    hi = lo + 3.0
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        t = h6.double().clone()
        t[row] = mid
        up = _ss64(t, g6, inv) < target
        lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
    out = h6.clone()
    out[row] = lo.float()
    for _ in range(3):
        ss = _ss64(out, g6, inv)
        wrong = (ss > target) if below else (ss < target)
        step = torch.full_like(out[row], -math.inf if below else math.inf)
        out[row] = torch.where(wrong, torch.nextafter(out[row], step), out[row])
    return out


def head_cases(seed, n, P, params=PARAMS[0]):
    """The inputs the CPU and the GPU tests share, as CPU float32 tensors: h [P n, 4], x, x2 (None for P = 7), offsets
    [P, 3] (numpy), the four upstream gradients and `blocks` {name: (lo, hi)}.  Each block's rows lie decidedly on their
    side of the threshold the block is named for; `straddle` alone may hold undecided rows.
      well       neighbours differ by order 1 in h: bounds of order 1e-6, where a subtle fault shows; in its first quarter
                 the upstream gradient is parallel to the normal (the projection cancels)
      near       neighbours within about 0.01 of the centre value
      zero       identical pre-activations, x = x2 = 0: |v|^2 = 0 exactly
      empty      centre near -26, |v|^2 in (0, 1e-20): empty space
      straddle   |v|^2 around 1e-20; half of its rows tuned to the float nearest the edge, from either side
      above      |v|^2 > 1e32 with v finite: pre-activations 36.5 .. 39 (|v|^2 finite in binary32) and 40 .. 80 (not)
      around15   pre-activations below, above and - where the blob term vanishes - exactly at trunc_exp's derivative clamp
      overflow1  one neighbour at 100: sigma = inf, v = -+inf, FLT_MAX out of nan_to_num
      overflow2  both neighbours of one axis at 100: inf - inf = NaN
      box        samples on and beyond the box: the stencil's clamp changes the blob
      blob       samples inside the blob"""
    bound, eps, density, radius = params
    two_r2, inv = host_constants(radius, eps)
    gen = torch.Generator().manual_seed(100003 * seed + 13 * n + P)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    nrm = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)     # noqa: E731
    K = 2 if P == 13 else 1
    offs = stencil(P, eps)
    blocks = block_rows(n)
    sl = {k: slice(*v) for k, v in blocks.items()}

    x = (rnd(n, 3) * 2 - 1) * 0.9 * bound
    jitter = 0.01 * nrm(n, 3)
    x[sl["blob"]] *= 0.5 * radius / bound
    jitter[sl["blob"]] *= 30 * radius
    lo, hi = blocks["box"]
    for i, s in enumerate(range(lo, hi)):
        x[s, i % 3] = (1.0 if i % 2 else -1.0) * bound * (1.0 if i % 4 < 2 else 1.0 + 0.2 * float(rnd(1)))
    x[sl["zero"]] = 0.0
    jitter[sl["zero"]] = 0.0
    x2 = (x + jitter).float() if P == 13 else None
    x = x.float()

    # ---- the pre-activations asked for: centre uc [n], neighbours un [K, 6, n]
    uc = 0.5 * nrm(n)
    un = 0.5 * nrm(K, 6, n)
    s_ = sl["near"]
    un[:, :, s_] = uc[s_] + 0.01 * 0.5 * nrm(K, 6, s_.stop - s_.start)
    s_ = sl["zero"]
    un[:, :, s_] = uc[s_]
    s_ = sl["empty"]
    m = s_.stop - s_.start
    uc[s_] = -27 + 2 * rnd(m)
    un[:, :, s_] = uc[s_] + 0.02 * (2 * rnd(K, 6, m) - 1)
    s_ = sl["straddle"]
    m = s_.stop - s_.start
    uc[s_] = -25.0
    un[:, :, s_] = -25.0
    # the x axis alone carries |v|^2 = t 1e-20, t log-uniform in [0.3, 3]; the tuned half is moved below
    t = torch.exp(math.log(0.3) + math.log(10.0) * rnd(K, m))
    un[:, 0, s_] = -25.0 + torch.log1p(torch.sqrt(t * LO) / (inv * math.exp(-25.0)))
    s_ = sl["above"]
    m = s_.stop - s_.start
    big = torch.arange(m) % 2 == 0
    uc[s_] = torch.where(big, 40 + 39.5 * rnd(m), 37 + 1.5 * rnd(m))
    un[:, :, s_] = uc[s_] + torch.where(big, 0.5, 0.3) * (2 * rnd(K, 6, m) - 1)
    un[:, 0, s_] = uc[s_] + 0.5
    un[:, 1, s_] = uc[s_] - 0.5
    s_ = sl["around15"]
    m = s_.stop - s_.start
    kind = torch.arange(m) % 3
    uc[s_] = torch.where(kind == 0, 13 + 1.9 * rnd(m), torch.where(kind == 1, 15.1 + 1.9 * rnd(m), torch.full((m,), 15.0)))
    un[:, :, s_] = 15.0 + 0.6 * nrm(K, 6, m)
    un[:, 0, s_] = torch.where(kind == 2, torch.full((m,), 15.0), un[0, 0, s_])
    for name, both in (("overflow1", False), ("overflow2", True)):
        lo, hi = blocks[name]
        for i, s in enumerate(range(lo, hi)):
            if both:
                un[:, 2 * (i % 3), s] = 100.0
                un[:, 2 * (i % 3) + 1, s] = 100.0
            else:
                un[:, i % 6, s] = 100.0
            if i % 4 == 3:
                uc[s] = 100.0                        # sigma itself overflows

    g = _blob64(x, x2, offs, float(np.float32(bound)), float(np.float32(density)), two_r2)      # [P, n]
    h = nrm(P, n, 4)
    h[0, :, 0] = uc - g[0]
    h[1:, :, 0] = un.reshape(6 * K, n) - g[1:]
    alb = 2.0 * nrm(n, 3)
    alb[1::7] = 20.0
    alb[2::7] = -20.0
    alb[3::7, 0] = 95.0                              # exp(-h) underflows / overflows: the sigmoid saturates
    alb[3::7, 1] = -95.0
    h[0, :, 1:] = alb
    h = h.float()
    s_ = sl["zero"]
    h[1:7, s_, 0] = h[1:2, s_, 0]
    if P == 13:
        h[7:13, s_, 0] = h[7:8, s_, 0]
    # the tuned half of the straddling block: the x axis to just below (1 - 5e-5) of the edge, then the z axis (3e-7 of the
    # edge per float) to the float nearest the edge - alternately the last one below and the first one above it
    lo, hi = blocks["straddle"]
    rows = torch.arange(lo, hi)[::2]
    if len(rows):
        for k in range(K):
            p0 = 1 + 6 * k
            h6, g6 = h[p0:p0 + 6, rows, 0].clone(), g[p0:p0 + 6, rows]
            h6 = _tune(h6, g6, inv, 0, (1 - 5e-5) * LO, True)
            even = torch.arange(len(rows)) % 2 == 0
            a = _tune(h6, g6, inv, 4, LO, True)
            b = _tune(h6, g6, inv, 4, LO, False)
            h[p0:p0 + 6, rows, 0] = torch.where(even, a, b)

    case = dict(h=h.reshape(P * n, 4).contiguous(), x=x.contiguous(), x2=None if x2 is None else x2.contiguous(),
                offsets=offs, blocks=blocks, params=params, n=n, P=P,
                dsigma=nrm(n).float(), dalbedo=nrm(n, 3).float(), dnormal=nrm(n, 3).float(),
                dnormal2=nrm(n, 3).float() if P == 13 else None)
    lo, hi = blocks["well"]
    q = lo + (hi - lo + 3) // 4
    if q > lo:
        f = head(case["h"], case["x"], case["x2"], offs, *_abi(params))
        case["dnormal"][lo:q] = (1.7 * f["normal"][lo:q]).float()
        if P == 13:
            case["dnormal2"][lo:q] = (-0.6 * f["normal2"][lo:q]).float()
    return case


def _abi(params):
    """(bound, blob_density, blob_radius, epsilon): the order of the C ABI, from PARAMS' (bound, epsilon, density, radius)."""
    bound, eps, density, radius = params
    return bound, density, radius, eps


def model_of(case, P_active=None, grads=("dsigma", "dalbedo", "dnormal", "dnormal2"), acc=torch.float64, faults=()):
    """The model on a case of head_cases, with the named upstream gradients (the others None)."""
    g = {k: (case[k] if k in grads else None) for k in ("dsigma", "dalbedo", "dnormal", "dnormal2")}
    return head(case["h"], case["x"], case["x2"], case["offsets"], *_abi(case["params"]), P_active=P_active, acc=acc,
                faults=faults, **g)


# ------------------------------------------------------------------------------------------------ the assertions

FORWARD = ("sigma", "albedo", "normal", "normal2")


def pattern(t):
    """1 NaN, 2 +inf, 3 -inf, 4 +FLT_MAX, 5 -FLT_MAX, 6 exact zero, 0 anything else."""
    t = t.double()
    code = torch.zeros(t.shape, dtype=torch.int8)
    for c, m in ((1, torch.isnan(t)), (2, t == math.inf), (3, t == -math.inf), (4, t == FLT_MAX), (5, t == -FLT_MAX),
                 (6, t == 0)):
        code[m] = c
    return code


def pattern_differs(a, w, e):
    """Elements whose pattern differs from the model's.  An exact zero against a number within its bound of zero (1 - a
    of a saturated sigmoid, say) is a rounding, not a pattern."""
    pa, pw = pattern(a), pattern(w)
    rounding = ((pa == 6) & (pw == 0) | (pa == 0) & (pw == 6)) & ((a.double() - w.double()).abs() <= e)
    return (pa != pw) & ~rounding


def _ratio(a, w, e):
    """|a - w| / e per element: 0 where they agree, inf where a non-zero difference meets no bound or is not a number."""
    d = (a.double() - w).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / e)
    same = (a.double() == w) | (torch.isnan(a.double()) & torch.isnan(w))
    r = torch.where(same, torch.zeros_like(r), r)
    return torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)


def _per_block(r, blocks, n):
    """The worst ratio per block of a [rows, ...] tensor of ratios; rows are samples, or point-major dh rows."""
    r = r.reshape(r.shape[0], -1).amax(1) if r.numel() else r.reshape(r.shape[0])
    r = r.view(-1, n).amax(0) if r.shape[0] != n else r
    return {name: float(r[lo:hi].max()) for name, (lo, hi) in blocks.items() if hi > lo}


def check(got, ref, blocks):
    """got: dict of any of sigma, albedo, normal, normal2 (float32 CPU tensors) and dh (the whole buffer, PAD_ROWS sentinel
    rows behind P_active n).  -> (figures, names of the failed assertions).  `figures[<output>]` is the worst share of a
    bound used, `figures["blocks"][<block>][<output>]` the same per block."""
    n = ref["n"]
    fig, fails = {"blocks": {name: {} for name, (lo, hi) in blocks.items() if hi > lo}}, []
    nf = torch.zeros(n, dtype=torch.bool)
    for name in NONFINITE_BLOCKS:
        nf[slice(*blocks[name])] = True
    und = ref["undecided"].any(0)
    fig["undecided_share"] = float(und.sum()) / n
    if fig["undecided_share"] > MAX_UNDECIDED:
        fails.append("undecided_cap")
    inside = torch.zeros(n, dtype=torch.bool)
    inside[slice(*blocks["straddle"])] = True
    if bool((und & ~inside).any()):
        fails.append("undecided_outside_straddle")

    def one(name, a, w, e, keep=None):
        if a.shape != w.shape:
            fails.append(name + "_bound")
            return
        rows_nf = nf if w.shape[0] == n else nf.repeat(w.shape[0] // n)
        pa, pw, differs = pattern(a), pattern(w), pattern_differs(a, w, e)
        bad = differs & rows_nf.view(-1, *[1] * (w.dim() - 1))
        bad |= differs & ((pa > 0) & (pa < 6) | (pw > 0) & (pw < 6))         # a non-finite value or FLT_MAX: anywhere
        if keep is not None:
            bad &= keep.view(-1, *[1] * (w.dim() - 1))
        if bool(bad.any()) and "nonfinite_pattern" not in fails:
            fails.append("nonfinite_pattern")
        r = _ratio(a, w, e)
        if keep is not None:
            r = torch.where(keep.view(-1, *[1] * (w.dim() - 1)), r, torch.zeros_like(r))
        fig[name] = float(r.max()) if r.numel() else 0.0
        for b, val in _per_block(r, blocks, n).items():
            fig["blocks"][b][name] = val
        if fig[name] > 1.0:
            fails.append(name + "_bound")

    for name in FORWARD:
        if got.get(name) is not None and name in ref:
            one(name, got[name], ref[name], ref[name + "_err"])
    if got.get("dh") is not None:
        rows = ref["dh"].shape[0]
        buf = got["dh"]
        if buf.shape[0] < rows + 1 or not bool((buf[rows:] == SENTINEL).all()):
            fails.append("sentinel_rows")
        dh = buf[:rows]
        one("dh", dh, ref["dh"], ref["dh_err"], keep=~ref["undecided_rows"])
        if rows > n and not bool((dh[n:, 1:] == 0).all()):
            fails.append("neighbour_cols_zero")
    return fig, fails


def as_got(m):
    """A model result standing in for the kernel's: float32 outputs, dh in a buffer with PAD_ROWS sentinel rows behind."""
    out = {name: m[name].float() for name in FORWARD if name in m}
    rows, n = m["dh"].shape[0], m["n"]
    buf = torch.full((rows + PAD_ROWS, 4), SENTINEL)
    buf[:rows] = m["dh"].float()
    if m.get("overrun") is not None:
        for p in range(m["P_active"]):
            buf[(p + 1) * n] = m["overrun"][p].float()
    out["dh"] = buf
    return out


def worst(fig):
    """One line for an assertion message: the worst ratio per output, and per block."""
    head_ = ", ".join(f"{k} {v:.3g}" for k, v in fig.items() if k not in ("blocks",))
    per = "; ".join(f"{b}: " + " ".join(f"{k} {v:.2g}" for k, v in d.items()) for b, d in fig["blocks"].items())
    return f"{head_} | {per}"
