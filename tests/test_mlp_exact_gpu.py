"""Every instance of the matrix-core MLP (csrc/field.hip, include/mi3d.h Part 4) against the rounding models of
tests/mlp_model.py, through the C ABI, with poison in every byte the call must not read into its result or touch.

SIZE CLASSES, from grid_for() in csrc/field.hip (one wave per 32-row tile, 4 waves per workgroup, at most 256 x 2
workgroups in the backward = 65 536 rows in flight, 256 x 5 in the forward = 163 840): a wave takes a second tile -
the prefetch of the next tile's rows, the weight-gradient registers kept across tiles, the per-tile laundering of the
lane offsets - only beyond those sizes.
  small     n = 19              one partial tile
  whole     n = 4096            whole tiles, no tail
  bwd_loop  n = 3 x 65 536 + 37  three tiles per backward wave (two for part of the forward's), with a tail
  fwd_loop  n = 2 x 163 840 + 101  three tiles per forward wave, with a tail (forward only)

INPUTS (mlp_model.make_case): rows n .. n + 40 of x and of dout hold 3e4; row n - 1 carries a thousand times the
upstream gradient of the others; out and dx are pre-filled with a sentinel that rows past n and planes past dim_in / 2
must still hold; the weight-gradient buffers are pre-filled with a known tensor the call has to ADD to.

ASSERTIONS (mlp_model.check_fp32 / check_half, proved sensitive by tests/test_mlp_model_cpu.py):
  fp32 mode  every element within the running bound of the fp64 model; rows with a ReLU mask undecided at that bound
             (at most 1 %) are left out of dx and their terms go into the weight gradients' bound
  half mode  at least 98 % of the elements of y and of dx bit-identical to model_half; the others within k binary16
             ulps of their row's largest element, k = 4 x what the model alone shows between fp32 and fp64 sums
             (mlp_model.K_MEASURED: 1.05, and 4.2 for 2 -> 32 -> 4); weight and bias gradients within their bound.
             MEASURED on the MI355X (profiles/mlp_exact.json): identical share 99.76 - 100 % of y and 99.34 - 100 % of dx
             (one element of a 19-row case); largest k 2.2 for y and 1.6 for dx; rows left out at most 0.81 % (half) and
             0.46 % (fp32); largest share of a bound used 0.05 (y, fp32), 0.13 (dx, fp32), 0.99 (the unrounded dx of the
             half mode, where one flipped hidden gradient IS the bound) and 0.84 (weight gradients: an undecided mask on
             row n - 1).
Every case appends its figures to mlp_exact.json BEFORE it asserts - in the directory MI3D_REPORT_DIR names, or in
test_reports/ at the root of the repository (git-ignored).
"""
import json
import os

import pytest
import torch

import mlp_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_PATH = os.path.join(os.environ.get("MI3D_REPORT_DIR") or os.path.join(ROOT, "test_reports"), "mlp_exact.json")
_REPORT = []

INVALID = 1            # hipErrorInvalidValue
SENT = -7776.0         # exact in binary16
EXTRA = 41             # rows of poison past n

SIZES = {"small": 19, "whole": 4096, "bwd_loop": 3 * M.BWD_LOOPS_ABOVE + 37, "fwd_loop": 2 * M.FWD_LOOPS_ABOVE + 101}
# mode -> (half_mode, planes, planes_half)
MODES = {"f32_rows": (0, False, 0), "f32_planes": (0, True, 0), "f16_rows": (1, False, 0), "f16_planes": (1, True, 0),
         "f16_hplanes": (1, True, 1)}

# The dispatcher's instances (the end of csrc/field.hip), one line each: P = precision policy, NTH = hidden / 32,
# LAYERS, HP = binary16 planes, FULL = dim_in 32 with binary16 planes.  Rows and fp32 planes share an instance (the
# layout is a run-time branch), so both are run.  test_matrix_reaches_every_instance holds the case matrix to this list.
INSTANCES = """
k_mlp_fwd_g<F32,2,3,0>      fp32           hidden 64  3 layers
k_mlp_fwd_g<F32,2,2,0>      fp32           hidden 64  2 layers
k_mlp_fwd_g<F32,1,3,0>      fp32           hidden 32  3 layers
k_mlp_fwd_g<F32,1,2,0>      fp32           hidden 32  2 layers
k_mlp_fwd_g<F16,2,3,0>      half           hidden 64  3 layers
k_mlp_fwd_g<F16,2,2,0>      half           hidden 64  2 layers
k_mlp_fwd_g<F16,1,3,0>      half           hidden 32  3 layers
k_mlp_fwd_g<F16,1,2,0>      half           hidden 32  2 layers
k_mlp_fwd_g<F16,2,3,1>      half, planes16 hidden 64  3 layers
k_mlp_fwd_g<F16,2,2,1>      half, planes16 hidden 64  2 layers
k_mlp_fwd_g<F16,1,3,1>      half, planes16 hidden 32  3 layers
k_mlp_fwd_g<F16,1,2,1>      half, planes16 hidden 32  2 layers
k_mlp_bwd_g<F32,2,3,0,0>    fp32           hidden 64  3 layers  every dim_in (one wave per SIMD)
k_mlp_bwd_g<F32,2,2,0,0>    fp32           hidden 64  2 layers
k_mlp_bwd_g<F32,1,3,0,0>    fp32           hidden 32  3 layers
k_mlp_bwd_g<F32,1,2,0,0>    fp32           hidden 32  2 layers
k_mlp_bwd_g<F16,2,3,0,0>    half           hidden 64  3 layers
k_mlp_bwd_g<F16,2,2,0,0>    half           hidden 64  2 layers
k_mlp_bwd_g<F16,1,3,0,0>    half           hidden 32  3 layers
k_mlp_bwd_g<F16,1,2,0,0>    half           hidden 32  2 layers
k_mlp_bwd_g<F16,2,3,1,0>    half, planes16 hidden 64  3 layers  dim_in < 32
k_mlp_bwd_g<F16,2,2,1,0>    half, planes16 hidden 64  2 layers  dim_in < 32
k_mlp_bwd_g<F16,1,3,1,0>    half, planes16 hidden 32  3 layers  dim_in < 32
k_mlp_bwd_g<F16,1,2,1,0>    half, planes16 hidden 32  2 layers  dim_in < 32
k_mlp_bwd_g<F16,2,3,1,1>    half, planes16 hidden 64  3 layers  dim_in = 32 (the product's instance)
k_mlp_bwd_g<F16,2,2,1,1>    half, planes16 hidden 64  2 layers  dim_in = 32
k_mlp_bwd_g<F16,1,3,1,1>    half, planes16 hidden 32  3 layers  dim_in = 32
k_mlp_bwd_g<F16,1,2,1,1>    half, planes16 hidden 32  2 layers  dim_in = 32
"""
INSTANCE_NAMES = [ln.split()[0] for ln in INSTANCES.strip().splitlines()]


def instances_of(mode, din, hid, layers):
    """(forward instance, backward instance) the dispatcher picks - restated from mi3d_mlp_forward_counted /
    mi3d_mlp_backward / launch_bwd."""
    half, _, hp = MODES[mode]
    pol, nth = ("F16" if half else "F32"), hid // 32
    fwd = f"k_mlp_fwd_g<{pol},{nth},{layers},{hp}>"
    return fwd, f"k_mlp_bwd_g<{pol},{nth},{layers},{hp},{int(bool(hp) and din == 32)}>"


CASES = [(mode, *sh) for sh in M.SHAPES for mode in MODES]


def test_matrix_reaches_every_instance():
    reached = set()
    for mode, din, hid, layers in CASES:
        reached |= set(instances_of(mode, din, hid, layers))
    assert reached == set(INSTANCE_NAMES) and len(INSTANCE_NAMES) == 28
    from mi3d import _lib as L
    for _, din, hid, layers in CASES:
        assert L.lib().mi3d_mlp_supported(din, hid, 4, layers) == 1


def test_round_half_on_the_device(cuda):
    """The model's binary16 rounding, evaluated on the GPU, is torch's own conversion of fp32 values."""
    v = torch.cat([torch.randn(100000, device=cuda) * s for s in (1e-7, 1e-4, 1.0, 3e4)])
    assert torch.equal(M.round_half(v), v.half().double())


# ------------------------------------------------------------------------------------------------ plumbing

def _report(entry):
    _REPORT.append(entry)
    os.makedirs(os.path.dirname(REPORT_PATH), exist_ok=True)
    with open(REPORT_PATH, "w") as f:
        json.dump(_REPORT, f, indent=0)


_cache = {}


def _cached(kind, key, make):
    """One entry per kind: the parametrisation keeps the cases of one (shape, size) together."""
    if _cache.get(kind, (None,))[0] != key:
        _cache[kind] = (key, make())
    return _cache[kind][1]


def _inputs(dev, din, hid, layers, n, seed=0):
    return _cached("in", (din, hid, layers, n, seed), lambda: M.make_case(din, hid, layers, n, seed, dev, EXTRA))


def _model(dev, din, hid, layers, n, half, hp, seed=0):
    x, ws, dout = _inputs(dev, din, hid, layers, n, seed)
    if half:   # binary16 planes differ in the rounding of dx alone
        ref = _cached("half", (din, hid, layers, n, seed), lambda: M.model_half(x[:n], ws, dout[:n], False))
        return dict(ref, planes_half=True, dx=M.round_half(ref["dx_exact"])) if hp else ref
    return _cached("fp32", (din, hid, layers, n, seed), lambda: M.model_fp32(x[:n], ws, dout[:n]))


def _small_seed(dev, din, hid, layers, n, half, hp):
    """A case of a few rows cannot leave 1 % of them out: take the first seed whose MODEL has no undecided ReLU mask
    (a property of the inputs alone; the kernel is not consulted)."""
    if n >= 1000:
        return 0
    for seed in range(50):
        x, ws, dout = M.make_case(din, hid, layers, n, seed, dev)
        m = M.model_half(x, ws, dout, bool(hp)) if half else M.model_fp32(x, ws, dout)
        if not bool(m["uncertain_rows"].any()):
            return seed
    raise AssertionError("no seed without an undecided mask")


def _wlist(ws):
    """[(W, b)] -> the six ABI slots W1, b1, W2, b2, W3, b3 (None = NULL: two layers)."""
    if len(ws) == 3:
        return [ws[0][0], ws[0][1], ws[1][0], ws[1][1], ws[2][0], ws[2][1]]
    return [ws[0][0], ws[0][1], None, None, ws[1][0], ws[1][1]]


def _x_for_kernel(x, din, planes, hp):
    """x [rows, din] -> what the ABI takes: the rows themselves, or level-major planes [din/2][rows][2]."""
    if not planes:
        return x.contiguous(), 0
    p = x.view(x.shape[0], din // 2, 2).permute(1, 0, 2).contiguous()
    return (p.half() if hp else p), x.shape[0]


def _dx_buffer(dev, rows, din, planes, hp):
    if not planes:
        return torch.full((rows, din), SENT, device=dev), 0
    return torch.full((16, rows, 2), SENT, device=dev, dtype=torch.float16 if hp else torch.float32), rows


def _dx_rows(dx, n, din, planes):
    """The kernel's dx as [n, din] numbers + whether every element it must not touch still holds the sentinel."""
    if not planes:
        return dx[:n].double(), bool((dx[n:] == SENT).all())
    got = dx[:din // 2, :n].permute(1, 0, 2).reshape(n, din).double()
    return got, bool((dx[:, n:] == SENT).all()) and bool((dx[din // 2:] == SENT).all())


def _prefill(t, k):
    return torch.linspace(-1.0, 1.0, t.numel(), device=t.device).view_as(t).roll(k).contiguous() + 0.25


def _forward(L, xk, x_rows, hp, n, wl, dims, half, out, count=None, n_stride=None):
    if count is None and n_stride is None:
        return L.lib().mi3d_mlp_forward(L.ptr(xk), x_rows, hp, n, *[L.ptr(t) for t in wl], *dims, half, L.ptr(out), L.stream())
    return L.lib().mi3d_mlp_forward_counted(L.ptr(xk), x_rows, hp, n, L.ptr(count), n_stride, *[L.ptr(t) for t in wl], *dims,
                                            half, L.ptr(out), L.stream())


def _backward(L, xk, x_rows, hp, dout, n, wl, dims, half, dx, dx_rows, grads):
    return L.lib().mi3d_mlp_backward(L.ptr(xk), x_rows, hp, L.ptr(dout), n, *[L.ptr(t) for t in wl], *dims, half, L.ptr(dx),
                                     dx_rows, *[L.ptr(t) for t in grads], L.stream())


def _run_backward(L, dev, x, ws, dout, n, din, hid, mode, in_place=False):
    """-> (got dict, sentinel ok, the prefills, the kernel's x buffer after the call)"""
    half, planes, hp = MODES[mode]
    xk, x_rows = _x_for_kernel(x, din, planes, hp)
    if in_place:
        xk = xk.clone()
        dx, dx_rows = xk, x_rows
    else:
        dx, dx_rows = _dx_buffer(dev, x.shape[0], din, planes, hp)
    wl = _wlist(ws)
    pre = [None if t is None else _prefill(t, i) for i, t in enumerate(wl)]
    grads = [None if t is None else t.clone() for t in pre]
    err = _backward(L, xk, x_rows, hp, dout, n, wl, (din, hid, 4), half, dx, dx_rows, grads)
    torch.cuda.synchronize()
    assert err == 0, err
    if in_place:
        got_dx = (dx[:, :n].permute(1, 0, 2).reshape(n, din) if planes else dx[:n]).double()
        untouched = bool(torch.equal(dx[:, n:], _x_for_kernel(x, din, planes, hp)[0][:, n:])) if planes else \
            bool(torch.equal(dx[n:], x[n:]))
    else:
        got_dx, untouched = _dx_rows(dx, n, din, planes)
    d = [None if g is None else g.double() - p.double() for g, p in zip(grads, pre)]
    got = dict(dx=got_dx, dW=[t for t in d[0::2] if t is not None], db=[t for t in d[1::2] if t is not None])
    return got, untouched, [p for p in pre if p is not None], dx


def _add_prefill_to_bounds(ref, pre, n):
    """The buffers hold prefill + gradient: every partial sum added to them rounds at the magnitude of the total."""
    ref = dict(ref)
    slack = M.wgrad_depth(n) * M.U32
    ref["dW_err"] = [e + slack * p.double().abs() for e, p in zip(ref["dW_err"], pre[0::2])]
    ref["db_err"] = [e + slack * p.double().abs() for e, p in zip(ref["db_err"], pre[1::2])]
    return ref


# ------------------------------------------------------------------------------------------------ the matrix

@pytest.mark.parametrize("mode", list(MODES))     # (the fastest index: the modes of one (shape, size) share a model)
@pytest.mark.parametrize("size", ["small", "whole", "bwd_loop", "fwd_loop"])
@pytest.mark.parametrize("din,hid,layers", M.SHAPES)
def test_forward(cuda, mode, din, hid, layers, size):
    from mi3d import _lib as L
    half, planes, hp = MODES[mode]
    n = SIZES[size]
    seed = _small_seed(cuda, din, hid, layers, n, half, hp)
    x, ws, _ = _inputs(cuda, din, hid, layers, n, seed)
    ref = _model(cuda, din, hid, layers, n, half, hp, seed)
    xk, x_rows = _x_for_kernel(x, din, planes, hp)
    out = torch.full((n + EXTRA, 4), SENT, device=cuda)
    err = _forward(L, xk, x_rows, hp, n, _wlist(ws), (din, hid, 4), half, out)
    torch.cuda.synchronize()
    assert err == 0, err
    got = dict(y=out[:n])
    fig, fails = (M.check_half(got, ref, M.k_cap(din, hid, layers), backward=False) if half
                  else M.check_fp32(got, ref, backward=False))
    if not bool((out[n:] == SENT).all()):
        fails.append("rows_past_n_untouched")
    _report(dict(direction="forward", instance=instances_of(mode, din, hid, layers)[0], mode=mode, dim_in=din, hidden=hid,
                 layers=layers, size=size, n=n, failed=fails, **fig))
    assert not fails, (fails, fig)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", ["small", "whole", "bwd_loop"])
@pytest.mark.parametrize("din,hid,layers", M.SHAPES)
def test_backward(cuda, mode, din, hid, layers, size):
    from mi3d import _lib as L
    half, planes, hp = MODES[mode]
    n = SIZES[size]
    seed = _small_seed(cuda, din, hid, layers, n, half, hp)
    x, ws, dout = _inputs(cuda, din, hid, layers, n, seed)
    ref = _model(cuda, din, hid, layers, n, half, hp, seed)
    got, untouched, pre, _ = _run_backward(L, cuda, x, ws, dout, n, din, hid, mode)
    ref = _add_prefill_to_bounds(ref, pre, n)
    fig, fails = (M.check_half(got, ref, M.k_cap(din, hid, layers), forward=False) if half
                  else M.check_fp32(got, ref, forward=False))
    if not untouched:
        fails.append("rows_and_planes_past_the_end_untouched")
    _report(dict(direction="backward", instance=instances_of(mode, din, hid, layers)[1], mode=mode, dim_in=din, hidden=hid,
                 layers=layers, size=size, n=n, failed=fails, **fig))
    assert not fails, (fails, fig)


# ------------------------------------------------------------------------------------------------ in place (dx == x)

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", ["small", "bwd_loop"])
@pytest.mark.parametrize("din,hid,layers", M.SHAPES)
def test_backward_in_place_equals_out_of_place(cuda, mode, din, hid, layers, size):
    """include/mi3d.h Part 4: dx may be x itself (same layout, same plane rows, same element type) - with a partial
    last tile too (n % 32 != 0: its idle lanes re-read row n - 1, which only their own wave writes, after its reads)
    and with plane rows past n, which stay what they were."""
    from mi3d import _lib as L
    n = SIZES[size]
    assert n % 32 != 0
    x, ws, dout = _inputs(cuda, din, hid, layers, n)
    a, ok_a, _, _ = _run_backward(L, cuda, x, ws, dout, n, din, hid, mode)
    b, ok_b, _, _ = _run_backward(L, cuda, x, ws, dout, n, din, hid, mode, in_place=True)
    assert ok_a and ok_b
    assert torch.equal(a["dx"], b["dx"])
    for nm in ("dW", "db"):   # float atomics across the workgroups: equal up to their order
        for s, t in zip(a[nm], b[nm]):
            assert float((s - t).abs().max()) <= 1e-5 * float(s.abs().max()) + 1e-6


def test_in_place_outside_the_rule_is_an_error(cuda):
    from mi3d import _lib as L
    n, din, hid = 64, 8, 32
    x, ws, dout = M.make_case(din, hid, 2, n, device=cuda)
    wl = _wlist(ws)
    grads = [None if t is None else torch.zeros_like(t) for t in wl]
    buf = torch.zeros(4, 2 * n, 2, device=cuda)     # big enough for either reading
    before = buf.clone()
    for x_rows, dx_rows in [(n, 0), (0, n), (n, 2 * n), (2 * n, n)]:
        assert _backward(L, buf, x_rows, 0, dout, n, wl, (din, hid, 4), 0, buf, dx_rows, grads) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and all(float(g.abs().max()) == 0 for g in grads if g is not None)
    assert _backward(L, buf, n, 0, dout, n, wl, (din, hid, 4), 0, buf, n, grads) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ edges

@pytest.mark.parametrize("mode", ["f16_rows", "f16_planes", "f16_hplanes"])
def test_negative_zero_passes_no_gradient(cuda, mode):
    """A pre-activation that rounds to -0 in binary16 (and one that rounds to +0 from above): torch.relu's backward
    passes nothing.  F16::masked multiplies by min(bits of the activation, 1), which is 1 for 0x8000 - so this holds
    only because the packed maximum of F16::relu hands back +0 for max(-0, +0)."""
    from mi3d import _lib as L
    x, ws, dout = M.zero_edge_case(cuda, n=37)
    ref = M.model_half(x, ws, dout, bool(MODES[mode][2]))
    got, untouched, pre, _ = _run_backward(L, cuda, x, ws, dout, 37, 2, 32, mode)
    fails = M.check_zero_edge(got)
    fig, f2 = M.check_half(got, _add_prefill_to_bounds(ref, pre, 37), M.k_cap(2, 32, 2), forward=False)
    _report(dict(direction="backward", edge="negative_zero", mode=mode, failed=fails + f2, **fig))
    assert untouched and not fails and not f2, (fails, f2, fig)
    if mode == "f16_rows":    # the fp32 kernel has no rounding to zero: the same data, its own model
        ref = M.model_fp32(x, ws, dout)
        got, _, pre, _ = _run_backward(L, cuda, x, ws, dout, 37, 2, 32, "f32_rows")
        assert M.check_fp32(got, _add_prefill_to_bounds(ref, pre, 37), forward=False)[1] == []


@pytest.mark.parametrize("kind", ["x", "dout"])
@pytest.mark.parametrize("mode", ["f16_rows", "f16_hplanes"])
@pytest.mark.parametrize("din,hid,layers", [(32, 64, 3), (8, 32, 2), (16, 64, 3)])
def test_non_finite_values_land_where_the_model_has_them(cuda, din, hid, layers, mode, kind):
    """x above 65 504 is inf once rounded (autocast's cast); an upstream row beyond binary16 is GradScaler's overflow."""
    from mi3d import _lib as L
    half, planes, hp = MODES[mode]
    n = 100
    x, ws, dout = M.nonfinite_case(kind, din, hid, layers, cuda, n)
    ref = M.model_half(x, ws, dout, bool(hp))
    xk, x_rows = _x_for_kernel(x, din, planes, hp)
    out = torch.full((n, 4), SENT, device=cuda)
    assert _forward(L, xk, x_rows, hp, n, _wlist(ws), (din, hid, 4), half, out) == 0
    got, untouched, _, _ = _run_backward(L, cuda, x, ws, dout, n, din, hid, mode)
    got["y"] = out
    fails = M.check_nonfinite(got, ref)
    _report(dict(direction="both", edge="non_finite_" + kind, mode=mode, dim_in=din, hidden=hid, layers=layers, failed=fails))
    assert untouched and not fails, fails


FWD_CASES = [(mode, *sh) for sh in [(32, 64, 3), (30, 64, 2), (8, 32, 3), (2, 32, 2)] for mode in MODES]


@pytest.mark.parametrize("mode,din,hid,layers", FWD_CASES)
def test_counted_forward(cuda, mode, din, hid, layers):
    """mi3d_mlp_forward_counted over 7 stencil points of n_stride rows each, of which the first `count` samples carry
    data: those rows equal the uncounted call bit for bit, every other row keeps its sentinel."""
    from mi3d import _lib as L
    half, planes, hp = MODES[mode]
    P, n, n_stride = 7, 100, 107
    rows = P * n_stride
    x, ws, _ = M.make_case(din, hid, layers, rows, seed=3, device=cuda)
    xk, x_rows = _x_for_kernel(x, din, planes, hp)
    wl, dims = _wlist(ws), (din, hid, 4)
    full = torch.full((rows, 4), SENT, device=cuda)
    assert _forward(L, xk, x_rows, hp, rows, wl, dims, half, full) == 0
    sample = torch.arange(rows, device=cuda) % n_stride
    for c in [0, 1, 31, 32, 33, n - 1, n, n + 5]:
        xc = x.clone()
        xc[sample >= c] = M.POISON          # rows without data: whatever is computed from them must not be stored
        xck, _ = _x_for_kernel(xc, din, planes, hp)
        out = torch.full((rows, 4), SENT, device=cuda)
        count = torch.tensor([c], dtype=torch.int32, device=cuda)
        assert _forward(L, xck, x_rows, hp, rows, wl, dims, half, out, count, n_stride) == 0
        torch.cuda.synchronize()
        live = (sample < c).unsqueeze(1)
        assert torch.equal(out[live.expand_as(out)], full[live.expand_as(full)]), (mode, c)
        assert bool((out[~live.expand_as(out)] == SENT).all()), (mode, c)
    out = torch.full((rows, 4), SENT, device=cuda)   # no count at all: every row
    assert _forward(L, xk, x_rows, hp, rows, wl, dims, half, out, None, n_stride) == 0
    assert torch.equal(out, full)


def test_arguments(cuda):
    """n == 0 returns 0 and touches nothing; every argument error the two entry points list is hipErrorInvalidValue."""
    from mi3d import _lib as L
    n, din, hid = 64, 8, 32
    x, ws3, dout = M.make_case(din, hid, 3, n, device=cuda)
    wl = _wlist(ws3)
    planes = torch.zeros(4, n, 2, device=cuda)
    hplanes = planes.half()
    out = torch.full((n, 4), SENT, device=cuda)
    dx = torch.full((n, din), SENT, device=cuda)
    dxp = torch.full((4, n, 2), SENT, device=cuda)
    grads = [torch.full_like(t, 0.5) for t in wl]
    dims = (din, hid, 4)

    def fwd(xk=x, x_rows=0, hp=0, n_=n, w=wl, d=dims, half=0, count=None, n_stride=n):
        return _forward(L, xk, x_rows, hp, n_, w, d, half, out, count, n_stride)

    def bwd(xk=x, x_rows=0, hp=0, n_=n, w=wl, d=dims, half=0, dx_=dx, dx_rows=0, g=grads):
        return _backward(L, xk, x_rows, hp, dout, n_, w, d, half, dx_, dx_rows, g)

    def without(lst, *idx):
        return [None if i in idx else t for i, t in enumerate(lst)]

    assert fwd(n_=0) == 0 and bwd(n_=0) == 0 and _forward(L, x, 0, 0, 0, wl, dims, 0, out) == 0
    bad_dims = [(7, hid, 4), (0, hid, 4), (34, hid, 4), (din, 48, 4), (din, 16, 4), (din, hid, 3)]
    errors = [fwd(n_stride=0), fwd(xk=planes, x_rows=n - 1), fwd(xk=hplanes, x_rows=n, hp=1, half=0),
              fwd(xk=hplanes, x_rows=0, hp=1, half=1)]
    errors += [fwd(d=d) for d in bad_dims] + [bwd(d=d) for d in bad_dims]
    errors += [fwd(w=without(wl, i)) for i in (0, 1, 2, 3, 4, 5)]          # W2 xor b2 missing: not a two-layer call
    errors += [bwd(w=without(wl, i)) for i in (0, 1, 2, 3, 4, 5)]
    errors += [bwd(g=without(grads, i)) for i in (0, 1, 2, 3, 4, 5)]
    errors += [bwd(xk=planes, x_rows=n - 1), bwd(dx_=dxp, dx_rows=n - 1),
               bwd(xk=hplanes, x_rows=n, hp=1, half=0, dx_=dxp.half(), dx_rows=n),
               bwd(xk=hplanes, x_rows=0, hp=1, half=1, dx_=dxp.half(), dx_rows=n),
               bwd(xk=hplanes, x_rows=n, hp=1, half=1, dx_=dx, dx_rows=0)]
    torch.cuda.synchronize()
    assert errors == [INVALID] * len(errors), errors
    assert bool((out == SENT).all()) and bool((dx == SENT).all()) and bool((dxp == SENT).all())
    assert all(bool((g == 0.5).all()) for g in grads)
    # and the same calls, well-formed, go through
    assert fwd() == 0 and bwd() == 0 and bwd(w=without(wl, 2, 3), g=without(grads, 2, 3)) == 0
    assert bwd(xk=hplanes, x_rows=n, hp=1, half=1, dx_=dxp.half(), dx_rows=n) == 0
    torch.cuda.synchronize()
