"""CPU: the binary64 model of the field head (tests/head_model.py) against torch's double-precision autograd over the plain
composition (mi3d.network.trunc_exp, mi3d.renderer.safe_normalize, torch.nan_to_num), its non-finite pattern against the
same composition in binary32, the same model with binary32 operations against its own bounds, its seeded faults, and the
conditions head_cases' inputs must meet (every block decidedly on its side; undecided rows in the straddling block only)."""
import pytest
import torch

import head_model as H

N = 4099
SIZES = (1, 255, 256, 257, N)
CASES = [(P, i) for P in (7, 13) for i in range(len(H.PARAMS))]
GRADS = ("dsigma", "dalbedo", "dnormal", "dnormal2")


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(P, i, n=N):
        if (P, i, n) not in cache:
            case = H.head_cases(0, n, P, H.PARAMS[i])
            cache[(P, i, n)] = (case, H.model_of(case))
        return cache[(P, i, n)]
    return get


def _composition(case, dtype):
    """(sigma, albedo, normal[, normal2]) and dh by torch autograd, in `dtype`, with the ABI's host-rounded constants."""
    from mi3d.network import trunc_exp
    from mi3d.renderer import safe_normalize
    bound, eps, density, radius = case["params"]
    two_r2, inv = H.host_constants(radius, eps)
    n, P = case["n"], case["P"]
    h = case["h"].clone().to(dtype).requires_grad_()
    hv = h.view(P, n, 4)
    base = case["x"].to(dtype).unsqueeze(0).expand(P, n, 3)
    if P == 13:
        base = torch.cat([base[:7], case["x2"].to(dtype).unsqueeze(0).expand(6, n, 3)], 0)
    pts = (base + torch.from_numpy(case["offsets"]).to(dtype).unsqueeze(1)).clamp(-bound, bound)
    gauss = density * torch.exp(-(pts ** 2).sum(-1) / two_r2)
    sig = trunc_exp(hv[..., 0] + gauss)

    def normal(s6):
        g = torch.stack([(s6[0] - s6[1]) * inv, (s6[2] - s6[3]) * inv, (s6[4] - s6[5]) * inv], -1)
        return torch.nan_to_num(safe_normalize(-g))
    out = [sig[0], torch.sigmoid(hv[0, :, 1:]), normal(sig[1:7])]
    if P == 13:
        out.append(normal(sig[7:13]))
    ups = [case[k].to(dtype) for k in GRADS[:len(out)]]
    torch.autograd.backward(out, ups)
    return [t.detach() for t in out], h.grad


def _finite_rows(case):
    keep = torch.ones(case["n"], dtype=torch.bool)
    for name in H.NONFINITE_BLOCKS:
        keep[slice(*case["blocks"][name])] = False
    return keep


@pytest.mark.parametrize("P,i", CASES)
def test_model_equals_torch_double_autograd(cases, P, i):
    case, ref = cases(P, i)
    out, dh = _composition(case, torch.float64)
    keep = _finite_rows(case)
    for name, w in zip(H.FORWARD, out):
        mag = (ref[name + "_err"] + H.U32 * ref[name].abs()) / H.U32      # the magnitude the bound is 2^-24 of
        assert bool(((ref[name] - w).abs() <= 1e-12 * mag)[keep].all()), name
    rows = keep.repeat(P)
    mag = (ref["dh_err"] + H.U32 * ref["dh"].abs()) / H.U32
    assert bool(((ref["dh"] - dh).abs() <= 1e-12 * mag)[rows].all())
    assert bool(torch.isfinite(ref["dh"][rows]).all()) and bool(torch.isfinite(dh[rows]).all())


@pytest.mark.parametrize("P,i", CASES)
def test_nonfinite_pattern_is_torch_binary32s(cases, P, i):
    """Which elements are NaN, +-inf, +-FLT_MAX or exact zeros where a neighbour overflows: the model's pattern is that of
    the composition run by torch in binary32 - this is what `where torch's do` means for 0 * inf."""
    case, ref = cases(P, i)
    out, dh = _composition(case, torch.float32)
    m32 = H.model_of(case, acc=torch.float32)
    rows = ~_finite_rows(case)
    assert int(rows.sum()) >= 12
    seen = set()
    for name, w in list(zip(H.FORWARD, out)) + [("dh", dh)]:
        r = rows.repeat(w.shape[0] // case["n"])
        pw = H.pattern(w)[r]
        assert not bool(H.pattern_differs(w, ref[name], ref[name + "_err"])[r].any()), name
        assert not bool(H.pattern_differs(w, m32[name], ref[name + "_err"])[r].any()), name
        seen |= set(pw.unique().tolist())
    assert {0, 1, 2, 6} <= seen and (4 in seen or 5 in seen)        # NaN, inf, FLT_MAX and zeros all occur
    # outside these blocks nothing is non-finite or saturated, in either evaluation
    for name, w in list(zip(H.FORWARD, out)) + [("dh", dh)]:
        r = ~rows.repeat(w.shape[0] // case["n"])
        for t in (w, ref[name]):
            p = H.pattern(t)[r]
            assert not bool(((p > 0) & (p < 6)).any()), name


@pytest.mark.parametrize("P,i", CASES)
def test_binary32_model_stays_inside_the_bounds(cases, P, i):
    """The model with binary32 operations is a correct evaluation in another order (torch's graph, a division where the
    bound counts reciprocal and product): it must stay inside the bounds."""
    case, ref = cases(P, i)
    fig, fails = H.check(H.as_got(H.model_of(case, acc=torch.float32)), ref, case["blocks"])
    print(f"[head] P={P} params={H.PARAMS[i]} binary32 model: {H.worst(fig)}")
    assert fails == [], (fails, H.worst(fig))


@pytest.mark.parametrize("P_active,grads", [(1, ("dsigma",)), (1, ()), (7, ("dnormal",)), (7, ("dalbedo", "dnormal"))])
def test_binary32_model_with_a_prefix_of_the_stencil(cases, P_active, grads):
    case, _ = cases(13, 2)
    ref = H.model_of(case, P_active=P_active, grads=grads)
    assert ref["dh"].shape == (P_active * N, 4)
    fig, fails = H.check(H.as_got(H.model_of(case, P_active=P_active, grads=grads, acc=torch.float32)), ref, case["blocks"])
    assert fails == [], (fails, H.worst(fig))
    if not grads:
        assert float(ref["dh"].nan_to_num().abs().max()) == 0.0


@pytest.mark.parametrize("fault", H.FAULTS)
def test_seeded_fault_is_caught(cases, fault):
    case, ref = cases(13, 2)
    _, clean = H.check(H.as_got(ref), ref, case["blocks"])
    assert clean == []
    bad = H.model_of(case, faults=(fault,))
    fig, fails = H.check(H.as_got(bad), ref, case["blocks"])
    print(f"[head] fault {fault}: {fails}")
    if H.FAULT_BREAKS[fault] is None:
        # unobservable with finite upstream gradients (head_model.FAULT_BREAKS): the seeded model returns the same bits,
        # on every parameter set
        for P, i in CASES:
            c, r = cases(P, i)
            b = H.model_of(c, faults=(fault,))
            for name in (*H.FORWARD[:2 + (P == 13) + 1], "dh"):
                assert torch.equal(b[name].nan_to_num(nan=123.0), r[name].nan_to_num(nan=123.0)), (fault, name)
        assert fails == []
        return
    assert H.FAULT_BREAKS[fault] in fails, (fault, fails, H.worst(fig))


@pytest.mark.parametrize("P,i", CASES)
def test_inputs_meet_their_conditions(cases, P, i):
    """Caps and blocks: conditions on head_cases' inputs that the model alone must satisfy."""
    for n in SIZES:
        case, ref = cases(P, i, n)
        blocks = case["blocks"]
        und = ref["undecided"].any(0)
        lo, hi = blocks["straddle"]
        outside = und.clone()
        outside[lo:hi] = False
        share = float(und.sum()) / n
        print(f"[head] P={P} params={H.PARAMS[i]} n={n}: undecided {int(und.sum())} rows ({100 * share:.2f} %)")
        assert not bool(outside.any()) and share <= H.MAX_UNDECIDED
        if n >= 255:
            assert int(und.sum()) >= 2                              # the tuned rows do straddle
            assert all(hi > lo for lo, hi in blocks.values())       # every block has rows
        ss, e = ref["ss"], ref["ss_err"]

        def rows(name):
            return slice(*blocks[name])
        assert bool((ss[:, rows("zero")] == 0).all())
        assert bool((ss[:, rows("empty")] > 0).all()) and bool(((ss + e)[:, rows("empty")] < 0.99 * H.LO).all())
        assert bool(((ss - e)[:, rows("above")] > 100 * H.HI).all())
        for name in ("well", "near", "around15", "box", "blob"):
            r = rows(name)
            assert bool(((ss - e)[:, r] > 1.01 * H.LO).all()) and bool(((ss + e)[:, r] < 0.99 * H.HI).all()), name
        assert bool(torch.isnan(ss[:, rows("overflow2")]).all()) and bool((ss[:, rows("overflow1")] == float("inf")).all())
        for name in (*H.FORWARD[:3 + (P == 13)], "dh"):             # a finite value has a finite bound
            assert bool(torch.isfinite(ref[name + "_err"]).all()), name
    # both sides of the derivative clamp, and the clamp itself
    case, ref = cases(P, i)
    u0 = case["h"].view(P, N, 4)[0, :, 0].double()[slice(*case["blocks"]["around15"])]
    assert bool((u0 < 14.95).any()) and bool((u0 > 15.05).any())
