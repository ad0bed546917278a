"""CPU: the binary64 model of the fused MLP's second-order pass (tests/mlp_grad2_model.py) against torch.autograd's double
backward of a binary64 Linear / ReLU stack, its seeded faults, the reference-alone check (the same model with fp32
products stays inside its own bounds) and the share of rows its undecided masks leave out."""
import pytest
import torch

import mlp_grad2_model as M2
import mlp_model as Mm

SIZES = (19, 4099)


def _autograd(x, ws, dout, r):
    """grad of <dx, r> with respect to dout, the weights, the biases and x, dx taken with create_graph=True; binary64."""
    x = x.double().requires_grad_()
    dout = dout.double().requires_grad_()
    W = [w.double().requires_grad_() for w, _ in ws]
    b = [bb.double().requires_grad_() for _, bb in ws]
    h = x
    for l in range(len(W)):
        h = h @ W[l].t() + b[l]
        if l < len(W) - 1:
            h = torch.relu(h)
    (dx,) = torch.autograd.grad(h, x, dout, create_graph=True)
    g = torch.autograd.grad((dx * r.double()).sum(), [dout, *W, *b, x], allow_unused=True)
    L = len(W)
    return dict(grad_dout=g[0], gW=list(g[1:1 + L]), gb=list(g[1 + L:1 + 2 * L]), grad_x=g[-1], dx=dx.detach())


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(shape, n):
        if (shape, n) not in cache:
            x, ws, dout, r = M2.make_case(*shape, n)
            cache[(shape, n)] = (x, ws, dout, r, M2.second_order(x, ws, dout, r))
        return cache[(shape, n)]
    return get


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("din,hid,layers", Mm.SHAPES)
def test_model_equals_autograd_double_backward(cases, din, hid, layers, n):
    x, ws, dout, r, ref = cases((din, hid, layers), n)
    want = _autograd(x, ws, dout, r)
    pairs = [("grad_dout", ref["grad_dout"], ref["grad_dout_err"], want["grad_dout"])]
    pairs += [(f"gW{l + 1}", ref["gW"][l], ref["gW_err"][l], want["gW"][l]) for l in range(layers)]
    for name, got, err, w in pairs:
        mag = (err + Mm.U32 * got.abs()) / Mm.U32           # the magnitude the bound is 2^-24 of
        assert bool(((got - w).abs() <= 1e-12 * mag).all()), name
    assert torch.allclose(ref["d"][0], want["dx"], rtol=0, atol=1e-9 * float(want["dx"].abs().max()))   # the first-order chain
    for name, g in [("grad_x", want["grad_x"])] + [(f"gb{l + 1}", want["gb"][l]) for l in range(layers)]:
        assert g is None or float(g.abs().max()) == 0.0, name
    assert float(ref["grad_x"].abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in ref["gb"])


@pytest.mark.parametrize("fault", M2.FAULTS)
@pytest.mark.parametrize("shape", [(32, 64, 3), (8, 32, 2)])
def test_seeded_fault_is_caught(cases, fault, shape):
    x, ws, dout, r, ref = cases(shape, 4099)
    _, clean = M2.check(M2.as_got(ref), ref)
    assert clean == []
    _, fails = M2.check(M2.as_got(M2.second_order(x, ws, dout, r, faults=(fault,))), ref)
    assert M2.FAULT_BREAKS[fault] in fails, (fault, fails)


def test_seeded_mask_fault_is_caught_by_the_zero_edge():
    x, ws, dout, r = M2.zero_edge_case()
    m = M2.second_order(x, ws, dout, r)
    assert M2.check_zero_edge(M2.as_got(m)) == []
    for fault in ("tangent_unmasked", "mask_from_tangent"):
        bad = M2.second_order(x, ws, dout, r, faults=(fault,))
        assert "zero_edge_control" in M2.check_zero_edge(M2.as_got(bad)), fault


@pytest.mark.parametrize("din,hid,layers", Mm.SHAPES)
def test_reference_alone_fp32(cases, din, hid, layers):
    """The model with fp32 products is a correct evaluation in another order: it must stay inside the bounds."""
    x, ws, dout, r, ref = cases((din, hid, layers), 4099)
    fig, fails = M2.check(M2.as_got(M2.second_order(x, ws, dout, r, acc=torch.float32)), ref)
    print(f"[mlp-grad2] {din}->{hid}x{layers - 1}->4 fp32 products: {fig}")
    assert fails == []


@pytest.mark.parametrize("din,hid,layers", Mm.SHAPES)
def test_rows_left_out_stay_below_the_cap(cases, din, hid, layers):
    for n in SIZES:
        ref = cases((din, hid, layers), n)[4]
        share = float(ref["uncertain_rows"].sum()) / n
        print(f"[mlp-grad2] {din}->{hid}x{layers - 1}->4 n={n}: rows left out {100 * share:.3f} %")
        assert share <= Mm.MAX_ROWS_LEFT_OUT


def test_geometry_figures():
    assert M2.BWD2_LOOPS_ABOVE == 65536 and M2.grid_for2(1) == 1 and M2.grid_for2(65536) == 512 == M2.grid_for2(10 ** 6)
    assert M2.wgrad2_depth(19) == 32 + 1 + 4 + 1 + 1
    assert M2.wgrad2_depth(3 * 65536 + 37) == 32 + 4 + 4 + 512 + 1
