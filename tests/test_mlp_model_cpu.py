"""The reference models of tests/mlp_model.py, checked without a GPU:
  1. model_half's forward = the C oracle's autocast restatement (oracle/field_ref.c, fp32 sequential sums);
  2. the reference-alone figures - the same model with fp32 against fp64 accumulation - on the inputs and shapes of
     tests/test_mlp_exact_gpu.py: they are what keeps that file's caps honest (98 % identical, K_CAP ulps, 1 % of rows);
  3. every seeded fault breaks a named assertion of that file when the faulty model stands in for the kernel."""
import numpy as np
import pytest
import torch

import mlp_model as M

N_REF = 70003


def test_model_half_forward_equals_the_oracle(oracle):
    cfg = oracle.GridConfig(log2_hashmap_size=14)
    fp = oracle.FieldParams(cfg, seed=3)
    rng = np.random.default_rng(5)
    fp.params = rng.uniform(-1.0, 1.0, cfg.n_params).astype(np.float32)
    x = rng.uniform(-1.0, 1.0, (4000, 3)).astype(np.float32)
    _, _, raw = oracle.field_density(x, fp, half_mode=True, return_raw=True)
    x01 = ((x + np.float32(fp.bound)) / np.float32(2 * fp.bound)).astype(np.float32)
    feats = torch.from_numpy(oracle.hashgrid_forward(x01, fp.params, cfg))
    layers = [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in zip(fp.W, fp.B)]
    ref = M.model_half(feats, layers, torch.zeros(len(x), 4), planes_half=True)
    fig, fails = M.check_half(dict(y=torch.from_numpy(raw)), ref, M.k_cap(32, 64, 3), backward=False)
    print(fig)
    assert not fails, (fails, fig)


@pytest.mark.parametrize("din,hid,layers", M.SHAPES)
def test_reference_alone_half(din, hid, layers):
    """fp32 against fp64 accumulation of model_half: nearly every element identical, the rest one binary16 ulp of the
    row's largest element away, the weight gradients inside their bound - a quarter of every cap of the GPU test."""
    x, ws, dout = M.make_case(din, hid, layers, N_REF)
    ref = M.model_half(x, ws, dout, planes_half=True)
    got = M.as_got(M.model_half(x, ws, dout, planes_half=True, acc=torch.float32))
    fig, fails = M.check_half(got, ref, k_cap=M.K_MEASURED[(din, hid, layers)])
    print(din, hid, layers, fig)
    assert not fails, (fails, fig)
    assert 1 - fig["y_identical"] <= (1 - M.MIN_IDENTICAL) / 4 and 1 - fig["dx_identical"] <= (1 - M.MIN_IDENTICAL) / 4, fig
    # fp32 rows / planes: the unrounded dx against its running bound
    ref = M.model_half(x, ws, dout, planes_half=False)
    got = M.as_got(M.model_half(x, ws, dout, planes_half=False, acc=torch.float32))
    fig, fails = M.check_half(got, ref, k_cap=M.K_MEASURED[(din, hid, layers)])
    assert not fails, (fails, fig)     # (a flipped hidden gradient uses the whole of dx's bound: it IS the bound)


@pytest.mark.parametrize("din,hid,layers", M.SHAPES)
def test_reference_alone_fp32(din, hid, layers):
    x, ws, dout = M.make_case(din, hid, layers, N_REF)
    ref = M.model_fp32(x, ws, dout)
    got = M.as_got(M.model_fp32(x, ws, dout, acc=torch.float32))
    fig, fails = M.check_fp32(got, ref)
    print(din, hid, layers, fig)
    assert not fails, (fails, fig)
    assert max(fig["y_bound_used"], fig["dx_bound_used"]) <= 0.25, fig


def test_geometry_figures():
    assert M.BWD_LOOPS_ABOVE == 65536 and M.FWD_LOOPS_ABOVE == 163840
    assert M.grid_for(1, 2) == 1 and M.grid_for(65536, 2) == 512 and M.grid_for(10 ** 6, 5) == 1280
    assert M.wgrad_depth(3 * 65536 + 37) == 32 + 4 + 4 + 512 + 1
    h = M.round_half(torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.9, 65520.0, -2.0 ** -28, 2.0 ** -25,
                                   3 * 2.0 ** -25, float("nan")], dtype=torch.float64))
    want = [1.0, 1.0 + 2.0 ** -9, 65504.0, float("inf"), -0.0, 0.0, 2.0 ** -23, float("nan")]
    assert np.array_equal(h.numpy(), np.array(want), equal_nan=True)
    assert np.signbit(h[4].item())
    v = torch.cat([torch.randn(100000) * s for s in (1e-7, 1e-4, 1.0, 3e4)])     # fp32 values: torch's own conversion
    assert torch.equal(M.round_half(v), v.half().double())


BIG = 3 * 65536 + 37   # the backward's looping size: where a double count is smallest against the sum's bound

# fault -> (half mode, shape, rows, the assertion that has to fail)
SEEDED = [
    ("dout_unrounded", True, (32, 64, 3), N_REF, "dx_identical"),
    ("dout_unrounded", True, (8, 32, 2), N_REF, "dx_identical"),
    ("bias_unrounded", True, (32, 64, 3), N_REF, "y_identical"),
    ("bias_unrounded", True, (8, 32, 2), N_REF, "y_identical"),
    ("hidden_grad_unrounded", True, (32, 64, 3), N_REF, "dx_identical"),
    ("hidden_grad_unrounded", True, (8, 32, 2), N_REF, "dx_identical"),
    ("last_row_twice", True, (32, 64, 3), BIG, "wgrad_bound"),
    ("last_row_twice", False, (8, 32, 2), BIG, "wgrad_bound"),
    ("poison_row", True, (16, 64, 3), BIG, "wgrad_bound"),
    ("poison_row", False, (32, 64, 3), BIG, "wgrad_bound"),
    ("swap_pairs", True, (32, 64, 3), 33, "dx_identical"),
    ("swap_pairs", False, (30, 64, 2), 33, "dx_bound"),
]


@pytest.mark.parametrize("fault,half,shape,n,broken", SEEDED)
def test_seeded_fault_is_caught(fault, half, shape, n, broken):
    x, ws, dout = M.make_case(*shape, n)
    if half:
        ref = M.model_half(x, ws, dout, planes_half=True)
        fig, fails = M.check_half(M.as_got(M.model_half(x, ws, dout, planes_half=True, faults=[fault])), ref, M.k_cap(*shape))
        clean = M.check_half(M.as_got(ref), ref, M.k_cap(*shape))[1]
    else:
        ref = M.model_fp32(x, ws, dout)
        fig, fails = M.check_fp32(M.as_got(M.model_fp32(x, ws, dout, faults=[fault])), ref)
        clean = M.check_fp32(M.as_got(ref), ref)[1]
    print(fault, shape, fig)
    assert not clean, clean
    assert broken in fails, (fault, fails, fig)


def test_seeded_mask_fault_is_caught_by_the_zero_edge():
    """A mask taken before the rounding differs from the right one only where a positive pre-activation rounds to zero:
    the zero edge case holds such a unit."""
    x, ws, dout = M.zero_edge_case()
    for half_planes in (False, True):
        ok = M.model_half(x, ws, dout, planes_half=half_planes)
        assert M.check_zero_edge(M.as_got(ok)) == []
        assert np.signbit(M.round_half(ok["pre"][0])[0, 0].item())     # unit 0 IS negative zero once rounded
        bad = M.model_half(x, ws, dout, planes_half=half_planes, faults=["mask_pre_rounding"])
        assert "zero_unit_gradient" in M.check_zero_edge(M.as_got(bad))
        assert "dx_identical" in M.check_half(M.as_got(bad), ok, M.k_cap(2, 32, 2))[1]


def test_nonfinite_cases_are_nonfinite_in_the_model():
    for kind in ("x", "dout"):
        x, ws, dout = M.nonfinite_case(kind, 8, 32, 2)
        ref = M.model_half(x, ws, dout, planes_half=True)
        assert M.check_nonfinite(M.as_got(ref), ref) == []
        assert not torch.isfinite(ref["dW"][0]).all()
        clean = M.model_half(*M.make_case(8, 32, 2, 100, seed=9), planes_half=True)
        assert M.check_nonfinite(M.as_got(clean), ref) != []
