"""GPU: the fused GroupNorm (+ SiLU) kernels (csrc/groupnorm.hip, mi3d/norm_ops.py) against an fp64 reference on the
binary16 input's exact values.  The bound is not a number fixed in advance: the stock route (F.group_norm or the
split-statistics node, F.silu, autograd) is measured on the same inputs under autocast(float16), its result rounded to
binary16 as the consuming conv sees it, and the fused result's max-abs and RMS errors may exceed that route's by at most a
factor of 2 (a one-ulp binary16 flip where the two fp32 values straddle a rounding boundary).  The pairs measured on an
MI355X for the shapes below are recorded in profiles/groupnorm_parity.json."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTOR = 2.0

# [B, C, H, W], groups - the smallest shapes at which the kernels can go wrong (a row is H * W contiguous elements, cut
# into chunks of 8192):
SHAPES = [
    ((1, 32, 5, 7), 32),       # rows of 35: every second one starts off a 4-byte boundary; scalar head and tail only
    ((2, 64, 17, 19), 32),     # B > 1, two channels per group, rows neither 16-byte aligned nor vector multiples
    ((1, 64, 96, 100), 32),    # rows of 9600 = 8192 + 1408: two chunks per row, four per group, a ragged last one
    ((2, 1280, 8, 8), 32),     # the U-Net's deepest level: 40 channels per group, 40 triples merged per workgroup
    ((1, 128, 64, 64), 4),     # a group count other than 32; 32 channels per group (the split-statistics stock route)
    ((1, 128, 258, 256), 4),   # rows of 66048 = 8 x 8192 + 512: 9 chunks x 32 channels = 288 partials per group, so the
                               # merge loops of k_groupnorm_apply / k_groupnorm_bwd go round twice (the second ragged)
]
IDS = ["1x32x5x7", "2x64x17x19", "1x64x96x100", "2x1280x8x8", "1x128x64x64g4", "1x128x258x256g4"]
MERGE_BLOCK = 256              # kBlock of csrc/groupnorm.hip: partials merged per round, `i += kBlock`
DISTS = ["randn", "offset30"]


def _inputs(shape, dist, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if dist == "offset30":
        x = 30 + 0.5 * x        # mean >> spread: the cancellation case, well inside binary16's range
    C = shape[1]
    w = 1 + 0.5 * torch.randn(C, generator=g)
    b = 0.5 * torch.randn(C, generator=g)
    dy = torch.randn(shape, generator=g)
    return x.half().cuda(), w.cuda(), b.cuda(), dy.half().cuda()


def _module(C, groups, eps, w, b):
    from mi3d import sd_standin as S
    m = S.GroupNorm(groups, C, eps=eps).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _run(m, x, dy, act, fused):
    """(y, dx) as binary16 through the module under autocast(float16); the stock route's fp32 output is rounded to
    binary16 (what the conv behind it gets), its input gradient arrives in binary16 through the cast's backward."""
    from mi3d import sd_standin as S
    old = S.GN_FUSED
    S.GN_FUSED = fused
    try:
        xr = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = m(xr, act=act)
        assert y.dtype == (torch.float16 if fused else torch.float32)
        y.backward(dy.to(y.dtype))
        return y.detach().half(), xr.grad.detach()
    finally:
        S.GN_FUSED = old


@functools.lru_cache(maxsize=None)
def measure(shape, groups, act, eps, dist):
    """Errors of both routes against fp64: {'y': {'fused': (max, rms), 'stock': (max, rms)}, 'dx': {...}}."""
    x, w, b, dy = _inputs(shape, dist)
    xd = x.double().requires_grad_(True)
    yd = F.group_norm(xd, groups, w.double(), b.double(), eps)
    yd = F.silu(yd) if act == "silu" else yd
    yd.backward(dy.double())
    ref = {"y": yd.detach(), "dx": xd.grad.detach()}
    m = _module(shape[1], groups, eps, w, b)
    out = {}
    for name, fused in (("fused", True), ("stock", False)):
        y, dx = _run(m, x, dy, act, fused)
        assert y.dtype == dx.dtype == torch.float16
        for k, v in (("y", y), ("dx", dx)):
            e = v.double() - ref[k]
            out.setdefault(k, {})[name] = (float(e.abs().max()), float(e.pow(2).mean().sqrt()))
    return out


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("act", [None, "silu"])
@pytest.mark.parametrize("shape,groups", SHAPES, ids=IDS)
def test_parity_with_fp64_no_worse_than_the_stock_route(shape, groups, act, eps, dist):
    r = measure(shape, groups, act, eps, dist)
    for k in ("y", "dx"):
        (fm, fr), (sm, sr) = r[k]["fused"], r[k]["stock"]
        msg = f"{k}: fused max {fm:.3e} rms {fr:.3e} | stock max {sm:.3e} rms {sr:.3e}"
        print(msg)
        assert fm == fm and fr == fr, msg     # not NaN
        assert fm <= FACTOR * sm and fr <= FACTOR * sr, msg


def test_the_last_shape_reaches_the_second_round_of_the_merge():
    """S = (C / G) x chunks partials per group, merged MERGE_BLOCK per round by k_groupnorm_apply / k_groupnorm_bwd; the
    chunk count is the library's own.  Every other shape stays within one round (the largest is 40)."""
    from mi3d import _lib as L

    def partials(shape, groups):
        return shape[1] // groups * int(L.lib().mi3d_groupnorm_chunks(shape[2] * shape[3]))
    assert [partials(s, g) for s, g in SHAPES[:-1]] == [1, 2, 4, 40, 32]
    S = partials(*SHAPES[-1])
    assert S == 288 and MERGE_BLOCK < S < 2 * MERGE_BLOCK and S % 64 != 0     # a second round, ragged: half a wave


def _fused_once(x, w, b, dy, groups, eps, act):
    from mi3d import norm_ops
    y, mean, rstd = norm_ops.forward(x, w, b, groups, eps, act)
    dx = norm_ops.backward(x, dy, mean, rstd, w, b, groups, act)
    return y, mean, rstd, dx


@pytest.mark.parametrize("shape,groups", SHAPES, ids=IDS)
def test_two_calls_are_bit_identical(shape, groups):
    x, w, b, dy = _inputs(shape, "offset30", seed=1)
    a = _fused_once(x, w, b, dy, groups, 1e-6, "silu")
    c = _fused_once(x, w, b, dy, groups, 1e-6, "silu")
    for u, v, name in zip(a, c, ("y", "mean", "rstd", "dx")):
        assert torch.equal(u, v), name


def test_saved_statistics_match_fp64():
    shape, groups = SHAPES[2]
    x, w, b, dy = _inputs(shape, "offset30", seed=2)
    _, mean, rstd, _ = _fused_once(x, w, b, dy, groups, 1e-5, None)
    xg = x.double().view(shape[0], groups, -1)
    var, mu = torch.var_mean(xg, dim=-1, unbiased=False)
    # fp32 carries 2^-24 relative per rounding; a handful of merges per element path: 1e-6 relative is generous for the
    # mean, and the variance (spread 0.5 around 30) sees the mean's error squared only
    assert float(((mean.double() - mu) / mu).abs().max()) < 1e-6
    assert float((rstd.double() * torch.sqrt(var + 1e-5) - 1).abs().max()) < 1e-5


def test_captured_graph_replays_like_eager():
    from mi3d import norm_ops
    shape, groups = SHAPES[1]
    xs = [_inputs(shape, d, seed=s) for d, s in (("randn", 3), ("offset30", 4))]
    w, b = xs[0][1], xs[0][2]
    eager = [norm_ops.forward(x[0], w, b, groups, 1e-5, "silu")[0] for x in xs]
    static = xs[0][0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        norm_ops.forward(static, w, b, groups, 1e-5, "silu")
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = norm_ops.forward(static, w, b, groups, 1e-5, "silu")[0]
    for x, want in zip(xs, eager):
        static.copy_(x[0])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_resblock_fused_and_stock_agree_through_fp64():
    """A ResBlock(32, 64) under autocast with GN_FUSED on and off, both against an fp64 copy of the block: the fused block's
    errors stay within the parity factor of the stock block's (convolutions and rounding points are the same in both)."""
    import copy
    from mi3d import sd_standin as S
    torch.manual_seed(7)
    blk = S.ResBlock(32, 64).cuda()
    for p in blk.parameters():
        p.requires_grad_(False)
    x = torch.randn(1, 32, 24, 24, device="cuda").half().float()    # binary16 values, as a conv under autocast delivers
    dy = torch.randn(1, 64, 24, 24, device="cuda")
    xd = x.double().requires_grad_(True)
    yd = copy.deepcopy(blk).double()(xd)
    yd.backward(dy.double())
    errs = {}
    old = S.GN_FUSED
    try:
        for fused in (True, False):
            S.GN_FUSED = fused
            xr = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.float16):
                # the block's input comes from a conv in the networks: binary16
                y = blk(xr.half())
            y.backward(dy.to(y.dtype))
            ey, eg = y.detach().double() - yd.detach(), xr.grad.double() - xd.grad
            errs[fused] = [float(e.abs().max()) for e in (ey, eg)] + [float(e.pow(2).mean().sqrt()) for e in (ey, eg)]
    finally:
        S.GN_FUSED = old
    msg = f"(y max, dx max, y rms, dx rms): fused {errs[True]} | stock {errs[False]}"
    print(msg)
    for f, s in zip(errs[True], errs[False]):
        assert f <= FACTOR * s, msg


@pytest.mark.parametrize("case", ["fp32", "non_contiguous", "trainable_affine"])
def test_fallback_is_bit_identical_to_the_switch_off(case):
    from mi3d import sd_standin as S
    shape, groups = SHAPES[1]
    x, w, b, _ = _inputs(shape, "randn", seed=5)
    m = _module(shape[1], groups, 1e-5, w, b)
    if case == "fp32":
        x = x.float()
    elif case == "non_contiguous":
        x = x.transpose(2, 3)
        assert not x.is_contiguous()
    else:
        m.weight.requires_grad_(True)
    outs = []
    old = S.GN_FUSED
    try:
        for fused in (True, False):
            S.GN_FUSED = fused
            with torch.autocast("cuda", dtype=torch.float16):
                outs.append(m(x, act="silu").detach())
    finally:
        S.GN_FUSED = old
    assert outs[0].dtype == outs[1].dtype == torch.float32
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("act", [None, "silu"])
def test_an_inf_in_x_never_gives_a_silently_finite_group(act):
    from mi3d import norm_ops
    shape, groups = SHAPES[1]
    x, w, b, _ = _inputs(shape, "randn", seed=6)
    # rows are 323 elements; row r starts 323 r elements in, so its scalar head is (-323 r) mod 8 elements long
    x[1, 5, 0, 0] = float("inf")           # row 69 starts at 7 mod 8: its first element is the scalar head
    x[0, 62, 16, 18] = float("inf")        # row 62 starts at 2 mod 8: head 6, 39 vectors, the last 5 are the scalar tail
    x[0, 10, 8, 8] = float("inf")          # row 10 starts at 6 mod 8: element 160 lies in a vector
    y, mean, rstd = norm_ops.forward(x, w, b, groups, 1e-5, act)
    per = shape[1] // groups
    clean = torch.ones(shape[0], groups, dtype=torch.bool, device="cuda")
    for bi, c in ((1, 5), (0, 62), (0, 10)):
        g = c // per
        assert not torch.isfinite(y[bi, g * per:(g + 1) * per]).any()
        clean[bi, g] = False
    assert torch.isfinite(y.view(shape[0], groups, -1)[clean]).all()


def test_bad_arguments_are_refused_not_launched():
    from mi3d import _lib as L
    from mi3d import norm_ops
    x, w, b, _ = _inputs((1, 32, 5, 7), "randn")
    with pytest.raises(L.Mi3dError):
        norm_ops.forward(x, w, b, 5, 1e-5)            # 5 does not divide 32
    with pytest.raises(L.Mi3dError):
        norm_ops.forward(x.float(), w, b, 32, 1e-5)   # fp32 input: the node is binary16 only
    with pytest.raises(L.Mi3dError):
        norm_ops.forward(x, w.half(), b, 32, 1e-5)    # the affine pair is fp32
