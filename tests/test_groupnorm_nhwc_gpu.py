"""GPU: the channels-last GroupNorm (+ SiLU) kernels (k_groupnorm_nhwc_* of csrc/groupnorm.hip through mi3d/norm_ops.py)
against an fp64 evaluation of the binary16 input's exact values, with the bound tests/test_groupnorm_gpu.py uses for the
NCHW kernels: the stock route (F.group_norm or the split-statistics node, F.silu, autograd) is measured on the same
inputs under autocast(float16), its result rounded to binary16, and the fused result's max-abs and RMS errors may exceed
that route's by at most a factor of 2.  The figures measured are appended to profiles/groupnorm_nhwc_parity.json before
the assertion.  Then the stand-in networks with a channels-last switch on against off."""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

pytestmark = pytest.mark.gpu

FACTOR = 2.0
CL = torch.channels_last
PARITY_JSON = os.path.join(ROOT, "profiles", "groupnorm_nhwc_parity.json")

# (B, C, G, H, W).  A workgroup owns a span of whole pixels of one sample and a slab of whole groups at least 64 channels
# wide; with 64 channels the span is 128 pixels (mi3d_groupnorm_nhwc_span, asserted below).
SHAPES = [
    (2, 320, 32, 8, 8),       # 10 channels per group: vectors of 8 straddle groups; 4 slabs of 80 channels
    (1, 128, 32, 16, 16),     # 4 channels per group, 2 slabs, 2 spans
    (2, 1280, 32, 4, 4),      # the U-Net's deepest level: 40 per group, 16 slabs, tile rows beyond the 16 pixels idle
    (1, 64, 32, 1, 1),        # one pixel (a tensor that is also NCHW-contiguous: the NHWC kernels are asked for by name)
    (1, 64, 32, 1, 127),      # one pixel short of a span
    (1, 64, 32, 3, 43),       # one pixel more than a span: a second span of a single pixel
    (1, 96, 32, 5, 7),        # 3 channels per group: slabs of 72 channels, a ragged last slab of 24
    (1, 64, 32, 96, 96),      # 34 spans: more than one round of the merge over spans (8 threads per group, 4 loads each)
    (1, 128, 4, 16, 16),      # a group count other than 32: 32 channels per group, 2 groups per slab, 2 spans
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
DISTS = ["randn", "offset30"]


def _inputs(shape, dist, seed=0):
    B, C, G, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    if dist == "offset30":
        x = 30 + 0.5 * x        # mean >> spread: the cancellation case, well inside binary16's range
    w = 1 + 0.5 * torch.randn(C, generator=g)
    b = 0.5 * torch.randn(C, generator=g)
    dy = torch.randn(B, C, H, W, generator=g)
    return (x.half().cuda().contiguous(memory_format=CL), w.cuda(), b.cuda(),
            dy.half().cuda().contiguous(memory_format=CL))


def _module(C, groups, eps, w, b):
    from mi3d import sd_standin as S
    m = S.GroupNorm(groups, C, eps=eps).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _stock(m, x, dy, act):
    """(y, dx) of the stock route under autocast(float16), as binary16."""
    from mi3d import sd_standin as S
    old = S.GN_FUSED
    S.GN_FUSED = False
    try:
        xr = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = m(xr, act=act)
        assert y.dtype == torch.float32
        y.backward(dy.to(y.dtype))
        return y.detach().half(), xr.grad.detach()
    finally:
        S.GN_FUSED = old


def _nhwc_once(x, w, b, dy, groups, eps, act):
    from mi3d import norm_ops
    assert norm_ops.layout(x, groups, family="nhwc") == "nhwc"
    y, mean, rstd = norm_ops.forward(x, w, b, groups, eps, act, family="nhwc")
    dx = norm_ops.backward(x, dy, mean, rstd, w, b, groups, act, family="nhwc")
    for t in (y, dx):
        assert t.dtype == torch.float16 and t.stride() == x.stride()
    return y, mean, rstd, dx


@functools.lru_cache(maxsize=None)
def measure(shape, act, eps, dist):
    """Errors of both routes against fp64: {'y': {'fused': (max, rms), 'stock': (max, rms)}, 'dx': {...}}."""
    B, C, G, H, W = shape
    x, w, b, dy = _inputs(shape, dist)
    xd = x.double().requires_grad_(True)
    yd = F.group_norm(xd, G, w.double(), b.double(), eps)
    yd = F.silu(yd) if act == "silu" else yd
    yd.backward(dy.double())
    ref = {"y": yd.detach(), "dx": xd.grad.detach()}
    y, _, _, dx = _nhwc_once(x, w, b, dy, G, eps, act)
    ys, dxs = _stock(_module(C, G, eps, w, b), x, dy, act)
    out = {}
    for name, (u, v) in (("fused", (y, dx)), ("stock", (ys, dxs))):
        for k, t in (("y", u), ("dx", v)):
            e = t.double() - ref[k]
            out.setdefault(k, {})[name] = (float(e.abs().max()), float(e.pow(2).mean().sqrt()))
    return out


def _record(key, figures):
    try:
        rows = json.load(open(PARITY_JSON)) if os.path.exists(PARITY_JSON) else {}
        rows[key] = figures
        json.dump(rows, open(PARITY_JSON, "w"), indent=1, sort_keys=True)
    except OSError:      # a read-only checkout: the figures are still printed
        pass


def test_the_span_is_what_the_shapes_assume():
    from mi3d import _lib
    lib = _lib.lib()
    assert lib.mi3d_groupnorm_nhwc_span(64, 127, 32) == 127 and lib.mi3d_groupnorm_nhwc_spans(64, 127, 32) == 1
    assert lib.mi3d_groupnorm_nhwc_span(64, 129, 32) == 128 and lib.mi3d_groupnorm_nhwc_spans(64, 129, 32) == 2
    assert lib.mi3d_groupnorm_nhwc_spans(64, 96 * 96, 32) == 34


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("act", [None, "silu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_fp64_no_worse_than_the_stock_route(shape, act, eps, dist):
    r = measure(shape, act, eps, dist)
    _record(f"{'x'.join(map(str, shape))},act={act},eps={eps:g},{dist}", r)
    for k in ("y", "dx"):
        (fm, fr), (sm, sr) = r[k]["fused"], r[k]["stock"]
        msg = f"{k}: fused max {fm:.3e} rms {fr:.3e} | stock max {sm:.3e} rms {sr:.3e}"
        print(msg)
        assert fm == fm and fr == fr, msg     # not NaN
        assert fm <= FACTOR * sm and fr <= FACTOR * sr, msg


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_calls_are_bit_identical(shape):
    x, w, b, dy = _inputs(shape, "offset30", seed=1)
    a = _nhwc_once(x, w, b, dy, shape[2], 1e-6, "silu")
    c = _nhwc_once(x, w, b, dy, shape[2], 1e-6, "silu")
    for u, v, name in zip(a, c, ("y", "mean", "rstd", "dx")):
        assert torch.equal(u, v), name


def test_saved_statistics_match_fp64():
    shape = SHAPES[7]
    x, w, b, dy = _inputs(shape, "offset30", seed=2)
    _, mean, rstd, _ = _nhwc_once(x, w, b, dy, shape[2], 1e-5, None)
    xg = x.double().contiguous().view(shape[0], shape[2], -1)
    var, mu = torch.var_mean(xg, dim=-1, unbiased=False)
    # the bounds of the NCHW test: fp32 carries 2^-24 relative per rounding, a handful of merges per element path
    assert float(((mean.double() - mu) / mu).abs().max()) < 1e-6
    assert float((rstd.double() * torch.sqrt(var + 1e-5) - 1).abs().max()) < 1e-5


def test_the_module_routes_by_memory_format_and_keeps_it():
    """Through GroupNorm.forward and autograd: a channels-last input takes the NHWC entry points, a contiguous one the
    NCHW ones, and y and dx come back in the input's format with the same values either way (to the parity factor)."""
    from mi3d import _lib as L
    shape = SHAPES[0]
    B, C, G, H, W = shape
    x, w, b, dy = _inputs(shape, "randn", seed=3)
    m = _module(C, G, 1e-5, w, b)
    seen, orig = [], L.call

    def spy(name, *a):
        seen.append(name)
        return orig(name, *a)
    outs = {}
    L.call = spy
    try:
        for fmt in (CL, torch.contiguous_format):
            del seen[:]
            xr = x.contiguous(memory_format=fmt).clone(memory_format=torch.preserve_format).requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.float16):
                y = m(xr, act="silu")
            y.backward(dy.contiguous())      # a contiguous gradient: the node brings it into x's format
            assert y.dtype == torch.float16 and y.is_contiguous(memory_format=fmt)
            assert xr.grad.is_contiguous(memory_format=fmt)
            assert len(seen) == 4 and all(("_nhwc_" in n) == (fmt is CL) for n in seen), seen
            outs[fmt] = (y.detach().float(), xr.grad.float())
    finally:
        L.call = orig
    for u, v in zip(outs[CL], outs[torch.contiguous_format]):
        # both are binary16 roundings of fp32 results that differ in summation order: a few ulps of binary16
        assert float((u - v).abs().max()) <= 4 * 2.0 ** -10 * float(v.abs().max())


def _standin():
    from mi3d import sd_standin as S
    g = S.StableDiffusionStandIn(torch.device("cuda:0"), unet_kw=dict(ch=(64, 128), ctx_dim=64), vae_kw=dict(ch=(32, 64)),
                                 graph_unet=False)
    return S, g


def _guidance(S, g, text, flags):
    """(U-Net output, latents, image gradient) of one guidance call on seeded inputs under the given switches."""
    old = (S.GN_FUSED, S.VAE_CHANNELS_LAST, S.UNET_CHANNELS_LAST)
    S.GN_FUSED, S.VAE_CHANNELS_LAST, S.UNET_CHANNELS_LAST = flags
    try:
        torch.manual_seed(11)
        rgb = torch.rand(2, 3, 32, 32, device="cuda", requires_grad=True)
        with torch.autocast("cuda", dtype=torch.float16):
            latents = g.encode_imgs(rgb)
            with torch.no_grad():
                t = torch.tensor([500], device="cuda")
                eps = g._unet_forward(latents.detach().half(), t, text.half()).float()
            latents.backward(gradient=eps.to(latents.dtype))
        return eps, latents.detach().float(), rgb.grad.detach()
    finally:
        S.GN_FUSED, S.VAE_CHANNELS_LAST, S.UNET_CHANNELS_LAST = old


@pytest.mark.parametrize("which", ["vae", "unet", "both"])
def test_standin_channels_last_against_nchw(which):
    """A small VAE encoder (ch = (32, 64)) and U-Net (ch = (64, 128): one attention head of 64 at the first level; its
    skip concatenations give 192 channels, 6 per group), 32 x 32 images, batch 2: with a channels-last switch on against
    off, the U-Net output, the latents and the image gradient differ by no more than 2 x what GN_FUSED on / off differ by
    on the same inputs (measured here, max-abs relative to the largest value, as profiles/sd_knobs_gn_fused.json does)."""
    S, g = _standin()
    text = torch.randn(2, 7, 64, generator=torch.Generator().manual_seed(3)).cuda()
    base = _guidance(S, g, text, (True, False, False))
    unfused = _guidance(S, g, text, (False, False, False))
    cl = _guidance(S, g, text, (True, which in ("vae", "both"), which in ("unet", "both")))
    assert g.vae_encoder.channels_last == (which in ("vae", "both"))
    assert g.unet.channels_last == (which in ("unet", "both"))
    for name, a, r, c in zip(("eps", "latents", "image_grad"), base, unfused, cl):
        scale = float(a.abs().max())
        ref, got = float((r - a).abs().max()) / scale, float((c - a).abs().max()) / scale
        msg = f"{name}: channels-last vs NCHW {got:.3e} | GN_FUSED off vs on {ref:.3e}"
        print(msg)
        assert torch.isfinite(c).all() and got <= FACTOR * ref, msg
