"""GroupNorm (+ SiLU) of the diffusion half as two HIP kernels per direction (csrc/groupnorm.hip, Part 10 of
include/mi3d.h) behind torch.autograd: binary16 in, binary16 out, fp32 arithmetic in registers.  The output is the
binary16 rounding of the fp32 result - what autocast hands the convolution or Linear that consumes a GroupNorm.  Input
gradient only: the affine parameters of both guidance networks are frozen.

Two kernel families, chosen by the input's memory format (`layout`): contiguous [B, C, ...] -> the NCHW kernels,
torch.channels_last [B, C, H, W] -> the NHWC kernels (C % 8 == 0, 16-byte aligned).  The output keeps the input's format."""
import torch
from torch.autograd import Function

from . import _lib as L

ACTS = {None: 0, "silu": 1}


def chunks(hw):
    """Chunks per (sample, channel) row: the workspaces hold one entry per (row, chunk)."""
    return int(L.lib().mi3d_groupnorm_chunks(int(hw)))


def _dims(x, groups):
    B, C = int(x.shape[0]), int(x.shape[1])
    HW = x[0, 0].numel()
    if C % groups:
        raise L.Mi3dError(f"{groups} groups do not divide {C} channels")
    return B, C, HW, int(groups)


def layout(x, groups, family=None):
    """"nchw" for a contiguous tensor, "nhwc" for a channels-last one that the NHWC kernels take, None for anything else.
    A tensor that is both (H = W = 1) is "nchw" unless family="nhwc" asks for the other kernels."""
    if x.is_contiguous() and family != "nhwc":
        return "nchw"
    if family == "nchw" or x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last) or x.data_ptr() % 16:
        return None
    B, C, H, W = x.shape
    if groups <= 0 or C % groups or C % 8 or B == 0 or H * W == 0:
        return None
    return "nhwc" if L.lib().mi3d_groupnorm_nhwc_spans(C, H * W, int(groups)) else None


def _like(x, t, name):
    """t in x's memory format, or an error: the kernels index both with the same strides."""
    if t.shape != x.shape:
        raise L.Mi3dError(f"{name} must have x's shape {tuple(x.shape)} (got {tuple(t.shape)})")
    ok = t.is_contiguous() if x.is_contiguous() else t.is_contiguous(memory_format=torch.channels_last)
    if not (t.is_cuda and t.dtype == torch.float16 and ok):
        raise L.Mi3dError(f"{name} must be a binary16 GPU tensor in x's memory format (got {t.dtype} on {t.device})")
    return t


def _typed(x, groups, family=None):
    """x validated, its kernel family, the entry-point prefix and the workspace entries per sample."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float16):
        raise L.Mi3dError(f"x must be a binary16 GPU tensor (got {x.dtype} on {x.device})")
    fmt = layout(x, groups, family) if x.dim() >= 2 and groups > 0 and x.shape[1] % groups == 0 else "nchw"
    if fmt is None:
        raise L.Mi3dError("x must be contiguous, or channels-last with a multiple of 8 channels and 16-byte aligned")
    B, C, HW, G = _dims(x, groups)
    if fmt == "nchw":
        L.dev_typed(x, "x", torch.float16)
        return B, C, HW, G, "mi3d_groupnorm_", C * chunks(HW)
    return B, C, HW, G, "mi3d_groupnorm_nhwc_", int(L.lib().mi3d_groupnorm_nhwc_spans(C, HW, G)) * G


def forward(x, weight, bias, groups, eps, act=None, family=None):
    """(y binary16 like x, mean fp32 [B, G], rstd fp32 [B, G]); x binary16 [B, C, ...], contiguous or channels-last;
    weight / bias fp32 [C].  family: see layout()."""
    B, C, HW, G, pre, entries = _typed(x, groups, family)
    L.dev_f32(weight, "weight", x.shape[1])
    L.dev_f32(bias, "bias", x.shape[1])
    ws = torch.empty(B * entries, 3, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    mean = torch.empty(B, G, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, G, dtype=torch.float32, device=x.device)
    with L.on(x):
        L.call(pre + "stats", L.ptr(x), B, C, HW, G, L.ptr(ws), L.stream(x))
        L.call(pre + "act_forward", L.ptr(x), L.ptr(ws), L.ptr(weight), L.ptr(bias), B, C, HW, G, float(eps),
               ACTS[act], L.ptr(_like(x, y, "y")), L.ptr(mean), L.ptr(rstd), L.stream(x))
    return y, mean, rstd


def backward(x, dy, mean, rstd, weight, bias, groups, act=None, family=None):
    """dx binary16 like x; dy in x's memory format."""
    B, C, HW, G, pre, entries = _typed(x, groups, family)
    _like(x, dy, "dy")
    partial = torch.empty(B * entries, 2, dtype=torch.float32, device=x.device)
    dx = _like(x, torch.empty_like(x), "dx")
    args = (L.ptr(x), L.ptr(dy), L.ptr(mean), L.ptr(rstd), L.ptr(weight), L.ptr(bias))
    with L.on(x):
        L.call(pre + "act_backward_sums", *args, B, C, HW, G, ACTS[act], L.ptr(partial), L.stream(x))
        L.call(pre + "act_backward", *args, L.ptr(partial), B, C, HW, G, ACTS[act], L.ptr(dx), L.stream(x))
    return dx


class _GroupNormAct(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, act):
        y, mean, rstd = forward(x, weight, bias, groups, eps, act)
        ctx.save_for_backward(x, mean, rstd, weight, bias)
        ctx.meta = (groups, act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, weight, bias = ctx.saved_tensors
        groups, act = ctx.meta
        fmt = torch.contiguous_format if x.is_contiguous() else torch.channels_last
        dx = backward(x, dy.to(torch.float16).contiguous(memory_format=fmt), mean, rstd, weight, bias, groups, act)
        return dx, None, None, None, None, None


def group_norm_act(x, weight, bias, groups, eps, act=None):
    """act(group_norm(x)) in binary16; weight, bias: frozen fp32 [C].  Autocast is off inside the node."""
    if act not in ACTS:
        raise L.Mi3dError(f"act must be None or 'silu' (got {act!r})")
    with torch.autocast("cuda", enabled=False):
        return _GroupNormAct.apply(x, weight, bias, int(groups), float(eps), act)
