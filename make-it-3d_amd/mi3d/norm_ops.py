"""GroupNorm (+ SiLU) of the diffusion half as two HIP kernels per direction (csrc/groupnorm.hip, Part 10 of
include/mi3d.h) behind torch.autograd: binary16 in, binary16 out, fp32 arithmetic in registers.  The output is the
binary16 rounding of the fp32 result - what autocast hands the convolution or Linear that consumes a GroupNorm.  Input
gradient only: the affine parameters of both guidance networks are frozen."""
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


def forward(x, weight, bias, groups, eps, act=None):
    """(y binary16 like x, mean fp32 [B, G], rstd fp32 [B, G]); x binary16 contiguous [B, C, ...], weight / bias fp32 [C]."""
    L.dev_typed(x, "x", torch.float16)
    L.dev_f32(weight, "weight", x.shape[1])
    L.dev_f32(bias, "bias", x.shape[1])
    B, C, HW, G = _dims(x, groups)
    ws = torch.empty(B * C * chunks(HW), 3, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    mean = torch.empty(B, G, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, G, dtype=torch.float32, device=x.device)
    with L.on(x):
        L.call("mi3d_groupnorm_stats", L.ptr(x), B, C, HW, G, L.ptr(ws), L.stream(x))
        L.call("mi3d_groupnorm_act_forward", L.ptr(x), L.ptr(ws), L.ptr(weight), L.ptr(bias), B, C, HW, G, float(eps),
               ACTS[act], L.ptr(y), L.ptr(mean), L.ptr(rstd), L.stream(x))
    return y, mean, rstd


def backward(x, dy, mean, rstd, weight, bias, groups, act=None):
    """dx binary16 like x."""
    L.dev_typed(x, "x", torch.float16)
    L.dev_typed(dy, "dy", torch.float16)
    if dy.shape != x.shape:
        raise L.Mi3dError(f"dy must have x's shape {tuple(x.shape)} (got {tuple(dy.shape)})")
    B, C, HW, G = _dims(x, groups)
    partial = torch.empty(B * C * chunks(HW), 2, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    args = (L.ptr(x), L.ptr(dy), L.ptr(mean), L.ptr(rstd), L.ptr(weight), L.ptr(bias))
    with L.on(x):
        L.call("mi3d_groupnorm_act_backward_sums", *args, B, C, HW, G, ACTS[act], L.ptr(partial), L.stream(x))
        L.call("mi3d_groupnorm_act_backward", *args, L.ptr(partial), B, C, HW, G, ACTS[act], L.ptr(dx), L.stream(x))
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
        dx = backward(x, dy.to(torch.float16).contiguous(), mean, rstd, weight, bias, groups, act)
        return dx, None, None, None, None, None


def group_norm_act(x, weight, bias, groups, eps, act=None):
    """act(group_norm(x)) in binary16; weight, bias: frozen fp32 [C].  Autocast is off inside the node."""
    if act not in ACTS:
        raise L.Mi3dError(f"act must be None or 'silu' (got {act!r})")
    with torch.autocast("cuda", enabled=False):
        return _GroupNormAct.apply(x, weight, bias, int(groups), float(eps), act)
