"""The field's MLP as ONE matrix-core kernel per direction (csrc/field.hip, Part 4 of include/mi3d.h) behind
torch.autograd.  Under torch.autocast(float16) the kernel runs its binary16-MFMA mode, which rounds exactly where
autocast rounds an nn.Linear stack; otherwise it is exact fp32."""
import torch
from torch.autograd import Function

from . import _lib as L
from . import grid_ops


def supported(dim_in, dim_hidden, dim_out, num_layers):
    return bool(L.lib().mi3d_mlp_supported(int(dim_in), int(dim_hidden), int(dim_out), int(num_layers)))


def layer_args(layers):
    """(W1, b1, W2, b2, W_last, b_last) of a 2- or 3-layer stack; the middle pair is None for two layers (the C ABI
    reads a null W2 / b2 as "two layers")."""
    layers = list(layers)
    if len(layers) == 3:
        l1, l2, l3 = layers
        return (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    if len(layers) == 2:
        l1, l3 = layers
        return (l1.weight, l1.bias, None, None, l3.weight, l3.bias)
    raise L.Mi3dError(f"the matrix-core MLP has 2 or 3 layers, not {len(layers)}")


def _weights(ts):
    return [None if t is None else L.dev_f32(t.contiguous(), "weight") for t in ts]


class _FusedMLP(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, W1, b1, W2, b2, W3, b3, half_mode):
        x = L.dev_f32(x.contiguous(), "x", W1.shape[1])
        ws = _weights((W1, b1, W2, b2, W3, b3))
        n = x.shape[0]
        out = torch.empty(n, W3.shape[0], dtype=torch.float32, device=x.device)
        dims = (W1.shape[1], W1.shape[0], W3.shape[0])
        with L.on(x):
            grid_ops._timed("mlp_fwd", lambda: L.call(
                "mi3d_mlp_forward", L.ptr(x), 0, 0, n, *[L.ptr(t) for t in ws], *dims, int(half_mode), L.ptr(out),
                L.stream(x)), n)
        ctx.save_for_backward(x, *ws)
        ctx.meta = (dims, int(half_mode))
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        x, *ws = ctx.saved_tensors
        dims, half_mode = ctx.meta
        dout = L.dev_f32(dout.float().contiguous(), "dout", dims[2])
        n = x.shape[0]
        dx = torch.empty_like(x)
        grads = [None if t is None else torch.zeros_like(t) for t in ws]
        with L.on(x):
            grid_ops._timed("mlp_bwd", lambda: L.call(
                "mi3d_mlp_backward", L.ptr(x), 0, 0, L.ptr(dout), n, *[L.ptr(t) for t in ws], *dims, half_mode, L.ptr(dx),
                0, *[L.ptr(g) for g in grads], L.stream(x)), n)
        return (dx, *grads, None)


_PARAM_GRADS = ("dW1", "db1", "dW2", "db2", "dW3", "db3")


class _FusedMLPGrad(Function):
    """The first-order backward as a node of its own: (dx, dW1, db1, dW2, db2, dW3, db3) from (x, dout, weights) by the
    unchanged mi3d_mlp_backward launch (two layers: W2, b2 and their gradients are None).  Its backward is the second-order
    pass (mi3d_mlp_backward_backward) for the gradient r arriving at dx; the parameter gradients stay once
    differentiable: a gradient sent into one raises, it is never a silent zero."""

    @staticmethod
    def forward(ctx, x, dout, W1, b1, W2, b2, W3, b3):
        ws = [W1, b1, W2, b2, W3, b3]
        dims = (W1.shape[1], W1.shape[0], W3.shape[0])
        n = x.shape[0]
        dx = torch.empty_like(x)
        grads = [None if t is None else torch.zeros_like(t) for t in ws]
        with L.on(x):
            grid_ops._timed("mlp_bwd", lambda: L.call(
                "mi3d_mlp_backward", L.ptr(x), 0, 0, L.ptr(dout), n, *[L.ptr(t) for t in ws], *dims, 0, L.ptr(dx),
                0, *[L.ptr(g) for g in grads], L.stream(x)), n)
        ctx.save_for_backward(x, dout, *ws)
        ctx.dims = dims
        ctx.set_materialize_grads(False)
        return (dx, *grads)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, r, *param_grads):
        hit = [nm for nm, g in zip(_PARAM_GRADS, param_grads) if g is not None]
        if hit:
            raise L.Mi3dError(f"fused_mlp(second_order=True): a gradient arrived at {', '.join(hit)} - the MLP's parameter "
                              "gradients are once differentiable; only its input gradient has a second-order pass")
        x, dout, *ws = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_dout, want_w = need[1], need[2] or need[4] or need[6]
        if r is None or not (want_dout or want_w):
            return (None,) * 8
        r = L.dev_f32(r.float().contiguous(), "r", ctx.dims[0])
        n = x.shape[0]
        g_dout = torch.empty_like(dout) if want_dout else None
        gW = [torch.zeros_like(ws[i]) if want_w and ws[i] is not None else None for i in (0, 2, 4)]
        with L.on(x):
            grid_ops._timed("mlp_bwd2", lambda: L.call(
                "mi3d_mlp_backward_backward", L.ptr(x), L.ptr(dout), L.ptr(r), n, *[L.ptr(t) for t in ws], *ctx.dims,
                L.ptr(g_dout), *[L.ptr(g) for g in gW], L.stream(x)), n)
        # x and the biases reach dx through the piecewise constant masks only: exact zeros, returned as None
        return (None, g_dout, gW[0] if need[2] else None, None, gW[1] if need[4] else None, None,
                gW[2] if need[6] else None, None)


class _FusedMLP2(Function):
    """_FusedMLP in exact fp32 whose backward is itself differentiable (fused_mlp(second_order=True)): the same forward
    launch; the backward hands the same mi3d_mlp_backward launch to _FusedMLPGrad."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, W1, b1, W2, b2, W3, b3):
        ws = [W1, b1, W2, b2, W3, b3]
        n = x.shape[0]
        out = torch.empty(n, W3.shape[0], dtype=torch.float32, device=x.device)
        dims = (W1.shape[1], W1.shape[0], W3.shape[0])
        with L.on(x):
            grid_ops._timed("mlp_fwd", lambda: L.call(
                "mi3d_mlp_forward", L.ptr(x), 0, 0, n, *[L.ptr(t) for t in ws], *dims, 0, L.ptr(out), L.stream(x)), n)
        ctx.save_for_backward(x, *ws)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        x, *ws = ctx.saved_tensors
        dout = L.dev_f32(dout.float().contiguous(), "dout", ws[4].shape[0])
        return _FusedMLPGrad.apply(x, dout, *ws)


def fused_mlp(x, layers, half_mode=None, second_order=False):
    """layers: the two or three nn.Linear modules.  half_mode None = follow torch.autocast.
    second_order: the input gradient can be differentiated again (create_graph=True) with respect to the upstream gradient
    and the weights - exact fp32 only; the parameter gradients stay once differentiable (a gradient sent into one raises),
    and the second-order gradients with respect to x and the biases are exact zeros, returned as None."""
    if half_mode is None:
        half_mode = torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16
    args = layer_args(layers)
    if second_order:
        if half_mode:
            raise L.Mi3dError('fused_mlp(second_order=True) is exact fp32 only: run it under '
                              'torch.autocast("cuda", enabled=False)')
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, *args)):
            # made contiguous out here, where autograd sees it: the node saves its own inputs, graph and all
            x = L.dev_f32(x.float().contiguous(), "x", args[0].shape[1])
            return _FusedMLP2.apply(x, *[None if t is None else L.dev_f32(t.contiguous(), "weight") for t in args])
    return _FusedMLP.apply(x, *args, bool(half_mode))
