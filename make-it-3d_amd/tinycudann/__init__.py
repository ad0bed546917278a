"""`tinycudann` - the slice of the tiny-cuda-nn torch bindings the reference uses
(/root/reference/nerf/network_tcnn.py:10,54-65,107,197): `tcnn.Encoding(n_input_dims=3,
encoding_config={"otype": "HashGrid", ...}, dtype=torch.float32)`, an nn.Module with ONE flat fp32
parameter tensor named `params` (state_dict key `encoder.params`), `forward(x [n,3] in [0,1]) ->
[n, n_levels*2]`, differentiable w.r.t. `params` and w.r.t. `x` when it requires grad, as tiny-cuda-nn's own
`Encoding` is.  The input gradient is first order by default; `Encoding(..., second_order=True)` (this package's own
keyword) produces it by a node that can be differentiated once more - tiny-cuda-nn's backward_backward_input - so a loss
that contains d(output)/dx (an eikonal term, a loss on analytic normals) trains the table and whatever feeds x.  The
parameter gradient stays once differentiable.  Backed by csrc/hashgrid.hip (gfx950).

tiny-cuda-nn itself is an un-vendored, un-pinned dependency of the reference: the arithmetic here
follows its published grid.h (see oracle/hashgrid_ref.c) - PARITY UNPINNED.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from mi3d import _lib as L
from mi3d.grid_ops import GridParameter, _timed

__all__ = ["Encoding", "Network", "NetworkWithInputEncoding"]


class _hashgrid(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, params, cfg):
        shape = x.shape
        x = L.dev_f32(x.contiguous().view(-1, 3), "x", 3)
        params = L.dev_f32(params, "params")
        n = x.shape[0]
        out = torch.empty(n, cfg["n_levels"] * 2, dtype=torch.float32, device=x.device)
        L.launch("mi3d_hashgrid_forward", x, L.ptr(x), n, L.ptr(params), cfg["n_levels"], cfg["base_resolution"],
               cfg["per_level_scale"], cfg["log2_hashmap_size"], L.ptr(out))
        if ctx.needs_input_grad[0]:  # the input gradient gathers from the table again
            ctx.save_for_backward(x, params)
        else:
            ctx.save_for_backward(x)
        ctx.cfg, ctx.n_params, ctx.x_shape = cfg, params.numel(), shape
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, dout):
        x = ctx.saved_tensors[0]
        cfg = ctx.cfg
        dout = L.dev_f32(dout.float().contiguous(), "dout")
        grid = (cfg["n_levels"], cfg["base_resolution"], cfg["per_level_scale"], cfg["log2_hashmap_size"])
        grad_x = grad = None
        if ctx.needs_input_grad[0]:  # first order only here: once_differentiable makes a second derivative raise
            grad_x = torch.empty_like(x)
            L.launch("mi3d_hashgrid_backward_input", x, L.ptr(x), x.shape[0], L.ptr(dout), L.ptr(ctx.saved_tensors[1]),
                     *grid, L.ptr(grad_x))
            grad_x = grad_x.view(ctx.x_shape)
        if ctx.needs_input_grad[1]:
            grad = torch.zeros(ctx.n_params, dtype=torch.float32, device=x.device)
            L.launch("mi3d_hashgrid_backward", x, L.ptr(x), x.shape[0], L.ptr(dout), *grid, L.ptr(grad))
        return grad_x, grad, None


# ------------------------------------------------------------------------------------------------ second order
# Encoding(second_order=True) with an x that requires grad: the same launches, behind nodes whose input gradient can be
# differentiated once more (mi3d_hashgrid_backward_input_backward, include/mi3d.h Part 2).  x and params are saved as the
# INPUTS they are - Encoding.forward casts and flattens x with tracked torch ops in front of the node - so that a backward
# pass run under create_graph=True finds their graph again.

def _grid_args(cfg):
    return (cfg["n_levels"], cfg["base_resolution"], cfg["per_level_scale"], cfg["log2_hashmap_size"])


class _hashgrid_input_grad(Function):
    """dL/dx of _hashgrid2 as a differentiable node.  Its backward is the second-order pass: the rows kernel for the
    gradients of dout and x, the table kernel for the table's, each only where needs_input_grad asks."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, dout, params, cfg):
        dout = L.dev_f32(dout.contiguous(), "dout")
        grad_x = torch.empty_like(x)
        L.launch("mi3d_hashgrid_backward_input", x, L.ptr(x), x.shape[0], L.ptr(dout), L.ptr(params), *_grid_args(cfg),
                 L.ptr(grad_x))
        ctx.save_for_backward(x, dout, params)
        ctx.cfg = cfg
        return grad_x

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, r):
        x, dout, params = ctx.saved_tensors
        r = L.dev_f32(r.float().contiguous().view(-1, 3), "r", 3)
        need_x, need_d, need_p = ctx.needs_input_grad[:3]
        gx = torch.empty_like(x) if need_x else None
        gd = torch.empty_like(dout) if need_d else None
        gp = torch.zeros_like(params) if need_p else None

        def launch(gd, gx, gp):
            L.launch("mi3d_hashgrid_backward_input_backward", x, L.ptr(x), x.shape[0], L.ptr(dout), L.ptr(params), L.ptr(r),
                     *_grid_args(ctx.cfg), L.ptr(gd), L.ptr(gx), L.ptr(gp))
        if gd is not None or gx is not None:
            _timed("second_order_rows", lambda: launch(gd, gx, None), x.shape[0])
        if gp is not None:
            _timed("second_order_table", lambda: launch(None, None, gp), x.shape[0])
        return gx, gd, gp, None


class _hashgrid_param_grad(Function):
    """The parameter gradient of _hashgrid2: _hashgrid's scatter.  It stays once differentiable - differentiating it again
    raises, it is never a silent zero."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, dout, n_params, cfg):
        dout = L.dev_f32(dout.contiguous(), "dout")
        grad = torch.zeros(n_params, dtype=torch.float32, device=x.device)
        L.launch("mi3d_hashgrid_backward", x, L.ptr(x), x.shape[0], L.ptr(dout), *_grid_args(cfg), L.ptr(grad))
        return grad

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError("the hash grid's parameter gradient is once differentiable: only the input gradient has a "
                           "second-order pass")


class _hashgrid2(Function):
    """_hashgrid for Encoding(second_order=True) with an x that requires grad: the same forward launch; the backward hands
    the same first-order launches to the two nodes above, so it can run under create_graph=True."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, params, cfg):
        L.dev_f32(x, "x", 3)
        L.dev_f32(params, "params")
        n = x.shape[0]
        out = torch.empty(n, cfg["n_levels"] * 2, dtype=torch.float32, device=x.device)
        L.launch("mi3d_hashgrid_forward", x, L.ptr(x), n, L.ptr(params), *_grid_args(cfg), L.ptr(out))
        ctx.save_for_backward(x, params)
        ctx.cfg = cfg
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        x, params = ctx.saved_tensors
        dout = dout.float().contiguous()
        grad_x = grad = None
        if ctx.needs_input_grad[0]:
            grad_x = _hashgrid_input_grad.apply(x, dout, params, ctx.cfg)
        if ctx.needs_input_grad[1]:
            grad = _hashgrid_param_grad.apply(x, dout, params.numel(), ctx.cfg)
        return grad_x, grad, None


def grid_levels(n_levels, base_resolution, per_level_scale, log2_hashmap_size):
    """(total entries, offsets[n_levels+1], resolutions, scales) of a HashGrid - host side, via the C ABI."""
    offs = (C.c_uint32 * (n_levels + 1))()
    res = (C.c_uint32 * n_levels)()
    scl = (C.c_float * n_levels)()
    total = L.lib().mi3d_hashgrid_levels(n_levels, base_resolution, per_level_scale, log2_hashmap_size, offs, res,
                                         scl)
    return int(total), np.array(offs, np.uint32), np.array(res, np.uint32), np.array(scl, np.float32)


class Encoding(nn.Module):
    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None, second_order=False):
        super().__init__()
        self.second_order = bool(second_order)
        if n_input_dims != 3:
            raise NotImplementedError("only 3-D inputs (the reference's use)")
        if encoding_config.get("otype", "HashGrid") not in ("HashGrid", "Grid"):
            raise NotImplementedError(f"encoding otype {encoding_config.get('otype')!r}: only HashGrid is built")
        if encoding_config.get("n_features_per_level", 2) != 2:
            raise NotImplementedError("n_features_per_level must be 2")
        if dtype not in (None, torch.float32):
            raise NotImplementedError("dtype=torch.float32 only (network_tcnn.py:64)")
        self.n_input_dims = n_input_dims
        self.encoding_config = dict(encoding_config)
        self.dtype = torch.float32
        self.seed = seed
        self.cfg = dict(n_levels=int(encoding_config.get("n_levels", 16)),
                        base_resolution=int(encoding_config.get("base_resolution", 16)),
                        per_level_scale=float(np.float32(encoding_config.get("per_level_scale", 2.0))),
                        log2_hashmap_size=int(encoding_config.get("log2_hashmap_size", 19)))
        if self.cfg["n_levels"] > 16:
            raise NotImplementedError("at most 16 levels")
        total, self.offsets, self.resolutions, self.scales = grid_levels(**self.cfg)
        self.n_output_dims = self.cfg["n_levels"] * 2
        g = torch.Generator().manual_seed(seed)
        # tcnn: U(-1e-4, 1e-4).  (A GridParameter IS an nn.Parameter; its `.grad` completes a deferred scatter first.)
        self.params = GridParameter((torch.rand(total * 2, generator=g) * 2 - 1) * 1e-4)

    def forward(self, x):
        if not x.is_cuda:
            raise L.Mi3dError("tinycudann.Encoding runs on the GPU only")
        if self.second_order and x.requires_grad and torch.is_grad_enabled():
            return _hashgrid2.apply(x.float().contiguous().view(-1, 3), self.params, self.cfg)
        return _hashgrid.apply(x, self.params, self.cfg)

    def extra_repr(self):
        return f"n_input_dims=3, n_output_dims={self.n_output_dims}, seed={self.seed}, {self.encoding_config}"


def _unsupported(name):
    def ctor(*a, **k):
        raise NotImplementedError(f"tinycudann.{name} is not used by Make-It-3D's hot path and is not provided; "
                                  "the fused field lives in mi3d.field")
    return ctor


Network = _unsupported("Network")
NetworkWithInputEncoding = _unsupported("NetworkWithInputEncoding")
