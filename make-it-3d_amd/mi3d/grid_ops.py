"""Stencil-aware hash-grid encode (autograd): all P evaluation points of every sample in one launch, backward through
the request-minimising scatter of csrc/hashgrid.hip (Part 3 of include/mi3d.h).  The positions' gradient is first order
by default; encode_points(second_order=True) returns it from a node with a second-order pass (the last section below)."""
import contextlib
import ctypes as C

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib as L

EPS = 1e-2  # finite_difference_normal epsilon (network_tcnn.py:115)
# the six offsets of network_tcnn.py:117-122, in that order: +x, -x, +y, -y, +z, -z
STENCIL6 = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32) * np.float32(EPS)


def stencil_offsets(center=True, second=False):
    """[P,3] offsets: optional centre point, the 6-point stencil around x, optionally the same 6 around x2."""
    parts = ([np.zeros((1, 3), np.float32)] if center else []) + [STENCIL6] + ([STENCIL6] if second else [])
    offs = np.concatenate(parts, 0)
    P0 = (1 if center else 0) + 6
    return offs, (P0 if second else offs.shape[0])


# bench.py sets this to {"scatter": [], "encode": []} to collect HIP-event pairs around the two grid kernels
# (events are recorded on torch's current stream, the stream the C ABI launches on).
PROFILE = None


# bench.py sets this to a list to collect, for every binned scatter of ONE untimed step, the fraction of (row, level)
# gradient pairs that are not exactly zero (the emit skips the others, as the reference's atomics add zeros).
CENSUS = None

# bench.py's `dense_gradients` variant sets this: every gradient pair that underflowed to an exact zero is replaced by the
# smallest binary16 subnormal before the scatter, so the emit cannot skip it (instrumentation, like CENSUS; never set by
# the product).
DENSIFY = False


@contextlib.contextmanager
def phase(kind):
    """HIP-event pair around a whole phase of the step (render, guidance, backward, optimizer): bench.py's
    phases_ms_per_step.  A no-op unless bench.py collects."""
    if PROFILE is None:
        yield
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    try:
        yield
    finally:
        e1.record()
        PROFILE.setdefault("phase:" + kind, []).append((e0, e1))


def _timed(kind, launch, evals):
    if PROFILE is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    PROFILE.setdefault(kind, []).append((e0, e1))
    PROFILE.setdefault(kind + "_evals", []).append(evals)


# The fused field's LAST backward pass through a forward (no retain_graph) over the whole stencil writes its feature-gradient
# planes over the feature planes it saved (field_ops._backward_mlp): the two 9.05 GB sets of planes were both live at the C2
# step's memory peak.  False = always a buffer of their own.
INPLACE_GRAD_PLANES = True

# The reference's SDS step back-propagates TWICE through one forward (nerf/sd.py:171 `latents.backward(gradient=grad,
# retain_graph=True)`, then nerf/utils.py:983 `scaler.scale(loss).backward()`).  The first pass reaches the field through
# the image only: sigma / albedo of stencil point 0.  With DEFER_POINT0 the fused field node does NOT scatter that pass's
# point-0 gradient planes on their own: it parks them on the hash table's parameter (a GridParameter) and the second
# pass's scatter takes them along (mi3d_grid_scatter_binned_plus) - one walk over the table instead of two.  Whatever
# is still parked when somebody READS `encoder.params.grad` is scattered then (GridParameter.grad), so every reader -
# GradScaler.unscale_, clip_grad_norm_, the optimizer, an all-reduce bucket - sees the complete gradient, second backward
# or not.  Set to False to scatter every pass immediately (round 3's behaviour).
#
# NOT supported together with readers that bypass Python: torch's DDP reducer hooks the parameter's AccumulateGrad node in
# C++ (no Python-visible attribute), FSDP and register_post_accumulate_grad_hook users read the gradient right after the
# pass - all of them would see it without the parked part whenever no second pass consumes it.  field_ops._may_defer
# therefore turns the deferral off (a) for a parameter that carries post-accumulate-grad hooks and (b) WHENEVER a
# torch.distributed process group is initialised, unless the gradient sync is known to read `.grad` from Python:
# mi3d.dp.FlatGradBucket says so by setting PYTHON_GRAD_SYNC (round 5 tested (a) only and its comment claimed that covered
# DDP - it does not, ADVICE round 5: the reference trainer's DDP wrap, nerf/utils.py:255-258, falls under (b)).
DEFER_POINT0 = True
PYTHON_GRAD_SYNC = False   # set by mi3d.dp.FlatGradBucket: the process group's gradient reader goes through GridParameter.grad


def deferral_allowed():
    """May a backward pass park gradient planes on a GridParameter (see DEFER_POINT0)?"""
    if not DEFER_POINT0:
        return False
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and not PYTHON_GRAD_SYNC:
            return False
    except Exception:  # noqa: BLE001 - a torch build without distributed: nothing can read gradients behind Python's back
        pass
    return True


def _rebuild_grid_parameter(data, requires_grad):
    """pickle / torch.save / mp.spawn: a GridParameter comes back as a GridParameter (module-level, so it pickles)."""
    return GridParameter(data, requires_grad)


class GridParameter(torch.nn.Parameter):
    """The hash table as a parameter (`tinycudann.Encoding.params`): an nn.Parameter whose `.grad` first scatters the
    gradient planes a backward pass may have parked on it (DEFER_POINT0 above).  autograd itself accumulates through the
    C++ accessor and is not affected; assigning `.grad` (zero_grad(set_to_none=True), a bucket view) drops what is
    parked, as it replaces what was accumulated."""

    def __new__(cls, data=None, requires_grad=True):
        if data is None:
            data = torch.empty(0)
        return torch.Tensor._make_subclass(cls, data, requires_grad)

    def __reduce_ex__(self, proto):
        """The per-process state this class keeps in its __dict__ - parked gradient planes with their HIP events
        (`_mi3d_pending`), the cached AccumulateGrad node (`_mi3d_acc_node`) - is not serialisable and means nothing in
        another process: whatever is parked is scattered first (the pickled gradient state is complete), and only
        (data, requires_grad) travel, re-built as a GridParameter (nn.Parameter's own __reduce_ex__ would pickle the
        __dict__ and fail on the events after the first deferred backward pass - ADVICE round 4)."""
        if self.__dict__.get("_mi3d_pending"):
            from . import field_ops
            field_ops.flush_pending(self)
        return _rebuild_grid_parameter, (self.data, self.requires_grad)

    @property
    def grad(self):
        if self.__dict__.get("_mi3d_pending"):
            from . import field_ops
            field_ops.flush_pending(self)
        return torch.Tensor.grad.__get__(self)

    @grad.setter
    def grad(self, value):
        pend = self.__dict__.get("_mi3d_pending")
        if pend:
            pend.clear()
        torch.Tensor.grad.__set__(self, value)


def _offs_arg(offsets):
    offsets = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1, 3)
    return offsets, offsets.ctypes.data_as(C.c_void_p)


class _EncodePoints(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, params, x, x2, offsets, P0, bound, cfg, step, count):
        wants_dx = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if wants_dx and count is not None:
            raise L.Mi3dError("encode_points with a device-side count does not differentiate the positions: the counted "
                              "rows belong to the inference loop")
        shapes = (x.shape, None if x2 is None else x2.shape)
        x = L.dev_f32(x.contiguous().view(-1, 3), "x", 3)
        if x2 is not None:
            x2 = L.dev_f32(x2.contiguous().view(-1, 3), "x2", 3)
        params = L.dev_f32(params, "params")
        offs, offs_p = _offs_arg(offsets)
        P, n = offs.shape[0], x.shape[0]
        out = torch.empty(n * P, cfg["n_levels"] * 2, dtype=torch.float32, device=x.device)
        if count is not None:  # rows past *count are not written by the kernel
            out.zero_()
        with L.on(x):
            _timed("encode_rows", lambda: L.call(
                "mi3d_grid_encode_points", L.ptr(x), L.ptr(x2), n, L.ptr(count), offs_p, int(P0), P, float(bound),
                L.ptr(params), cfg["n_levels"], cfg["base_resolution"], cfg["per_level_scale"],
                cfg["log2_hashmap_size"], L.ptr(out), L.stream(x)), n * P)
        saved = (x, x2 if x2 is not None else x, count if count is not None else x)
        ctx.save_for_backward(*saved, *((params,) if wants_dx else ()))  # the input gradient gathers from the table again
        ctx.meta = (offs, int(P0), float(bound), cfg, float(step), x2 is not None, count is not None, params.numel())
        ctx.shapes = shapes
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, dout):
        x, x2, count = ctx.saved_tensors[:3]
        offs, P0, bound, cfg, step, has_x2, has_count, n_params = ctx.meta
        dout = L.dev_f32(dout.float().contiguous(), "dout")
        grid = (cfg["n_levels"], cfg["base_resolution"], cfg["per_level_scale"], cfg["log2_hashmap_size"])
        _, offs_p = _offs_arg(offs)
        grad = grad_x = grad_x2 = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:  # first order only here (once_differentiable): _EncodePoints2
            grad_x = torch.empty_like(x)
            grad_x2 = torch.empty_like(x2) if has_x2 else None
            with L.on(x):
                _timed("input_grad_rows", lambda: L.call(
                    "mi3d_grid_points_backward_input", L.ptr(x), L.ptr(x2 if has_x2 else None), x.shape[0], offs_p, P0,
                    offs.shape[0], bound, L.ptr(dout), L.ptr(ctx.saved_tensors[3]), *grid, L.ptr(grad_x), L.ptr(grad_x2),
                    L.stream(x)), x.shape[0] * offs.shape[0])
            grad_x = grad_x.view(ctx.shapes[0]) if ctx.needs_input_grad[1] else None
            grad_x2 = grad_x2.view(ctx.shapes[1]) if has_x2 and ctx.needs_input_grad[2] else None
        if ctx.needs_input_grad[0]:
            grad = torch.zeros(n_params, dtype=torch.float32, device=x.device)
            with L.on(x):
                _timed("scatter_rows", lambda: L.call(
                    "mi3d_grid_scatter_points", L.ptr(x), L.ptr(x2 if has_x2 else None), x.shape[0],
                    L.ptr(count if has_count else None), offs_p, P0, offs.shape[0], bound, L.ptr(dout), *grid, step,
                    L.ptr(grad), L.stream(x)), x.shape[0] * offs.shape[0])
        return grad, grad_x, grad_x2, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------ second order
# encode_points(second_order=True) with positions that require grad: the same launches in the same order, behind nodes
# whose input gradient can be differentiated once more (mi3d_grid_points_backward_input_backward, include/mi3d.h Part 3).
# The positions and the table are saved as the INPUTS they are - flat fp32 tensors, cast and reshaped by tracked torch ops
# in front of the node - so that a backward pass run under create_graph=True finds their graph again.

def _grid_args(cfg):
    return (cfg["n_levels"], cfg["base_resolution"], cfg["per_level_scale"], cfg["log2_hashmap_size"])


class _PointsInputGrad(Function):
    """dL/dx, dL/dx2 of encode_points as a differentiable node.  Its backward is the second-order pass: the rows kernel for
    the gradients of dout and of the positions, the table kernel for the table's, each only where needs_input_grad asks."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, x2, dout, params, meta):
        offs, P0, bound, cfg, _ = meta
        dout = L.dev_f32(dout.contiguous(), "dout")
        _, offs_p = _offs_arg(offs)
        grad_x = torch.empty_like(x)
        grad_x2 = torch.empty_like(x2) if x2 is not None else None
        with L.on(x):
            _timed("input_grad_rows", lambda: L.call(
                "mi3d_grid_points_backward_input", L.ptr(x), L.ptr(x2), x.shape[0], offs_p, P0, offs.shape[0], bound,
                L.ptr(dout), L.ptr(params), *_grid_args(cfg), L.ptr(grad_x), L.ptr(grad_x2), L.stream(x)),
                x.shape[0] * offs.shape[0])
        ctx.save_for_backward(x, dout, params, *(() if x2 is None else (x2,)))
        ctx.meta = meta
        return grad_x, grad_x2

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, r, r2):
        x, dout, params = ctx.saved_tensors[:3]
        x2 = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        offs, P0, bound, cfg, _ = ctx.meta
        _, offs_p = _offs_arg(offs)
        n, evals = x.shape[0], x.shape[0] * offs.shape[0]
        r = L.dev_f32(r.float().contiguous().view(-1, 3), "r", 3)
        if x2 is not None:
            r2 = L.dev_f32((torch.zeros_like(x2) if r2 is None else r2.float().contiguous()).view(-1, 3), "r2", 3)
        need_x, need_x2, need_d, need_p = ctx.needs_input_grad[:4]
        gx = torch.empty_like(x) if need_x or need_x2 else None
        gx2 = torch.empty_like(x2) if gx is not None and x2 is not None else None
        gd = torch.empty_like(dout) if need_d else None
        gp = torch.zeros_like(params) if need_p else None

        def launch(gd, gx, gx2, gp):
            L.call("mi3d_grid_points_backward_input_backward", L.ptr(x), L.ptr(x2), n, offs_p, P0, offs.shape[0], bound,
                   L.ptr(dout), L.ptr(params), L.ptr(r), L.ptr(r2 if x2 is not None else None), *_grid_args(cfg),
                   L.ptr(gd), L.ptr(gx), L.ptr(gx2), L.ptr(gp), L.stream(x))
        with L.on(x):
            if gd is not None or gx is not None:
                _timed("second_order_rows", lambda: launch(gd, gx, gx2, None), evals)
            if gp is not None:
                _timed("second_order_table", lambda: launch(None, None, None, gp), evals)
        return (gx if need_x else None), (gx2 if need_x2 else None), gd, gp, None


class _PointsParamGrad(Function):
    """The parameter gradient of encode_points under second_order=True: the scatter of the first-order node.  It stays once
    differentiable - differentiating it again raises, it is never a silent zero."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, x2, dout, n_params, meta):
        offs, P0, bound, cfg, step = meta
        dout = L.dev_f32(dout.contiguous(), "dout")
        _, offs_p = _offs_arg(offs)
        grad = torch.zeros(n_params, dtype=torch.float32, device=x.device)
        with L.on(x):
            _timed("scatter_rows", lambda: L.call(
                "mi3d_grid_scatter_points", L.ptr(x), L.ptr(x2), x.shape[0], L.ptr(None), offs_p, P0, offs.shape[0], bound,
                L.ptr(dout), *_grid_args(cfg), step, L.ptr(grad), L.stream(x)), x.shape[0] * offs.shape[0])
        return grad

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError("the hash grid's parameter gradient is once differentiable: only the input gradient has a "
                           "second-order pass")


class _EncodePoints2(Function):
    """_EncodePoints for encode_points(second_order=True) with positions that require grad: the same forward launch; the
    backward hands the same first-order launches to the two nodes above, so it can run under create_graph=True."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, params, x, x2, offsets, P0, bound, cfg, step):
        L.dev_f32(x, "x", 3)
        if x2 is not None:
            L.dev_f32(x2, "x2", 3)
        L.dev_f32(params, "params")
        offs, offs_p = _offs_arg(offsets)
        P, n = offs.shape[0], x.shape[0]
        out = torch.empty(n * P, cfg["n_levels"] * 2, dtype=torch.float32, device=x.device)
        with L.on(x):
            _timed("encode_rows", lambda: L.call(
                "mi3d_grid_encode_points", L.ptr(x), L.ptr(x2), n, L.ptr(None), offs_p, int(P0), P, float(bound),
                L.ptr(params), *_grid_args(cfg), L.ptr(out), L.stream(x)), n * P)
        ctx.save_for_backward(params, x, *(() if x2 is None else (x2,)))
        ctx.meta = (offs, int(P0), float(bound), cfg, float(step))
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        params, x = ctx.saved_tensors[:2]
        x2 = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        dout = dout.float().contiguous()
        grad = grad_x = grad_x2 = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            grad_x, grad_x2 = _PointsInputGrad.apply(x, x2, dout, params, ctx.meta)
        if ctx.needs_input_grad[0]:
            grad = _PointsParamGrad.apply(x, x2, dout, params.numel(), ctx.meta)
        return (grad, grad_x if ctx.needs_input_grad[1] else None, grad_x2 if ctx.needs_input_grad[2] else None, None, None,
                None, None, None)


def encode_points(params, x, offsets, cfg, bound=1.0, x2=None, P0=None, step=0.0, count=None, second_order=False):
    """features [P*n, 2L] (point-major: row = point*n + sample) of clamp(base + offsets[p]) for every sample;
    differentiable w.r.t. `params` and - without `count` - w.r.t. `x` and `x2`.  The input gradient is first order only
    unless `second_order` is set: then it comes from a node that can be differentiated once more (an eikonal term, a loss
    on analytic normals), by the same kernels with the same bits; the parameter gradient stays once differentiable.  With
    the flag off, or with positions that do not require grad, nodes, saved tensors and launches are unchanged."""
    P = np.asarray(offsets).reshape(-1, 3).shape[0]
    if P0 is None:
        P0 = P
    if second_order and torch.is_grad_enabled() and (x.requires_grad or (x2 is not None and x2.requires_grad)):
        if count is not None:
            raise L.Mi3dError("encode_points with a device-side count does not differentiate the positions: the counted "
                              "rows belong to the inference loop")
        flat = [None if t is None else t.float().contiguous().view(-1, 3) for t in (x, x2)]
        return _EncodePoints2.apply(params, flat[0], flat[1], offsets, P0, bound, cfg, step)
    return _EncodePoints.apply(params, x, x2, offsets, P0, bound, cfg, step, count)
