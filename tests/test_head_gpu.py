"""GPU parity of the fused field head (csrc/field.hip Part 5: sigma, albedo and both finite-difference normals from the
MLP output of the 7 / 13 stencil points) against the plain PyTorch composition of the same ops, forward and backward,
including the degenerate rows where safe_normalize's clamp and nan_to_num decide the gradient.

Below that test: the C ABI (mi3d_field_head_forward, _forward_counted, _backward) and field_ops.field_head against the
binary64 model of tests/head_model.py on head_cases' inputs (tests/test_head_model_cpu.py proves what these inputs are).
THE BOUNDS are the model's running error bounds, derived from the operation chain; every element must use at most 1.0 of
its bound and no tolerance is tuned.  Where a neighbour overflows the pattern of NaN, +-inf, +-FLT_MAX and exact zeros
must be the model's, which is torch's.  Only the rows of dh behind a normal whose clamp gate is undecided (the straddling
block: at most 2 % of the samples) are left out; no forward element ever is.

MEASURED on the MI355X (profiles/head_parity.json, written by tools/head_parity.py from these same calls; the tests write no
files): worst share of a bound used 0.957 by sigma (pre-activations of 40 - 80, where one expf decides), 0.737 by albedo,
0.882 and 0.858 by the normals (empty space and |v|^2 > 1e32), 0.873 by dh (empty space); 1.0 - 1.2 % of the samples
undecided, all in the straddling block.  The model with binary32 operations on the CPU uses 0.957 / 0.723 / 0.882 / 0.858 /
0.873 of the same bounds.  Per block: DESIGN.md 16.
"""
import itertools

import numpy as np
import pytest
import torch

import head_model as H

pytestmark = pytest.mark.gpu


def _torch_head(h, x, x2, offs, bound, density, radius, eps=1e-2):
    n, P = x.shape[0], offs.shape[0]
    h = h.view(P, n, 4).transpose(0, 1)   # rows are point-major: p*n + s
    o = torch.from_numpy(offs).to(x.device)
    base = x.unsqueeze(1).expand(n, P, 3)
    if x2 is not None:
        base = torch.cat([base[:, :7], x2.unsqueeze(1).expand(n, P - 7, 3)], 1)
    pts = (base + o).clamp(-bound, bound)
    gauss = density * torch.exp(-(pts ** 2).sum(-1) / (2 * radius ** 2))
    from mi3d.network import trunc_exp
    from mi3d.renderer import safe_normalize
    sig = trunc_exp(h[..., 0] + gauss)

    def normal(s6):
        g = torch.stack([0.5 * (s6[:, 0] - s6[:, 1]) / eps, 0.5 * (s6[:, 2] - s6[:, 3]) / eps,
                         0.5 * (s6[:, 4] - s6[:, 5]) / eps], -1)
        return torch.nan_to_num(safe_normalize(-g))
    out = [sig[:, 0], torch.sigmoid(h[:, 0, 1:]), normal(sig[:, 1:7])]
    if P == 13:
        out.append(normal(sig[:, 7:13]))
    return out


@pytest.mark.parametrize("second", [False, True])
def test_head_matches_torch_composition(cuda, second):
    from mi3d import field_ops, grid_ops
    torch.manual_seed(3)
    n = 5000
    offs, P0 = grid_ops.stencil_offsets(center=True, second=second)
    P = offs.shape[0]
    x = (torch.rand(n, 3, device=cuda) * 2 - 1) * 0.9
    x[:50] *= 0.05           # inside the blob: large sigma
    x[50:60] = 1.0           # stencil clamps at the box
    x2 = (x + torch.randn_like(x) * 0.01) if second else None
    h = (torch.randn(n * P, 4, device=cuda) * 0.5)
    hv = h.view(P, n, 4).transpose(0, 1)
    hv[100:200, 1:, 0] = hv[100:200, 1:2, 0]   # identical neighbours: zero finite difference -> clamp regime
    hv[200:210, :, 0] = 30.0                  # beyond trunc_exp's derivative clamp
    hv[:, 1:7, 0] = hv[:, 1:7, 0] * 0.01 + hv[:, :1, 0]   # neighbours close to the centre value
    h = h.detach().requires_grad_(True)
    got = field_ops.field_head(h, x, offs, 1.0, 5.0, 0.1, x2)
    got = [g for g in got if g is not None]
    href = h.detach().clone().requires_grad_(True)
    want = _torch_head(href, x, x2, offs, 1.0, 5.0, 0.1)
    assert len(got) == len(want)
    for a, b, name in zip(got, want, ["sigma", "albedo", "normal", "normal2"]):
        # normals are ratios of differences of nearly equal exponentials: 1 ulp of expf moves them by ~1e-5
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=2e-5,
                                   atol=5e-5 if name.startswith("normal") else 2e-6, err_msg=name)
    gs = [torch.randn_like(t) for t in want]
    torch.autograd.backward(got, gs)
    torch.autograd.backward(want, gs)
    a, b = h.grad.view(P, n, 4).transpose(0, 1), href.grad.view(P, n, 4).transpose(0, 1)
    scale = b.abs().amax(dim=(1, 2), keepdim=True) + 1e-20   # per sample: the normal gradients span many decades
    assert float(((a - b).abs() / scale).max()) < 2e-3
    assert torch.isfinite(a).all() == torch.isfinite(b).all()


# ------------------------------------------------------------------------------------------------ C ABI against the model

INVALID = 1            # hipErrorInvalidValue
SIZES = (1, 255, 256, 257, 4099)
GRADS = ("dsigma", "dalbedo", "dnormal", "dnormal2")
ALLOWED = {1: GRADS[:2], 7: GRADS[:3], 13: GRADS}
_cache = {}


def head_case(P, n, i, cuda):
    """head_cases' inputs (seed 0) on the CPU and on the GPU; generated once per case and left unchanged."""
    key = (P, n, i)
    if key not in _cache:
        case = H.head_cases(0, n, P, H.PARAMS[i])
        dev = {k: (None if case[k] is None else case[k].to(cuda)) for k in ("h", "x", "x2", *GRADS)}
        _cache[key] = (case, dev)
    return _cache[key]


def _abi_args(case):
    bound, density, radius, eps = H._abi(case["params"])
    return float(bound), float(density), float(radius), float(eps)


def c_forward(case, dev, count=None, P=None, n=None, x2=True, normal2=True, rc=False):
    """The C ABI's forward into sentinel-filled buffers -> dict of sigma, albedo, normal, normal2 (GPU tensors)."""
    from mi3d import _lib as L
    P = case["P"] if P is None else P
    n = case["n"] if n is None else n
    rows = max(case["n"], 1)
    out = dict(sigma=torch.full((rows,), H.SENTINEL, device=dev["h"].device),
               albedo=torch.full((rows, 3), H.SENTINEL, device=dev["h"].device),
               normal=torch.full((rows, 3), H.SENTINEL, device=dev["h"].device),
               normal2=torch.full((rows, 3), H.SENTINEL, device=dev["h"].device) if (case["P"] == 13 and normal2) else None)
    offs = np.ascontiguousarray(case["offsets"], np.float32)
    with L.on(dev["h"]):
        if count is None:
            err = L.lib().mi3d_field_head_forward(
                L.ptr(dev["h"]), L.ptr(dev["x"]), L.ptr(dev["x2"] if x2 else None), n, offs.ctypes.data, P,
                *_abi_args(case), L.ptr(out["sigma"]), L.ptr(out["albedo"]), L.ptr(out["normal"]), L.ptr(out["normal2"]),
                L.stream(dev["h"]))
        else:
            err = L.lib().mi3d_field_head_forward_counted(
                L.ptr(dev["h"]), L.ptr(dev["x"]), L.ptr(dev["x2"] if x2 else None), n, L.ptr(count), offs.ctypes.data, P,
                *_abi_args(case), L.ptr(out["sigma"]), L.ptr(out["albedo"]), L.ptr(out["normal"]), L.ptr(out["normal2"]),
                L.stream(dev["h"]))
    if rc:
        return err, out
    assert err == 0, err
    return out


def c_backward(case, dev, P_active, grads, zeros=False, P=None, n=None, x2=True, rc=False):
    """The C ABI's backward with the named upstream gradients (the others NULL, or zeros) -> the whole dh buffer:
    [P_active n, 4] and PAD_ROWS sentinel rows behind it."""
    from mi3d import _lib as L
    P = case["P"] if P is None else P
    n = case["n"] if n is None else n
    rows = (P_active if P_active in (1, 7, 13) else 13) * case["n"]
    dh = torch.full((rows + H.PAD_ROWS, 4), H.SENTINEL, device=dev["h"].device)
    g = [dev[k] if k in grads else (torch.zeros_like(dev[k]) if zeros and dev[k] is not None else None) for k in GRADS]
    offs = np.ascontiguousarray(case["offsets"], np.float32)
    with L.on(dev["h"]):
        err = L.lib().mi3d_field_head_backward(
            L.ptr(dev["h"]), L.ptr(dev["x"]), L.ptr(dev["x2"] if x2 else None), n, offs.ctypes.data, P, P_active,
            *_abi_args(case), *[L.ptr(t) for t in g], L.ptr(dh), L.stream(dev["h"]))
    if rc:
        return err, dh
    assert err == 0, err
    return dh


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cpu(out):
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def forward_figures(case, dev):
    out = c_forward(case, dev)
    return out, H.check(_cpu(out), H.model_of(case), case["blocks"])


def backward_figures(case, dev, P_active, grads):
    dh = c_backward(case, dev, P_active, grads)
    return dh, H.check(dict(dh=dh.cpu()), H.model_of(case, P_active=P_active, grads=grads), case["blocks"])


@pytest.mark.parametrize("i", range(len(H.PARAMS)))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("P", [7, 13])
def test_forward_against_the_model(cuda, P, n, i):
    case, dev = head_case(P, n, i, cuda)
    out, (fig, fails) = forward_figures(case, dev)
    print(f"[head] forward P={P} n={n} params={H.PARAMS[i]}: {H.worst(fig)}")
    assert fails == [], (fails, H.worst(fig))
    again = c_forward(case, dev)
    for name in H.FORWARD[:3 + (P == 13)]:
        assert torch.equal(_bits(out[name]), _bits(again[name])), name
    # the counted entry point: rows at or past the device count keep the sentinel, rows below it are the same bits
    for cnt in sorted({0, 1, n - 1, n}):
        count = torch.tensor([cnt], dtype=torch.int32, device=cuda)
        part = c_forward(case, dev, count=count)
        for name in H.FORWARD[:3 + (P == 13)]:
            assert torch.equal(_bits(part[name][:cnt]), _bits(out[name][:cnt])), (name, cnt)
            assert bool((part[name][cnt:] == H.SENTINEL).all()), (name, cnt)


@pytest.mark.parametrize("i", range(len(H.PARAMS)))
@pytest.mark.parametrize("P,P_active", [(7, 1), (7, 7), (13, 1), (13, 7), (13, 13)])
def test_backward_against_the_model(cuda, P, P_active, i):
    """Every subset of the upstream gradients the combination allows, the all-null set included."""
    n = 4099
    case, dev = head_case(P, n, i, cuda)
    names = ALLOWED[P_active]
    for k in range(len(names) + 1):
        for grads in itertools.combinations(names, k):
            dh, (fig, fails) = backward_figures(case, dev, P_active, grads)
            tag = f"P={P} P_active={P_active} params={H.PARAMS[i]} grads={'+'.join(grads) or 'none'}"
            print(f"[head] backward {tag}: {H.worst(fig)}")
            assert fails == [], (tag, fails, H.worst(fig))
            # a NULL upstream gradient is a gradient of zeros, bit for bit - and so is a second call
            assert torch.equal(_bits(dh), _bits(c_backward(case, dev, P_active, grads, zeros=True))), tag
            assert torch.equal(_bits(dh), _bits(c_backward(case, dev, P_active, grads))), tag


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("P,P_active", [(7, 7), (13, 1), (13, 7), (13, 13)])
def test_backward_around_the_block_size(cuda, P, P_active, n):
    case, dev = head_case(P, n, 2, cuda)
    for grads in (ALLOWED[P_active], ALLOWED[P_active][-1:]):
        dh, (fig, fails) = backward_figures(case, dev, P_active, grads)
        assert fails == [], (grads, fails, H.worst(fig))


@pytest.mark.parametrize("which", ["sigma", "normal", "normal2"])
def test_autograd_reaches_the_model(cuda, which):
    """field_ops.field_head with a gradient on one output alone returns the model's dh, zero-padded to [P n, 4]."""
    from mi3d import field_ops
    P, n = 13, 4099
    case, dev = head_case(P, n, 2, cuda)
    bound, density, radius, eps = H._abi(case["params"])
    h = dev["h"].clone().requires_grad_()
    sigma, albedo, normal, normal2 = field_ops.field_head(h, dev["x"], case["offsets"], bound, density, radius, dev["x2"],
                                                          epsilon=eps)
    idx = ("sigma", "albedo", "normal", "normal2").index(which)
    P_active = {"sigma": 1, "normal": 7, "normal2": 13}[which]
    (sigma, albedo, normal, normal2)[idx].backward(dev[GRADS[idx]])
    g = h.grad
    assert g.shape == (P * n, 4)
    rows = P_active * n
    assert bool((g[rows:] == 0).all())
    buf = torch.cat([g[:rows].cpu(), torch.full((H.PAD_ROWS, 4), H.SENTINEL)], 0)
    fig, fails = H.check(dict(dh=buf), H.model_of(case, P_active=P_active, grads=(GRADS[idx],)), case["blocks"])
    print(f"[head] autograd {which}: {H.worst(fig)}")
    assert fails == [], (fails, H.worst(fig))
    # the same bits as the C ABI's call
    assert torch.equal(_bits(g[:rows]), _bits(c_backward(case, dev, P_active, (GRADS[idx],))[:rows]))


def test_invalid_arguments_launch_nothing(cuda):
    case, dev = head_case(13, 257, 0, cuda)
    case7, dev7 = head_case(7, 257, 0, cuda)
    outs = []

    def fwd(c, d, **kw):
        err, out = c_forward(c, d, rc=True, **kw)
        outs.extend(t for t in out.values() if t is not None)
        return err

    def bwd(c, d, P_active, **kw):
        err, dh = c_backward(c, d, P_active, GRADS[:2], rc=True, **kw)
        outs.append(dh)
        return err
    assert fwd(case, dev, P=5) == INVALID and fwd(case, dev, P=6) == INVALID and fwd(case, dev, P=14) == INVALID
    assert fwd(case, dev, x2=False) == INVALID and fwd(case, dev, normal2=False) == INVALID      # P = 13 needs both
    assert bwd(case, dev, 1, P=5) == INVALID and bwd(case, dev, 1, P=12) == INVALID
    assert bwd(case, dev, 13, x2=False) == INVALID and bwd(case, dev, 1, x2=False) == INVALID
    for bad in (0, 2, 6, 8, 12, 14):
        assert bwd(case, dev, bad) == INVALID, bad
    assert bwd(case7, dev7, 13) == INVALID                                                        # P_active > P
    assert fwd(case, dev, n=0) == 0 and bwd(case, dev, 13, n=0) == 0 and bwd(case7, dev7, 7, n=0) == 0
    count = torch.tensor([5], dtype=torch.int32, device=cuda)
    assert fwd(case, dev, count=count, P=5) == INVALID and fwd(case, dev, count=count, n=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == H.SENTINEL).all()) for t in outs)                                       # nothing was launched
