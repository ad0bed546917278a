"""GPU: the fused Adan step and the gradient's sum of squares (csrc/optim.hip through mi3d.optim.Adan, include/mi3d.h
Part 6) above the size at which their capped grid goes round again.  `grid_for` launches at most 2048 workgroups of 256
threads with a float4 each: 2 097 152 floats per sweep.  The product's hash table takes six sweeps in every optimiser
step; the other tests of these kernels stay within one.  Here a tensor of two full sweeps, a ragged third and a
scalar tail of three elements, next to a small odd tensor in a second parameter group.

Reference: the update rule of mi3d/optim.py's torch-op path written out below in binary64 (`Adan64`), started from the
same binary32 parameters, fed the same binary32 gradients, advanced over three steps (the first one is `first_step`).

Bound for the parameter and the four state tensors, per tensor and in max-abs: nothing fixed in advance.  The binary32
torch-op path (`_fused_ok = lambda: False`) runs on the same inputs; the kernel's error against binary64 may be 4 x that
path's (it associates value * (m / denom) where addcdiv has value * m / denom) plus one binary32 ulp at the tensor's
largest magnitude.  Two things this bound found, both mended in csrc/optim.hip: 1 - beta formed as 1.0f - (float)beta is
off by 1e-6 relative, which put exp_avg and exp_avg_sq sixteen times further from binary64 than the torch-op path (the
entry point takes the betas in binary64 now); and a binary32 sum of squares through 2048 float atomics gave a clip factor
3.5 to 7 times worse than that path's, differently in every run (the sum and the factor are binary64 now).  Every pair
of figures is printed and written to second_round_parity.json BEFORE anything is asserted - in the directory
MI3D_REPORT_DIR names, or test_reports/ at the root of the repository (git-ignored); the kept copy is
profiles/second_round_parity.json."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

GRID_CAP, BLOCK, PER_THREAD = 2048, 256, 4      # grid_for of csrc/optim.hip: workgroups at most, threads, floats per thread
SWEEP = GRID_CAP * BLOCK * PER_THREAD           # floats one pass of k_adan / k_sumsq covers: 2 097 152
N_BIG = 2 * SWEEP + 1027                        # two sweeps, 256 float4 of a third, then 3 elements on the scalar tail
N_SMALL = 1003
STEPS = 3
BETAS, EPS, WD, MAX_NORM = (0.98, 0.92, 0.99), 1e-8, 2e-5, 5.0     # the product's configuration (mi3d/optim.py's header)
LRS = (5e-2, 5e-3)                              # the grid's group and the networks'
STATE = ("exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad")
FACTOR = 4.0
SUMSQ_RTOL = 2200 * 2.0 ** -24                  # the longest chain of additions a square passes through, were they all binary32:
#                                                 12 in the thread, 6 shuffles, 3 across waves, at most 2048 atomic adds; all
#                                                 terms >= 0.  (The kernel adds in binary64: it stays far inside.)
REPORT_PATH = os.path.join(os.environ.get("MI3D_REPORT_DIR") or os.path.join(ROOT, "test_reports"),
                           "second_round_parity.json")
_REPORT = {}


def test_the_size_reaches_a_ragged_third_sweep():
    assert N_BIG > 2 * SWEEP and N_BIG - 2 * SWEEP < SWEEP
    assert (N_BIG - 2 * SWEEP) // PER_THREAD > BLOCK - 1        # more than one workgroup takes part in the last sweep
    assert N_BIG % PER_THREAD == 3                              # and its last thread walks the scalar tail
    assert N_SMALL % PER_THREAD == 3 and N_SMALL < BLOCK * PER_THREAD


def _record(key, **figures):
    print(key, " ".join(f"{k}={v:.3e}" for k, v in figures.items()))
    _REPORT[key] = figures
    os.makedirs(os.path.dirname(REPORT_PATH), exist_ok=True)
    with open(REPORT_PATH, "w") as f:
        json.dump({"adan": _REPORT}, f, indent=1)


class Adan64:
    """Adan.step of mi3d/optim.py (the torch-op path) in binary64, out of place, one line per line of the rule."""

    def __init__(self, params, lrs, max_grad_norm, no_prox):
        self.p = [p.detach().double().clone() for p in params]
        self.lrs, self.max_grad_norm, self.no_prox, self.k = lrs, max_grad_norm, no_prox, 0
        zeros = lambda: [torch.zeros_like(p) for p in self.p]      # noqa: E731
        self.state = {"exp_avg": zeros(), "exp_avg_sq": zeros(), "exp_avg_diff": zeros(), "neg_pre_grad": zeros()}
        self.clip = 1.0

    def step(self, grads):
        """grads: the binary32 gradients.  Returns the clipped gradients (what the step leaves in p.grad)."""
        b1, b2, b3 = BETAS
        g64 = [g.detach().double() for g in grads]
        self.clip = 1.0
        if self.max_grad_norm > 0:
            total = math.sqrt(sum(float((g * g).sum()) for g in g64))
            self.clip = min(self.max_grad_norm / (total + EPS), 1.0)
        self.k += 1
        k = self.k
        bc1, bc2, bc3s = 1 - b1 ** k, 1 - b2 ** k, math.sqrt(1 - b3 ** k)
        st = self.state
        for i, (g, lr) in enumerate(zip(g64, self.lrs)):
            g = g * self.clip
            g64[i] = g
            if k == 1:
                st["neg_pre_grad"][i] = -g
            diff = st["neg_pre_grad"][i] + g                           # g_t - g_{t-1}
            m = st["exp_avg"][i] * b1 + g * (1 - b1)
            d = st["exp_avg_diff"][i] * b2 + diff * (1 - b2)
            u = diff * b2 + g                                          # g_t + b2 (g_t - g_{t-1})
            n = st["exp_avg_sq"][i] * b3 + u * u * (1 - b3)
            denom = n.sqrt() / bc3s + EPS
            p = self.p[i]
            if self.no_prox:
                p = p * (1 - lr * WD) - (lr / bc1) * (m / denom) - (lr * b2 / bc2) * (d / denom)
            else:
                p = (p - (lr / bc1) * (m / denom) - (lr * b2 / bc2) * (d / denom)) / (1 + lr * WD)
            self.p[i], st["exp_avg"][i], st["exp_avg_diff"][i], st["exp_avg_sq"][i] = p, m, d, n
            st["neg_pre_grad"][i] = -g
        return g64


def plant(x, sweep2, sweep3, unit):
    """Each sweep's part of the large tensor gets content of its own, the three tail elements fixed values: a sweep that
    is dropped, done twice or done on another sweep's addresses changes the result by the size of the content."""
    x[SWEEP:2 * SWEEP] *= sweep2
    x[2 * SWEEP:] *= sweep3
    x[-3:] = torch.tensor([1.5, -2.5, 0.75], dtype=x.dtype, device=x.device) * unit
    return x


@functools.lru_cache(maxsize=None)
def inputs(scale):
    """(parameters, [gradients of step 1, 2, 3]) on the GPU, binary32; made once per gradient scale, never changed."""
    gen = torch.Generator(device="cuda").manual_seed(1234)
    rand = lambda n: torch.randn(n, generator=gen, device="cuda")      # noqa: E731
    params = [plant(rand(N_BIG), 1.0, 1.0, 1.0), rand(N_SMALL)]
    params[0][2 * SWEEP:] += 8.0                                       # the third sweep's parameters: another binade
    grads = [[plant(rand(N_BIG) * scale, 2.0, -0.5, scale), rand(N_SMALL) * scale] for _ in range(STEPS)]
    return params, grads


def make(params, max_grad_norm, no_prox, fused):
    from mi3d import optim
    ps = [p.clone().requires_grad_(True) for p in params]
    opt = optim.Adan([{"params": ps[:1], "lr": LRS[0]}, {"params": ps[1:], "lr": LRS[1]}], betas=BETAS, eps=EPS,
                     weight_decay=WD, max_grad_norm=max_grad_norm, no_prox=no_prox)
    if not fused:
        opt._fused_ok = lambda: False                                  # force the torch-op path
    return ps, opt


def ulp32(x):
    return float(np.spacing(np.float32(x)))


# gradient scales as tests/test_sds_step_gpu.py chooses them: 1e-3 leaves the global norm below max_grad_norm (clip factor
# exactly 1), 50 puts it far above; "off" is max_grad_norm = 0: a null grad_sumsq pointer, no clip
CLIP = {"inactive": (1e-3, MAX_NORM), "active": (50.0, MAX_NORM), "off": (50.0, 0.0)}


@pytest.mark.parametrize("no_prox", [False, True], ids=["prox", "no_prox"])
@pytest.mark.parametrize("clip", list(CLIP))
def test_three_steps_against_binary64(cuda, clip, no_prox):
    scale, max_norm = CLIP[clip]
    params, grads = inputs(scale)
    ref = Adan64(params, LRS, max_norm, no_prox)
    (kp, kopt), (tp, topt) = make(params, max_norm, no_prox, True), make(params, max_norm, no_prox, False)
    failures, clips = [], []
    for step in range(STEPS):
        for ps in (kp, tp):
            for p, g in zip(ps, grads[step]):
                p.grad = g.clone()
        assert kopt._fused_ok()                                        # the kernels, not the fall-back
        kopt.step()
        topt.step()
        want_g = ref.step(grads[step])
        clips.append(ref.clip)
        for i, tensor in enumerate(("big", "small")):
            pairs = [("param", kp[i].detach(), tp[i].detach(), ref.p[i])]
            pairs += [(s, kopt.state[kp[i]][s], topt.state[tp[i]][s], ref.state[s][i]) for s in STATE]
            for name, got, stock, want in pairs:
                err = float((got.double() - want).abs().max())
                yard = float((stock.double() - want).abs().max())
                bound = FACTOR * yard + ulp32(float(want.abs().max()))
                _record(f"adan[{clip},{'no_prox' if no_prox else 'prox'}] step {step + 1} {tensor} {name}",
                        kernel_err=err, torch_fp32_err=yard, bound=bound)
                if not err <= bound:
                    failures.append((step + 1, tensor, name, err, bound))
            # the clipped gradient, left in place: g * clip, the sum behind clip within the chain bound above
            assert torch.allclose(kp[i].grad.double(), want_g[i], rtol=SUMSQ_RTOL, atol=0), (step, tensor)
        # the update itself (about lr per step wherever |g| >> eps) is far above every bound: a sweep left out would show
        moved = (kp[0].detach().double() - params[0].double()).abs() > 1e-3
        for lo, hi in ((0, SWEEP), (SWEEP, 2 * SWEEP), (2 * SWEEP, N_BIG - 3), (N_BIG - 3, N_BIG)):
            assert float(moved[lo:hi].double().mean()) > 0.9, (step, lo, hi)
    print(f"clip factors of the three steps: {clips}")
    assert all(c == 1.0 for c in clips) if clip != "active" else all(c < 0.01 for c in clips)
    assert not failures, failures


def test_sum_of_squares_over_three_sweeps(cuda):
    """A gradient that is zero over the whole first sweep: what the clip factor is made of lies in the later sweeps alone,
    so a missed sweep shows as a factor, not as an ulp."""
    from mi3d import _lib as L
    from mi3d import optim
    gen = torch.Generator(device="cuda").manual_seed(99)
    g = torch.randn(N_BIG, generator=gen, device=cuda)
    g[:SWEEP] = 0
    g[2 * SWEEP:] *= 30.0                                              # the ragged sweep carries a third of the sum
    g[-3:] = torch.tensor([400.0, -300.0, 500.0], device=cuda)         # and the scalar tail a tenth
    total = float((g.double() ** 2).sum())
    parts = [float((g[lo:hi].double() ** 2).sum()) / total for lo, hi in ((0, SWEEP), (SWEEP, 2 * SWEEP),
                                                                         (2 * SWEEP, N_BIG - 3), (N_BIG - 3, N_BIG))]
    print(f"shares of the sum: {parts}")
    assert parts[0] == 0 and all(s > 0.05 for s in parts[1:])
    acc = torch.zeros(1, dtype=torch.float64, device=cuda)
    L.call("mi3d_sumsq_accumulate", L.ptr(g), C.c_size_t(N_BIG), L.ptr(acc), L.stream(g))
    err = abs(float(acc) - total) / total
    _record("sumsq three sweeps", rel_err=err, bound=SUMSQ_RTOL)
    assert err <= SUMSQ_RTOL
    # through the optimiser: the clipped gradient left in p.grad
    p = torch.zeros(N_BIG, device=cuda, requires_grad=True)
    p.grad = g.clone()
    opt = optim.Adan([p], lr=1e-3, eps=EPS, max_grad_norm=MAX_NORM)
    assert opt._fused_ok()
    opt.step()
    factor = min(MAX_NORM / (math.sqrt(total) + EPS), 1.0)
    assert factor < 0.01
    want = g.double() * factor
    worst = float(((p.grad.double() - want).abs() / want.abs().clamp(min=1e-300)).max())
    _record("clipped gradient three sweeps", rel_err=worst, bound=SUMSQ_RTOL)
    assert bool((p.grad[:SWEEP] == 0).all())
    assert torch.allclose(p.grad.double(), want, rtol=SUMSQ_RTOL, atol=0)


def test_a_base_pointer_off_16_bytes_is_refused_and_nothing_launched(cuda):
    from mi3d import _lib as L
    n = 4096
    bufs = [torch.full((n + 4,), float(i + 1), device=cuda) for i in range(6)]
    keep = [b.clone() for b in bufs]
    acc = torch.zeros(1, dtype=torch.float64, device=cuda)
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    for off in (1, 2, 3):
        with pytest.raises(L.Mi3dError):
            L.call("mi3d_sumsq_accumulate", L.ptr(bufs[0][off:]), C.c_size_t(n), L.ptr(acc), L.stream(acc))
    b1, b2, b3 = BETAS
    hyper = (MAX_NORM, EPS, 1, b1, b2, b3, 1 - b1, 1 - b2, math.sqrt(1 - b3), 1e-3, WD, EPS, 0)
    for which in range(6):
        ptrs = [L.ptr(b[1:] if i == which else b[:n]) for i, b in enumerate(bufs)]
        with pytest.raises(L.Mi3dError):
            L.call("mi3d_adan_step", *ptrs, C.c_size_t(n), L.ptr(None), *hyper, L.stream(acc))
    torch.cuda.synchronize(cuda)
    assert float(acc) == 0 and all(torch.equal(a, b) for a, b in zip(bufs, keep))
    # the same calls with every pointer aligned go through
    L.call("mi3d_sumsq_accumulate", L.ptr(bufs[1]), C.c_size_t(n), L.ptr(acc), L.stream(acc))
    assert float(acc) == 4.0 * n
    L.call("mi3d_adan_step", *[L.ptr(b) for b in bufs], C.c_size_t(n), L.ptr(None), *hyper, L.stream(acc))
    assert not torch.equal(bufs[0], keep[0])
