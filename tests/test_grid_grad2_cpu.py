"""CPU: the closed forms of the hash grid's second-order pass (tests/grid_grad2_model.py) against torch.autograd through
grid_grad_model.forward in binary64: the first gradient with create_graph=True, then the gradient of <g, r> with respect
to dout, the table and the displacement.  Both sides are binary64: they agree within 1e-12 x B, B the model's rounding
magnitude of the output."""
import numpy as np
import pytest
import torch

import grid_grad2_model as M2
import grid_grad_model as M

N = 200
TOL = 1e-12


def _close(name, got, ref, B):
    err = (got - ref).abs()
    ratio = torch.where(B > 0, err / B, err)
    print(f"[grid-grad2] {name}: worst |closed form - autograd| / B = {float(ratio.max()):.2e}")
    assert bool((err <= TOL * B).all()), name


def _table_close(name, sums, grad_table):
    _close(name, sums.grad, grad_table.reshape(-1, 2), sums.B)


@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_mode0_closed_forms_are_autograds(name):
    levels = M.Levels(**M.CONFIGS[name])
    q = M.points01(levels, N, seed=61)
    table = M.table_uniform(levels, seed=62)
    g = torch.Generator().manual_seed(63)
    dout = torch.randn(N, levels.n_levels * 2, generator=g)
    r = torch.randn(N, 3, generator=g)
    want = M2.second_order(q, dout, r, table, levels)

    t64 = table.double().requires_grad_()
    d64 = dout.double().requires_grad_()
    dq = torch.zeros(N, 3, dtype=torch.float64, requires_grad=True)
    y = M.forward(q, t64, levels, torch.float64, dq)
    (g1,) = torch.autograd.grad((y * d64).sum(), dq, create_graph=True)
    gd, gt, gq = torch.autograd.grad((g1 * r.double()).sum(), [d64, t64, dq])
    # the first order is grid_grad_model's own
    g_first, B_first = M.grad_q(q, dout, table, levels)
    _close(f"{name} first order", g1.detach(), g_first, B_first)
    _close(f"{name} grad_dout", gd, want["grad_dout"], want["B_dout"])
    _close(f"{name} grad_x", gq, want["grad_x"], want["B_x"])
    _table_close(f"{name} grad_params", want["table"], gt)
    assert float(want["grad_x"].abs().max()) > 0 and float(want["table"].grad.abs().max()) > 0
    assert int(want["table"].N.sum()) == N * levels.n_levels * 8


@pytest.mark.parametrize("name", list(M.CONFIGS))
@pytest.mark.parametrize("P", [1, 7, 13])
def test_mode1_closed_forms_are_autograds(name, P):
    from mi3d import grid_ops
    levels = M.Levels(**M.CONFIGS[name])
    bound = 1.5 if P == 7 else 1.0
    if P == 1:
        offs, P0 = np.zeros((1, 3), np.float32), 1
    else:
        offs, P0 = grid_ops.stencil_offsets(center=True, second=P == 13)
    assert offs.shape[0] == P
    second = P0 < P
    x, x2, census = M2.stencil_inputs(levels, offs, P0, bound, N, seed=71)
    assert min(census[:3]) >= 1                                  # on +bound, on -bound, outside the box
    if not second:
        x2 = None
    table = M.table_uniform(levels, seed=72)
    g = torch.Generator().manual_seed(73)
    dout = torch.randn(P * N, levels.n_levels * 2, generator=g)
    r, r2 = torch.randn(N, 3, generator=g), (torch.randn(N, 3, generator=g) if second else None)
    want = M2.points_second_order(x, x2, offs, P0, bound, dout, r, r2, table, levels)

    bnd = float(np.float32(bound))
    t64 = table.double().requires_grad_()
    d64 = dout.double().requires_grad_()
    dx = [torch.zeros(N, 3, dtype=torch.float64, requires_grad=True) for _ in range(2 if second else 1)]
    ys = []
    for p in range(P):
        which = 0 if p < P0 else 1
        q, t = M.point_q(x if which == 0 else x2, torch.from_numpy(offs[p]), bound)
        m = (t.abs() <= bnd).double()
        ys.append(M.forward(q, t64, levels, torch.float64, m * dx[which] / (2.0 * bnd)))
    y = torch.cat(ys)
    g1 = torch.autograd.grad((y * d64).sum(), dx, create_graph=True)
    loss = (g1[0] * r.double()).sum() + ((g1[1] * r2.double()).sum() if second else 0)
    got = torch.autograd.grad(loss, [d64, t64, *dx])
    _close(f"{name} P={P} grad_dout", got[0], want["grad_dout"], want["B_dout"])
    _table_close(f"{name} P={P} grad_params", want["table"], got[1])
    _close(f"{name} P={P} grad_x", got[2], want["grad_x"], want["B_x"])
    if second:
        _close(f"{name} P={P} grad_x2", got[3], want["grad_x2"], want["B_x2"])
    else:
        assert want["grad_x2"] is None
    # a coordinate the clamp stopped receives nothing and sends nothing
    outside = x[:, 2].abs() > bnd + 0.02
    assert bool(outside.any()) and bool((want["grad_x"][outside, 2] == 0).all())
