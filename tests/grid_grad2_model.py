"""The yardstick of the hash grid's SECOND-ORDER pass (include/mi3d.h Part 2 / Part 3: the backward of the input
gradient): the closed forms in binary64 on the CPU, with explicit loops over levels, dimensions and corners.

Cell, fraction, clamp and map are the kernel's own binary32 ones (grid_grad_model.cell_frac / point_q); everything after
is binary64.  With g_d = sum_l sum_c dout[l,c] s_l T_{d,c} the first-order result and r = dL/dg, per level
rho_d = r_d s_l (mode 1: r_d m_d / (2 bound) s_l), sigma(0) = -1, sigma(1) = +1, corner k = bx | by << 1 | bz << 2:

    grad_dout[l,c]           = sum_d rho_d sum_k sigma(b_d) w_e(b_e) w_e'(b_e') v[k].c
    grad_params[entry(k), c] += dout[l,c] kappa_k,   kappa_k = sum_d rho_d sigma(b_d) w_e(b_e) w_e'(b_e')
    grad_q_d'                = s_l sum_c dout[l,c] sum_{d != d'} rho_d sum_k sigma(b_d) sigma(b_d') w_e(b_e) v[k].c

Beside every output comes its rounding magnitude B: the same sum with every factor replaced by its absolute value and every
corner difference by |hi| + |lo| - a difference of two differences by the sum of its four |v| - which is the sum over all
eight corners of the weights times |v[k]|.  For the table N counts, per entry, the contributions a point ISSUES (its dout
pair not zero, its three rho not all zero): the atomic additions of an entry come in any order, N - 1 of them.
"""
import numpy as np
import torch

import grid_grad_model as M

SIGMA = (-1.0, 1.0)


class TableSums:
    """grad_params, its B ([entries, 2] each) and N ([entries]) accumulated over points and levels."""

    def __init__(self, levels):
        self.grad = torch.zeros(levels.n_entries, 2, dtype=torch.float64)
        self.B = torch.zeros(levels.n_entries, 2, dtype=torch.float64)
        self.N = torch.zeros(levels.n_entries, dtype=torch.int64)


def second_order_q(q32, dout, rq, table, levels, sums):
    """One set of m points at q32 [m, 3] with dout [m, 2 L] and rq [m, 3] = dL/d(dL/dq): returns grad_dout [m, 2 L], its B,
    grad_q [m, 3], its B, and adds the table's share into `sums`."""
    table, dout, rq = table.reshape(-1, 2).double(), dout.double(), rq.double()
    m, F = q32.shape[0], 2 * levels.n_levels
    gd, Bd = torch.zeros(m, F, dtype=torch.float64), torch.zeros(m, F, dtype=torch.float64)
    gq, Bq = torch.zeros(m, 3, dtype=torch.float64), torch.zeros(m, 3, dtype=torch.float64)
    live = (rq != 0).any(-1)
    for l, L in enumerate(levels.level):
        cell, f = M.cell_frac(q32, L["scale"])
        f = f.double()
        v = M._corners(L, table, cell)                                  # [m, 8, 2]
        s = float(L["scale"])
        rho = rq * s
        d2 = dout[:, 2 * l:2 * l + 2]
        issued = (live & (d2 != 0).any(-1)).long()
        w = [(1 - f[:, d], f[:, d]) for d in range(3)]
        for k in range(8):
            b = [(k >> d) & 1 for d in range(3)]
            kappa, kabs = torch.zeros(m, dtype=torch.float64), torch.zeros(m, dtype=torch.float64)
            for d in range(3):
                e0, e1 = [i for i in range(3) if i != d]
                wt = w[e0][b[e0]] * w[e1][b[e1]]
                kappa += rho[:, d] * SIGMA[b[d]] * wt
                kabs += rho[:, d].abs() * wt
            gd[:, 2 * l:2 * l + 2] += kappa[:, None] * v[:, k]
            Bd[:, 2 * l:2 * l + 2] += kabs[:, None] * v[:, k].abs()
            e = M.entry(L, (cell[:, 0] + b[0]) & M.M32, (cell[:, 1] + b[1]) & M.M32, (cell[:, 2] + b[2]) & M.M32) + L["offset"]
            sums.grad.index_add_(0, e, kappa[:, None] * d2)
            sums.B.index_add_(0, e, kabs[:, None] * d2.abs())
            sums.N.index_add_(0, e, issued)
            dv, dva = (d2 * v[:, k]).sum(-1), (d2.abs() * v[:, k].abs()).sum(-1)
            for dp in range(3):
                for d in range(3):
                    if d == dp:
                        continue
                    e_ = 3 - d - dp
                    gq[:, dp] += s * SIGMA[b[d]] * SIGMA[b[dp]] * w[e_][b[e_]] * rho[:, d] * dv
                    Bq[:, dp] += s * w[e_][b[e_]] * rho[:, d].abs() * dva
    return gd, Bd, gq, Bq


def second_order(q32, dout, r, table, levels):
    """Mode 0.  dict: grad_dout, B_dout [n, 2 L]; grad_x, B_x [n, 3]; table (a TableSums)."""
    sums = TableSums(levels)
    gd, Bd, gq, Bq = second_order_q(q32, dout, r, table, levels, sums)
    return dict(grad_dout=gd, B_dout=Bd, grad_x=gq, B_x=Bq, table=sums)


def points_second_order(x32, x2_32, offsets, P0, bound, dout, r, r2, table, levels):
    """Mode 1.  dout [P n, 2 L] point-major; r, r2 [n, 3] (r2 None without x2).  dict as second_order's, plus grad_x2, B_x2
    (None without x2)."""
    n, offs = x32.shape[0], torch.from_numpy(np.ascontiguousarray(offsets, np.float32).reshape(-1, 3))
    bnd = float(np.float32(bound))
    sums = TableSums(levels)
    gds, Bds = [], []
    gx = [[torch.zeros(n, 3, dtype=torch.float64) for _ in range(2)] for _ in range(2)]     # [base][grad, B]
    for p in range(offs.shape[0]):
        which = 0 if p < P0 else 1
        q, t = M.point_q(x32 if which == 0 else x2_32, offs[p], bound)
        mask = (t.abs() <= bnd).double()
        rq = (r if which == 0 else r2).double() * mask / (2.0 * bnd)
        gd, Bd, gq, Bq = second_order_q(q, dout[p * n:(p + 1) * n], rq, table, levels, sums)
        gds.append(gd)
        Bds.append(Bd)
        gx[which][0] += mask * gq / (2.0 * bnd)
        gx[which][1] += mask * Bq / (2.0 * bnd)
    has2 = x2_32 is not None
    return dict(grad_dout=torch.cat(gds), B_dout=torch.cat(Bds), grad_x=gx[0][0], B_x=gx[0][1],
                grad_x2=gx[1][0] if has2 else None, B_x2=gx[1][1] if has2 else None, table=sums)


def first_order_table(q32, a, levels):
    """The FIRST-order parameter gradient (the pointwise scatter, mode 0) of dout = a [m, 2 L]: grad_params[entry(k), c] +=
    a[l,c] w_k with the trilinear weight w_k; a TableSums whose B is the same sum of |a| w_k and whose N counts the points
    with a non-zero pair."""
    sums, a = TableSums(levels), a.double()
    for l, L in enumerate(levels.level):
        cell, f = M.cell_frac(q32, L["scale"])
        f = f.double()
        d2 = a[:, 2 * l:2 * l + 2]
        issued = (d2 != 0).any(-1).long()
        for k in range(8):
            b = [(k >> d) & 1 for d in range(3)]
            wk = torch.ones(q32.shape[0], dtype=torch.float64)
            for d in range(3):
                wk = wk * (f[:, d] if b[d] else 1 - f[:, d])
            e = M.entry(L, (cell[:, 0] + b[0]) & M.M32, (cell[:, 1] + b[1]) & M.M32, (cell[:, 2] + b[2]) & M.M32) + L["offset"]
            sums.grad.index_add_(0, e, wk[:, None] * d2)
            sums.B.index_add_(0, e, wk[:, None] * d2.abs())
            sums.N.index_add_(0, e, issued)
    return sums


# ------------------------------------------------------------------------------------------------ inputs

def stencil_inputs(levels, offs, P0, bound, n, seed):
    """n samples (x, x2) in and around the box whose every stencil point passes the face filter; the first candidates sit
    exactly on +bound, on -bound, outside the box in one coordinate and on a corner of the box (12 candidates each, random
    in the other coordinates or in x2).  Returns x, x2 and how many of each kind survived."""
    g = torch.Generator().manual_seed(seed)
    m = 8 * n
    b = float(np.float32(bound))
    x = (torch.rand(m, 3, generator=g) * 2 - 1) * (1.1 * b)
    x[0:12, 0], x[12:24, 1], x[24:36, 2] = b, -b, 1.3 * b
    x[36:48] = torch.tensor([b, -b, b])
    x2 = x + 0.01 * torch.randn(m, 3, generator=g)
    offs = np.ascontiguousarray(offs, np.float32).reshape(-1, 3)
    ok = M.keep_points(x, offs[:P0], bound, levels)
    if P0 < len(offs):
        ok &= M.keep_points(x2, offs[P0:], bound, levels)
    idx = torch.nonzero(ok)[:n, 0]
    assert idx.numel() == n, "the face filter left too few samples"
    census = [int(((idx >= lo) & (idx < lo + 12)).sum()) for lo in (0, 12, 24, 36)]
    return x[idx].contiguous(), x2[idx].contiguous(), census
