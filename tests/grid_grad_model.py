"""The yardstick of the hash grid's input gradient (include/mi3d.h Part 2 / Part 3): a binary64 restatement on the CPU.

Cell and fraction are the kernel's own - p = float32(float64(s_l) * float64(q) + 0.5) is its fmaf, exact except for
double-rounding ties that random inputs do not hit - and in mode 1 q comes from the same binary32 clamp and map point_of
does; the entry indices follow grid_entry's rule on the level table `tinycudann.grid_levels` reports.  Everything after is
binary64.  Besides the gradient the model returns the magnitude every rounding of the kernel is relative to,

    B[i, d] = sum_l s_l sum_feat |dout| sum_(j,k) w_e(j) w_e'(k) (|v_hi| + |v_lo|)

and the input generator keeps only points whose fraction lies in [2^-10, 1 - 2^-10] at every level and in every
dimension: away from the cell faces, where a last-bit difference of p would pick another cell.  The kept points ARE the
tests' inputs; nothing is excluded at comparison time.
"""
import numpy as np
import torch

PRIME_Y, PRIME_Z = 2654435761, 805459861
M32 = 0xFFFFFFFF
FACE = 2.0 ** -10

CONFIGS = {  # the three of tests/test_hashgrid_gpu.py
    "default16": dict(n_levels=16, log2_hashmap_size=19, base_resolution=16,
                      per_level_scale=float(np.float32(np.exp2(np.log2(2048 / 16) / 15)))),
    "c1_L4": dict(n_levels=4, log2_hashmap_size=19, base_resolution=16, per_level_scale=float(np.float32(128 ** (1 / 3)))),
    "small_hash": dict(n_levels=8, log2_hashmap_size=12, base_resolution=4, per_level_scale=float(np.float32(1.7))),
}


class Levels:
    """The level table: scale (binary32), res, offset, size, and grid_entry's two switches (hashed, dims)."""

    def __init__(self, n_levels, base_resolution, per_level_scale, log2_hashmap_size):
        import tinycudann as tcnn
        self.cfg = dict(n_levels=n_levels, base_resolution=base_resolution, per_level_scale=per_level_scale,
                        log2_hashmap_size=log2_hashmap_size)
        total, offs, res, scl = tcnn.grid_levels(n_levels, base_resolution, per_level_scale, log2_hashmap_size)
        self.n_levels, self.n_entries = n_levels, total
        self.level = []
        for l in range(n_levels):
            size, r = int(offs[l + 1]) - int(offs[l]), int(res[l])
            stride, dims = 1, 0
            while dims < 3 and stride <= size:      # the dense stride loop of the level table's builder
                stride *= r
                dims += 1
            self.level.append(dict(scale=np.float32(scl[l]), res=r, offset=int(offs[l]), size=size, dims=dims,
                                   hashed=size < stride))


def entry(L, px, py, pz):
    """grid_entry: uint32 arithmetic on int64 tensors."""
    size = L["size"]
    if L["hashed"]:
        idx = px ^ ((py * PRIME_Y) & M32) ^ ((pz * PRIME_Z) & M32)
        return idx & (size - 1) if size & (size - 1) == 0 else idx % size
    idx = px
    if L["dims"] > 1:
        idx = (idx + py * L["res"]) & M32
    if L["dims"] > 2:
        idx = (idx + ((pz * L["res"]) & M32) * L["res"]) & M32
    idx = torch.where(idx >= size, idx - size, idx)
    return torch.where(idx >= size, idx % size, idx)


def cell_frac(q32, scale):
    """The kernel's grid_cell on binary32 q [m, 3]: cell (as uint32 in int64), fraction (binary32, exact), p."""
    p = (float(scale) * q32.double() + 0.5).float()
    fl = torch.floor(p)
    return fl.long() & M32, p - fl


def keep(q32, levels):
    """True for the points whose fraction is at least FACE away from a cell face at every level, in every dimension."""
    ok = torch.ones(q32.shape[0], dtype=torch.bool)
    for L in levels.level:
        _, f = cell_frac(q32, L["scale"])
        ok &= ((f >= FACE) & (f <= 1 - FACE)).all(-1)
    return ok


def _corners(L, table, cell):
    """v [m, 8, 2] binary64: corner k = x-bit | y-bit << 1 | z-bit << 2."""
    vs = []
    for k in range(8):
        e = entry(L, (cell[:, 0] + (k & 1)) & M32, (cell[:, 1] + ((k >> 1) & 1)) & M32, (cell[:, 2] + (k >> 2)) & M32)
        vs.append(table[L["offset"] + e])
    return torch.stack(vs, 1)


def forward(q32, table, levels, dtype=torch.float64, dq=None):
    """The encoding [m, 2 L] in `dtype` at q32 + dq: the kernel's binary32 cell and fraction, moved by s_l dq INSIDE that
    cell (dq: a `dtype` tensor [m, 3] that may require grad; None: no displacement)."""
    table = table.reshape(-1, 2).to(dtype)
    out = []
    for L in levels.level:
        cell, f = cell_frac(q32, L["scale"])
        f = f.to(dtype)
        if dq is not None:
            f = f + torch.tensor(float(L["scale"]), dtype=dtype) * dq
        v = _corners(L, table, cell)
        y = 0
        for k in range(8):
            w = 1
            for d in range(3):
                w = w * (f[:, d] if (k >> d) & 1 else 1 - f[:, d])
            y = y + w[:, None] * v[:, k]
        out.append(y)
    return torch.cat(out, 1)


def grad_q(q32, dout, table, levels):
    """dL/dq [m, 3] of the interpolant inside its cell and the rounding magnitude B [m, 3], binary64.  dout [m, 2 L]."""
    table, dout = table.reshape(-1, 2).double(), dout.double()
    m = q32.shape[0]
    g, B = torch.zeros(m, 3, dtype=torch.float64), torch.zeros(m, 3, dtype=torch.float64)
    for l, L in enumerate(levels.level):
        cell, f = cell_frac(q32, L["scale"])
        f = f.double()
        v = _corners(L, table, cell)
        d2 = dout[:, 2 * l:2 * l + 2]
        s = float(L["scale"])
        for d in range(3):
            e0, e1 = [i for i in range(3) if i != d]
            for j in range(2):
                for k in range(2):
                    w = (f[:, e0] if j else 1 - f[:, e0]) * (f[:, e1] if k else 1 - f[:, e1])
                    lo = (j << e0) | (k << e1)
                    hi = lo | (1 << d)
                    g[:, d] += s * w * (d2 * (v[:, hi] - v[:, lo])).sum(-1)
                    B[:, d] += s * w * (d2.abs() * (v[:, hi].abs() + v[:, lo].abs())).sum(-1)
    return g, B


# ------------------------------------------------------------------------------------------------ mode 1 (point_of)

def pow2b(bound):
    return float(np.frexp(np.float32(2.0) * np.float32(bound))[0]) == 0.5


def point_q(base32, off32, bound):
    """point_of in binary32: q = (clamp(base + off, -bound, bound) + bound) / (2 bound) [m, 3] and the sum base + off."""
    b = torch.tensor(float(np.float32(bound)), dtype=torch.float32)
    t = base32 + off32
    w = torch.minimum(b, torch.maximum(-b, t))
    q = (w + b) * (1.0 / (2.0 * b)) if pow2b(bound) else (w + b) / (2.0 * b)
    return q, t


def points_grad(x32, x2_32, offsets, P0, bound, dout, table, levels, inclusive=True):
    """dL/dx, dL/dx2 [n, 3] (x2 None: the second is None) and their B, binary64: per point grad_q / (2 bound), passed to
    the base only where |base + off| <= bound (`inclusive`; False: the strict rule, for the test that tells them apart)."""
    n, offs = x32.shape[0], torch.from_numpy(np.ascontiguousarray(offsets, np.float32).reshape(-1, 3))
    bnd = float(np.float32(bound))
    out = [[torch.zeros(n, 3, dtype=torch.float64) for _ in range(2)] for _ in range(2)]   # [base][grad, B]
    for p in range(offs.shape[0]):
        which = 0 if p < P0 else 1
        q, t = point_q(x32 if which == 0 else x2_32, offs[p], bound)
        g, B = grad_q(q, dout[p * n:(p + 1) * n], table, levels)
        ok = (t.abs() <= bnd) if inclusive else (t.abs() < bnd)
        out[which][0] += torch.where(ok, g / (2.0 * bnd), torch.zeros_like(g))
        out[which][1] += torch.where(ok, B / (2.0 * bnd), torch.zeros_like(B))
    return out[0][0], (out[1][0] if x2_32 is not None else None), out[0][1], (out[1][1] if x2_32 is not None else None)


def keep_points(x32, offsets, bound, levels):
    """keep() for every stencil point of every sample."""
    offs = torch.from_numpy(np.ascontiguousarray(offsets, np.float32).reshape(-1, 3))
    ok = torch.ones(x32.shape[0], dtype=torch.bool)
    for p in range(offs.shape[0]):
        ok &= keep(point_q(x32, offs[p], bound)[0], levels)
    return ok


# ------------------------------------------------------------------------------------------------ inputs

def points01(levels, n, seed, hand=True):
    """n kept points in [0, 1]^3 (binary32 [n, 3]): the hand-placed ones that pass the filter first, random ones behind."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.rand(3 * n + 64, 3, generator=g)
    if hand:
        placed = torch.tensor([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0.5], [0.5, 0.5, 0.5], [0.25, 0.75, 1]],
                              dtype=torch.float32)
        cand = torch.cat([placed, cand])
    out = cand[keep(cand, levels)][:n]
    assert out.shape[0] == n, "the face filter left too few points"
    return out.contiguous()


def table_uniform(levels, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(levels.n_entries * 2, generator=g) * 2 - 1) * scale).float()
