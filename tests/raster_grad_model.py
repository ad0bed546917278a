"""A torch restatement of include/mi3d.h Part 7 with the visibility GIVEN, for tests/test_raster_positions_cpu.py and
tests/test_raster_positions_gpu.py: projection -> `dists` from a given idx -> alphas -> composite, in whatever dtype
its inputs have (float64 is the reference, float32 on the CPU the yardstick of fp32 rounding).  Whole-image tensor
arithmetic whose gradients come from torch autograd: no closed form, no recurrence, nothing of the kernels' shape.
`brute_rasterize` is the float64 visibility the CPU test feeds it."""
import numpy as np
import torch


def pix_to_ndc(i, S1, S2):
    """Centre of pixel i (a tensor) along an axis of S1 pixels, the other axis having S2 - in i's dtype, operations in
    the rasteriser's order."""
    rng = torch.tensor(2.0, dtype=i.dtype)
    if S1 > S2:
        rng = (torch.tensor(float(S1), dtype=i.dtype) * rng) / torch.tensor(float(S2), dtype=i.dtype)
    off = rng / 2.0
    return -off + (rng * i + off) / torch.tensor(float(S1), dtype=i.dtype)


def pixel_centres(H, W, dtype=torch.float64):
    """(xf [W], yf [H]): the NDC point output pixel (yi, xi) looks at - both axes mirrored (+X left, +Y up)."""
    xf = pix_to_ndc(torch.arange(W - 1, -1, -1).to(dtype), W, H)
    yf = pix_to_ndc(torch.arange(H - 1, -1, -1).to(dtype), H, W)
    return xf, yf


def project(points, world2cam, Kmat, H, W):
    """render_point's projection, out of place: world [P,3] -> (x_ndc, y_ndc, depth)."""
    p = torch.matmul(points, world2cam[:3, :3].T) + world2cam[:3, 3]
    p = torch.matmul(p, Kmat.T)
    xy = p[:, 0:2] / p[:, 2:]
    x = (xy[:, 0] / W * 2 - 1.0) * -1
    y = (xy[:, 1] / H * 2 - 1.0) * -1
    return torch.stack((x, y, p[:, 2]), 1)


def dists_from_idx(ndc, idx):
    """Squared NDC distance of every slot's point to its pixel's centre [H,W,K]; -1 (and no gradient) where unused."""
    H, W, _ = idx.shape
    xf, yf = pixel_centres(H, W, ndc.dtype)
    safe = idx.clamp(min=0).long()
    d = (xf[None, :, None] - ndc[safe, 0]) ** 2 + (yf[:, None, None] - ndc[safe, 1]) ** 2
    return torch.where(idx >= 0, d, torch.full_like(d, -1.0))


def clamp_argument(dists, radius):
    """u = 0.1 dist / radius^2, the quantity the alpha formula clamps to [1e-3, 1]."""
    return 0.1 * dists / (radius * radius)


def alphas(dists, radius):
    return 1 - torch.sqrt(torch.clamp(clamp_argument(dists, radius), 1e-3, 1.0))


def composite(idx, alpha, feats):
    """alpha_composite, front to back over the K slots; slots with idx < 0 are skipped.  -> [C,H,W]"""
    H, W, K = idx.shape
    out = torch.zeros(H, W, feats.shape[1], dtype=feats.dtype)
    T = torch.ones(H, W, dtype=feats.dtype)
    for k in range(K):
        used = idx[..., k] >= 0
        a = torch.where(used, alpha[..., k], torch.zeros_like(T))
        out = out + (T * a)[..., None] * feats[idx[..., k].clamp(min=0).long()]
        T = T * (1 - a)
    return out.permute(2, 0, 1)


def render_from_dists(dists, idx, feats, radius):
    return composite(idx, alphas(dists, radius), feats)


def render(points, feats, idx, world2cam, Kmat, H, W, radius):
    """render_point for the given visibility."""
    return render_from_dists(dists_from_idx(project(points, world2cam, Kmat, H, W), idx), idx, feats, radius)


def brute_rasterize(ndc, H, W, radius, K):
    """float64 visibility: for every pixel the K nearest covering points (dist < radius^2 strictly, z >= 0) in
    ascending (z, index); idx int32 [H,W,K], -1 where unused."""
    ndc = ndc.detach().double()
    xf, yf = pixel_centres(H, W)
    d2 = (xf[None, :, None] - ndc[None, None, :, 0]) ** 2 + (yf[:, None, None] - ndc[None, None, :, 1]) ** 2
    cover = ((d2 < radius * radius) & (ndc[:, 2] >= 0)[None, None]).numpy()
    z = ndc[:, 2].numpy()
    idx = -np.ones((H, W, K), np.int32)
    for yi in range(H):
        for xi in range(W):
            cand = np.flatnonzero(cover[yi, xi])
            cand = cand[np.lexsort((cand, z[cand]))][:K]
            idx[yi, xi, :cand.size] = cand
    return torch.from_numpy(idx)
