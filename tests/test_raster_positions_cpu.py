"""CPU: the position gradient of the refine-stage point renderer (include/mi3d.h Part 7).  The float64 model the GPU
tests compare the kernels with (tests/raster_grad_model.py) is first checked against itself - autograd against central
differences, with the visibility asserted unchanged along every probe - and the two new entry points must refuse bad
arguments on the host, before any launch (there is no GPU here)."""
import numpy as np
import torch

import raster_grad_model as M

H = W = 16
P, K, CN = 40, 4, 3
RADIUS = 2.0 / H * 2.0                   # 2 px
STEP = 1e-6
# Agreement reached by this scene (seed 3, three directions): 2.6e-9, 1.4e-9 and 8.6e-9 relative.  Central differences
# in float64 with h = 1e-6 leave h^2 f''' / 6 + eps |f| / h, which near the clamp's 1 / sqrt(u) is of this order; a wrong
# sign or a missing term is an O(1) error.  The bound is ten times the agreement reached (and never above 1e-4).
BOUND = 8.6e-8


def _scene():
    g = torch.Generator().manual_seed(3)
    d = torch.randn(P, 3, generator=g, dtype=torch.float64)
    pts = d / d.norm(dim=-1, keepdim=True) * 0.12 * (1 + 0.05 * torch.randn(P, 1, generator=g, dtype=torch.float64))
    ang = torch.tensor(0.3, dtype=torch.float64)
    rot = torch.tensor([[torch.cos(ang), 0, torch.sin(ang)], [0, 1, 0], [-torch.sin(ang), 0, torch.cos(ang)]],
                       dtype=torch.float64)
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3] = rot
    w2c[:3, 3] = torch.tensor([0.01, -0.02, 1.25], dtype=torch.float64)
    focal = 1.0 / (2 * np.tan(np.radians(20) / 2))
    Kmat = torch.tensor([[focal * W, 0, 0.5 * W], [0, focal * H, 0.5 * H], [0, 0, 1]], dtype=torch.float64)
    feats = torch.rand(P, CN, generator=g, dtype=torch.float64)
    gout = torch.randn(CN, H, W, generator=g, dtype=torch.float64)
    dirs = [(torch.randn(P, 3, generator=g, dtype=torch.float64), torch.randn(4, 4, generator=g, dtype=torch.float64))
            for _ in range(3)]
    return pts, w2c, Kmat, feats, gout, dirs


def test_model_autograd_matches_central_differences():
    pts, w2c, Kmat, feats, gout, dirs = _scene()
    idx = M.brute_rasterize(M.project(pts, w2c, Kmat, H, W), H, W, RADIUS, K)
    used = idx >= 0
    assert float(used[..., 0].float().mean()) > 0.2 and bool(used[..., K - 1].any())     # deep pixels exist
    u = M.clamp_argument(M.dists_from_idx(M.project(pts, w2c, Kmat, H, W), idx), RADIUS)[used]
    assert bool((u < 1e-3).any()) and bool((u > 1e-3).any())                             # both sides of the clamp

    def loss(x, cam):
        return (M.render(x, feats, idx, cam, Kmat, H, W, RADIUS) * gout).sum()

    x, cam = pts.clone().requires_grad_(True), w2c.clone().requires_grad_(True)
    loss(x, cam).backward()
    assert float(x.grad.abs().max()) > 0 and float(cam.grad[:3].abs().max()) > 0
    worst = 0.0
    for vx, vc in dirs:
        vc = vc.clone()
        vc[3] = 0                                            # the projection never reads the bottom row
        for sign in (1, -1):                                 # the condition: the probes see the same visibility
            there = M.brute_rasterize(M.project(pts + sign * STEP * vx, w2c + sign * STEP * vc, Kmat, H, W), H, W,
                                      RADIUS, K)
            assert torch.equal(there, idx)
        with torch.no_grad():
            numeric = (loss(pts + STEP * vx, w2c + STEP * vc) - loss(pts - STEP * vx, w2c - STEP * vc)) / (2 * STEP)
        analytic = (x.grad * vx).sum() + (cam.grad * vc).sum()
        rel = abs(float(numeric - analytic)) / abs(float(analytic))
        print(f"directional derivative {float(analytic):+.9e}, central difference {float(numeric):+.9e}, rel {rel:.2e}")
        worst = max(worst, rel)
    assert worst <= BOUND, worst


def test_new_entry_points_validate_on_the_host():
    """hipErrorInvalidValue (1) for C = 0, C = 33, K = 9 and radius <= 0, from pointers never read: the checks come
    before any launch.  mi3d_points_rasterize_backward takes neither C nor a radius: of the four only K applies to it,
    with K = 0 and an empty image, its forward's own checks."""
    import ctypes as C
    from mi3d import _lib as L
    lib, null = L.lib(), C.c_void_p(0)

    def comp(Cn, Kpp, radius):
        return lib.mi3d_points_composite_backward_dists(null, null, 8, 8, Kpp, null, null, Cn, C.c_double(radius), null,
                                                        null)

    def rast(Hh, Ww, Kpp):
        return lib.mi3d_points_rasterize_backward(null, 16, null, null, Hh, Ww, Kpp, null, null)

    for args in ((0, 8, 0.1), (33, 8, 0.1), (19, 9, 0.1), (19, 8, 0.0), (19, 8, -1.0), (19, 8, float("nan"))):
        assert comp(*args) == 1, args
    for args in ((8, 8, 9), (8, 8, 0), (0, 8, 8), (8, 0, 8)):
        assert rast(*args) == 1, args
