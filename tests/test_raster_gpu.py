"""GPU parity of the refine-stage point renderer (csrc/raster.hip, C ABI Part 7; mi3d.refine.render_point) against the
numpy oracle (oracle/raster_ref.py: refine_utils.py:306-333 with pytorch3d's rasterize_points / alpha_composite
restated - PARITY UNPINNED for those two, pytorch3d is absent).  Indices bit-exact, squared distances and composited
features to fp32 rounding, feature gradients against the oracle's closed form; at BASELINE config 5's size (512 x 512,
half a million points) through properties checked against a brute-force torch evaluation of sampled pixels.  NDC points
fed to the rasteriser directly cover what the camera's clouds do not reach: more tiles than one round of the tile scan,
portrait images, discs wider than a tile (the worst-case workspace), the compositor's channel limits, an empty cloud."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cloud(rng, P, spread=0.35):
    """points on a noisy sphere shell around the origin + a few degenerate ones"""
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (d * spread * (1 + 0.05 * rng.normal(size=(P, 1)))).astype(np.float32)
    return pts


def _camera(dev, radius=1.25):
    from mi3d import rays as R
    c2w = R.orbit_pose(radius, 80.0, 30.0, device=dev)[0]
    return torch.linalg.inv(c2w)


# the last two are portrait: range_y, pix_to_ndc with S1 > S2 on the y axis and the y half of point_bbox
@pytest.mark.parametrize("H,W,K", [(64, 64, 8), (48, 80, 8), (40, 40, 1), (33, 70, 3), (70, 33, 3), (80, 48, 8)])
def test_rasterize_and_composite_match_the_oracle(cuda, H, W, K):
    from mi3d import refine
    from oracle import raster_ref as O
    rng = np.random.default_rng(H * 100 + K)
    P, Cn = 6000, 19
    pts = _cloud(rng, P)
    pts[:40] = pts[40:80]                     # coincident points: equal depth, the index decides
    pts[100:120, 2] += 5.0                    # far behind the camera after projection? (depends on the pose) - keep finite
    w2c = _camera(cuda)
    focal = 1.0 / (2 * np.tan(np.radians(20) / 2))
    Kmat = refine.intrinsics(focal, H, W, cuda)
    x = T(pts, cuda)
    proj = torch.matmul(x, w2c[:3, :3].T) + w2c[:3, 3]
    proj = torch.matmul(proj, Kmat.T)
    proj[:, 0:2] = proj[:, 0:2] / proj[:, 2:]
    proj[:, 0] = (proj[:, 0] / W * 2 - 1.0) * -1
    proj[:, 1] = (proj[:, 1] / H * 2 - 1.0) * -1
    proj[200:230, 2] = -0.5                   # behind the camera: must be skipped
    radius = 2.0 / H * 2.0
    idx, zbuf, dists = refine.rasterize_points(proj, (H, W), radius, K)
    ndc = proj.cpu().numpy()
    idx_o, zbuf_o, dists_o = O.rasterize_points(ndc, H, W, radius, K)
    assert (idx_o >= 0).mean() > 0.05
    assert np.array_equal(idx.cpu().numpy(), idx_o)
    np.testing.assert_allclose(dists.cpu().numpy(), dists_o, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(zbuf.cpu().numpy(), zbuf_o, rtol=0, atol=0)
    # composite forward / backward on these hits
    feats = rng.uniform(0, 1, (P, Cn)).astype(np.float32)
    f = T(feats, cuda).requires_grad_(True)
    out = refine._PointComposite.apply(f, idx, dists, float(radius))
    img_o, w_o = O.alpha_composite(idx_o, O.point_alphas(dists_o, radius), feats)
    np.testing.assert_allclose(out.detach().cpu().numpy(), img_o, rtol=1e-5, atol=1e-6)
    dout = rng.normal(size=(Cn, H, W)).astype(np.float32)
    out.backward(T(dout, cuda))
    g_o = O.alpha_composite_backward(idx_o, w_o, dout, P)
    scale = np.abs(g_o).max()
    assert np.abs(f.grad.cpu().numpy() - g_o).max() <= 2e-5 * scale


TILE_PX = 16             # kTilePx of csrc/raster.hip: a tile is 16 x 16 pixels, one workgroup of k_raster_tiles
SCAN_ROUND = 1024        # tiles per round of k_raster_scan's single workgroup: kRowThreads of scan_row in csrc/mi3d_scan.h
TILE_CHUNK = 256         # kTileThreads: points of a tile's list k_raster_tiles stages in LDS per round


def _tile_of(H, W):
    """[H, W]: the index of the tile every pixel lies in, and the tile count."""
    tiles_x, tiles_y = -(-W // TILE_PX), -(-H // TILE_PX)
    return (np.arange(H)[:, None] // TILE_PX) * tiles_x + np.arange(W)[None, :] // TILE_PX, tiles_x * tiles_y


def _centres(H, W):
    """(xs [W], ys [H]): the NDC point every pixel column / row looks at, as the oracle computes it."""
    from oracle import raster_ref as O
    return O.pix_to_ndc(W - 1 - np.arange(W), W, H), O.pix_to_ndc(H - 1 - np.arange(H), H, W)


def _against_the_oracle(cuda, ndc, H, W, radius, K):
    """The assertions of test_rasterize_and_composite_match_the_oracle on NDC points; returns both sides' outputs."""
    from mi3d import refine
    from oracle import raster_ref as O
    got = refine.rasterize_points(T(ndc, cuda), (H, W), radius, K)
    want = O.rasterize_points(ndc, H, W, radius, K)
    idx, zbuf, dists = (a.cpu().numpy() for a in got)
    assert np.array_equal(idx, want[0])
    np.testing.assert_allclose(dists, want[2], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(zbuf, want[1], rtol=0, atol=0)
    return got, want


def _composite_against_the_oracle(cuda, rng, got, want, P, Cn, radius):
    """Forward and feature gradient on the given hits, with the bounds of test_rasterize_and_composite_match_the_oracle."""
    from mi3d import refine
    from oracle import raster_ref as O
    idx, _, dists = got
    idx_o, _, dists_o = want
    H, W, _ = idx_o.shape
    feats = rng.uniform(0, 1, (P, Cn)).astype(np.float32)
    f = T(feats, cuda).requires_grad_(True)
    out = refine._PointComposite.apply(f, idx, dists, float(radius))
    img_o, w_o = O.alpha_composite(idx_o, O.point_alphas(dists_o, radius), feats)
    np.testing.assert_allclose(out.detach().cpu().numpy(), img_o, rtol=1e-5, atol=1e-6)
    dout = rng.normal(size=(Cn, H, W)).astype(np.float32)
    out.backward(T(dout, cuda))
    g_o = O.alpha_composite_backward(idx_o, w_o, dout, P)
    assert np.abs(g_o).max() > 0
    assert np.abs(f.grad.cpu().numpy() - g_o).max() <= 2e-5 * np.abs(g_o).max()


@pytest.mark.parametrize("H,W", [(528, 512), (512, 528)])
def test_more_tiles_than_one_round_of_the_scan(cuda, H, W):
    """1056 tiles: the offsets of tiles 1024 .. 1055 are made in the scan's second round, from the count of everything
    before them.  Those tiles are the bottom 16 rows (portrait: all of them; landscape: all but their first tile); a
    block of points is planted on pixel centres there, in front of everything else."""
    rng = np.random.default_rng(H)
    tile, n_tiles = _tile_of(H, W)
    assert SCAN_ROUND < n_tiles < 2 * SCAN_ROUND and n_tiles % 64 != 0           # a second round, ragged
    P, K, radius = 3000, 8, 2.0 / min(H, W) * 2.0                                 # 2 pixels
    ndc = np.concatenate([rng.uniform(-1.05, 1.05, (P, 2)), rng.uniform(0.5, 2.0, (P, 1))], 1).astype(np.float32)
    ys, xs = np.nonzero((tile >= SCAN_ROUND) & (np.arange(H)[:, None] % 5 == 2) & (np.arange(W)[None, :] % 5 == 2))
    assert len(ys) >= 250 and set(np.unique(tile[ys, xs])) == set(range(SCAN_ROUND, n_tiles))    # every late tile
    planted = np.arange(100, 100 + len(ys))
    cx, cy = _centres(H, W)
    ndc[planted] = np.stack([cx[xs], cy[ys], np.full(len(ys), 0.25, np.float32)], 1)
    got, want = _against_the_oracle(cuda, ndc, H, W, radius, K)
    idx = got[0].cpu().numpy()
    assert np.array_equal(idx[ys, xs, 0], planted)                                # hits in the late tiles, the planted ones
    early = idx[tile < SCAN_ROUND]
    assert (early[:, 0] >= 0).mean() > 0.05 and (idx[tile >= SCAN_ROUND][:, 0] >= 0).mean() > 0.05
    assert (idx[..., 1] >= 0).any()


@pytest.mark.parametrize("K", [8, 1])
@pytest.mark.parametrize("H,W", [(96, 40), (40, 96)])
def test_discs_wider_than_a_tile(cuda, H, W, K):
    """A radius of 30 pixels: a disc's bounding box spans up to 5 x 5 tiles (tiles_per_point_max and the multi-tile loops
    of k_raster_count / k_raster_fill), and a tile's list runs to several rounds of k_raster_tiles.  Agreement with the
    brute force is the test that the worst-case workspace is enough: a list cut short would lose points.  Then the
    compositor on these hits, at the register limit C = 32 and at C = 1."""
    from mi3d import _lib as L
    rng = np.random.default_rng(H * 10 + K)
    P = 1500
    short = min(H, W)
    radius = 30 * 2.0 / short                              # 30 pixels in NDC of the shorter side, which spans [-1, 1]
    assert 2 * 30 + 1 > 3 * TILE_PX
    half_long = max(H, W) / short                          # the longer side spans [-half_long, half_long]
    # the cloud fills the image's lower three quarters along the long axis and overhangs every other edge by the radius:
    # discs centred outside the image reach in, and the far quarter is covered by disc edges or not at all
    along = rng.uniform(-half_long - radius, 0.5 * half_long - radius, P)
    across = rng.uniform(-1 - radius, 1 + radius, P)
    xy = np.stack([across, along] if H > W else [along, across], 1)
    ndc = np.concatenate([xy, rng.uniform(0.5, 2.0, (P, 1))], 1).astype(np.float32)
    # planted: within a pixel of tile corners, and outside the image by less than the radius along either axis
    cx, cy = _centres(H, W)
    px = 2.0 / short
    # (the corners of the image's far third only: a disc this wide, centred anywhere else, would close the uncovered part)
    corners = [(ty, tx) for ty in range(TILE_PX, H, TILE_PX) for tx in range(TILE_PX, W, TILE_PX)
               if max(ty, tx) >= 2 * max(H, W) // 3]
    assert len(corners) == 4
    for n, (ty, tx) in enumerate(corners):                 # the corner between pixels (ty - 1, tx - 1) and (ty, tx)
        mid = np.array([(cx[tx - 1] + cx[tx]) / 2, (cy[ty - 1] + cy[ty]) / 2])
        ndc[10 + n, :2] = mid + rng.uniform(-1, 1, 2) * px
    n0 = 10 + len(corners)
    outside = np.array([[cx[0] + 0.9 * radius, 0.0], [cx[-1] - 0.9 * radius, 0.3], [0.1, cy[0] + 0.9 * radius],
                        [-0.2, cy[-1] - 0.9 * radius], [cx[0] + 0.99 * radius, cy[0] + 0.1 * radius]], np.float32)
    ndc[n0:n0 + len(outside), :2] = outside
    ndc[n0:n0 + len(outside), 2] = 0.25                    # in front of everything: where they reach, slot 0 is theirs
    ndc[n0 + len(outside), 2] = -0.5                       # one behind the camera
    ws = int(L.lib().mi3d_points_rasterize_workspace(P, H, W, radius))
    tiles = _tile_of(H, W)[1]
    per_point = (ws - (3 * tiles + 4) * 4) // (4 * P)
    assert per_point >= 25, per_point                      # the worst case: 5 x 5 tiles and more
    got, want = _against_the_oracle(cuda, ndc, H, W, radius, K)
    idx_o = want[0]
    covered = (idx_o[..., 0] >= 0).mean()
    print(f"{H}x{W} K={K}: {covered:.3f} of the pixels covered, {per_point} list entries per point provided")
    assert 0.5 < covered < 0.95                            # both outcomes, and the discs' edges cross the image
    assert all((idx_o == n0 + i).any() for i in range(len(outside))) and not (idx_o == n0 + len(outside)).any()
    if K > 1:
        assert (idx_o[..., K - 1] >= 0).mean() > 0.4       # K overflow: more covering points than slots
    for Cn in (32, 1):
        _composite_against_the_oracle(cuda, rng, got, want, P, Cn, radius)


@pytest.mark.parametrize("H,W,K", [(70, 33, 3)])
def test_compositor_limits_on_portrait_hits(cuda, H, W, K):
    """C = 32 (the register limit) and C = 1 on a portrait image; C = 33 and K = 9 are refused; an empty cloud gives -1
    everywhere."""
    from mi3d import _lib as L
    from mi3d import refine
    rng = np.random.default_rng(3)
    P, radius = 2000, 2.0 / W * 2.0
    half = H / W
    ndc = np.concatenate([rng.uniform(-1.05, 1.05, (P, 1)), rng.uniform(-half * 1.05, half * 1.05, (P, 1)),
                          rng.uniform(0.5, 2.0, (P, 1))], 1).astype(np.float32)
    got, want = _against_the_oracle(cuda, ndc, H, W, radius, K)
    assert (want[0][..., 0] >= 0).mean() > 0.3 and (want[0][H // 2:, :, 0] >= 0).any() and (want[0][:H // 2, :, 0] >= 0).any()
    for Cn in (32, 1):
        _composite_against_the_oracle(cuda, rng, got, want, P, Cn, radius)
    idx, _, dists = got
    with pytest.raises(L.Mi3dError):
        refine._PointComposite.apply(torch.rand(P, 33, device=cuda), idx, dists, float(radius))
    with pytest.raises(L.Mi3dError):
        refine.rasterize_points(T(ndc, cuda), (H, W), radius, 9)
    for shape in ((H, W), (33, 70), (512, 528)):
        e_idx, e_z, e_d = refine.rasterize_points(torch.empty(0, 3, device=cuda), shape, radius, K)
        assert e_idx.shape == shape + (K,) and bool((e_idx == -1).all() and (e_z == -1).all() and (e_d == -1).all())
        blank = refine._PointComposite.apply(torch.empty(0, 5, device=cuda), e_idx, e_d, float(radius))
        assert blank.shape == (5,) + shape and bool((blank == 0).all())


def test_render_point_end_to_end_against_the_oracle(cuda):
    """mi3d.refine.render_point (torch projection + HIP rasteriser + compositor) vs the oracle's own projection and
    brute-force rasteriser: a pixel may differ only where a point sits within rounding of the radius."""
    from mi3d import refine
    from oracle import raster_ref as O
    rng = np.random.default_rng(5)
    P, Cn, H, W = 8000, 19, 64, 64
    pts = _cloud(rng, P)
    feats = rng.uniform(0, 1, (P, Cn)).astype(np.float32)
    w2c = _camera(cuda)
    focal = 1.0 / (2 * np.tan(np.radians(20) / 2))
    Kmat = refine.intrinsics(focal, H, W, cuda)
    radius = 2.0 / H * 2.0
    out = refine.render_point(T(pts, cuda), T(feats, cuda), H, W, Kmat, w2c, (H, W), radius, 8)[0].cpu().numpy()
    img_o, _, _, _ = O.render_point(pts, feats, H, W, Kmat.cpu().numpy(), w2c.cpu().numpy(), radius, 8)
    bad = np.abs(out - img_o).max(0) > 1e-4
    assert bad.mean() < 2e-3, bad.mean()


def test_config5_size_properties(cuda):
    """512 x 512, 500 000 points, 19 channels, radius 2 px, 8 points per pixel: every pixel's slots are sorted by
    (depth, index), hold only covering points in front of the camera, and agree with a brute-force top-K over ALL
    points on a sample of pixels; composited coverage stays in [0, 1]; gradient = adjoint of the forward."""
    from mi3d import refine
    rng = np.random.default_rng(9)
    P, Cn, H, W, K = 500_000, 19, 512, 512, 8
    pts = T(_cloud(rng, P), cuda)
    w2c = _camera(cuda)
    focal = 1.0 / (2 * np.tan(np.radians(20) / 2))
    Kmat = refine.intrinsics(focal, H, W, cuda)
    proj = torch.matmul(torch.matmul(pts, w2c[:3, :3].T) + w2c[:3, 3], Kmat.T)
    proj[:, 0:2] = proj[:, 0:2] / proj[:, 2:]
    proj[:, 0] = (proj[:, 0] / W * 2 - 1.0) * -1
    proj[:, 1] = (proj[:, 1] / H * 2 - 1.0) * -1
    radius = 2.0 / H * 2.0
    idx, zbuf, dists = refine.rasterize_points(proj, (H, W), radius, K)
    used = idx >= 0
    assert float(used[..., 0].float().mean()) > 0.05
    assert bool((used[..., 1:] <= used[..., :-1]).all())                       # used slots form a prefix
    z = torch.where(used, zbuf, torch.full_like(zbuf, float("inf")))
    later = (z[..., 1:] > z[..., :-1]) | ((z[..., 1:] == z[..., :-1]) & ((idx[..., 1:] > idx[..., :-1]) | ~used[..., 1:]))
    assert bool(later.all())
    assert bool((dists[used] < radius * radius).all() and (dists[used] >= 0).all())
    # brute force over all points for sampled pixels
    ys = torch.randint(0, H, (64,), device=cuda)
    xs = torch.randint(0, W, (64,), device=cuda)
    xf = 1 - (2 * xs.float() + 1) / W
    yf = 1 - (2 * ys.float() + 1) / H
    d2 = (xf[:, None] - proj[None, :, 0]) ** 2 + (yf[:, None] - proj[None, :, 1]) ** 2
    cover = (d2 < radius * radius) & (proj[None, :, 2] >= 0)
    for i in range(64):
        cand = torch.nonzero(cover[i]).flatten()
        zc = proj[cand, 2]
        order = np.lexsort((cand.cpu().numpy(), zc.cpu().numpy()))[:K]
        want = cand.cpu().numpy()[order]
        got = idx[ys[i], xs[i]].cpu().numpy()
        assert np.array_equal(got[:want.size], want) and (got[want.size:] == -1).all(), i
    feats = torch.rand(P, Cn, device=cuda, requires_grad=True)
    out = refine._PointComposite.apply(feats, idx, dists, float(radius))
    ones = refine._PointComposite.apply(torch.ones(P, 1, device=cuda), idx, dists, float(radius))
    assert float(ones.min()) >= 0 and float(ones.max()) <= 1 + 1e-5
    g = torch.rand_like(out)
    out.backward(g)
    lhs = float((out.detach().double() * g.double()).sum())
    rhs = float((feats.detach().double() * feats.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_refine_train_step_draws_its_own_timestep(cuda):
    """mi3d.refine.refine_train_step with t=None (nerf/utils.py:839-894): without a CLIP model every draw must land on
    the SDS branch (the denoise + CLIP branch of sd.py:153 cannot run without one); with the CLIP stand-in, ref_rgb and
    ref_text the t <= 400 draws take that branch and its loss value joins the step's loss."""
    from mi3d import rays as R, refine, sd_standin as S
    torch.manual_seed(0)
    P, H = 4000, 64
    d = torch.randn(P, 3, device=cuda)
    points = (d / d.norm(dim=-1, keepdim=True) * 0.35).contiguous()
    colour = torch.nn.Parameter(torch.rand(P, 3, device=cuda))
    feat = torch.nn.Parameter(torch.randn(P, 16, device=cuda))
    origin = colour.detach().clone()
    unet = refine.UNet(num_input_channels=19).to(cuda).train()
    opt = torch.optim.Adam([colour, feat] + list(unet.parameters()), lr=1e-3)
    g = S.StableDiffusionStandIn(cuda, dtype=torch.float32, with_decoder=True,
                                 unet_kw=dict(ch=(64, 64, 64, 64), ctx_dim=32, layers=1),
                                 vae_kw=dict(ch=(32, 32, 32, 32), layers=1), decoder_kw=dict(ch=(32, 32, 32, 32), layers=1))
    text_z = torch.randn(2, 77, 32, device=cuda)
    w2c = torch.linalg.inv(R.orbit_pose(1.25, 80.0, 30.0, device=cuda)[0])
    focal = 1.0 / (2 * np.tan(np.radians(20) / 2))
    args = (unet, {"colour": colour, "feat": feat}, opt, g, text_z, points, w2c, focal, H, H, 2.0 / H * 2.0, 8, origin)
    for _ in range(12):   # (0.2, 0.6) step range: about half of unrestricted draws would be <= 400
        loss = refine.refine_train_step(*args)
        assert torch.isfinite(loss)
    clip = S.CLIPStandIn(width=64, layers=2, heads=2, embed=32, text_width=32, text_layers=2, text_heads=2).to(cuda)
    for p in clip.parameters():
        p.requires_grad_(False)
    ref_rgb = torch.rand(1, 3, 512, 512, device=cuda)
    base = float(refine.refine_train_step(*args, t=500, clip_model=clip, ref_rgb=ref_rgb, ref_text="a toy"))
    with_clip = float(refine.refine_train_step(*args, t=300, clip_model=clip, ref_rgb=ref_rgb, ref_text="a toy"))
    assert np.isfinite(base) and np.isfinite(with_clip)
    for _ in range(6):
        assert torch.isfinite(refine.refine_train_step(*args, clip_model=clip, ref_rgb=ref_rgb, ref_text="a toy"))


def test_refine_train_step_with_the_trainer_level_terms(cuda):
    """nerf/utils.py:872-884 as the trainer issues them: the front view's masked L1 against the reference image, the novel
    view's guidance step + 10 x CLIP image-image + contextual (VGG19 relu5_4) terms - both change the point colours, the
    learned features and the U-Net; the novel view's extra terms really back-propagate (the step differs from one
    without them)."""
    from mi3d import rays as R, refine, sd_standin as S
    torch.manual_seed(0)
    P, H = 4000, 64
    d = torch.randn(P, 3, device=cuda)
    points = (d / d.norm(dim=-1, keepdim=True) * 0.35).contiguous()
    g = S.StableDiffusionStandIn(cuda, dtype=torch.float32, unet_kw=dict(ch=(64, 64, 64, 64), ctx_dim=32, layers=1),
                                 vae_kw=dict(ch=(32, 32, 32, 32), layers=1))
    text_z = torch.randn(2, 77, 32, device=cuda)
    w2c = torch.linalg.inv(R.orbit_pose(1.25, 80.0, 30.0, device=cuda)[0])
    focal = 1.0 / (2 * np.tan(np.radians(20) / 2))
    clip = S.CLIPStandIn(width=64, layers=2, heads=2, embed=32, text_width=32, text_layers=2, text_heads=2).to(cuda)
    cx = refine.ContextualLoss().to(cuda)
    for p in list(clip.parameters()) + list(cx.parameters()):
        p.requires_grad_(False)
    ref_rgb = torch.rand(1, 3, H, H, device=cuda)
    gt_mask = (torch.rand(1, 1, H, H, device=cuda) > 0.3).float()

    def fresh():
        torch.manual_seed(1)
        colour = torch.nn.Parameter(torch.rand(P, 3, device=cuda))
        feat = torch.nn.Parameter(torch.randn(P, 16, device=cuda))
        unet = refine.UNet(num_input_channels=19).to(cuda).train()
        opt = torch.optim.Adam([colour, feat] + list(unet.parameters()), lr=1e-3)
        return colour, feat, unet, (unet, {"colour": colour, "feat": feat}, opt, g, text_z, points, w2c, focal, H, H,
                                   2.0 / H * 2.0, 8, colour.detach().clone())
    # front view
    colour, feat, unet, args = fresh()
    c0, f0, w0 = colour.detach().clone(), feat.detach().clone(), unet.start.block["conv_f"].weight.detach().clone()
    loss = refine.refine_train_step(*args, is_front=True, ref_rgb=ref_rgb, gt_mask=gt_mask)
    assert torch.isfinite(loss) and float(loss) > 0
    assert float((colour - c0).abs().max()) > 0 and float((feat - f0).abs().max()) > 0
    assert float((unet.start.block["conv_f"].weight - w0).abs().max()) > 0
    with pytest.raises(ValueError):
        refine.refine_train_step(*args, is_front=True)
    # novel view, with and without the trainer-level terms (same seeds, same timestep: the SDS branch)
    outs = []
    for extra in (False, True):
        colour, feat, unet, args = fresh()
        torch.manual_seed(7)
        kw = dict(clip_model=clip, ref_rgb=ref_rgb, ref_text="a toy", cx_model=cx) if extra else {}
        loss = refine.refine_train_step(*args, t=500, **kw)
        assert torch.isfinite(loss)
        outs.append((float(loss), feat.detach().clone()))
    assert outs[1][0] != outs[0][0] and float((outs[1][1] - outs[0][1]).abs().max()) > 0
