"""GPU: the refine stage's point cloud (mi3d/pointcloud.py over csrc/pointcloud.hip, include/mi3d.h Part 11).

`project` / `z_buffer` / `depth2point` are PINNED: tests/golden/pointcloud.npz holds what the reference's own functions
return (tests/golden/make_golden_pointcloud.py).  The canonical-depth filter is compared with its lines restated here on
NumPy and CPU F.grid_sample; the compaction and the box morphology with NumPy; multidepth2point_mask with a composition
of the pieces tested above it."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_pointcloud", os.path.join(GOLDEN, "make_golden_pointcloud.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)          # look_at, intrinsics, points_a, sphere_depth, noise_image: the fixture's inputs

POINT_TOL = 1e-12                       # fp64 values of magnitude <= 2, evaluation-order differences only


def colour_tol(W):
    """The sample coordinate is formed in fp32 at magnitude <= W in four operations, image values lie in [0, 1]."""
    return 8 * W * 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "pointcloud.npz")))


@pytest.fixture(scope="module")
def case_b(golden):
    H, W = (int(s) for s in golden["b_hw"])
    mask = np.unpackbits(golden["b_mask"])[:H * W].reshape(H, W).astype(bool)
    return dict(H=H, W=W, K=golden["b_K"], c2w=golden["b_c2w"], D=golden["b_depth_mm"] / 1000.0, mask=mask,
                rgb=gen.noise_image(int(golden["b_seed"]), H, W), points=golden["b_points"], colours=golden["b_colours"])


def project_np(v, K, RT):
    cam = v @ RT[:3, :3].T + RT[:3, 3]
    q = cam @ K.T
    return q[:, :2] / q[:, 2:], q[:, 2]


def unproject_np(D, K, c2w):
    """Every pixel's world point, row-major [H * W, 3]."""
    H, W = D.shape
    pix = np.stack([np.tile(np.arange(W), H), np.repeat(np.arange(H), W), np.ones(H * W)], 1).astype(np.float64)
    v = (pix @ np.linalg.inv(K).T) * D.reshape(-1, 1)
    return v @ c2w[:3, :3].T + c2w[:3, 3]


def box_np(img, kh, kw, dilate):
    """Sliding minimum / maximum; what lies outside the image is padded with +inf / -inf, so it is never picked."""
    pad = -np.inf if dilate else np.inf
    p = np.pad(img, ((kh // 2, kh // 2), (kw // 2, kw // 2)), constant_values=pad)
    win = np.lib.stride_tricks.sliding_window_view(p, (kh, kw))
    return (win.max((2, 3)) if dilate else win.min((2, 3))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ z_buffer
def test_z_buffer_matches_the_reference_on_every_point(cuda, golden):
    from mi3d import pointcloud as pc
    H, W = (int(s) for s in golden["a_hw"])
    n = int(golden["a_n"])
    assert float(golden["a_tie_margin"]) >= 1e-9 and float(golden["a_depth_margin"]) >= 1e-9
    v = gen.points_a(int(golden["a_seed"]))
    assert v.shape == (n, 3) and n == 20000 and (H, W) == (48, 64)
    want = np.unpackbits(golden["a_mask"])[:n].astype(bool)
    got = pc.z_buffer(v, golden["a_w2c"], H, W, golden["a_K"], device=cuda)
    assert str(got.dtype) == "torch.bool" and got.is_cuda and got.shape == (n,)
    got = got.cpu().numpy()
    print(f"z_buffer case A: {got.sum()} visible, reference {want.sum()}, mismatches {(got != want).sum()}")
    assert np.array_equal(got, want)


def test_z_buffer_by_hand(cuda):
    from mi3d import pointcloud as pc
    H, W = 48, 64
    K = gen.intrinsics(40.0, H, W)                     # focal * W = 87.9: x = 32 + 87.9 X / Z, y = 24 + 65.9 Y / Z
    v = np.array([[0.100, 0.0, 1.0],                   # 0, 1: one pixel (41, 24), exactly equal depth: both visible
                  [0.101, 0.0, 1.0],
                  [0.101, 0.0, 1.01],                  # 2: same pixel, within 1 / H = 0.0208 of the minimum
                  [0.150, 0.0, 1.5],                   # 3: same pixel, behind
                  [np.nan, 0.0, 1.0],                  # 4: NaN
                  [0.1, 0.1, 0.0],                     # 5: z = 0: the projection is infinite
                  [0.0, 0.0, -1.0],                    # 6, 7: pixel (32, 24), negative depths: -2 is the minimum
                  [0.0, 0.0, -2.0],
                  [-0.2, 0.2, 1.0],                    # 8: alone on its pixel
                  [1.0, 0.0, 1.0],                     # 9: x = 119.9: out of bounds
                  [0.0, -0.37, 1.0]])                  # 10: y = -0.4 rounds to 0: in bounds (row 0)
    got = pc.z_buffer(v, np.eye(4), H, W, K, device=cuda).cpu().numpy()
    assert got.tolist() == [True, True, True, False, False, False, False, True, True, False, True]
    assert pc.z_buffer(np.zeros((0, 3)), np.eye(4), H, W, K, device=cuda).shape == (0,)


def test_project_matches_numpy(cuda, golden):
    from mi3d import pointcloud as pc
    v = gen.points_a(int(golden["a_seed"]))[:4096]
    xy, z = pc.project(v, golden["a_K"], golden["a_w2c"][:3, :4], device=cuda)
    want_xy, want_z = project_np(v, golden["a_K"], golden["a_w2c"])
    assert xy.shape == (4096, 2) and z.shape == (4096, 1) and xy.dtype == z.dtype and str(z.dtype) == "torch.float64"
    # these points lie in the cube, 0.4 <= z <= 2.2: about ten roundings of 1.1e-16 on terms of magnitude <= 200
    assert np.abs(z.cpu().numpy()[:, 0] - want_z).max() <= 1e-12
    assert np.abs(xy.cpu().numpy() - want_xy).max() <= 1e-12


# --------------------------------------------------------------------------------------------------------- depth2point
def test_depth2point_matches_the_reference(cuda, case_b):
    from mi3d import pointcloud as pc
    b = case_b
    v, c = pc.depth2point(b["D"], b["mask"], b["c2w"], b["rgb"], b["H"], b["W"], b["K"], device=cuda)
    assert str(v.dtype) == "torch.float64" and str(c.dtype) == "torch.float32" and v.is_cuda and c.is_cuda
    assert v.shape == b["points"].shape and c.shape == b["colours"].shape
    dv = np.abs(v.cpu().numpy() - b["points"]).max()
    dc = np.abs(c.cpu().numpy() - b["colours"]).max()
    print(f"depth2point case B: {v.shape[0]} rows, max |point error| {dv:.3e}, max |colour error| {dc:.3e} "
          f"(bounds {POINT_TOL:g}, {colour_tol(b['W']):.3e})")
    assert dv <= POINT_TOL
    assert dc <= colour_tol(b["W"])


# ---------------------------------------------------------------------------------------------------------- compaction
PC_BLOCK = 256                          # kBlock of csrc/pointcloud.hip: pixels per workgroup of k_pc_count / k_pc_unproject
PC_SCAN_ROUND = 1024                    # workgroup sums per round of k_pc_scan: kRowThreads of scan_row in csrc/mi3d_scan.h
SMALL, LARGE = (70, 67), (520, 513)     # 19 workgroups; 266 760 pixels = 1043 workgroups: a second, ragged scan round
KINDS = ["random", "zero", "one", "last"]
COMPACT_CASES = ([pytest.param(*SMALL, k, id=k) for k in KINDS] + [pytest.param(*LARGE, k, id=f"520x513-{k}") for k in KINDS]
                 + [pytest.param(*LARGE, "late", id="520x513-late")])


@pytest.mark.parametrize("H,W,kind", COMPACT_CASES)
def test_unproject_compacts_in_pixel_order(cuda, H, W, kind):
    import torch
    from mi3d import _lib
    from mi3d import pointcloud as pc
    # SMALL: 4690 pixels, the last workgroup partial, W no multiple of 64.  The workgroup count is the library's own: the
    # workspace holds one uint32 per workgroup, padded to 8 bytes
    nb = -(-H * W // PC_BLOCK)
    assert int(_lib.lib().mi3d_pc_unproject_workspace(H, W)) == (nb * 4 + 7) // 8 * 8
    if (H, W) == SMALL:
        assert nb == 19
    else:
        assert PC_SCAN_ROUND < nb < 2 * PC_SCAN_ROUND and nb % 64 != 0     # the second round exists and is ragged
    rng = np.random.default_rng(11)
    D = rng.uniform(0.5, 2.0, (H, W))
    mask = {"random": rng.random((H, W)) < 0.4, "zero": np.zeros((H, W), bool), "one": np.ones((H, W), bool),
            "last": np.zeros((H, W), bool), "late": np.zeros((H, W), bool)}[kind]
    if kind == "last":
        mask[-1, -1] = True
    if kind == "late":                                 # only image rows that lie wholly in workgroups of the second scan
        first = -(-PC_SCAN_ROUND * PC_BLOCK // W)      # round: every kept pixel's offset is made there ("random" and "one"
        assert 0 < first < H - 1                       # have kept pixels in both rounds: they check the base carried over)
        mask[first:] = rng.random((H - first, W)) < 0.4
        assert mask.sum() > 1000 and not mask.reshape(-1)[:PC_SCAN_ROUND * PC_BLOCK].any()
    if (H, W) == LARGE and kind in ("random", "one"):  # kept pixels on both sides of the round boundary
        flat = mask.reshape(-1)
        assert flat[:PC_SCAN_ROUND * PC_BLOCK].any() and flat[PC_SCAN_ROUND * PC_BLOCK:].any()
    K = gen.intrinsics(40.0, H, W)
    c2w = gen.look_at([0.4, 0.3, 1.1])
    want = unproject_np(D, K, c2w)[mask.reshape(-1)]
    got = pc.unproject(D, mask, c2w, K, device=cuda)
    again = pc.unproject(D, mask, c2w, K, device=cuda)
    assert got.shape == want.shape and str(got.dtype) == "torch.float64"
    assert torch.equal(got, again) and got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    if len(want):
        assert np.abs(got.cpu().numpy() - want).max() <= POINT_TOL     # a row out of place would be off by far more


# ----------------------------------------------------------------------------------------------------------- box morph
@pytest.fixture(scope="module")
def morph_images():
    rng = np.random.default_rng(7)
    return {"random": rng.standard_normal((37, 53)).astype(np.float32),
            "mask": (rng.random((37, 53)) < 0.9).astype(np.float32)}


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("box", [5, 11, 15, (5, 15)])
def test_box_morph_is_bit_equal_to_numpy(cuda, morph_images, box, iterations):
    from mi3d import pointcloud as pc
    kh, kw = (box, box) if isinstance(box, int) else box
    for name, img in morph_images.items():
        for dilate, fn in ((False, pc.erode), (True, pc.dilate)):
            want = img
            for _ in range(iterations):
                want = box_np(want, kh, kw, dilate)
            got = fn(img, box, iterations=iterations, device=cuda)
            assert str(got.dtype) == "torch.float32" and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), want), (name, dilate)


def test_box_morph_window_larger_than_the_image(cuda):
    from mi3d import pointcloud as pc
    img = np.random.default_rng(8).standard_normal((7, 9)).astype(np.float32)
    assert np.array_equal(pc.erode(img, 15, device=cuda).cpu().numpy(), box_np(img, 15, 15, False))
    assert np.array_equal(pc.dilate(img, 15, device=cuda).cpu().numpy(), box_np(img, 15, 15, True))
    assert np.array_equal(pc.erode(img, 15, device=cuda).cpu().numpy(), np.full((7, 9), img.min(), np.float32))


# ---------------------------------------------------------------------------------------------------- canonical filter
SECOND_EYE = (0.9, -0.2, 0.6)           # case B's sphere from a second camera, 1.25 away


def second_view(case_b, eye=SECOND_EYE):
    H, W, K = case_b["H"], case_b["W"], case_b["K"]
    c2w = gen.look_at(np.asarray(eye) / np.linalg.norm(eye) * 1.25)
    depth, hit = gen.sphere_depth(c2w, K, H, W)
    D = (depth * 1000.0).astype(np.uint16) / 1000.0
    return c2w, D, hit


def cano_filter_restated(v, K, cano_c2w, cano_D, H):
    """refine_utils.py:100-107 with NumPy and CPU F.grid_sample.  Returns (keep, d)."""
    import torch
    import torch.nn.functional as F
    xy, z = project_np(v, K, np.linalg.inv(cano_c2w))
    grid = torch.Tensor(np.round(xy).astype(np.int32)[None, None]) / H * 2. - 1.
    sampled = F.grid_sample(torch.Tensor(cano_D)[None, None], grid, align_corners=False)[0, 0, 0].numpy()
    d = z - sampled
    return ~((d <= 1 / H) & (d >= -0.2)), d


def test_cano_filter_matches_its_restatement(cuda, case_b):
    from mi3d import pointcloud as pc
    b = case_b
    H, W, K = b["H"], b["W"], b["K"]
    c2w, D, hit = second_view(b)
    v = unproject_np(D, K, c2w)[hit.reshape(-1)]
    cano_D = b["D"] * b["mask"]
    want, d = cano_filter_restated(v, K, b["c2w"], cano_D, H)
    near = int(((np.abs(d - 1 / H) < 1e-5) | (np.abs(d + 0.2) < 1e-5)).sum())
    print(f"cano_filter: {len(v)} points, {want.sum()} kept, {near} within 1e-5 of a threshold")
    assert near == 0                                   # two orders above fp32 bilinear evaluation-order differences
    assert 0 < want.sum() < len(v)                     # both outcomes occur
    got = pc.cano_filter(v, K, b["c2w"], cano_D, H, W, device=cuda).cpu().numpy()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ multidepth2point_mask
NOVEL_EYES = (SECOND_EYE, (-0.8, 0.3, 0.7), (0.1, 0.9, 0.5))


@pytest.fixture(scope="module")
def novel(cuda, case_b):
    """Three novel views of case B's sphere and the full result of multidepth2point_mask on them."""
    from mi3d import pointcloud as pc
    b = case_b
    views = [second_view(b, eye) for eye in NOVEL_EYES]
    c2w = np.stack([v[0] for v in views])
    allD = np.stack([v[1] for v in views])
    masks = np.stack([v[2] for v in views])
    imgs = np.stack([gen.noise_image(20 + i, b["H"], b["W"]) for i in range(len(views))])
    cano_v = b["points"]
    cano_D = b["D"] * b["mask"]
    args = (allD, masks, imgs, b["K"], c2w, cano_v, b["c2w"], cano_D, b["H"], b["W"], 2, 8)
    v, c = pc.multidepth2point_mask(*args, device=cuda, npoint=10 ** 6)
    return dict(args=args, c2w=c2w, allD=allD, masks=masks, imgs=imgs, cano_v=cano_v, cano_D=cano_D, v=v, c=c)


def test_multidepth2point_mask_is_the_composition_of_its_pieces(cuda, case_b, novel):
    import torch
    from mi3d import pointcloud as pc, refine
    b, nv = case_b, novel
    H, W, K = b["H"], b["W"], b["K"]
    cano_v = torch.tensor(nv["cano_v"], device=cuda).float()
    vs, cs = [], []
    for i in range(len(NOVEL_EYES)):
        w2c = np.linalg.inv(nv["c2w"][i])
        cover = refine.render_point(cano_v, torch.ones_like(cano_v), H, W, torch.tensor(K, device=cuda).float(),
                                    torch.tensor(w2c, device=cuda).float(), (H, W), 2.0 / H * 2.0, 8)
        cover = np.array(cover[0].permute(1, 2, 0).cpu().numpy() * 255, dtype=np.uint8) / 255
        eroded = np.stack([box_np(cover[:, :, ch], 15, 15, False) for ch in range(3)], -1)
        covered = (eroded[:, :, 0] > 0.9) | (eroded[:, :, 1] > 0.9) | (eroded[:, :, 2] > 0.9)
        mask = np.logical_and(nv["masks"][i], ~covered)
        v = pc.unproject(nv["allD"][i], mask, nv["c2w"][i], K, device=cuda)
        v = v[pc.cano_filter(v, K, b["c2w"], nv["cano_D"], H, W)]
        v = v[pc.z_buffer(v, w2c, H, W, K)]
        vs.append(v)
        cs.append(pc.colour(v, w2c, nv["imgs"][i], H, W, K))
    want_v, want_c = torch.cat(vs), torch.cat(cs)
    print(f"multidepth2point_mask: {[len(v) for v in vs]} points per view")
    assert all(len(v) > 0 for v in vs)
    assert nv["v"].shape == want_v.shape and nv["c"].shape == want_c.shape
    assert str(nv["v"].dtype) == "torch.float64" and str(nv["c"].dtype) == "torch.float32"
    assert (nv["v"] - want_v).abs().max().item() <= POINT_TOL
    assert (nv["c"] - want_c).abs().max().item() <= colour_tol(W)


def test_multidepth2point_mask_draws_a_subset_above_npoint(cuda, novel):
    import torch
    from mi3d import pointcloud as pc
    total = novel["v"].shape[0]
    npoint = total // 3
    assert npoint > 10
    draw = lambda seed: pc.multidepth2point_mask(*novel["args"], device=cuda, npoint=npoint,
                                                 generator=torch.Generator().manual_seed(seed))
    v1, c1 = draw(5)
    v2, c2 = draw(5)
    assert v1.shape == (npoint, 3) and c1.shape == (npoint, 3)
    assert torch.equal(v1, v2) and torch.equal(c1, c2)
    rows = {r.tobytes() for r in np.concatenate([novel["v"].cpu().numpy(), novel["c"].cpu().numpy().astype(np.float64)], 1)}
    got = np.concatenate([v1.cpu().numpy(), c1.cpu().numpy().astype(np.float64)], 1)
    assert all(r.tobytes() in rows for r in got)
    assert len({r.tobytes() for r in got}) == npoint   # drawn without replacement (the full result's rows are distinct)
    assert not torch.equal(draw(6)[0], v1)


# ---------------------------------------------------------------------------------------- from_model / export_point_cloud
@pytest.fixture(scope="module")
def model(cuda):
    import torch
    from mi3d import sds_step
    opt = sds_step.make_opt(max_steps=64, lambda_smooth=0.0, fp16=False)
    m, _, _ = sds_step.build_training_state(opt, cuda, bitfield=0.5)
    with torch.no_grad():
        m.encoder.params.uniform_(-0.3, 0.3)
    return m


FOV, SIDE = 8.0, 32                     # the density blob of the untrained field fills most of a 32 x 32 frame


def five_poses():
    from mi3d import rays
    return np.concatenate([rays.orbit_pose(1.25, 80.0, 30.0 + 25.0 * k).numpy() for k in range(5)]).astype(np.float64)


def test_from_model_points_lie_on_the_rendered_depth(cuda, model):
    from mi3d import pointcloud as pc
    H = W = SIDE
    poses = five_poses()
    rgbs, depths, masks = pc.render_views(model, poses, FOV, H, W, max_steps=64)
    assert model.training                              # the caller's mode is restored
    K = pc.intrinsics(FOV, H, W)
    v_cano, c_cano, v_novel, c_novel = pc.build(rgbs[2], rgbs, depths, masks, poses, K, H, W)
    print(f"from_model: masks {[int(m.sum()) for m in masks]}, {len(v_cano)} canonical and {len(v_novel)} novel points")
    assert len(v_cano) > 0
    assert c_cano.shape == v_cano.shape and c_novel.shape == v_novel.shape
    xy, z = pc.project(v_cano, K, np.linalg.inv(poses[2])[:3, :4])
    xy, z = xy.cpu().numpy(), z.cpu().numpy()[:, 0]
    pix = np.rint(xy)
    assert np.abs(xy - pix).max() <= 1e-9
    D = depths[2].cpu().numpy()
    assert np.abs(z - D[pix[:, 1].astype(int), pix[:, 0].astype(int)]).max() <= 1e-9


def test_export_point_cloud_writes_the_four_files(cuda, model, tmp_path):
    import torch
    from mi3d import pointcloud as pc
    out = tmp_path / "refine"
    ref_rgb = np.random.default_rng(3).random((SIDE, SIDE, 3))
    arrays = model.export_point_cloud(str(out), five_poses(), ref_rgb, FOV, SIDE, SIDE, max_steps=64)
    names = ("vertices_cano.npy", "vertices_color_cano.npy", "vertices_novel.npy", "vertices_color_novel.npy")
    assert pc.FILES == names and sorted(os.listdir(out)) == sorted(names)
    for name, a, dtype in zip(names, arrays, (np.float64, np.float32, np.float64, np.float32)):
        f = np.load(out / name)
        assert f.dtype == dtype and f.ndim == 2 and f.shape[1] == 3
        assert isinstance(a, torch.Tensor) and a.is_cuda and np.array_equal(f, a.cpu().numpy())
    assert len(arrays[0]) == len(arrays[1]) > 0 and len(arrays[2]) == len(arrays[3])
