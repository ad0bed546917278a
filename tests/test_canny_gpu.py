"""GPU: the Canny depth-edge detector (mi3d.pointcloud.canny / depth_edge_mask / build(depth_edges=True) over
csrc/canny.hip, include/mi3d.h Part 12).  Every comparison is bit-equal with tests/canny_model.py, the NumPy restatement
of the contract that tests/test_canny_cpu.py checks against scipy and by hand.  Parity with cv2 is UNPINNED: cv2 is on no
machine this project builds or runs on."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import canny_model as cm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_pointcloud", os.path.join(GOLDEN, "make_golden_pointcloud.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)          # look_at, intrinsics, noise_image

THRESHOLDS = [(10, 10), (30, 30), (40, 120), (120, 40)]
SIZES = [(1, 1), (1, 70), (70, 1), (33, 65), (96, 130)]      # one pixel; one row / column; one past the tile; many tiles


@pytest.fixture(scope="module")
def wave():
    """The 45 x 67 image (odd sizes, a partial tile on both axes) and the model's classes for every threshold pair."""
    img = cm.wave_image(45, 67, seed=0)
    return img, {t: cm.classify(img, *t) for t in THRESHOLDS}


# ------------------------------------------------------------------------------------------------------------- classify
def test_the_model_reaches_every_branch(wave):
    _, want = wave
    sector = want[(10, 10)][1]
    hit = [int((sector == s).sum()) for s in range(4)]
    cls = want[(40, 120)][0]
    print(f"NMS candidates per branch {hit}; 40/120: {(cls == 1).sum()} weak, {(cls == 2).sum()} strong")
    assert all(h > 0 for h in hit)                     # horizontal, vertical and both diagonals
    assert (cls == 1).any() and (cls == 2).any()


@pytest.mark.parametrize("thresholds", THRESHOLDS)
def test_classify_is_bit_equal_to_the_model(cuda, wave, thresholds):
    from mi3d import pointcloud as pc
    img, want = wave
    cls, counts = pc.canny_classify(img, *thresholds, device=cuda)
    assert str(cls.dtype) == "torch.uint8" and cls.is_cuda and tuple(cls.shape) == img.shape
    w = want[thresholds][0]
    assert np.array_equal(cls.cpu().numpy(), w)
    assert counts.tolist() == [int((w == 1).sum()), int((w == 2).sum())]


@pytest.mark.parametrize("size", SIZES)
def test_classify_and_canny_at_other_sizes(cuda, size):
    import torch
    from mi3d import pointcloud as pc
    img = cm.wave_image(*size, seed=3)
    for t in ((10, 10), (40, 120)):
        w = cm.classify(img, *t)[0]
        cls, counts = pc.canny_classify(torch.from_numpy(img), *t, device=cuda)
        assert np.array_equal(cls.cpu().numpy(), w), t
        assert counts.tolist() == [int((w == 1).sum()), int((w == 2).sum())]
        assert np.array_equal(pc.canny(img, *t, device=cuda).cpu().numpy(), cm.canny(img, *t)), t


@pytest.mark.parametrize("thresholds", THRESHOLDS + [(40.9, 120.9)])
def test_canny_is_bit_equal_to_the_model(cuda, wave, thresholds):
    from mi3d import pointcloud as pc
    img, _ = wave
    got = pc.canny(img, *thresholds, device=cuda)
    assert str(got.dtype) == "torch.uint8" and got.is_cuda and tuple(got.shape) == img.shape
    want = cm.canny(img, *thresholds)
    assert set(np.unique(want).tolist()) == {0, 255}
    assert np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------- hysteresis
def class_maps():
    H, W = 96, 130
    maps = {"serpentine": cm.serpentine(H, W)}
    m = np.zeros((H, W), np.uint8)
    m[H - 1, 20:90] = 1                                # a weak segment on the last row, no strong pixel: must vanish
    maps["orphan"] = m
    m = np.zeros((H, W), np.uint8)
    m[63, 5:64] = 1                                    # a chain joined only through a diagonal step, across a tile corner
    m[64, 64:125] = 1
    m[63, 5] = 2
    maps["diagonal"] = m
    m = cm.serpentine(H, W)
    m[50, 60:62] = 0                                   # a cut of two pixels: everything behind it must drop
    maps["cut"] = m
    m = np.random.default_rng(5).choice(np.array([0, 1, 2], np.uint8), (H, W), p=[0.55, 0.44, 0.01])
    maps["random"] = m
    return maps


@pytest.fixture(scope="module")
def fixed_points():
    maps = class_maps()
    return {k: (m, cm.hysteresis(m)) for k, m in maps.items()}


@pytest.mark.parametrize("sweeps", [1, 7])
@pytest.mark.parametrize("name", ["serpentine", "orphan", "diagonal", "cut", "random"])
def test_hysteresis_reaches_the_models_fixed_point(cuda, fixed_points, name, sweeps):
    from mi3d import pointcloud as pc
    m, want = fixed_points[name]
    if name == "serpentine":
        assert (want[m > 0] == 2).all()
    if name == "orphan":
        assert not (want == 2).any()
    if name == "diagonal":
        assert (want[m > 0] == 2).all() and want[64, 124] == 2
    if name == "cut":
        assert want[50, 59] == 2 and want[50, 62] == 1 and (want == 1).sum() > 100
    got = pc.hysteresis(m, sweeps=sweeps, device=cuda)
    assert str(got.dtype) == "torch.uint8" and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)


def test_the_host_loop_iterates_and_a_stable_map_reports_no_change(cuda, fixed_points):
    import torch
    from mi3d import _lib, pointcloud as pc
    m, want = fixed_points["serpentine"]
    calls, orig = [], _lib.launch

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    pc._lib.launch = spy
    try:
        got = pc.hysteresis(m, sweeps=1, device=cuda)
    finally:
        pc._lib.launch = orig
    print(f"serpentine, one sweep per call: {len(calls)} calls")
    assert np.array_equal(got.cpu().numpy(), want)
    # a tile runs once per sweep and the path comes back into the leftmost tile of a tile row four times (rows 6, 14, 22,
    # 30 from the right): five sweeps per tile row at the very least, whatever the scheduling - the host must iterate
    assert calls.count("mi3d_canny_hysteresis") > 8
    # the raw entry point on the fixed point: nothing to promote
    stable = got.clone()
    changed = torch.full((1,), 7, dtype=torch.int32, device=cuda)
    _lib.launch("mi3d_canny_hysteresis", stable, _lib.ptr(stable), 96, 130, 3, _lib.ptr(changed))
    assert int(changed) == 0 and torch.equal(stable, got)
    # and on the start map: the final sweep of a short call still promotes
    start = torch.from_numpy(m).to(cuda)
    _lib.launch("mi3d_canny_hysteresis", start, _lib.ptr(start), 96, 130, 2, _lib.ptr(changed))
    assert int(changed) != 0


# ------------------------------------------------------------------------------------------------------ depth_edge_mask
def test_depth_edge_mask_matches_the_model(cuda):
    from mi3d import pointcloud as pc
    depth, mask = cm.disc_view()
    m = cm.box(mask, 11, 11, False) == 1
    want = cm.depth_edge_mask(depth, m, 10, 11)
    assert (want & m).any() and (m & ~want).any()       # not vacuous: the model marks pixels inside the eroded mask
    got = pc.depth_edge_mask(depth, m, device=cuda)
    assert str(got.dtype) == "torch.bool" and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    # negative, wrapping and non-finite depths quantise as the model does
    odd = depth.copy()
    odd[20:24, 20:40], odd[30, 30], odd[31, 31], odd[40:44, 20:40] = -0.3, np.nan, np.inf, 7.7
    want = cm.depth_edge_mask(odd, m, 10, 11)
    assert np.array_equal(pc.depth_edge_mask(odd, m, threshold=10, k=11, device=cuda).cpu().numpy(), want)
    assert np.array_equal(pc.depth_edge_mask(odd, m, threshold=40, k=5, device=cuda).cpu().numpy(),
                          cm.depth_edge_mask(odd, m, 40, 5))


# ---------------------------------------------------------------------------------------------------------------- build
EYES = ((0.9, -0.2, 0.6), (0.1, 0.2, 1.0), (-0.8, 0.3, 0.7))


@pytest.fixture(scope="module")
def scene():
    """Three 64 x 64 views of the disc-before-a-square kind, far below `npoint`, and the model's edge masks."""
    H = W = 64
    K = gen.intrinsics(40.0, H, W)
    c2ws = np.stack([gen.look_at(np.asarray(e) / np.linalg.norm(e) * 1.25) for e in EYES])
    views = [cm.disc_view(H, W, centre=c, radius=r) for c, r in (((30, 33), 12), ((32, 32), 14), ((34, 29), 11))]
    depths = np.stack([v[0] for v in views])
    masks = np.stack([v[1] for v in views])
    rgbs = np.stack([gen.noise_image(60 + i, H, W) for i in range(3)])
    eroded = np.stack([cm.box(m, 11, 11, False) == 1 for m in masks])
    M = np.stack([cm.depth_edge_mask(depths[i], eroded[i], 10, 11) for i in range(3)])
    return dict(args=(rgbs[1], rgbs, depths, masks, c2ws, K, H, W), eroded=eroded, M=M)


def same(a, b):
    import torch
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def test_build_with_depth_edges_equals_build_with_the_models_masks(cuda, scene):
    from mi3d import pointcloud as pc
    M, eroded = scene["M"], scene["eroded"]
    assert all((M[i] & eroded[i]).any() for i in (0, 2))            # the novel masks lose pixels
    plain = pc.build(*scene["args"], device=cuda)
    assert same(pc.build(*scene["args"], device=cuda, depth_edges=False), plain)
    got = pc.build(*scene["args"], device=cuda, depth_edges=True)
    want = pc.build(*scene["args"], device=cuda, edge_masks=M)
    print(f"build: rows {[len(t) for t in plain]} without depth edges, {[len(t) for t in got]} with")
    assert same(got, want)
    assert same(got[:2], plain[:2])                                  # the canonical view computes no edge mask
    assert 0 < len(got[2]) < len(plain[2]) < 10 ** 6                 # no random subset is drawn
    extra = np.zeros_like(M)
    extra[:, 24:40, 24:30] = True
    union = pc.build(*scene["args"], device=cuda, depth_edges=True, edge_masks=extra)
    assert same(union, pc.build(*scene["args"], device=cuda, edge_masks=M | extra))
    assert len(union[2]) < len(got[2])


# --------------------------------------------------------------------------------------------------------------- errors
def test_errors(cuda):
    import torch
    from mi3d import _lib, pointcloud as pc
    from mi3d._lib import Mi3dError
    img = cm.wave_image(8, 9)
    with pytest.raises(TypeError):
        pc.canny(img.astype(np.float32), 10, 10, device=cuda)
    with pytest.raises(TypeError):
        pc.canny(torch.from_numpy(img).to(cuda).float(), 10, 10)
    with pytest.raises(Mi3dError):
        pc.canny(img, float("nan"), 10, device=cuda)
    with pytest.raises(Mi3dError):
        pc.canny(np.zeros((3, 8, 9), np.uint8), 10, 10, device=cuda)
    with pytest.raises(Mi3dError):
        pc.canny(img, 10, 10, device="cpu")              # a CPU-only call: there is no CPU path
    with pytest.raises(Mi3dError):
        pc.hysteresis(img, sweeps=0, device=cuda)
    # the entry points refuse what the contract excludes, before any launch
    t = torch.zeros(8, 9, dtype=torch.uint8, device=cuda)
    counts = torch.zeros(2, dtype=torch.int64, device=cuda)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda)
    with pytest.raises(Mi3dError):
        _lib.launch("mi3d_canny_classify", t, _lib.ptr(t), 0, 9, 10, 10, _lib.ptr(t.clone()), _lib.ptr(counts))
    with pytest.raises(Mi3dError):
        _lib.launch("mi3d_canny_classify", t, _lib.ptr(t), 65536, 32768, 10, 10, _lib.ptr(t.clone()), _lib.ptr(counts))
    with pytest.raises(Mi3dError):
        _lib.launch("mi3d_canny_classify", t, _lib.ptr(t), 8, 9, 10, 10, _lib.ptr(t), _lib.ptr(counts))
    with pytest.raises(Mi3dError):
        _lib.launch("mi3d_canny_hysteresis", t, _lib.ptr(t), 8, 9, 0, _lib.ptr(flag))
    with pytest.raises(Mi3dError):
        _lib.launch("mi3d_canny_hysteresis", t, C.c_void_p(0), 8, 9, 1, _lib.ptr(flag))
