"""CPU: tests/canny_model.py - the NumPy restatement of include/mi3d.h Part 12 that tests/test_canny_gpu.py compares the
kernels with - checked against things that do not share its code: scipy.ndimage's Sobel and connected components,
hand-worked tie rules, NumPy's own uint8 conversion where that is defined.  Then what mi3d.pointcloud refuses before it
touches a device."""
import math

import numpy as np
import pytest

import canny_model as cm


@pytest.fixture(scope="module")
def wave():
    return cm.wave_image(45, 67, seed=0)


def test_sobel_matches_scipy(wave):
    from scipy import ndimage
    for img in (wave, np.random.default_rng(1).integers(0, 256, (9, 5)).astype(np.uint8), wave[:1], wave[:, :1]):
        gx, gy = cm.sobel(img)
        assert np.array_equal(gx, ndimage.sobel(img.astype(np.int32), axis=1, mode="nearest"))
        assert np.array_equal(gy, ndimage.sobel(img.astype(np.int32), axis=0, mode="nearest"))


@pytest.mark.parametrize("thresholds", [(10, 10), (30, 30), (40, 120)])
def test_hysteresis_is_the_components_that_hold_a_strong_pixel(wave, thresholds):
    from scipy import ndimage
    cls, _ = cm.classify(wave, *thresholds)
    labels, n = ndimage.label(cls > 0, structure=np.ones((3, 3)))
    with_strong = np.unique(labels[cls == 2])
    want = np.isin(labels, with_strong[with_strong > 0])
    assert np.array_equal(cm.hysteresis(cls) == 2, want)
    assert np.array_equal(cm.canny(wave, *thresholds) == 255, want)
    serp = cm.serpentine()
    assert np.array_equal(cm.hysteresis(serp) == 2, serp > 0)


def test_tie_rules_by_hand():
    a, b = 5, 3
    v = np.zeros((8, 12), np.uint8)
    v[:, a + 1:] = 200                                   # a vertical step between columns a and a + 1
    e = cm.canny(v, 10, 10)
    assert (e[:, a] == 255).all() and (np.delete(e, a, axis=1) == 0).all()
    h = np.zeros((8, 12), np.uint8)
    h[b + 1:] = 200                                      # a horizontal step between rows b and b + 1
    e = cm.canny(h, 10, 10)
    assert (e[b] == 255).all() and (np.delete(e, b, axis=0) == 0).all()
    assert (cm.canny(np.full((8, 12), 77, np.uint8), 10, 10) == 0).all()
    assert cm.canny(np.array([[200]], np.uint8), 10, 10).tolist() == [[0]]


def test_thresholds_swap_and_floor(wave):
    assert np.array_equal(cm.canny(wave, 120, 40), cm.canny(wave, 40, 120))
    assert np.array_equal(cm.classify(wave, 40.9, 120.9)[0], cm.classify(wave, 40, 120)[0])
    assert not np.array_equal(cm.canny(wave, 40, 120), cm.canny(wave, 120, 120))
    with pytest.raises(ValueError):
        cm.classify(wave, float("nan"), 10)


def test_the_serpentine_needs_more_than_one_batch_of_sweeps():
    from mi3d import pointcloud as pc
    sweeps = cm.tile_synchronous_sweeps(cm.serpentine(), 32)
    print(f"tile-synchronous sweeps for the serpentine at 32 x 32 tiles: {sweeps}")
    assert sweeps > 2 * pc.HYSTERESIS_SWEEPS


def test_depth_quantise():
    v = np.concatenate([np.linspace(0, 256, 4097)[:-1], [0.999999, 255.999999, 229.5]])
    assert np.array_equal(cm.depth_quantise(v), v.astype(np.uint8))           # defined in NumPy: 0 <= v < 256
    beyond = np.array([256.0, 331.5, 511.9, 512.0, 65536.5, -0.5, -1.0, -3.7, -256.0, -257.2, 1e30, 2.0 ** 63])
    want = [0, 75, 255, 0, 0, 0, 255, 253, 0, 255, int(1e30) % 256, 0]
    assert cm.depth_quantise(beyond).tolist() == want
    assert cm.depth_quantise(np.array([[np.nan, np.inf], [-np.inf, 1.5]])).tolist() == [[0, 0], [0, 1]]


def test_the_disc_view_has_an_edge_inside_its_eroded_mask():
    depth, mask = cm.disc_view()
    m = cm.box(mask, 11, 11, False) == 1
    edges = cm.depth_edge_mask(depth, m)
    assert (edges & m).any() and (m & ~edges).any()
    # 1.3 * 255 = 331.5 wraps to 75: the quirk the default inherits
    assert set(np.unique(cm.depth_quantise(depth * m * 255.0)).tolist()) == {0, 75, 229}


# ---------------------------------------------------------------------------------- refused before a device is touched
def test_canny_refuses_what_is_not_a_uint8_image():
    import torch
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    img = cm.wave_image(8, 9)
    with pytest.raises(TypeError):
        pc.canny(img.astype(np.float32), 10, 10)
    with pytest.raises(TypeError):
        pc.canny(torch.from_numpy(img).int(), 10, 10)
    with pytest.raises(Mi3dError):
        pc.canny(img, float("nan"), 10)
    with pytest.raises(Mi3dError):
        pc.canny(img, 10, math.nan)
    with pytest.raises(Mi3dError):
        pc.canny(np.zeros((3, 8, 9), np.uint8), 10, 10)
    with pytest.raises(Mi3dError):
        pc.canny(img, 10, 10, device="cpu")              # there is no CPU path
    with pytest.raises(Mi3dError):
        pc.depth_edge_mask(np.zeros((8, 9)), np.ones((8, 9)), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(Mi3dError):
            pc.canny(img, 10, 10)


def test_depth_edges_is_an_explicit_keyword():
    import inspect
    from mi3d import pointcloud as pc
    for fn in (pc.build, pc.from_model):
        p = inspect.signature(fn).parameters["depth_edges"]
        assert p.default is False and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
