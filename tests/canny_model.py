"""A NumPy restatement of include/mi3d.h Part 12 (the Canny detector's contract), for tests/test_canny_cpu.py and
tests/test_canny_gpu.py: `sobel`, `classify`, `hysteresis`, `canny`, `depth_quantise`, and the sliding maximum / minimum
the box morphology is compared with.  Whole-image array arithmetic: no tiles, no sweeps, nothing of the kernels' shape."""
import math

import numpy as np

TG22 = 13573                            # tan(22.5 deg) in 15 fractional bits


def sobel(image):
    """(gx, gy) int32 [H, W] of a uint8 image, borders replicated."""
    p = np.pad(np.asarray(image).astype(np.int32), 1, mode="edge")
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return gx, gy


def thresholds(t1, t2):
    if math.isnan(t1) or math.isnan(t2):
        raise ValueError("NaN threshold")
    low, high = math.floor(t1), math.floor(t2)
    return (high, low) if low > high else (low, high)


def classify(image, t1, t2):
    """Returns (cls uint8 [H, W] of 0 / 1 / 2, sector int8 [H, W]): sector is -1 where mag <= low, else 0 horizontal,
    1 vertical, 2 diagonal with gx, gy of one sign, 3 the other diagonal - the branch that decided the pixel."""
    low, high = thresholds(t1, t2)
    gx, gy = sobel(image)
    mag = (np.abs(gx) + np.abs(gy)).astype(np.int64)
    m = np.pad(mag, 1, constant_values=0)               # magnitudes outside the image are 0
    at = lambda dy, dx: m[1 + dy:m.shape[0] - 1 + dy, 1 + dx:m.shape[1] - 1 + dx]
    ax = np.abs(gx).astype(np.int64)
    ay = np.abs(gy).astype(np.int64) << 15
    t22 = ax * TG22
    t67 = t22 + (ax << 16)
    horizontal, vertical = ay < t22, ay > t67
    same = (gx ^ gy) >= 0
    keep_h = (mag > at(0, -1)) & (mag >= at(0, 1))
    keep_v = (mag > at(-1, 0)) & (mag >= at(1, 0))
    keep_d = (mag > at(-1, -1)) & (mag > at(1, 1))
    keep_a = (mag > at(-1, 1)) & (mag > at(1, -1))
    sector = np.where(horizontal, 0, np.where(vertical, 1, np.where(same, 2, 3))).astype(np.int8)
    keep = np.choose(sector, [keep_h, keep_v, keep_d, keep_a])
    candidate = mag > low
    sector[~candidate] = -1
    cls = np.where(candidate & keep, np.where(mag > high, 2, 1), 0).astype(np.uint8)
    return cls, sector


def grow(strong):
    """The 8-neighbourhood dilation of a bool map."""
    p = np.pad(strong, 1, constant_values=False)
    out = np.zeros_like(strong)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= p[dy:dy + strong.shape[0], dx:dx + strong.shape[1]]
    return out


def hysteresis(cls):
    """The fixed point of "a weak pixel with a strong 8-neighbour becomes strong"."""
    cls = np.asarray(cls).astype(np.uint8).copy()
    while True:
        promote = (cls == 1) & grow(cls == 2)
        if not promote.any():
            return cls
        cls[promote] = 2


def tile_synchronous_sweeps(cls, tile=32):
    """Sweeps until the first one that promotes nothing (that one included), if every tile of a sweep reads its halo as
    the previous sweep left it and runs to its own fixed point: what a sweep-per-launch schedule needs at the least
    favourable timing."""
    cls = np.asarray(cls).astype(np.uint8).copy()
    H, W = cls.shape
    sweeps = 0
    while True:
        sweeps += 1
        before = np.pad(cls, 1, constant_values=0)
        for y0 in range(0, H, tile):
            for x0 in range(0, W, tile):
                y1, x1 = min(y0 + tile, H), min(x0 + tile, W)
                t = before[y0:y1 + 2, x0:x1 + 2].copy()
                inner = np.zeros(t.shape, bool)
                inner[1:-1, 1:-1] = True
                while True:
                    promote = (t == 1) & grow(t == 2) & inner
                    if not promote.any():
                        break
                    t[promote] = 2
                cls[y0:y1, x0:x1] = t[1:-1, 1:-1]
        if np.array_equal(np.pad(cls, 1, constant_values=0), before):
            return sweeps


def canny(image, t1, t2):
    return np.where(hysteresis(classify(image, t1, t2)[0]) == 2, 255, 0).astype(np.uint8)


def depth_quantise(v):
    """`np.uint8(v)` of a float64 array as the reference's platforms evaluate it: truncation toward zero, then mod 256,
    in exact integer arithmetic; a non-finite value gives 0."""
    v = np.asarray(v, np.float64)
    one = lambda x: int(x) % 256 if math.isfinite(x) else 0
    return np.array([one(x) for x in v.ravel().tolist()], np.uint8).reshape(v.shape)


def box(img, kh, kw, dilate):
    """Sliding maximum (dilate) / minimum over the in-image part of a kh x kw window, float32."""
    pad = -np.inf if dilate else np.inf
    p = np.pad(np.asarray(img, np.float32), ((kh // 2, kh // 2), (kw // 2, kw // 2)), constant_values=pad)
    win = np.lib.stride_tricks.sliding_window_view(p, (kh, kw))
    return (win.max((2, 3)) if dilate else win.min((2, 3))).astype(np.float32)


def depth_edge_mask(depth, mask, threshold=10, k=11):
    """refine_utils.py:386-393 on the model."""
    v = np.asarray(depth, np.float64) * np.asarray(mask) * 255.0
    return box(canny(depth_quantise(v), threshold, threshold), k, k, True) == 255


# ------------------------------------------------------------------------------------------------------- the tests' inputs
def wave_image(H, W, seed=0):
    """clip(128 + 100 sin(x / 5) cos(y / 7) + U{-6..6}, 0, 255): gradients of every direction, ties broken by the noise."""
    y, x = np.mgrid[:H, :W]
    noise = np.random.default_rng(seed).integers(-6, 7, (H, W))
    return np.clip(128 + 100 * np.sin(x / 5) * np.cos(y / 7) + noise, 0, 255).astype(np.uint8)


def serpentine(H=96, W=130):
    """A one-pixel-wide weak path: rows 2, 6, 10, ... joined alternately at the right and the left end, one strong pixel
    at (2, 2)."""
    cls = np.zeros((H, W), np.uint8)
    rows = list(range(2, H - 2, 4))
    for j, r in enumerate(rows):
        cls[r, 2:W - 2] = 1
        if j + 1 < len(rows):
            c = W - 3 if j % 2 == 0 else 2
            cls[r:rows[j + 1] + 1, c] = 1
    cls[2, 2] = 2
    return cls


def disc_view(H=64, W=64, centre=(32, 32), radius=14, near=0.9, far=1.3, side=40):
    """A disc at depth `near` in front of a side x side square at depth `far`; the mask is 1 on the square."""
    y, x = np.mgrid[:H, :W]
    depth = np.zeros((H, W))
    mask = np.zeros((H, W))
    y0, x0 = (H - side) // 2, (W - side) // 2
    depth[y0:y0 + side, x0:x0 + side] = far
    mask[y0:y0 + side, x0:x0 + side] = 1.0
    depth[(y - centre[0]) ** 2 + (x - centre[1]) ** 2 <= radius ** 2] = near
    return depth, mask
