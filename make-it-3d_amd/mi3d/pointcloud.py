"""The refine stage's data preparation: the coarse stage's depth / mask / rgb views, or the trained field itself, ->
the coloured point cloud `refine_train_step` starts from (the reference's nerf/refine_utils.py:36-208, :335-410, fed by
`Trainer.refine`, nerf/utils.py:747-788).  The kernels are csrc/pointcloud.hip; include/mi3d.h Part 11 states their
arithmetic (geometry in binary64, sampling in binary32, as NumPy and torch give the reference).

  project, z_buffer, depth2point   the reference's names, argument order and results (PINNED by fixtures its own functions
                                   generate, tests/golden/pointcloud.npz)
  erode, dilate                    cv2.erode / cv2.dilate by a box of ones; the border rule is this project's contract
  canny, depth_edge_mask           cv2.Canny (aperture 3, L1 gradient) and the depth-edge mask load_views builds from it
                                   (:386-393); csrc/canny.hip, include/mi3d.h Part 12 states the arithmetic, which is
                                   restated from memory: this project's contract, cv2 parity unpinned
  multidepth2point_mask            the novel views' points: coverage of the canonical cloud (refine.render_point), erosion,
                                   unprojection, the canonical-depth filter, z_buffer, colours
  build                            `load_views` for arrays already in memory at H x W
  render_views, from_model         the views rendered with the model's eval route and quantised as the reference's files
                                   are; then build
  save                             the four .npy files under the reference's names

Inputs may be NumPy arrays or tensors; results are tensors on the GPU (float64 points, float32 colours, bool masks).
3 x 3 and 4 x 4 inverses are taken on the host in NumPy float64.  There is no CPU path: a CPU device raises Mi3dError.

Not comparable with the reference: the subset draw above `npoint` (torch.randperm under `generator`; the reference
shuffles with NumPy's global state), and the erosion's border and the Canny detector's arithmetic (cv2 is on no machine
this project builds on).  The depth-edge mask is opt-in (`depth_edges=True`); the default leaves it out, as before.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import Mi3dError

MAX_SIDE, MAX_BOX = 16384, 31
HYSTERESIS_SWEEPS = 8                   # sweeps per host read of `changed`: a sweep is a launch, the read is what costs
FILES = ("vertices_cano.npy", "vertices_color_cano.npy", "vertices_novel.npy", "vertices_color_novel.npy")


def _device(device=None, *like):
    """The GPU the work runs on: `device`, else the device of the first GPU tensor among `like`, else the current one."""
    if device is None:
        device = next((t.device for t in like if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if device is None:
        if not torch.cuda.is_available():
            raise Mi3dError("the point-cloud kernels need a GPU: there is no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise Mi3dError(f"the point-cloud kernels need a GPU device (got {device}): there is no CPU path")
    return device


def _host(a, shape, name):
    """A NumPy float64 copy of a small matrix, on the host."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise Mi3dError(f"{name} must have shape {shape} (got {a.shape})")
    return a


def _doubles(a):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return (C.c_double * a.size)(*a.tolist())


def _camera(K, RT):
    """(rt, k) argument blocks: the rows [R | t] of a world-to-camera matrix (3 x 4 or 4 x 4) and the intrinsics."""
    RT = RT.detach().cpu().numpy() if isinstance(RT, torch.Tensor) else np.asarray(RT)
    if RT.shape not in ((3, 4), (4, 4)):
        raise Mi3dError(f"a world-to-camera matrix must be 3 x 4 or 4 x 4 (got {RT.shape})")
    return _doubles(RT[:3, :4]), _doubles(_host(K, (3, 3), "K"))


def _upload(a, dtype, device):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.detach().to(device=device, dtype=dtype).contiguous()


def _size(H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise Mi3dError(f"H and W must lie in [1, {MAX_SIDE}] (got {H} x {W})")
    return H, W


def _check(shapes):
    """Every (array, shape, name) before anything is uploaded or launched."""
    for a, shape, name in shapes:
        got = tuple(np.shape(a)) if not isinstance(a, torch.Tensor) else tuple(a.shape)
        if got != tuple(shape):
            raise Mi3dError(f"{name} must have shape {tuple(shape)} (got {got}): resizing is not restated")


def _image(a, shape, dtype, device, name):
    _check([(a, shape, name)])
    return _upload(a, dtype, device)


def _poses(c2w, V, name):
    c2w = c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w)
    c2w = np.ascontiguousarray(c2w, dtype=np.float64)
    if c2w.shape != (V, 4, 4):
        raise Mi3dError(f"{name} must be [{V}, 4, 4] (got {c2w.shape})")
    return c2w


def _points(v, device):
    shape = tuple(v.shape) if isinstance(v, torch.Tensor) else np.shape(v)
    if len(shape) != 2 or shape[1] != 3:
        raise Mi3dError(f"points must be [n, 3] (got {tuple(shape)})")
    return _upload(v, torch.float64, device)


# ------------------------------------------------------------------------------------------------ the reference's names
def project(xyz, K, RT, device=None):
    """refine_utils.py:154-158.  Returns (xy float64 [n, 2], z float64 [n, 1]) on the GPU."""
    dev = _device(device, xyz)
    v = _points(xyz, dev)
    rt, k = _camera(K, RT)
    n = v.shape[0]
    xy = torch.empty(n, 2, dtype=torch.float64, device=dev)
    z = torch.empty(n, 1, dtype=torch.float64, device=dev)
    _lib.launch("mi3d_pc_project", v, _lib.ptr(v), n, rt, k, _lib.ptr(xy), _lib.ptr(z))
    return xy, z


def _visible(v, rt, k, H, W):
    n, dev = v.shape[0], v.device
    zkeys = torch.empty(H, W, dtype=torch.int64, device=dev)
    vis = torch.empty(n, dtype=torch.uint8, device=dev)
    _lib.launch("mi3d_pc_zmin", v, _lib.ptr(v), n, rt, k, H, W, _lib.ptr(zkeys))
    _lib.launch("mi3d_pc_visible", v, _lib.ptr(v), n, rt, k, H, W, _lib.ptr(zkeys), _lib.ptr(vis))
    return vis.bool()


def z_buffer(vertices, world2cam, H, W, K, device=None):
    """refine_utils.py:167-208: bool [n], True where a point projects into the image and lies within 1 / H of the
    smallest depth on its pixel."""
    H, W = _size(H, W)
    dev = _device(device, vertices)
    rt, k = _camera(K, world2cam)
    return _visible(_points(vertices, dev), rt, k, H, W)


def _unproject(D, mask, K, c2w):
    """D float64 [H, W] and mask uint8 [H, W] on the GPU -> the kept pixels' world points float64 [n, 3], row-major."""
    H, W = D.shape
    dev = D.device
    kinv = _doubles(np.linalg.inv(_host(K, (3, 3), "cam")))
    pose = _doubles(_host(c2w, (4, 4), "c2w")[:3, :4])
    ws_bytes = int(_lib.lib().mi3d_pc_unproject_workspace(H, W))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    points = torch.empty(H * W, 3, dtype=torch.float64, device=dev)
    _lib.launch("mi3d_pc_unproject", D, _lib.ptr(D), _lib.ptr(mask), H, W, kinv, pose, _lib.ptr(ws), ws_bytes,
                _lib.ptr(points), H * W, _lib.ptr(count))
    return points[:int(count)]                           # the one host read of an unprojection


def _colour(v, rt, k, image, H, W):
    out = torch.empty(v.shape[0], 3, dtype=torch.float32, device=v.device)
    _lib.launch("mi3d_pc_colour", v, _lib.ptr(v), v.shape[0], rt, k, _lib.ptr(image), H, W, _lib.ptr(out))
    return out


def _planes(rgb, H, W, device, name):
    """[H, W, 3] in [0, 1] -> float32 [3, H, W], as the reference's torch.Tensor(..).permute(..) makes it."""
    return _image(rgb, (H, W, 3), torch.float32, device, name).permute(2, 0, 1).contiguous()


def colour(vertices, world2cam, gt_rgb, H, W, K, device=None):
    """refine_utils.py:147-151 alone: gt_rgb [H, W, 3] sampled bilinearly at the unrounded projections, float32 [n, 3]."""
    H, W = _size(H, W)
    dev = _device(device, vertices, gt_rgb)
    rt, k = _camera(K, world2cam)
    return _colour(_points(vertices, dev), rt, k, _planes(gt_rgb, H, W, dev, "gt_rgb"), H, W)


def unproject(D, alphamask, c2w, cam, device=None):
    """The first half of depth2point (:131-139): the world points of the pixels whose mask is set, in row-major pixel
    order, float64 [n, 3]."""
    dev = _device(device, D, alphamask)
    H, W = _size(*D.shape)
    D = _upload(D, torch.float64, dev)
    mask = (_image(alphamask, (H, W), torch.float64, dev, "alphamask") != 0).to(torch.uint8)
    return _unproject(D, mask, cam, c2w)


def depth2point(D, alphamask, c2w, gt_rgb, H, W, cam, device=None):
    """refine_utils.py:129-152: unproject the pixels with `alphamask == 1`, keep what z_buffer sees from the view's own
    camera, colour from gt_rgb [H, W, 3].  Returns (points float64 [n, 3], colours float32 [n, 3])."""
    H, W = _size(H, W)
    dev = _device(device, D, alphamask, gt_rgb)
    _check([(D, (H, W), "D"), (alphamask, (H, W), "alphamask"), (gt_rgb, (H, W, 3), "gt_rgb")])
    D = _image(D, (H, W), torch.float64, dev, "D")
    image = _planes(gt_rgb, H, W, dev, "gt_rgb")
    mask = (_image(alphamask, (H, W), torch.float64, dev, "alphamask") == 1).to(torch.uint8)
    c2w = _host(c2w, (4, 4), "c2w")
    v = _unproject(D, mask, cam, c2w)
    rt, k = _camera(cam, np.linalg.inv(c2w))
    v = v[_visible(v, rt, k, H, W)]
    return v, _colour(v, rt, k, image, H, W)


# ------------------------------------------------------------------------------------------------------------ morphology
def _box(k):
    kh, kw = (k, k) if isinstance(k, (int, np.integer)) else k
    kh, kw = int(kh), int(kw)
    if kh < 1 or kw < 1 or kh % 2 == 0 or kw % 2 == 0 or kh > MAX_BOX or kw > MAX_BOX:
        raise Mi3dError(f"a box must have odd sides in [1, {MAX_BOX}] (got {kh} x {kw})")
    return kh, kw


def _morph(img, k, iterations, dilate, device):
    kh, kw = _box(k)
    if int(iterations) < 1:
        raise Mi3dError(f"iterations must be at least 1 (got {iterations})")
    if not isinstance(img, torch.Tensor):
        img = np.asarray(img)
    if len(img.shape) != 2:
        raise Mi3dError(f"a single-channel [H, W] image is expected (got {tuple(img.shape)})")
    H, W = _size(*img.shape)
    dev = _device(device, img)
    src = _upload(img, torch.float32, dev)
    for _ in range(int(iterations)):
        dst = torch.empty_like(src)
        _lib.launch("mi3d_box_morph", src, _lib.ptr(src), _lib.ptr(dst), H, W, kh, kw, int(dilate))
        src = dst
    return src


def erode(img, k, iterations=1, device=None):
    """cv2.erode(img, np.ones((kh, kw)), iterations=iterations) for a single-channel image: float32 [H, W] on the GPU.
    `k` is an odd side or a pair (kh, kw), at most 31.  Pixels outside the image are ignored (cv2's default border)."""
    return _morph(img, k, iterations, False, device)


def dilate(img, k, iterations=1, device=None):
    """cv2.dilate, as `erode`."""
    return _morph(img, k, iterations, True, device)


# ----------------------------------------------------------------------------------------------------------- depth edges
def _threshold(t, name):
    """floor(t) as an int32; NaN is refused.  (No magnitude exceeds 2040: clamping to the int32 range changes nothing.)"""
    t = float(t)
    if math.isnan(t):
        raise Mi3dError(f"{name} is NaN")
    return int(min(max(math.floor(t) if math.isfinite(t) else t, -2.0 ** 31), 2.0 ** 31 - 1))


def _gray(image, device, name="image"):
    """uint8 [H, W], torch or NumPy -> a contiguous uint8 tensor on the GPU.  Any other dtype raises TypeError."""
    if not isinstance(image, torch.Tensor):
        image = np.asarray(image)
    if str(image.dtype).replace("torch.", "") != "uint8":
        raise TypeError(f"{name} must be uint8 (got {image.dtype}): quantise it first, as depth_edge_mask does")
    if len(image.shape) != 2:
        raise Mi3dError(f"a single-channel [H, W] image is expected (got {tuple(image.shape)})")
    H, W = int(image.shape[0]), int(image.shape[1])
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise Mi3dError(f"H, W >= 1 and H * W < 2^31 are needed (got {H} x {W})")
    dev = _device(device, image)
    return _upload(image, torch.uint8, dev), H, W


def canny_classify(image, threshold1, threshold2, device=None):
    """mi3d_canny_classify: Sobel, magnitude, non-maximum suppression and the double threshold in one launch.  Returns
    (cls uint8 [H, W]: 0 not an edge, 1 weak, 2 strong; counts int64 [2] = {weak, strong}), both on the GPU."""
    low, high = _threshold(threshold1, "threshold1"), _threshold(threshold2, "threshold2")
    img, H, W = _gray(image, device)
    cls = torch.empty_like(img)
    counts = torch.empty(2, dtype=torch.int64, device=img.device)
    _lib.launch("mi3d_canny_classify", img, _lib.ptr(img), H, W, low, high, _lib.ptr(cls), _lib.ptr(counts))
    return cls, counts


def hysteresis(cls, sweeps=HYSTERESIS_SWEEPS, device=None):
    """A class map (uint8 [H, W] of 0 / 1 / 2) -> its fixed point under "a weak pixel with a strong 8-neighbour becomes
    strong", a new tensor.  mi3d_canny_hysteresis runs `sweeps` sweeps per call; the host reads `changed` after each call
    and stops at 0.  The result depends on neither `sweeps` nor scheduling.  H * W sweeps always suffice: more calls than
    that raise Mi3dError."""
    sweeps = int(sweeps)
    if sweeps < 1:
        raise Mi3dError(f"sweeps must be at least 1 (got {sweeps})")
    src, H, W = _gray(cls, device, "cls")
    out = src.clone()
    changed = torch.empty(1, dtype=torch.int32, device=out.device)
    for _ in range(-(-H * W // sweeps) + 1):
        _lib.launch("mi3d_canny_hysteresis", out, _lib.ptr(out), H, W, sweeps, _lib.ptr(changed))
        if int(changed) == 0:                            # the one host read of a batch
            return out
    raise Mi3dError(f"hysteresis did not settle within {H * W} sweeps of a {H} x {W} map")


def canny(image, threshold1, threshold2, device=None):
    """cv2.Canny(image, threshold1, threshold2) with apertureSize=3, L2gradient=False, for a uint8 [H, W] image (torch or
    NumPy; any other dtype raises TypeError): uint8 [H, W] of 0 / 255 on the GPU.  The arithmetic is include/mi3d.h Part
    12's, restated from memory and this project's own contract: thresholds floored and swapped if out of order (NaN
    raises), replicated borders, L1 magnitude, integer direction sectors.  One host read (the weak / strong counts); the
    hysteresis is skipped when either count is 0 - with threshold1 == threshold2, the pipeline's case, no pixel is weak."""
    cls, counts = canny_classify(image, threshold1, threshold2, device)
    weak, strong = counts.tolist()
    if weak and strong:
        cls = hysteresis(cls)
    return (cls == 2).to(torch.uint8) * 255


def depth_edge_mask(depth, mask, threshold=10, k=11, device=None):
    """refine_utils.py:386-393: bool [H, W] on the GPU, True within a k x k box of a Canny edge of the masked depth.
    `v = depth * mask * 255.0` in float64, left to right; `np.uint8(v)` as the reference's platforms evaluate it:
    truncation toward zero, then mod 256 (exact for every finite v; NumPy leaves an out-of-range conversion undefined);
    a non-finite v gives 0.  Then canny(., threshold, threshold) and dilate(., k) == 255.
    The quirk this inherits: the quantisation WRAPS above 256 / 255 = 1.004 scene units, so the reference also finds an
    "edge" along that depth contour (and every further multiple); it is kept, because the default reproduces the
    reference."""
    dev = _device(device, depth, mask)
    shape = tuple(depth.shape) if isinstance(depth, torch.Tensor) else np.shape(depth)
    if len(shape) != 2:
        raise Mi3dError(f"a single-channel [H, W] depth is expected (got {tuple(shape)})")
    depth = _image(depth, shape, torch.float64, dev, "depth")
    mask = _image(mask, shape, torch.float64, dev, "mask")
    v = depth * mask * 255.0
    v = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    q = torch.fmod(torch.trunc(v), 256.0)                # exact; the sign of v
    q = torch.where(q < 0, q + 256.0, q).to(torch.uint8)
    return dilate(canny(q, threshold, threshold, device=dev), k, device=dev) == 255


# ------------------------------------------------------------------------------------------------------- the novel views
def _subset(n, npoint, generator, device):
    g_dev = generator.device if generator is not None else torch.device("cpu")
    return torch.randperm(n, generator=generator, device=g_dev)[:npoint].to(device)


def multidepth2point_mask(allD, alphamask, allimg, cam, c2w, cano_v, cano_c2w, cano_D, H, W, radius, ppp, outputdir=None,
                          device=None, npoint=1000000, generator=None):
    """refine_utils.py:61-127.  allD [V, H, W], alphamask [V, H, W], allimg [V, H, W, 3], c2w [V, 4, 4]; cano_v the
    canonical cloud, cano_D its masked depth [H, W].  Per view: the canonical cloud's coverage (refine.render_point with
    white features, radius / H * 2), its 8-bit round trip, 15 x 15 erosion, `> 0.9`; the view's mask without what is
    covered; unprojection; the canonical-depth filter; z_buffer against the view's own camera; colours.  No file is
    written (`outputdir` is accepted and unused).  With `npoint` or more points a uniform subset of `npoint` is drawn by
    torch.randperm under `generator` - the reference shuffles with NumPy's global state, so this step is not comparable.
    Returns (points float64 [n, 3], colours float32 [n, 3])."""
    from . import refine
    del outputdir
    H, W = _size(H, W)
    if H != W:
        raise Mi3dError(f"the canonical-depth filter divides both image axes by H, as the reference does: it needs "
                        f"H == W (got {H} x {W})")
    dev = _device(device, allD, cano_v)
    V = int(allD.shape[0])
    _check([(allD, (V, H, W), "allD"), (alphamask, (V, H, W), "alphamask"), (allimg, (V, H, W, 3), "allimg"),
            (cano_D, (H, W), "cano_D")])
    poses = _poses(c2w, V, "c2w")
    allD = _image(allD, (V, H, W), torch.float64, dev, "allD")
    alphamask = _image(alphamask, (V, H, W), torch.float64, dev, "alphamask") != 0
    allimg = _image(allimg, (V, H, W, 3), torch.float32, dev, "allimg")
    cano_D = _image(cano_D, (H, W), torch.float32, dev, "cano_D")
    K = _host(cam, (3, 3), "cam")
    cano_rt, k = _camera(K, np.linalg.inv(_host(cano_c2w, (4, 4), "cano_c2w")))
    cano_v = _points(cano_v, dev).float()
    white = torch.ones_like(cano_v)
    K32 = torch.tensor(K, device=dev).float()
    r_ndc = float(radius) / float(H) * 2.0
    v_list, c_list = [], []
    with torch.no_grad():
        for i in range(V):
            w2c = np.linalg.inv(poses[i])
            cover = refine.render_point(cano_v, white, H, W, K32, torch.tensor(w2c, device=dev).float(), (H, W), r_ndc,
                                        ppp)[0]
            cover = (cover * 255).to(torch.uint8).float() / 255          # imageio.imwrite / imread / 255
            covered = torch.zeros(H, W, dtype=torch.bool, device=dev)
            for ch in range(3):
                covered |= erode(cover[ch].contiguous(), 15) > 0.9
            mask = (alphamask[i] & ~covered).to(torch.uint8)
            v = _unproject(allD[i], mask, K, poses[i])
            keep = torch.empty(v.shape[0], dtype=torch.uint8, device=dev)
            _lib.launch("mi3d_pc_cano_filter", v, _lib.ptr(v), v.shape[0], cano_rt, k, _lib.ptr(cano_D), H, W,
                        _lib.ptr(keep))
            v = v[keep.bool()]
            rt, _ = _camera(K, w2c)
            v = v[_visible(v, rt, k, H, W)]
            v_list.append(v)
            c_list.append(_colour(v, rt, k, allimg[i].permute(2, 0, 1).contiguous(), H, W))
    v = torch.cat(v_list) if v_list else torch.empty(0, 3, dtype=torch.float64, device=dev)
    c = torch.cat(c_list) if c_list else torch.empty(0, 3, dtype=torch.float32, device=dev)
    if v.shape[0] < npoint:
        return v, c
    pick = _subset(v.shape[0], int(npoint), generator, dev)
    return v[pick], c[pick]


def cano_filter(v, cam, cano_c2w, cano_D, H, W, device=None):
    """refine_utils.py:100-107 alone: bool [n], True for the points the canonical view does NOT already explain (the
    rows multidepth2point_mask keeps)."""
    H, W = _size(H, W)
    if H != W:
        raise Mi3dError(f"the canonical-depth filter needs H == W (got {H} x {W})")
    dev = _device(device, v, cano_D)
    v = _points(v, dev)
    cano_D = _image(cano_D, (H, W), torch.float32, dev, "cano_D")
    rt, k = _camera(cam, np.linalg.inv(_host(cano_c2w, (4, 4), "cano_c2w")))
    keep = torch.empty(v.shape[0], dtype=torch.uint8, device=dev)
    _lib.launch("mi3d_pc_cano_filter", v, _lib.ptr(v), v.shape[0], rt, k, _lib.ptr(cano_D), H, W, _lib.ptr(keep))
    return keep.bool()


def build(ref_rgb, rgbs, depths, masks, c2ws, K, H, W, radius=2, ppp=8, edge_masks=None, device=None, npoint=1000000,
          generator=None, depth_edges=False):
    """`load_views` (refine_utils.py:335-410) for views already in memory at H x W: rgbs [V, H, W, 3] in [0, 1], depths
    [V, H, W], masks [V, H, W] in [0, 1], c2ws [V, 4, 4], ref_rgb [H, W, 3] (the canonical view's colours).  Another size
    raises: cv2.resize is not restated.  The canonical view is (V - 1) // 2; its mask is eroded 11 x 11 twice and compared
    `== 1`, the novel views' once.  `depth_edges=True` removes `depth_edge_mask(depth, eroded mask, 10, 11)` from every
    novel view's mask, as the reference does (:386-395); the canonical view computes none (the reference computes one and
    discards it, :360 is commented out).  `edge_masks` [V, H, W] (bool, the canonical entry unused), if given, is removed
    from the novel masks too (with `depth_edges`: the union).  The default, `depth_edges=False`, leaves every output what
    it was before the detector existed.  Returns (vertices_cano, vertices_color_cano, vertices_novel,
    vertices_color_novel)."""
    H, W = _size(H, W)
    dev = _device(device, depths, masks, rgbs)
    V = int(depths.shape[0])
    if V < 2:
        raise Mi3dError(f"a canonical view and at least one novel view are needed (got {V} views)")
    _check([(depths, (V, H, W), "depths"), (masks, (V, H, W), "masks"), (rgbs, (V, H, W, 3), "rgbs"),
            (ref_rgb, (H, W, 3), "ref_rgb")] + ([(edge_masks, (V, H, W), "edge_masks")] if edge_masks is not None else []))
    poses = _poses(c2ws, V, "c2ws")
    depths = _image(depths, (V, H, W), torch.float64, dev, "depths")
    masks = _image(masks, (V, H, W), torch.float32, dev, "masks")
    rgbs = _image(rgbs, (V, H, W, 3), torch.float32, dev, "rgbs")
    if edge_masks is not None:
        edge_masks = _image(edge_masks, (V, H, W), torch.bool, dev, "edge_masks")
    ind = (V - 1) // 2
    mask_cano = erode(masks[ind], 11, iterations=2) == 1
    depth_cano = depths[ind]
    v_cano, c_cano = depth2point(depth_cano, mask_cano, poses[ind], ref_rgb, H, W, K, device=dev)
    novel = [i for i in range(V) if i != ind]
    all_mask = []
    for i in novel:
        m = erode(masks[i], 11) == 1
        if depth_edges:
            m = m & ~depth_edge_mask(depths[i], m, 10, 11, device=dev)
        if edge_masks is not None:
            m = m & ~edge_masks[i]
        all_mask.append(m)
    v_novel, c_novel = multidepth2point_mask(depths[novel], torch.stack(all_mask), rgbs[novel], K, poses[novel], v_cano,
                                             poses[ind], depth_cano * mask_cano, H, W, radius, ppp, device=dev,
                                             npoint=npoint, generator=generator)
    return v_cano, c_cano, v_novel, c_novel


def intrinsics(fov, H, W):
    """nerf/utils.py:758-759."""
    focal = 1 / (2 * np.tan(np.deg2rad(fov) / 2))
    return np.array([[focal * W, 0, 0.5 * W], [0, focal * H, 0.5 * H], [0, 0, 1]])


def render_views(model, poses, fov, H, W, **render_kwargs):
    """Every pose of `poses` [V, 4, 4] rendered with the eval route the reference's test_step uses (staged, no
    perturbation, all rays, white background, albedo) and quantised as the reference's files are (nerf/utils.py:697-731):
    rgb uint8(. * 255) / 255, depth uint16(depth * 1000) / 1000, mask weights_sum > 0.9.  Returns (rgbs float64
    [V, H, W, 3], depths float64 [V, H, W], masks float32 [V, H, W]) on the model's device."""
    from . import rays
    H, W = _size(H, W)
    dev = model.aabb_train.device
    if dev.type != "cuda":
        raise Mi3dError(f"the point cloud needs the model on the GPU (it is on {dev}): the kernels have no CPU path")
    poses = _upload(poses, torch.float32, dev)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise Mi3dError(f"poses must be [V, 4, 4] (got {tuple(poses.shape)})")
    kwargs = dict(staged=True, perturb=False, force_all_rays=True, bg_color=torch.ones(3, device=dev), shading="albedo",
                  ambient_ratio=1.0)
    kwargs.update(render_kwargs)
    was_training = model.training
    model.eval()
    rgbs, depths, masks = [], [], []
    try:
        with torch.no_grad():
            for pose in poses:
                ro, rd, ds = rays.pinhole_rays(pose[None], H, W, fov)
                out = model.render(ro, rd, depth_scale=ds, **kwargs)
                depth = (out["depth"].reshape(H, W).float() * 1000.0).clamp(0, 65535).to(torch.int32)   # uint16
                depths.append(depth.double() / 1000.0)
                masks.append((out["weights_sum"].reshape(H, W) > 0.9).float())
                rgbs.append((out["image"].reshape(H, W, 3).float() * 255).clamp(0, 255).to(torch.uint8).double() / 255.0)
    finally:
        model.train(was_training)
    return torch.stack(rgbs), torch.stack(depths), torch.stack(masks)


def from_model(model, poses, fov, H, W, ref_rgb=None, radius=2, ppp=8, edge_masks=None, npoint=1000000, generator=None,
               depth_edges=False, **render_kwargs):
    """The trained field -> the four arrays: `render_views`, K as Trainer.refine builds it (nerf/utils.py:758-759), then
    `build`.  `ref_rgb` [H, W, 3] colours the canonical view; without it the canonical render does.  `depth_edges` is
    `build`'s: True drops the novel views' pixels on a depth discontinuity, as the reference does."""
    rgbs, depths, masks = render_views(model, poses, fov, H, W, **render_kwargs)
    if ref_rgb is None:
        ref_rgb = rgbs[(rgbs.shape[0] - 1) // 2]
    poses = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
    return build(ref_rgb, rgbs, depths, masks, poses.astype(np.float64), intrinsics(fov, H, W), H, W, radius=radius,
                 ppp=ppp, edge_masks=edge_masks, device=rgbs.device, npoint=npoint, generator=generator,
                 depth_edges=depth_edges)


def save(outputdir, vertices_cano, vertices_color_cano, vertices_novel, vertices_color_novel):
    """nerf/utils.py:785-788: the four arrays as float64 / float32 / float64 / float32 .npy files.  Returns the paths."""
    os.makedirs(outputdir, exist_ok=True)
    arrays = (vertices_cano, vertices_color_cano, vertices_novel, vertices_color_novel)
    arrays = [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in arrays]
    for name, a in zip(FILES, arrays):
        if a.ndim != 2 or a.shape[1] != 3:
            raise Mi3dError(f"{name}: an [n, 3] array is expected (got {a.shape})")
    if len(arrays[0]) != len(arrays[1]) or len(arrays[2]) != len(arrays[3]):
        raise Mi3dError("points and colours must have the same number of rows")
    paths = [os.path.join(outputdir, name) for name in FILES]
    for path, a, dtype in zip(paths, arrays, (np.float64, np.float32, np.float64, np.float32)):
        np.save(path, a.astype(dtype, copy=False))
    return paths
