"""Generates tests/golden/pointcloud.npz from the reference's OWN nerf/refine_utils.py (`project`, `z_buffer`,
`depth2point`, imported unchanged through oracle.ref_import.install() with the packages it cannot have stubbed), run in
the build container only:   python tests/golden/make_golden_pointcloud.py

Case A, z_buffer in the general case: H, W = 48, 64 (non-square: an x / y or H / W swap shows), 19 950 points uniform in
  [-0.5, 0.5]^3 and 50 uniform in [-3, 3]^3 (out of bounds, z <= 0) from np.random.default_rng(seed), a camera at
  distance 1.3 looking at the origin, fov 40 degrees: every pixel's minimum is contended.  An independent NumPy
  restatement (np.minimum.at) must give the identical mask.  Two margins are computed and stored, and the fixture is
  REFUSED if either falls below 1e-9: the smallest distance of a projected coordinate to a rounding tie, and the smallest
  distance of a depth difference to the threshold 1 / H.  Above them the mask cannot depend on the order in which two
  correctly rounded binary64 evaluations add their terms.
Case B, depth2point: H = W = 64, an analytic sphere of radius 0.45 seen from distance 1.25, depth quantised to uint16
  millimetres, a seeded noise image as gt_rgb.

Random inputs are stored as seeds; camera matrices, the quantised depth, the packed masks and the expected points and
colours are stored as arrays.  The file is written with fixed zip timestamps, so a rerun reproduces it byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SEED_A, SEED_B = 3, 5
MARGIN = 1e-9


def look_at(eye):
    """Camera-to-world matrix of a camera at `eye` whose +z axis points at the origin."""
    eye = np.asarray(eye, np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, np.array([0.0, -1.0, 0.0]))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([right, up, fwd], 1)
    c2w[:3, 3] = eye
    return c2w


def intrinsics(fov, H, W):
    focal = 1 / (2 * np.tan(np.deg2rad(fov) / 2))
    return np.array([[focal * W, 0, 0.5 * W], [0, focal * H, 0.5 * H], [0, 0, 1]])


def points_a(seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-0.5, 0.5, (19950, 3)), rng.uniform(-3.0, 3.0, (50, 3))])


def sphere_depth(c2w, K, H, W, radius=0.45):
    """z-depth of the unit-z ray through every pixel (x, y) to the sphere about the origin; 0 and mask False on a miss."""
    pix = np.stack([np.tile(np.arange(W), H), np.repeat(np.arange(H), W), np.ones(H * W)], 1)
    d = pix @ np.linalg.inv(K).T @ c2w[:3, :3].T
    o = c2w[:3, 3]
    a, b, c = (d * d).sum(1), 2 * d.dot(o), o.dot(o) - radius ** 2
    disc = b * b - 4 * a * c
    hit = disc > 0
    t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), 0.0)
    return t.reshape(H, W), hit.reshape(H, W)


def noise_image(seed, H, W):
    return np.random.default_rng(seed).random((H, W, 3))


def save_npz(path, arrays):
    """np.savez_compressed with every member's timestamp fixed: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    from oracle import ref_import
    ref_import.install()
    import nerf.refine_utils as ref

    out = {}
    # ---- case A
    H, W = 48, 64
    K = intrinsics(40.0, H, W)
    c2w = look_at(np.array([0.3, 0.45, 0.84]) / np.linalg.norm([0.3, 0.45, 0.84]) * 1.3)
    w2c = np.linalg.inv(c2w)
    v = points_a(SEED_A)
    mask = ref.z_buffer(v, w2c, H, W, K)
    xy, z = ref.project(v, K, w2c[:3, :4])
    z = z[:, 0]
    with np.errstate(invalid="ignore"):
        r = np.round(xy)
        inb = (r[:, 0] >= 0) & (r[:, 0] <= W - 1) & (r[:, 1] >= 0) & (r[:, 1] <= H - 1)
    pix = (r[inb, 1] * W + r[inb, 0]).astype(np.int64)
    zmin = np.full(H * W, np.inf)
    np.minimum.at(zmin, pix, z[inb])
    restated = np.zeros(len(v), bool)
    restated[inb] = z[inb] - zmin[pix] <= 1.0 / H
    assert np.array_equal(mask, restated), "the reference's z_buffer and its np.minimum.at restatement disagree"
    tie_margin = float(np.abs(np.abs(xy - np.floor(xy) - 0.5)).min())
    depth_margin = float(np.abs((z[inb] - zmin[pix]) - 1.0 / H).min())
    if tie_margin < MARGIN or depth_margin < MARGIN:
        raise SystemExit(f"case A refused: margins {tie_margin:.3g} / {depth_margin:.3g} below {MARGIN:g}: another seed")
    out.update(a_seed=np.int64(SEED_A), a_hw=np.array([H, W], np.int64), a_K=K, a_w2c=w2c, a_mask=np.packbits(mask),
               a_n=np.int64(len(v)), a_tie_margin=np.float64(tie_margin), a_depth_margin=np.float64(depth_margin),
               a_in_bounds=np.int64(inb.sum()), a_z_nonpositive=np.int64((z <= 0).sum()))
    print(f"case A: {mask.sum()} of {len(v)} visible, {inb.sum()} in bounds on {len(np.unique(pix))} pixels, "
          f"{(z <= 0).sum()} with z <= 0, margins {tie_margin:.3g} / {depth_margin:.3g}")

    # ---- case B
    H = W = 64
    K = intrinsics(40.0, H, W)
    c2w = look_at(np.array([0.25, -0.35, 0.9]) / np.linalg.norm([0.25, -0.35, 0.9]) * 1.25)
    depth, hit = sphere_depth(c2w, K, H, W)
    depth_mm = (depth * 1000.0).astype(np.uint16)
    D = depth_mm / 1000.0
    rgb = noise_image(SEED_B, H, W)
    pts, col = ref.depth2point(D, hit, c2w, rgb, H, W, K)
    assert pts.dtype == np.float64 and col.dtype == np.float32 and len(pts) == len(col)
    out.update(b_seed=np.int64(SEED_B), b_hw=np.array([H, W], np.int64), b_K=K, b_c2w=c2w, b_depth_mm=depth_mm,
               b_mask=np.packbits(hit), b_points=pts, b_colours=col)
    print(f"case B: {hit.sum()} masked pixels, {len(pts)} points")

    path = os.path.join(HERE, "pointcloud.npz")
    save_npz(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
