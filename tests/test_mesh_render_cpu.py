"""CPU: the NumPy restatement of include/mi3d.h Part 17 (tests/mesh_render_model.py) - the model the GPU tests compare the
rasteriser with bit for bit - checked here on its own: its visibility against Part 15's depth maps, its
perspective-correct interpolation against a binary64 ray-plane intersection within the running bounds that module's
header derives (counted from the rounding chain, not picked), the bilinear taps on an affine texture, the tie rule; then
mesh.fidelity on hand-built images and the argument checks of mesh.render and export_mesh(preview=) that need no device.

THE BLEND'S BOUND (u = 2^-24).  For texel coordinates gx >= 1 the fractions fx = gx - i0 and hx = 1 - fx are exact
(gx has an ulp of at least 2^-23 there).  top = c00 hx + c10 fx passes two products and a sum, 3 u max|c| at most; so
does bot; c = top hy + bot fy passes three more on top of theirs, and the division by 255 one: a first-order bound of
7 u max|c| / 255 on the colour, of which the tests below allow 8 (a unit of slack for the second-order terms)."""
import numpy as np
import pytest

import mesh_render_model as R
import texture_views_model as M
from test_texture_views_cpu import quad_mesh, sphere_mesh

F = np.float32
H, W = 37, 53
FOCAL = 1.2
Y0 = np.float64(F(0.4))  # the quad's corners as binary32 holds them: y = -+ Y0, and quad_uv gives them v = 0 and 1 exactly
MAX_UNDECIDED = 0.01     # the share of a case's covered pixels that may lie within the margins: a condition of the test


def slanted_views():
    """Three cameras that see the quad at a slant (the depth varies by a third across it), one of them from behind."""
    return np.stack([M.look_at((0.9, 0.3, 1.3), up=(0, 1, 0)), M.look_at((-0.7, 0.8, 1.1), up=(0, 1, 0)),
                     M.look_at((0.5, -0.6, -1.2), up=(0, 1, 0))])


def quad_uv(v, t):
    """Unshared corners vt [3 nt, 2]: an affine function of the quad's own (x, y)."""
    p = v[t.reshape(-1)]
    return np.stack([p[:, 0] + 0.5, (p[:, 1] + 0.4) / 0.8], -1).astype(F)


def test_key_upper_words_equal_the_depth_maps_bitwise():
    v, t = sphere_mesh()
    rec = M.view_records(np.concatenate([M.orbit(2, 2.4, 0.3, 0.2), M.look_at((0.55, 0.0, 0.3), target=(-1, 0, 0))[None]]),
                         M.pinhole(FOCAL, H, W))
    depth, tri, counts = R.visibility(v, t, rec, H, W)
    want, want_counts = M.depth_maps(v, t, rec, H, W)
    assert depth.dtype == F and depth.tobytes() == want.tobytes() and counts == want_counts
    assert counts[1] > 0 and np.isfinite(want).mean() > 0.1     # the close view skips triangles, and something is drawn
    key = R.keys(depth, tri)
    drawn = tri >= 0
    assert (drawn == np.isfinite(want)).all() and (key[~drawn] == R.EMPTY).all()
    assert ((key[drawn] >> np.uint64(32)).astype(np.uint32) == want.view(np.uint32)[drawn]).all()
    assert ((key[drawn] & np.uint64(0xFFFFFFFF)).astype(np.int64) == tri[drawn]).all()


@pytest.fixture(scope="module")
def slant():
    v, t = quad_mesh()
    rec = M.view_records(slanted_views(), M.pinhole(FOCAL, H, W))
    vt = quad_uv(v, t)
    tex = np.zeros((64, 64, 3), np.uint8)
    m32 = R.render(v, t, rec, H, W, vt=vt, texture=tex)
    m64 = R.render(v, t, rec, H, W, F=np.float64, bounds=True, vt=vt, texture=tex)
    return dict(v=v, t=t, rec=rec, vt=vt, m32=m32, m64=m64)


def ray_plane_uv(rec, H, W):
    """Binary64: where the ray through every pixel centre of the view record meets the quad's plane z = 0.1, as the
    (u, v) of quad_uv.  Solves R p + t = z K^-1 (px, py, 1) for (p_x, p_y, z)."""
    rec = rec.astype(np.float64)
    Rm, tv, K = rec[:9].reshape(3, 3), rec[9:12], rec[12:21].reshape(3, 3)
    j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([i, j, np.ones_like(i)], -1) @ np.linalg.inv(K).T
    A = np.empty((H, W, 3, 3))
    A[..., :2] = Rm[:, :2]
    A[..., 2] = -d
    sol = np.linalg.solve(A, np.broadcast_to(-tv - Rm[:, 2] * np.float64(F(0.1)), (H, W, 3))[..., None])[..., 0]
    return np.stack([sol[..., 0] + 0.5, (sol[..., 1] + Y0) / (2 * Y0)], -1)


def test_perspective_correct_uv_against_the_ray_plane_intersection(slant):
    m32, m64 = slant["m32"], slant["m64"]
    covered = m64["tri"] >= 0
    und = m64["undecided"]
    share = und[covered].mean()
    assert covered.sum(axis=(1, 2)).min() > 100                  # every view sees the quad
    print(f"[mesh render] slanted quad: covered {covered.sum(axis=(1, 2))}, undecided {share:.4%}")
    assert share <= MAX_UNDECIDED
    ok = covered & ~und
    assert ((m32["tri"] >= 0)[~und] == covered[~und]).all()      # decided pixels are covered in binary32 iff in binary64
    exact = np.stack([ray_plane_uv(r, H, W) for r in slant["rec"]])
    uv64 = np.stack([m64["u"], m64["v"]], -1)
    bound = m64["Euv"]
    diff64 = np.abs(uv64 - exact)
    print(f"[mesh render] float64 model against the ray-plane intersection: max {diff64[ok].max():.3e}; bound min "
          f"{bound[ok].min():.3e} max {bound[ok].max():.3e}")
    assert (diff64[ok] <= bound[ok]).all()
    assert bound[ok].max() < 1e-4                                # the bound itself says something
    # and the binary32 restatement lies within the same bound of both
    T = 64
    u32 = (m32["gx"].astype(np.float64) + 0.5) / T
    v32 = 1.0 - (m32["gy"].astype(np.float64) + 0.5) / T
    slack = 4 * M.U                                              # gx = u T - 0.5 and gy = (1 - v) T - 0.5: two roundings each
    diff32 = np.abs(np.stack([u32, v32], -1) - exact)
    print(f"[mesh render] binary32 restatement against it: max {diff32[ok].max():.3e}")
    assert (diff32[ok] <= bound[ok] + slack).all()
    lam32, lam64 = m32["bary"].astype(np.float64), m64["bary"]
    same = ok & (m32["tri"] == m64["tri"])
    assert (np.abs(lam32 - lam64)[same] <= m64["Ebary"][same]).all()
    assert np.abs(lam64.sum(-1)[ok] - 1).max() < 1e-12
    # the depth against the exact one of the intersection point
    for k, rec in enumerate(slant["rec"]):
        r = rec.astype(np.float64)
        p = np.concatenate([exact[k][..., :1] - 0.5, exact[k][..., 1:] * (2 * Y0) - Y0,
                            np.full((H, W, 1), np.float64(F(0.1)))], -1)
        z = p @ r[6:9] + r[11]
        assert np.abs(m64["depth"][k] - z)[ok[k]].max() < 1e-9


def test_an_affine_texture_is_reproduced_within_the_blends_bound():
    """Texel (X, Y) holds (X + 2 Y, 3 X, 255 - 2 X - Y): bilinear interpolation reproduces an affine function exactly, so
    the colour is the function at (gx, gy) up to the blend's roundings (this file's header)."""
    v, t = quad_mesh()
    T = 64
    Y, X = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    tex = np.stack([X + 2 * Y, 3 * X, 255 - 2 * X - Y], -1).astype(np.uint8)
    assert tex.max() == 255 and tex[..., 0].max() == 189
    p = v[t.reshape(-1)]
    vt = np.stack([0.1 + 0.8 * (p[:, 0] + 0.5), 0.15 + 0.7 * (p[:, 1] + 0.4) / 0.8], -1).astype(F)   # inside the image
    rec = M.view_records(slanted_views()[:2], M.pinhole(FOCAL, H, W))
    m = R.render(v, t, rec, H, W, vt=vt, texture=tex)
    ok = m["tri"] >= 0
    gx, gy = m["gx"].astype(np.float64)[ok], m["gy"].astype(np.float64)[ok]
    assert ok.sum() > 300 and gx.min() >= 1 and gy.min() >= 1 and gx.max() <= T - 2 and gy.max() <= T - 2
    want = np.stack([gx + 2 * gy, 3 * gx, 255 - 2 * gx - gy], -1) / 255.0
    diff = np.abs(m["image"][ok].astype(np.float64) - want)
    print(f"[mesh render] affine texture: max error {diff.max() / M.U:.2f} u")
    assert m["image"].dtype == F and diff.max() <= 8 * M.U * 255 / 255


def test_two_coincident_triangles_show_the_smaller_index():
    v, t = quad_mesh()
    rec = M.view_records(slanted_views()[:1], M.pinhole(FOCAL, H, W))
    for order in ([0, 1, 0, 1], [1, 0, 1, 0]):
        tt = t[order]
        depth, tri, _ = R.visibility(v, tt, rec, H, W)
        first = np.array([order.index(k) for k in (0, 1)])
        inner = tri >= 0
        assert inner.sum() > 100
        assert set(np.unique(tri[inner])) <= set(first.tolist())      # never a later copy
        single, _, _ = R.visibility(v, t, rec, H, W)
        assert single.tobytes() == depth.tobytes()
    depth, tri, _ = R.visibility(v, t[[0, 0]], rec, H, W)
    assert (tri[tri >= 0] == 0).all() and (tri >= 0).sum() > 50


# ------------------------------------------------------------------------------------------------ fidelity

def test_fidelity_on_hand_built_images():
    from mi3d import mesh
    rng = np.random.default_rng(0)
    a = rng.random((2, 6, 5, 3)).astype(F)
    ones = np.ones((2, 6, 5), F)
    same = mesh.fidelity(a, ones, a.copy(), ones)
    assert same["psnr_union"] == float("inf") and same["psnr_intersection"] == float("inf") and same["iou"] == 1.0
    assert len(same["views"]) == 2 and all(r["iou"] == 1.0 for r in same["views"])
    # a constant offset of 0.1 in every channel: mse = 0.01, 20 dB
    b = (a.astype(np.float64) * 0.5)
    off = mesh.fidelity(b, ones, b + 0.1, ones)
    assert abs(off["psnr_union"] - 20.0) < 1e-9 and abs(off["psnr_intersection"] - 20.0) < 1e-9
    # disjoint masks: no pixel in both
    left, right = np.zeros((2, 6, 5), F), np.zeros((2, 6, 5), F)
    left[:, :, :2], right[:, :, 3:] = 1, 1
    apart = mesh.fidelity(a, left, a, right)
    assert apart["iou"] == 0.0 and np.isnan(apart["psnr_intersection"]) and apart["psnr_union"] == float("inf")
    # half overlap, an offset only where just one mask is set: the union sees it, the intersection does not
    wide = np.zeros((2, 6, 5), F)
    wide[:, :, :4] = 1
    c = b.copy()
    c[:, :, 2:4] += 0.1
    part = mesh.fidelity(b, left, c, wide)
    assert part["iou"] == 0.5 and part["psnr_intersection"] == float("inf")
    assert abs(part["psnr_union"] - 10 * np.log10(1 / (0.01 * 0.5))) < 1e-9
    # per view: view 1 alone differs
    d = b.copy()
    d[1] += 0.01
    views = mesh.fidelity(b, ones, d, ones)["views"]
    assert views[0]["psnr_union"] == float("inf") and abs(views[1]["psnr_union"] - 40.0) < 1e-9
    with pytest.raises(mesh.Mi3dError, match="one size"):
        mesh.fidelity(a, ones, a[:, :5], ones)


def test_box_average_and_quantise():
    import torch
    from mi3d import mesh
    x = torch.arange(2 * 4 * 6 * 3, dtype=torch.float32).reshape(2, 4, 6, 3) / 7
    y = mesh.box_average(x, 2).numpy()
    n = x.numpy().reshape(2, 2, 2, 3, 2, 3)
    want = (((n[:, :, 0, :, 0] + n[:, :, 0, :, 1]) + n[:, :, 1, :, 0]) + n[:, :, 1, :, 1]) * F(0.25)
    assert y.tobytes() == want.tobytes() and mesh.box_average(x, 1) is x
    q = mesh.quantise(torch.tensor([-0.5, 0.0, 0.5, 0.999, 1.0, 2.0, float("nan")]))
    assert q.tolist() == [0, 0, 127, 254, 255, 255, 0]


# ------------------------------------------------------------------------------------------------ argument checks

def test_render_checks_its_options_before_the_mesh():
    from mi3d import mesh
    c2w, K = M.orbit(2), M.pinhole(1.0, 8, 6)
    for kw, words in ((dict(shading="phong"), "shading"), (dict(ssaa=3), "ssaa"), (dict(ambient_ratio=2.0), "ambient_ratio"),
                      (dict(bg_color=(1.0, 2.0)), "bg_color"), (dict(light_d=(0.0, 0.0, 0.0)), "light_d"),
                      (dict(H=1), "1 x 6"), (dict(K=np.eye(4)), "(4, 4)")):
        args = dict(c2w=c2w, K=K, H=8, W=6)
        args.update(kw)
        with pytest.raises(mesh.Mi3dError) as e:
            mesh.render(None, None, **args)                      # no mesh, no device: the options are refused first
        assert words in str(e.value)


def test_export_mesh_checks_preview_before_any_work(tmp_path):
    from mi3d import mesh
    good = dict(c2w=M.orbit(2), K=M.pinhole(1.0, 8, 6), H=8, W=6)
    for change, words in ((dict(colour=1), "colour"), (dict(H=1), "1 x 6"), (dict(ssaa=3), "ssaa"),
                          (dict(shading="phong"), "shading"), (dict(fidelity=1), "fidelity"),
                          (dict(fidelity=True, shading="normal"), "albedo"), (dict(c2w=np.zeros((2, 3, 4))), "(2, 3, 4)")):
        with pytest.raises(mesh.Mi3dError) as e:
            mesh.export(None, str(tmp_path), preview={**good, **change})
        assert words in str(e.value)
    with pytest.raises(mesh.Mi3dError, match="missing keys \\['K'\\]"):
        mesh.export(None, str(tmp_path), preview={k: a for k, a in good.items() if k != "K"})
    with pytest.raises(mesh.Mi3dError, match="dict"):
        mesh.export(None, str(tmp_path), preview=[1])
    assert not any(tmp_path.iterdir())


def test_camera_rays_project_to_the_pixel_centres():
    """The property test_pinhole_rays_hit_the_point_that_projects_to_the_pixels_centre pins for rays.pinhole_rays, for the
    rays the preview's field render uses: a point on the ray of pixel (i, j) projects to (i + 0.5, j + 0.5) by Part 15's
    projection, within the projection's own running bound plus the direction's rounding seen through the focal length."""
    import torch
    from mi3d import mesh
    c2w, K = M.orbit(2, 2.4, 0.3, 0.4), M.pinhole(FOCAL, H, W)
    o, d = mesh.camera_rays(c2w, K, H, W, torch.device("cpu"))
    assert tuple(o.shape) == (2, H * W, 3) and o.dtype == torch.float32
    rec = M.view_records(c2w, K)
    j, i = np.divmod(np.arange(H * W), W)
    for v in range(2):
        p = o[v].numpy().astype(np.float64) + 2.2 * d[v].numpy().astype(np.float64)
        x, y, z, Ex, Ey, _ = M.project(rec[v], p, np.float64, True)
        slack = 16 * M.U * FOCAL * max(H, W) * 2
        assert (abs(x - (i + 0.5)) <= 2 * Ex + slack).all() and (abs(y - (j + 0.5)) <= 2 * Ey + slack).all()
        assert (2 * Ex + slack).max() < 2e-3 and (z > 0).all()
