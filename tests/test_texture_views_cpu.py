"""CPU: the NumPy restatement of include/mi3d.h Part 15 (tests/texture_views_model.py) - the model the GPU tests compare
the kernels with bit for bit - checked here on its own: against a plain binary64 evaluation of the same definitions with
error bounds counted from the rounding chain, and for properties that need no second evaluation (watertight silhouettes,
order independence, exact quantisation of a constant image).  Then the argument checks of mesh.bake_views and
export_mesh(views=) that need no device."""
import numpy as np
import pytest

import texture_views_model as M
from test_mc_tables_cpu import marching_cubes_ref, sphere_volume
from test_texture_gpu import atlas_ref

F = np.float32
H, W = 96, 80
FOCAL = 1.2
MAX_UNDECIDED = 0.01     # the share of a case's samples that may lie within the margins: a condition of the test


def sphere_mesh(R=32, r0=0.6):
    h = F(2.0 / (R - 1))
    return marching_cubes_ref(sphere_volume(R, r0), 0.0, (-1, -1, -1), (h, h, h))


def torus_mesh(R=32):
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.22 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).astype(F)
    h = F(2.0 / (R - 1))
    return marching_cubes_ref(vol, 0.0, (-1, -1, -1), (h, h, h))


def quad_mesh():
    """Two triangles sharing the edge 1 - 2, facing +z."""
    v = np.array([[-0.5, -0.4, 0.1], [0.5, -0.4, 0.1], [-0.5, 0.4, 0.1], [0.5, 0.4, 0.1]], F)
    return v, np.array([[0, 1, 2], [2, 1, 3]], np.int32)


def smooth_images(V, H, W, seed=0):
    """float32 [V, H, W, 3] in [0, 1]: low-frequency waves, different per view and channel."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty((V, H, W, 3), F)
    for v in range(V):
        for ch in range(3):
            a, b, ph = rng.uniform(0.05, 0.3, 3)
            out[v, :, :, ch] = 0.5 + 0.45 * np.sin(a * i + b * j + 10 * ph)
    return out


def looking_away():
    """A camera beside the object that looks away from it: it sees nothing (and every vertex lies behind it)."""
    return M.look_at((2.4, 0.0, 0.0), target=(5.0, 0.0, 0.0))


def make_case(name):
    rng = np.random.default_rng(5)
    if name == "sphere":
        v, t = sphere_mesh()
        c2w = np.concatenate([M.orbit(4, 2.4, 0.3, 0.2), looking_away()[None]])
        T = 256
    elif name == "torus":
        v, t = torus_mesh()
        c2w = M.orbit(4, 2.6, 0.35, 0.5)         # low enough that the near side of the ring hides the far side's inside
        T = 256
    else:
        v, t = quad_mesh()
        c2w = np.stack([M.look_at((0.1, 0.05, 2.0), up=(0, 1, 0)), M.look_at((0.9, 0.3, 1.2), up=(0, 1, 0)),
                        M.look_at((0.0, 0.0, -2.0), up=(0, 1, 0))])     # the last one sees the back
        T = 64
    V = len(c2w)
    K = M.pinhole(FOCAL, H, W)
    images = smooth_images(V, H, W)
    masks = np.ones((V, H, W), np.uint8)
    masks[1, :, : W // 2] = 0
    weights = np.linspace(0.5, 2.0, V).astype(F)
    _, _, owner, xyz = atlas_ref(v, t, T, 1)
    keep = owner.ravel() >= 0
    xyz, own = xyz.reshape(-1, 3)[keep], owner.ravel()[keep]
    base = rng.random((len(xyz), 3)).astype(F)
    return dict(v=v, t=t, c2w=c2w, K=K, images=images, masks=masks, weights=weights, xyz=xyz, owner=own, base=base,
                rec=M.view_records(c2w, K))


@pytest.fixture(scope="module", params=["sphere", "torus", "quad"])
def evaluated(request):
    """One case evaluated once by the binary32 model and once in binary64 with the running bounds."""
    c = make_case(request.param)
    power, min_cos2, tol = 4, float(F(0.2) * F(0.2)), 0.02
    d32, counts = M.depth_maps(c["v"], c["t"], c["rec"], H, W)
    col32, hits32 = M.project_views(c["xyz"], c["owner"], c["v"], c["t"], c["rec"], H, W, d32, c["images"], c["masks"],
                                    c["weights"], power, min_cos2, tol, c["base"])
    d64, counts64, doubtful, err = M.depth_maps(c["v"], c["t"], c["rec"], H, W, np.float64, True)
    col64, hits64, undecided, Ecol = M.project_views(c["xyz"], c["owner"], c["v"], c["t"], c["rec"], H, W, d64,
                                                     c["images"], c["masks"], c["weights"], power, min_cos2, tol,
                                                     c["base"], np.float64, (doubtful, err))
    return dict(name=request.param, case=c, d32=d32, counts=counts, counts64=counts64, col32=col32, hits32=hits32,
                col64=col64, hits64=hits64, undecided=undecided, Ecol=Ecol)


def test_model_is_binary32_throughout(evaluated):
    assert evaluated["d32"].dtype == F and evaluated["col32"].dtype == F and evaluated["hits32"].dtype == np.uint8


def test_few_samples_lie_within_the_margins(evaluated):
    share = evaluated["undecided"].mean()
    print(f"[texture views] {evaluated['name']}: {len(evaluated['undecided'])} samples, undecided {share:.4%}, "
          f"hit {np.mean(evaluated['hits32'] > 0):.3f}")
    assert share <= MAX_UNDECIDED
    assert evaluated["counts"] == evaluated["counts64"]


def test_decided_samples_agree_on_hits_exactly(evaluated):
    ok = ~evaluated["undecided"]
    assert np.array_equal(evaluated["hits32"][ok], evaluated["hits64"][ok])
    assert (evaluated["hits32"] > 0).mean() > 0.3                # the case is not empty
    assert (evaluated["hits32"] == 0).any()                      # and something is hidden, masked or back-facing


def test_decided_samples_agree_on_colour_within_the_counted_bound(evaluated):
    ok = ~evaluated["undecided"]
    seen = ok & (evaluated["hits32"] > 0)
    diff = np.abs(evaluated["col32"].astype(np.float64) - evaluated["col64"]).max(1)
    print(f"[texture views] {evaluated['name']}: max colour difference {diff[seen].max():.3e}, "
          f"bound min {evaluated['Ecol'][seen].min():.3e} max {evaluated['Ecol'][seen].max():.3e}")
    assert (diff[seen] <= evaluated["Ecol"][seen]).all()
    assert evaluated["Ecol"][seen].max() < 1e-3                   # the bound itself says something
    unseen = ok & (evaluated["hits32"] == 0)
    assert np.array_equal(evaluated["col32"][unseen], evaluated["case"]["base"][unseen])


# ------------------------------------------------------------------------------------------------ the model alone

def ray_hits_sphere(c2w, K, H, W, r):
    """bool [H, W]: the ray through the pixel's centre passes within r of the origin (binary64)."""
    j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([i, j, np.ones_like(i)], -1) @ np.linalg.inv(K).T @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = c2w[:3, 3]
    along = -(d @ o)
    closest = o + along[..., None] * d
    return (along > 0) & (np.linalg.norm(closest, axis=-1) < r)


def erode(m):
    p = np.pad(m, 1, constant_values=False)
    out = np.ones_like(m)
    for dj in (0, 1, 2):
        for di in (0, 1, 2):
            out &= p[dj:dj + m.shape[0], di:di + m.shape[1]]
    return out


def test_no_hole_inside_the_silhouette():
    v, t = sphere_mesh()
    c2w, K = M.orbit(5, 2.4, 0.3, 0.1), M.pinhole(FOCAL, H, W)
    depth, counts = M.depth_maps(v, t, M.view_records(c2w, K), H, W)
    assert counts == (0, 0)
    for k in range(len(c2w)):
        inside = erode(ray_hits_sphere(c2w[k], K, H, W, 0.6))
        assert inside.sum() > 1500
        assert np.isfinite(depth[k][inside]).all()
        assert not np.isfinite(depth[k][~ray_hits_sphere(c2w[k], K, H, W, 0.6 + 2 * 2.4 / (FOCAL * W))]).any()


def test_depth_does_not_depend_on_the_order_of_the_triangles():
    v, t = torus_mesh()
    rec = M.view_records(M.orbit(3, 2.6, 0.35, 0.5), M.pinhole(FOCAL, H, W))
    a, _ = M.depth_maps(v, t, rec, H, W)
    b, _ = M.depth_maps(v, t[np.random.default_rng(1).permutation(len(t))], rec, H, W)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k", [0, 1, 100, 254])
def test_a_constant_image_quantises_exactly(k):
    c = make_case("sphere")
    images = np.full_like(c["images"], F((k + 0.5) / 255))
    depth, _ = M.depth_maps(c["v"], c["t"], c["rec"], H, W)
    for power in (2, 16):
        col, hits = M.project_views(c["xyz"], c["owner"], c["v"], c["t"], c["rec"], H, W, depth, images, None,
                                    c["weights"], power, 0.04, 0.02, c["base"])
        q = M.pack(col[:, None, None, :], np.zeros((len(col), 1), np.int32), 1)[:, 0]
        assert (hits > 0).sum() > 1000
        assert (q[hits > 0] == k).all()


def test_a_triangle_behind_the_camera_is_skipped_and_a_bad_index_counted():
    v, t = quad_mesh()
    t = np.concatenate([t, [[0, 1, 4]], [[-1, 0, 1]], [[1, 1, 2]]]).astype(np.int32)
    c2w = np.stack([M.look_at((0.0, 0.0, 2.0), up=(0, 1, 0)), M.look_at((0.0, 0.0, 0.3), target=(0, 0, 5), up=(0, 1, 0))])
    depth, (bad, skipped) = M.depth_maps(v, t, M.view_records(c2w, M.pinhole(FOCAL, H, W)), H, W)
    assert bad == 2 and skipped == 3                # the second camera has all three valid triangles behind it
    assert np.isfinite(depth[0]).any() and not np.isfinite(depth[1]).any()


# ------------------------------------------------------------------------------------------------ argument checks

def view_args(V=2, h=8, w=6):
    return dict(images=np.zeros((V, h, w, 3), F), c2w=M.orbit(V), K=M.pinhole(1.0, h, w))


@pytest.mark.parametrize("change,words", [
    (dict(images=np.zeros((2, 8, 6), F)), "(2, 8, 6)"),
    (dict(images=np.zeros((2, 8, 6, 4), F)), "(2, 8, 6, 4)"),
    (dict(images=np.zeros((2, 1, 6, 3), F)), "1 x 6"),
    (dict(images=np.zeros((2, 8, 6, 3), np.uint8)), "floating"),
    (dict(c2w=M.orbit(3)), "(3, 4, 4)"),
    (dict(K=np.eye(4)), "(4, 4)"),
    (dict(K=np.array([[1.0, 0, 0], [0, 1, 0], [0, 0.5, 1]])), "0 0 1"),
    (dict(masks=np.ones((2, 8, 5), np.uint8)), "(2, 8, 5)"),
    (dict(weights=np.ones(3, F)), "(3,)"),
    (dict(weights=np.array([1.0, -1.0])), "weights"),
    (dict(weights=np.array([1.0, np.nan])), "weights"),
    (dict(power=3), "power"),
    (dict(min_cos=1.5), "min_cos"),
    (dict(depth_tol=-0.1), "depth_tol"),
    (dict(depth_tol=float("nan")), "depth_tol"),
])
def test_bake_views_checks_its_view_arguments_before_the_mesh(change, words):
    from mi3d import mesh
    args = {**view_args(), **change}
    with pytest.raises(mesh.Mi3dError) as e:
        mesh.bake_views(None, None, None, 256, **args)           # no mesh, no device: the views are refused first
    assert words in str(e.value)


def test_more_than_64_views_are_refused():
    from mi3d import mesh
    with pytest.raises(mesh.Mi3dError, match="64"):
        mesh.bake_views(None, None, None, 256, np.zeros((65, 4, 4, 3), F), np.tile(np.eye(4), (65, 1, 1)),
                        M.pinhole(1.0, 4, 4))


def test_export_mesh_checks_views_before_any_work(tmp_path):
    from mi3d import mesh
    with pytest.raises(mesh.Mi3dError, match="texture_size"):
        mesh.export(None, str(tmp_path), views=view_args())
    with pytest.raises(mesh.Mi3dError, match="colour"):
        mesh.export(None, str(tmp_path), texture_size=256, views={**view_args(), "colour": 1})
    with pytest.raises(mesh.Mi3dError, match="missing keys \\['K'\\]"):
        mesh.export(None, str(tmp_path), texture_size=256, views={k: a for k, a in view_args().items() if k != "K"})
    with pytest.raises(mesh.Mi3dError, match="dict"):
        mesh.export(None, str(tmp_path), texture_size=256, views=[1])
    with pytest.raises(mesh.Mi3dError, match="\\(3, 4, 4\\)"):
        mesh.export(None, str(tmp_path), texture_size=256, views={**view_args(), "c2w": M.orbit(3)})
    assert not any(tmp_path.iterdir())


def test_view_records_are_the_models():
    from mi3d import mesh
    c2w, K = M.orbit(3, 2.4, 0.3, 0.2), M.pinhole(FOCAL, H, W)
    assert mesh.view_records(c2w, K).tobytes() == M.view_records(c2w, K).tobytes()
