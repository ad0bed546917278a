"""CPU: the yardstick of the hash grid's input gradient (tests/grid_grad_model.py) checked against itself and the oracle,
and `mesh.write_obj(normals=...)`."""
import numpy as np
import pytest
import torch

import grid_grad_model as M


@pytest.fixture(scope="module", params=list(M.CONFIGS))
def case(request):
    """(levels, points [257, 3], table, dout) of one configuration, made once."""
    levels = M.Levels(**M.CONFIGS[request.param])
    q = M.points01(levels, 257, seed=11)
    table = M.table_uniform(levels, seed=12)
    dout = torch.randn(q.shape[0], levels.n_levels * 2, generator=torch.Generator().manual_seed(13))
    return request.param, levels, q, table, dout


def test_hand_placed_points_pass_the_filter(case):
    """0 (fraction 1/2 at every level) always does; the generator puts the survivors first."""
    _, _, q, _, _ = case
    assert torch.equal(q[0], torch.zeros(3))


def test_gradient_is_the_central_difference_of_the_models_forward(case):
    """Inside a cell the interpolant is multilinear: a central difference in one coordinate is exact up to the binary64
    rounding of the two forwards, ~1e-16 |L| / h with h = 2^-12 / (finest scale) - 1e-9 of the gradient's own scale B
    leaves two orders of room."""
    name, levels, q32, table, dout = case
    g, B = M.grad_q(q32, dout, table, levels)
    h = 2.0 ** -12 / max(float(L["scale"]) for L in levels.level)     # s_l h <= 2^-12 < FACE: the step stays in the cell
    worst = 0.0
    for d in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[d] = h
        lp = (M.forward(q32, table, levels, dq=e.expand(q32.shape[0], 3)) * dout.double()).sum(-1)
        lm = (M.forward(q32, table, levels, dq=-e.expand(q32.shape[0], 3)) * dout.double()).sum(-1)
        err = ((lp - lm) / (2 * h) - g[:, d]).abs()
        worst = max(worst, float((err / B[:, d]).max()))
        assert bool((err <= 1e-9 * B[:, d]).all())
    print(f"[grid-grad] {name}: central difference vs model, worst error / B = {worst:.2e}")


def test_forward_is_the_oracles(case, oracle):
    """Same cells, same entries: the yardstick shares the pinned indexing.  The oracle sums 8 binary32 products of weights
    with 5 roundings in them: 16 x 2^-24 of max |v| = 1."""
    name, levels, q32, table, _ = case
    cfg = oracle.GridConfig(n_features_per_level=2, **{k: v for k, v in M.CONFIGS[name].items()})
    assert cfg.n_entries == levels.n_entries
    ref = oracle.hashgrid_forward(q32.numpy(), table.numpy(), cfg)
    got = M.forward(q32, table, levels).numpy()
    assert np.abs(got - ref).max() <= 16 * 2.0 ** -24


def test_mode1_map_and_clamp_rule():
    """point_q is point_of: the bounds map to 0 and 1, a point outside is clamped, and |base + off| == bound passes the
    inclusive rule but not the strict one."""
    levels = M.Levels(**M.CONFIGS["c1_L4"])
    x = torch.tensor([[1.5, -1.5, 0.0], [2.0, 0.25, -3.0]], dtype=torch.float32)
    q, t = M.point_q(x, torch.zeros(3), 1.5)
    assert q[0].tolist() == [1.0, 0.0, 0.5] and q[1, 0] == 1.0 and q[1, 2] == 0.0
    assert not M.pow2b(1.5) and M.pow2b(1.0) and M.pow2b(2.0)
    table = M.table_uniform(levels, seed=3)
    dout = torch.ones(2, 8)
    gi, _, Bi, _ = M.points_grad(x, None, np.zeros((1, 3), np.float32), 1, 1.5, dout, table, levels)
    gs, _, _, _ = M.points_grad(x, None, np.zeros((1, 3), np.float32), 1, 1.5, dout, table, levels, inclusive=False)
    assert bool((gi[0, :2] != 0).all()) and bool((gs[0, :2] == 0).all())         # on the bound
    assert gi[1, 0] == 0 and gi[1, 2] == 0 and gi[1, 1] != 0 and Bi[1, 0] == 0    # outside: nothing passes


# ------------------------------------------------------------------------------------------------ write_obj

def parse(path):
    out = {"v": [], "vt": [], "vn": [], "f": [], "order": []}
    for line in open(path):
        tok = line.split()
        if tok and tok[0] in out:
            out[tok[0]].append(tok[1:])
            if not out["order"] or out["order"][-1] != tok[0]:
                out["order"].append(tok[0])
    return out


@pytest.fixture()
def tiny_mesh():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (9, 3)).astype(np.int32)
    c = rng.random((7, 3)).astype(np.float32)
    n = rng.normal(size=(7, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    uv = rng.random((27, 2)).astype(np.float32)
    return v, f, c, n, uv, np.arange(27, dtype=np.int64).reshape(-1, 3)


def test_write_obj_normals_vertex_coloured(tiny_mesh, tmp_path):
    from mi3d import mesh
    v, f, c, n, _, _ = tiny_mesh
    obj, _ = mesh.write_obj(str(tmp_path), v, f, c, normals=n)
    p = parse(obj)
    assert p["order"] == ["v", "vn", "f"] and len(p["vn"]) == len(v)
    assert np.array_equal(np.array(p["vn"], np.float64).astype(np.float32), n)     # %.9g round-trips binary32
    idx = np.array([[t.split("//") for t in face] for face in p["f"]], np.int64)   # [nt, 3, 2]
    assert np.array_equal(idx[..., 0] - 1, f) and np.array_equal(idx[..., 1], idx[..., 0])


def test_write_obj_normals_textured(tiny_mesh, tmp_path):
    from mi3d import mesh
    v, f, c, n, uv, uvf = tiny_mesh
    obj, mtl = mesh.write_obj(str(tmp_path), v, f, c, uvs=uv, uv_faces=uvf, texture="albedo.png", normals=n)
    p = parse(obj)
    assert p["order"] == ["v", "vt", "vn", "f"] and len(p["vn"]) == len(v) and len(p["vt"]) == len(uv)
    idx = np.array([[t.split("/") for t in face] for face in p["f"]], np.int64)    # [nt, 3, 3]: a/ta/a
    assert np.array_equal(idx[..., 0] - 1, f) and np.array_equal(idx[..., 1] - 1, uvf)
    assert np.array_equal(idx[..., 2], idx[..., 0])
    assert open(mtl).read().endswith("map_Kd albedo.png\n")


def test_write_obj_without_normals_is_unchanged(tiny_mesh, tmp_path):
    from mi3d import mesh
    v, f, c, _, uv, uvf = tiny_mesh
    for kw in ({}, dict(uvs=uv, uv_faces=uvf, texture="albedo.png")):
        a = mesh.write_obj(str(tmp_path / "a"), v, f, c, **kw)
        b = mesh.write_obj(str(tmp_path / "b"), v, f, c, normals=None, **kw)
        for x, y in zip(a, b):
            assert open(x, "rb").read() == open(y, "rb").read()
        assert b"vn " not in open(a[0], "rb").read() and b"//" not in open(a[0], "rb").read()


@pytest.mark.parametrize("shape", [(6, 3), (7, 2), (21,)])
def test_write_obj_refuses_normals_of_the_wrong_shape(tiny_mesh, tmp_path, shape):
    from mi3d import mesh
    v, f, c, _, _, _ = tiny_mesh
    with pytest.raises(ValueError, match="normals"):
        mesh.write_obj(str(tmp_path), v, f, c, normals=np.zeros(shape, np.float32))
    assert not (tmp_path / "mesh.obj").exists()
