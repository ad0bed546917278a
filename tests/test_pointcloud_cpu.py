"""CPU: the point-cloud module's argument validation, its file writer and the Part 11 ABI (no kernel runs here)."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

PART11 = ("mi3d_pc_unproject_workspace", "mi3d_pc_unproject", "mi3d_pc_project", "mi3d_pc_zmin", "mi3d_pc_visible",
          "mi3d_box_morph", "mi3d_pc_cano_filter", "mi3d_pc_colour")


def test_part11_is_declared_bound_and_exported():
    from mi3d import _lib
    hdr = open(os.path.join(ROOT, "include", "mi3d.h")).read()
    part = hdr[hdr.index("Part 11"):]
    code = re.sub(r"/\*.*?\*/", "", part, flags=re.S)
    assert sorted(set(re.findall(r"\b(mi3d_[A-Za-z0-9_]+)\s*\(", code))) == sorted(PART11)
    assert "PARITY UNPINNED" in part                   # the erosion's border rule says what it is
    lib = _lib.lib()
    for name in PART11:
        assert hasattr(lib, name)
        assert (name in _lib._SIGNATURES) != (name in _lib._LATE_SIGNATURES), name
    assert "mi3d_pc_unproject_workspace" in _lib._LATE_SIGNATURES
    assert lib.mi3d_abi_version() == 5


def test_unproject_workspace_is_a_host_query():
    from mi3d import _lib
    ws = _lib.lib().mi3d_pc_unproject_workspace
    assert ws(70, 67) == 80 and ws(1, 1) == 8          # 19 workgroup sums of 4 bytes, rounded up to 8
    assert ws(0, 5) == 0 and ws(5, 16385) == 0
    assert ws(16384, 16384) == 4 * 2 ** 20


def test_pointcloud_unit_is_built_without_contraction():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mi3d_build", os.path.join(ROOT, "make-it-3d_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("pointcloud.hip", ["-ffp-contract=off"]) in b.UNITS


def test_a_cpu_device_is_refused():
    import torch
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    v, K = np.zeros((4, 3)), np.eye(3)
    with pytest.raises(Mi3dError, match="no CPU path"):
        pc.z_buffer(v, np.eye(4), 8, 8, K, device="cpu")
    with pytest.raises(Mi3dError, match="no CPU path"):
        pc.project(torch.zeros(4, 3), K, np.eye(4)[:3], device=torch.device("cpu"))
    with pytest.raises(Mi3dError, match="no CPU path"):
        pc.erode(np.ones((8, 8), np.float32), 3, device="cpu")
    with pytest.raises(Mi3dError, match="no CPU path"):
        pc.depth2point(np.ones((8, 8)), np.ones((8, 8)), np.eye(4), np.zeros((8, 8, 3)), 8, 8, K, device="cpu")


def test_a_cpu_model_is_refused():
    import types
    import torch
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    model = types.SimpleNamespace(aabb_train=torch.zeros(6))
    with pytest.raises(Mi3dError, match="on the GPU"):
        pc.from_model(model, np.eye(4)[None].repeat(3, 0), 20.0, 8, 8)


@pytest.mark.parametrize("box", [4, (3, 2), 33, 0, (5, 35)])
def test_an_even_or_oversized_box_is_refused(box):
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    with pytest.raises(Mi3dError, match="odd sides"):
        pc.erode(np.ones((8, 8), np.float32), box, device="cuda")
    with pytest.raises(Mi3dError, match="odd sides"):
        pc.dilate(np.ones((8, 8), np.float32), box, device="cuda")


def test_morphology_takes_one_channel_and_a_positive_count():
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    with pytest.raises(Mi3dError, match="single-channel"):
        pc.erode(np.ones((8, 8, 3), np.float32), 3, device="cuda")
    with pytest.raises(Mi3dError, match="iterations"):
        pc.erode(np.ones((8, 8), np.float32), 3, iterations=0, device="cuda")


def test_the_canonical_filter_route_needs_a_square_image():
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    H, W = 8, 12
    with pytest.raises(Mi3dError, match="H == W"):
        pc.multidepth2point_mask(np.ones((1, H, W)), np.ones((1, H, W)), np.zeros((1, H, W, 3)), np.eye(3), np.eye(4)[None],
                                 np.zeros((4, 3)), np.eye(4), np.ones((H, W)), H, W, 2, 8, device="cuda")
    with pytest.raises(Mi3dError, match="H == W"):
        pc.cano_filter(np.zeros((4, 3)), np.eye(3), np.eye(4), np.ones((H, W)), H, W, device="cuda")


def test_another_image_size_is_refused_before_any_launch():
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    H = W = 8
    good = dict(ref_rgb=np.zeros((H, W, 3)), rgbs=np.zeros((3, H, W, 3)), depths=np.ones((3, H, W)),
                masks=np.ones((3, H, W)), c2ws=np.eye(4)[None].repeat(3, 0), K=np.eye(3), H=H, W=W, device="cuda")
    for key, bad in (("depths", np.ones((3, H, W + 1))), ("masks", np.ones((3, H + 2, W))),
                     ("rgbs", np.zeros((3, 2 * H, 2 * W, 3)))):
        with pytest.raises(Mi3dError, match="resizing is not restated"):
            pc.build(**{**good, key: bad})
    with pytest.raises(Mi3dError, match="c2ws"):
        pc.build(**{**good, "c2ws": np.eye(4)[None].repeat(2, 0)})
    with pytest.raises(Mi3dError, match="at least one novel view"):
        pc.build(**{**good, "rgbs": good["rgbs"][:1], "depths": good["depths"][:1], "masks": good["masks"][:1],
                    "c2ws": good["c2ws"][:1]})
    with pytest.raises(Mi3dError, match="resizing is not restated"):
        pc.depth2point(np.ones((H, W)), np.ones((H, W)), np.eye(4), np.zeros((H, W + 1, 3)), H, W, np.eye(3), device="cuda")
    with pytest.raises(Mi3dError, match=r"\[n, 3\]"):
        pc.z_buffer(np.zeros((4, 2)), np.eye(4), H, W, np.eye(3), device="cuda")


def test_save_writes_the_reference_s_names_and_dtypes(tmp_path):
    import torch
    from mi3d import pointcloud as pc
    from mi3d._lib import Mi3dError
    rng = np.random.default_rng(0)
    arrays = (rng.random((5, 3)), torch.rand(5, 3, dtype=torch.float64), torch.rand(7, 3), rng.random((7, 3)))
    out = tmp_path / "a" / "refine"                    # created
    paths = pc.save(str(out), *arrays)
    names = ["vertices_cano.npy", "vertices_color_cano.npy", "vertices_novel.npy", "vertices_color_novel.npy"]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out)) == sorted(names)
    for name, a, dtype in zip(names, arrays, (np.float64, np.float32, np.float64, np.float32)):
        f = np.load(out / name)
        assert f.dtype == dtype and f.shape == tuple(a.shape)
        assert np.array_equal(f, np.asarray(a).astype(dtype))
    with pytest.raises(Mi3dError, match="same number of rows"):
        pc.save(str(tmp_path / "b"), arrays[0], arrays[2], arrays[2], arrays[3])
    assert not os.path.exists(tmp_path / "b" / names[0])
    with pytest.raises(Mi3dError, match=r"\[n, 3\]"):
        pc.save(str(tmp_path / "c"), np.zeros((5, 2)), arrays[1], arrays[2], arrays[3])


def test_intrinsics_are_the_trainer_s():
    from mi3d import pointcloud as pc
    K = pc.intrinsics(20.0, 800, 800)
    focal = 1 / (2 * np.tan(np.deg2rad(20.0) / 2))
    assert np.array_equal(K, np.array([[focal * 800, 0, 400.0], [0, focal * 800, 400.0], [0, 0, 1]]))


def test_the_fixture_holds_what_the_tests_read():
    g = np.load(os.path.join(GOLDEN, "pointcloud.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "pointcloud.npz")) < 512 * 1024
    assert tuple(g["a_hw"]) == (48, 64) and int(g["a_n"]) == 20000 and tuple(g["b_hw"]) == (64, 64)
    assert float(g["a_tie_margin"]) >= 1e-9 and float(g["a_depth_margin"]) >= 1e-9
    assert g["a_mask"].shape == (2500,) and g["b_points"].dtype == np.float64 and g["b_colours"].dtype == np.float32
    assert g["b_points"].shape == g["b_colours"].shape and int(np.unpackbits(g["b_mask"]).sum()) >= len(g["b_points"])
