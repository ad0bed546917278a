"""CPU: the host side of mesh export - export_mesh refuses a CPU model (there is no eager path for the kernels), and the
OBJ / MTL writer produces files a plain parser reads back."""
import os

import numpy as np
import pytest


def parse_obj(path):
    """The ten-line OBJ reader of these tests: (mtllib, vertices [nv,3], colours [nv,3], faces [nt,3] one-based, usemtl)."""
    mtllib = usemtl = None
    v, f = [], []
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "v":
            v.append([float(x) for x in tok[1:7]])
        elif tok[0] == "f":
            f.append([int(x.split("/")[0]) for x in tok[1:4]])
        elif tok[0] == "mtllib":
            mtllib = tok[1]
        elif tok[0] == "usemtl":
            usemtl = tok[1]
    v = np.array(v, np.float64).reshape(-1, 6)
    return mtllib, v[:, :3], v[:, 3:], np.array(f, np.int64).reshape(-1, 3), usemtl


def test_export_mesh_on_a_cpu_model_raises_mi3d_error(tmp_path):
    import torch
    from mi3d import _lib, network, sds_step
    torch.manual_seed(0)
    model = network.NeRFNetwork(sds_step.make_opt(fp16=False))
    with pytest.raises(_lib.Mi3dError, match="GPU"):
        model.export_mesh(str(tmp_path / "mesh"), resolution=8)
    assert not os.path.exists(tmp_path / "mesh" / "mesh.obj")


def test_marching_cubes_refuses_a_cpu_tensor():
    import torch
    from mi3d import _lib, mesh
    with pytest.raises(_lib.Mi3dError):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)


def test_obj_writer_round_trip(tmp_path):
    from mi3d import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.1, 0.2, 1 / 3]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    c = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.25, 0.5, 0.123456]], np.float32)
    out = tmp_path / "new" / "dir"                      # created if missing
    obj, mtl = mesh.write_obj(str(out), v, f, c)
    assert obj == str(out / "mesh.obj") and mtl == str(out / "mesh.mtl")
    mtllib, pv, pc, pf, usemtl = parse_obj(obj)
    assert mtllib == "mesh.mtl" and usemtl == "mat0"
    assert np.array_equal(pv.astype(np.float32), v)     # %.9g round-trips binary32
    np.testing.assert_allclose(pc, c, atol=5e-7)
    assert np.array_equal(pf, f.astype(np.int64) + 1)
    lines = open(obj).read().splitlines()
    assert lines[0] == "mtllib mesh.mtl" and lines[1].startswith("v ") and lines[5] == "usemtl mat0"
    assert len(lines) == 1 + 4 + 1 + 4
    text = open(mtl).read()
    assert text.startswith("newmtl mat0") and "Kd 1.000000 1.000000 1.000000" in text
    assert "map_" not in text and ".png" not in text    # no texture


def test_obj_writer_rejects_mismatched_arrays(tmp_path):
    from mi3d import mesh
    with pytest.raises(ValueError):
        mesh.write_obj(str(tmp_path), np.zeros((4, 3)), np.zeros((2, 3), np.int32), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        mesh.write_obj(str(tmp_path), np.zeros((4, 3)), np.zeros((2, 4), np.int32), np.zeros((4, 3)))
