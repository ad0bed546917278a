"""CPU: the host side of texture baking - the PNG writer against a standard-library decoder (and PIL where it imports),
the OBJ / MTL writer with UVs against a plain parser, the atlas cell size of include/mi3d.h Part 9 through the library
against its defining formula, and the refusal of a CPU model."""
import os
import struct
import zlib

import numpy as np
import pytest


def decode_png(path):
    """The twenty-line PNG reader of these tests: 8-bit RGB, non-interlaced, all five filter types -> uint8 [H, W, 3]."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head, tags = 8, b"", None, []
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body), tag
        tags.append(tag)
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert tags[0] == b"IHDR" and tags[-1] == b"IEND" and pos == len(data)
    W, H, depth, colour, comp, filt, lace = head
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    out = np.zeros((H, 3 * W), np.int64)
    for y in range(H):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(3 * W, np.int64)
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = (line + up) % 256
        else:  # 1 (sub), 3 (average), 4 (Paeth): sequential along the row
            for x in range(3 * W):
                a, b, c = (out[y, x - 3], up[x], up[x - 3]) if x >= 3 else (0, up[x], 0)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                out[y, x] = (line[x] + pred) % 256
    return out.astype(np.uint8).reshape(H, W, 3)


def parse_textured_obj(path):
    """(mtllib, v [nv,3], extra columns of the v lines, vt [nuv,2], faces [nt,3] and uv faces [nt,3] one-based, usemtl)."""
    mtllib = usemtl = None
    v, vt, f, ft, extra = [], [], [], [], 0
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "v":
            v.append([float(x) for x in tok[1:4]])
            extra = max(extra, len(tok) - 4)
        elif tok[0] == "vt":
            assert len(tok) == 3
            vt.append([float(x) for x in tok[1:3]])
        elif tok[0] == "f":
            pairs = [x.split("/") for x in tok[1:4]]
            assert len(tok) == 4 and all(len(p) == 2 for p in pairs), line
            f.append([int(p[0]) for p in pairs])
            ft.append([int(p[1]) for p in pairs])
        elif tok[0] == "mtllib":
            mtllib = tok[1]
        elif tok[0] == "usemtl":
            usemtl = tok[1]
    return (mtllib, np.array(v, np.float64).reshape(-1, 3), extra, np.array(vt, np.float64).reshape(-1, 2),
            np.array(f, np.int64).reshape(-1, 3), np.array(ft, np.int64).reshape(-1, 3), usemtl)


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (64, 64), (33, 301)])
def test_png_round_trip(tmp_path, shape):
    from mi3d import mesh
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[0, 0] = (255, 0, 128)
    path = str(tmp_path / "albedo.png")
    assert mesh.write_png(path, img) == path
    got = decode_png(path)
    assert got.shape == img.shape and np.array_equal(got, img)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), img)


def test_png_writer_emits_several_idat_chunks_for_a_large_image(tmp_path):
    from mi3d import mesh
    img = np.random.default_rng(3).integers(0, 256, (3000, 2100, 3), dtype=np.uint8)      # 18.9 MB of rows: two blocks
    path = str(tmp_path / "big.png")
    mesh.write_png(path, img)
    assert open(path, "rb").read().count(b"IDAT") >= 2
    assert np.array_equal(decode_png(path), img)


def test_png_writer_rejects_what_is_not_8_bit_rgb(tmp_path):
    from mi3d import mesh
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8),
                np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            mesh.write_png(str(tmp_path / "bad.png"), bad)
    assert not os.path.exists(tmp_path / "bad.png")


def test_obj_writer_with_uvs(tmp_path):
    from mi3d import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.1, 0.2, 1 / 3]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    c = np.full((4, 3), 0.5, np.float32)
    uv = np.random.default_rng(0).random((12, 2)).astype(np.float32)
    uv[0] = (np.float32(1 / 3), np.float32(0.1))
    ft = np.arange(12).reshape(4, 3)
    obj, mtl = mesh.write_obj(str(tmp_path / "t"), v, f, c, uvs=uv, uv_faces=ft, texture="albedo.png")
    mtllib, pv, extra, pvt, pf, pft, usemtl = parse_textured_obj(obj)
    assert mtllib == "mesh.mtl" and usemtl == "mat0"
    assert extra == 0                                                   # plain `v x y z`: no colour columns
    assert np.array_equal(pv.astype(np.float32), v) and np.array_equal(pvt.astype(np.float32), uv)   # %.9g round-trips
    assert np.array_equal(pf, f.astype(np.int64) + 1) and np.array_equal(pft, ft + 1)
    lines = open(obj).read().splitlines()
    assert lines[0] == "mtllib mesh.mtl" and lines[1 + 4 + 12] == "usemtl mat0" and len(lines) == 1 + 4 + 12 + 1 + 4
    assert [l.split()[0] for l in lines[1:17]] == ["v"] * 4 + ["vt"] * 12
    assert lines[-1] == "f 3/10 1/11 4/12"
    text = open(mtl).read()
    assert text.startswith("newmtl mat0") and text.rstrip().endswith("map_Kd albedo.png")
    assert text.count("map_Kd") == 1


def test_obj_writer_wants_all_three_texture_arguments(tmp_path):
    from mi3d import mesh
    v, f, c = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), np.zeros((3, 3), np.float32)
    uv, ft = np.zeros((3, 2), np.float32), np.array([[0, 1, 2]])
    for kw in ({"uvs": uv}, {"uvs": uv, "uv_faces": ft}, {"texture": "albedo.png"},
               {"uvs": uv, "uv_faces": np.zeros((2, 3), np.int64), "texture": "a.png"},
               {"uvs": np.zeros((3, 3), np.float32), "uv_faces": ft, "texture": "a.png"}):
        with pytest.raises(ValueError):
            mesh.write_obj(str(tmp_path / "x"), v, f, c, **kw)
    assert not os.path.exists(tmp_path / "x" / "mesh.obj")


def capacity(T, c):
    return 2 * (T // (c + 1)) * (T // c)


def cell_by_the_formula(nt, T):
    """The largest c >= 4 with 2 * (T // (c + 1)) * (T // c) >= nt, by exhaustive search; 0 if there is none."""
    best = 0
    for c in range(4, T):
        if capacity(T, c) >= nt:
            best = c
    return best


def test_atlas_cell_against_the_formula():
    from mi3d import mesh
    sizes = [64, 65, 100, 127, 256, 1000, 2048, 4096, 8192, 16384]
    for T in sizes:
        caps = sorted({capacity(T, c) for c in range(4, min(T, 200))})
        nts = {1, 2, 3, 7, 100, 99_999, 100_000, 300_000, 1_000_000, capacity(T, 4), capacity(T, 4) + 1}
        for cap in caps[:40] + caps[-40:]:
            nts |= {cap - 1, cap, cap + 1}
        for nt in sorted(n for n in nts if n >= 1):
            c = mesh.atlas_cell(nt, T)
            assert c == cell_by_the_formula(nt, T), (nt, T, c)
            if c == 0:
                assert capacity(T, 4) < nt
            else:
                assert c >= 4 and capacity(T, c) >= nt                  # it holds them
                assert c + 1 > T - 1 or capacity(T, c + 1) < nt         # and no larger cell does
    # the table of the issue
    table = {(100_000, 2048): 8, (100_000, 4096): 17, (100_000, 8192): 36, (300_000, 2048): 4, (300_000, 4096): 10,
             (300_000, 8192): 20, (1_000_000, 2048): 0, (1_000_000, 4096): 5, (1_000_000, 8192): 11}
    for (nt, T), c in table.items():
        assert mesh.atlas_cell(nt, T) == c, (nt, T)
    assert capacity(16384, 4) == 26_836_992 and mesh.atlas_cell(31_600_000, 16384) == 0
    for T in (0, 1, 63, 16385, 1 << 20):                                # texture sizes out of range fit nothing
        assert mesh.atlas_cell(10, T) == 0


def test_capacity_is_non_increasing_in_c():
    for T in (64, 100, 2048, 4097, 16384):
        caps = [capacity(T, c) for c in range(4, T)]
        assert all(a >= b for a, b in zip(caps, caps[1:]))


def test_textured_export_on_a_cpu_model_raises_mi3d_error(tmp_path):
    import torch
    from mi3d import _lib, network, sds_step
    torch.manual_seed(0)
    model = network.NeRFNetwork(sds_step.make_opt(fp16=False))
    with pytest.raises(_lib.Mi3dError, match="GPU"):
        model.export_mesh(str(tmp_path / "mesh"), resolution=8, texture_size=64)
    assert not os.path.exists(tmp_path / "mesh")


def test_bake_texture_refuses_cpu_tensors_and_bad_sizes():
    import torch
    from mi3d import _lib, mesh
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(_lib.Mi3dError):
        mesh.bake_texture(None, v, t, 64)
    for size, ssaa in ((63, 1), (16385, 1), (64.5, 1), (64, 3), (64, 0), (64, 8)):
        with pytest.raises(_lib.Mi3dError):
            mesh.bake_texture(None, v, t, size, ssaa)
