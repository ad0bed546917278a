"""GPU: the area-adaptive atlas (csrc/atlasadaptive.hip through mi3d.mesh, include/mi3d.h Part 20).  Every kernel output
against the NumPy float32 restatement of tests/atlas_adaptive_model.py, bit for bit; the no-bleed property on the
kernels' output alone; the baked image against the field at the kernels' positions; a texture that is sharper where the
triangles are large; export_mesh through the files; and the uniform atlas untouched.

The sharpness test prints its two RMS errors and writes them to atlas_adaptive.json BEFORE it asserts - in the directory
MI3D_REPORT_DIR names, or in test_reports/ at the root of the repository (git-ignored); the kept copy is the `sharpness`
entry of profiles/atlas_adaptive.json."""
import json
import os

import numpy as np
import pytest

import atlas_adaptive_model as M
from test_mesh_gpu import vol_a
from test_texture_cpu import decode_png, parse_textured_obj
from test_texture_gpu import albedo_at, model, quantise  # noqa: F401  (model: the fixture, a random-weight field)

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_PATH = os.path.join(os.environ.get("MI3D_REPORT_DIR") or os.path.join(ROOT, "test_reports"), "atlas_adaptive.json")
SIZES = (256, 512, 777)          # 777: right and bottom margins, a band tail
BAND = 37                        # bands start inside cells


# ------------------------------------------------------------------------------------------------ the kernels

def run_adaptive(cuda, vertices, triangles, T, ssaa, band=BAND, plan_words=None):
    """measure -> the library's host plan -> sort -> uv -> positions over the whole image in bands of `band` rows, every
    output as a NumPy array; None under "words" (and nothing after the measure) when the mesh does not fit."""
    import torch
    from mi3d import _lib, mesh
    v = torch.from_numpy(np.ascontiguousarray(vertices, F)).to(cuda)
    t = torch.from_numpy(np.ascontiguousarray(triangles, np.int32)).to(cuda)
    nv, nt, ss2, p = len(vertices), len(triangles), ssaa * ssaa, _lib.ptr
    shape = torch.full((nt,), -7, dtype=torch.int32, device=cuda)
    hist = torch.zeros(4096, dtype=torch.int32, device=cuda)
    bad = torch.zeros(1, dtype=torch.int64, device=cuda)
    _lib.launch("mi3d_atlas_adaptive_measure", v, p(v), nv, p(t), nt, p(shape), p(hist), p(bad))
    out = dict(shape=shape.cpu().numpy().view(np.uint32), hist=hist.cpu().numpy().view(np.uint32).reshape(64, 64),
               bad=int(bad))
    words = mesh.atlas_adaptive_plan(out["hist"], T) if plan_words is None else plan_words
    out["words"] = words
    if words is None:
        return out
    plan = torch.from_numpy(words).to(cuda)
    ws_bytes = int(_lib.lib().mi3d_atlas_adaptive_workspace(nt))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=cuda)
    slot = torch.full((nt,), -7, dtype=torch.int32, device=cuda)
    triangle_of = torch.full((nt,), -7, dtype=torch.int32, device=cuda)
    vt = torch.full((3 * nt, 2), -7.0, device=cuda)
    owner = torch.full((T, T), -7, dtype=torch.int32, device=cuda)
    xyz = torch.full((T, T, ss2, 3), -7.0, device=cuda)
    _lib.launch("mi3d_atlas_adaptive_sort", v, p(shape), nt, p(plan), p(ws), ws_bytes, p(slot), p(triangle_of))
    _lib.launch("mi3d_atlas_adaptive_uv", v, p(shape), p(slot), nt, p(plan), T, p(vt))
    for row0 in range(0, T, band):
        rows = min(band, T - row0)
        _lib.launch("mi3d_atlas_adaptive_positions", v, p(v), nv, p(t), nt, p(shape), p(triangle_of), p(plan), T, ssaa,
                    row0, rows, p(xyz[row0]), p(owner[row0]))
    out.update(slot=slot.cpu().numpy().view(np.uint32), triangle_of=triangle_of.cpu().numpy().view(np.uint32),
               vt=vt.cpu().numpy(), owner=owner.cpu().numpy(), xyz=xyz.cpu().numpy())
    return out


@pytest.fixture(scope="module")
def meshes(cuda):
    """name -> (vertices, triangles): the graded plane, the latitude-longitude sphere, the marching-cubes sphere of
    test_mesh_gpu.py and that sphere after mesh.collapse to one eighth of its faces."""
    import torch
    from mi3d import mesh
    out = {"plane": M.graded_plane(), "latlong": M.latlong_sphere()}
    vol, iso, frame = vol_a()
    v, t = mesh.marching_cubes(torch.from_numpy(vol).to(cuda), iso, origin=frame[0], spacing=frame[1])
    out["mc_sphere"] = (v.cpu().numpy(), t.cpu().numpy())
    cv, ct, _ = mesh.collapse(v, t, t.shape[0] // 8)
    out["collapsed"] = (cv.cpu().numpy(), ct.cpu().numpy())
    for name, (v, t) in out.items():
        print(f"[atlas-adaptive] {name}: nv {len(v)} nt {len(t)}")
    return out


def variant(v, t, kind):
    v, t = v.copy(), t.copy()
    if kind == "drop":                       # odd class counts
        t = t[:-1]
    elif kind == "dup":                      # a zero-length edge in every triangle at the vertex
        v[t[0, 1]] = v[t[0, 0]]
    elif kind == "nan":
        v[t[3, 2], 1] = np.nan
    elif kind == "one":
        t = t[:1]
    else:
        assert kind == "plain"
    return v, t


_MODEL = {}


def model_layout(meshes, name, kind, T, ssaa):
    """The restatement of a case, computed once."""
    key = (name, kind, T, ssaa)
    if key not in _MODEL:
        _MODEL[key] = M.layout(*variant(*meshes[name], kind), T, ssaa)
    return _MODEL[key]


CASES = ([(name, "plain", T, ssaa) for name in ("plane", "latlong", "mc_sphere", "collapsed") for T in SIZES
          for ssaa in (1, 2)] +
         [("plane", "drop", 256, 1), ("plane", "dup", 512, 2), ("plane", "nan", 777, 1), ("plane", "one", 256, 2),
          ("collapsed", "drop", 777, 2), ("collapsed", "dup", 256, 1), ("collapsed", "nan", 512, 2),
          ("latlong", "one", 512, 1)])


# ------------------------------------------------------------------------------------------------ bit for bit

@pytest.mark.parametrize("name,kind,T,ssaa", CASES)
def test_every_output_against_the_restatement_bitwise(cuda, meshes, name, kind, T, ssaa):
    v, t = variant(*meshes[name], kind)
    want = model_layout(meshes, name, kind, T, ssaa)
    got = run_adaptive(cuda, v, t, T, ssaa)
    shape, hist, bad = M.measure(v, t)
    assert got["bad"] == bad == 0
    assert np.array_equal(got["shape"], shape) and np.array_equal(got["hist"], hist)
    if want is None:                         # the mesh does not fit: the library's plan says so too
        print(f"[atlas-adaptive] {name} {kind} nt {len(t)} T {T}: does not fit")
        assert got["words"] is None and name == "mc_sphere" and T == 256
        return
    p = want["plan"]
    print(f"[atlas-adaptive] {name} {kind} nt {len(t)} T {T} ssaa {ssaa}: shift {p['shift']}, rows {p['rows']}, "
          f"{len(p['records'])} classes in {len(p['groups'])} height groups, owned texels {p['owned']}, clamped legs "
          f"{p['clamped_small']} + {p['clamped_large']}")
    assert np.array_equal(got["words"], p["words"])
    assert np.array_equal(got["slot"], want["slot"]) and np.array_equal(got["triangle_of"], want["triangle_of"])
    assert got["vt"].tobytes() == want["vt"].tobytes()
    assert np.array_equal(got["owner"], want["owner"])
    assert got["xyz"].shape == want["xyz"].shape and got["xyz"].tobytes() == want["xyz"].tobytes()
    assert (want["owner"] >= 0).sum() == p["owned"]
    if kind == "dup":
        assert ((((shape >> 8) & 63) == 0) | (((shape >> 16) & 63) == 0)).any()               # the zero-length edge: bin 0
    if kind == "nan":
        assert not np.isnan(got["xyz"]).any() and ((((shape >> 8) & 63) == 0) | (((shape >> 16) & 63) == 0)).any()


def test_the_cases_cover_every_mesh_size_and_variant():
    assert {c[0] for c in CASES} == {"plane", "latlong", "mc_sphere", "collapsed"}
    assert {(c[0], c[2]) for c in CASES} == {(n, T) for n in ("plane", "latlong", "mc_sphere", "collapsed") for T in SIZES}
    assert {c[1] for c in CASES} == {"plain", "drop", "dup", "nan", "one"} and {c[3] for c in CASES} == {1, 2}


def test_two_runs_give_the_same_bytes(cuda, meshes):
    v, t = meshes["collapsed"]
    a, b = run_adaptive(cuda, v, t, 512, 2), run_adaptive(cuda, v, t, 512, 2, band=64)
    for key in ("shape", "hist", "words", "slot", "triangle_of", "vt", "owner", "xyz"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_atlas_plan_reports_what_the_plan_holds(cuda, meshes):
    import torch
    from mi3d import _lib, mesh
    for name, T in (("latlong", 256), ("collapsed", 512)):
        v, t = meshes[name]
        d = mesh.atlas_plan(torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), T)
        p = model_layout(meshes, name, "plain", T, 1)["plan"]
        assert (d["shift"], d["rows"], d["kmax"], d["texture_size"]) == (p["shift"], p["rows"], p["kmax"], T)
        assert d["fill"] == p["owned"] / (T * T) and np.array_equal(d["classes"], p["classes"])
        assert (d["clamped_small"], d["clamped_large"]) == (p["clamped_small"], p["clamped_large"])
        assert d["classes"].shape == (16, 16) and d["classes"].sum() == len(t)
    v, t = meshes["mc_sphere"]
    with pytest.raises(_lib.Mi3dError, match="512"):
        mesh.atlas_plan(torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), 256)


# ------------------------------------------------------------------------------------------------ no bleed

@pytest.mark.parametrize("name,T", [("plane", 256), ("latlong", 777), ("collapsed", 512)])
def test_no_bleed_from_the_kernels_alone(cuda, meshes, name, T):
    """The method of test_texture_gpu.py: for every triangle, at its corners, edge midpoints and 64 random interior
    points, each texel that bilinear filtering reads with a weight above 1e-9 is owned by that triangle - from vt and
    owner of the kernels only.  And every triangle owns exactly the texel count its class predicts."""
    v, t = meshes[name]
    nt = len(t)
    out = run_adaptive(cuda, v, t, T, 1)
    vt, owner, words = out["vt"], out["owner"], out["words"]
    assert out["bad"] == 0 and (vt > 0).all() and (vt < 1).all()
    keys = M.keys_of(out["shape"], int(words[0]), int(words[2]))
    legs = np.array(M.LEGS)
    predicted = np.array([M.half0_mask(a, b).sum() for a, b in zip(legs[keys % 16], legs[keys // 16])])
    counts = np.bincount(owner[owner >= 0], minlength=nt)
    assert counts.shape == (nt,) and np.array_equal(counts, predicted)
    assert owner.min() == -1 and owner.max() == nt - 1 and (owner >= 0).sum() == words[7]

    px = np.stack([vt[:, 0].astype(np.float64) * T - 0.5, (1.0 - vt[:, 1].astype(np.float64)) * T - 0.5], -1)
    corner = np.rint(px)
    snap = np.abs(px - corner).max()
    print(f"[atlas-adaptive] {name} T {T}: vt denote texel centres within {snap:.3e} texels (T * 2^-23 = {T * 2.0 ** -23:.3e})")
    assert snap <= T * 2.0 ** -23
    corner = corner.reshape(nt, 3, 2)
    rng = np.random.default_rng(T)
    w = rng.dirichlet(np.ones(3), size=(nt, 64))
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]], np.float64)
    w = np.concatenate([np.broadcast_to(fixed, (nt, 6, 3)), w], 1)
    pts = np.einsum("nkb,nbd->nkd", w, corner)
    base = np.floor(pts)
    frac = pts - base
    checked = 0
    for dx in (0, 1):
        for dy in (0, 1):
            weight = np.where(dx, frac[..., 0], 1 - frac[..., 0]) * np.where(dy, frac[..., 1], 1 - frac[..., 1])
            X, Y = base[..., 0].astype(np.int64) + dx, base[..., 1].astype(np.int64) + dy
            used = weight > 1e-9
            assert (X[used] >= 0).all() and (X[used] < T).all() and (Y[used] >= 0).all() and (Y[used] < T).all()
            got = owner[Y[used], X[used]]
            want = np.broadcast_to(np.arange(nt)[:, None], used.shape)[used]
            assert np.array_equal(got, want), (dx, dy, np.flatnonzero(got != want)[:8])
            checked += int(used.sum())
    print(f"[atlas-adaptive] {name} T {T}: {checked} footprint texels checked over {nt} triangles x 70 points")
    assert checked > nt * 70


# ------------------------------------------------------------------------------------------------ refusals, bounds

def test_a_vertex_index_out_of_range_is_counted_not_read(cuda, meshes):
    import torch
    from mi3d import _lib, mesh
    v, t = meshes["latlong"]
    t = t.copy()
    t[5, 1] = len(v)
    t[100, 0] = -1
    t[101, 2] = 2 ** 31 - 1
    out = run_adaptive(cuda, v, t, 512, 1)
    want = M.layout(v, t, 512, 1)
    assert out["bad"] == want["bad"] == 3
    for i in (5, 100, 101):
        assert not (out["owner"] == i).any() and out["shape"][i] == 0x80000000
    assert np.array_equal(out["owner"], want["owner"]) and out["xyz"].tobytes() == want["xyz"].tobytes()
    assert out["vt"].tobytes() == want["vt"].tobytes() and np.array_equal(out["words"], want["plan"]["words"])
    assert (out["xyz"][out["owner"] < 0] == 0).all() and np.isfinite(out["xyz"]).all()
    with pytest.raises(_lib.Mi3dError, match="3 of the"):
        mesh.bake_texture(Stripes(), torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), 512, atlas="adaptive")


def test_c_abi_rejects_bad_arguments_and_writes_nothing_past_a_band(cuda, meshes):
    """hipErrorInvalidValue (1) from the entry points themselves, nothing launched; a band of 3 rows of a 777-wide image
    leaves the bytes behind it alone."""
    import torch
    from mi3d import _lib
    lib = _lib.lib()
    v, t = meshes["plane"]
    dv, dt = torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)
    nv, nt, T, rows = len(v), len(t), 777, 3
    good = run_adaptive(cuda, v, t, T, 1)
    p, s = _lib.ptr, _lib.stream(dv)
    shape = torch.from_numpy(good["shape"].view(np.int32)).to(cuda)
    slot = torch.from_numpy(good["slot"].view(np.int32)).to(cuda)
    tri_of = torch.from_numpy(good["triangle_of"].view(np.int32)).to(cuda)
    plan = torch.from_numpy(good["words"]).to(cuda)
    hist = torch.zeros(4096, dtype=torch.int32, device=cuda)
    bad = torch.zeros(2, dtype=torch.int64, device=cuda)
    ws_bytes = int(lib.mi3d_atlas_adaptive_workspace(nt))
    ws = torch.zeros(ws_bytes // 8 + 1, dtype=torch.int64, device=cuda)
    out_shape = torch.full((nt,), -7, dtype=torch.int32, device=cuda)
    out_slot, out_tri = torch.full((nt,), -7, dtype=torch.int32, device=cuda), torch.full((nt,), -7, dtype=torch.int32, device=cuda)
    vt = torch.full((3 * nt, 2), -7.0, device=cuda)
    xyz = torch.full((rows * T * 3 + 64,), -7.0, device=cuda)
    owner = torch.full((rows * T + 64,), -7, dtype=torch.int32, device=cuda)

    def measure(**kw):
        a = dict(vertices=p(dv), nv=nv, triangles=p(dt), nt=nt, shape=p(out_shape), hist=p(hist), bad=p(bad))
        a.update(kw)
        return lib.mi3d_atlas_adaptive_measure(*a.values(), s)
    for kw in (dict(vertices=None), dict(triangles=None), dict(shape=None), dict(hist=None), dict(bad=None), dict(nv=0),
               dict(nt=0), dict(nt=2 ** 31), dict(nv=2 ** 31), dict(bad=_lib.C.c_void_p(bad.data_ptr() + 4))):
        assert measure(**kw) == 1, kw

    def sort(**kw):
        a = dict(shape=p(shape), nt=nt, plan=p(plan), ws=p(ws), ws_bytes=ws_bytes, slot=p(out_slot), triangle_of=p(out_tri))
        a.update(kw)
        return lib.mi3d_atlas_adaptive_sort(*a.values(), s)
    for kw in (dict(shape=None), dict(nt=0), dict(plan=None), dict(ws=None), dict(ws_bytes=ws_bytes - 1), dict(slot=None),
               dict(triangle_of=None), dict(ws=_lib.C.c_void_p(ws.data_ptr() + 4))):
        assert sort(**kw) == 1, kw

    def uv(**kw):
        a = dict(shape=p(shape), slot=p(slot), nt=nt, plan=p(plan), T=T, vt=p(vt))
        a.update(kw)
        return lib.mi3d_atlas_adaptive_uv(*a.values(), s)
    for kw in (dict(shape=None), dict(slot=None), dict(nt=0), dict(plan=None), dict(T=63), dict(T=16385), dict(vt=None)):
        assert uv(**kw) == 1, kw

    def positions(**kw):
        a = dict(vertices=p(dv), nv=nv, triangles=p(dt), nt=nt, shape=p(shape), triangle_of=p(tri_of), plan=p(plan), T=T,
                 ssaa=1, row0=0, rows=rows, xyz=p(xyz), owner=p(owner))
        a.update(kw)
        return lib.mi3d_atlas_adaptive_positions(*a.values(), s)
    for kw in (dict(ssaa=3), dict(ssaa=0), dict(rows=0), dict(row0=T), dict(row0=T - 2, rows=3), dict(T=16385), dict(T=63),
               dict(nt=0), dict(nv=0), dict(vertices=None), dict(triangles=None), dict(shape=None), dict(triangle_of=None),
               dict(plan=None), dict(xyz=None)):
        assert positions(**kw) == 1, kw
    torch.cuda.synchronize()
    for buf, fill in ((out_shape, -7), (out_slot, -7), (out_tri, -7), (vt, -7), (xyz, -7), (owner, -7), (hist, 0), (bad, 0)):
        assert (buf == fill).all()
    # a band in the middle of a cell row: exactly rows * T texels are written
    row0 = 40
    assert positions(row0=row0) == 0
    torch.cuda.synchronize()
    got_xyz, got_owner = xyz.cpu().numpy(), owner.cpu().numpy()
    assert (got_xyz[rows * T * 3:] == -7).all() and (got_owner[rows * T:] == -7).all()
    assert got_xyz[:rows * T * 3].tobytes() == good["xyz"][row0:row0 + rows].tobytes()
    assert np.array_equal(got_owner[:rows * T].reshape(rows, T), good["owner"][row0:row0 + rows])
    assert positions(owner=None) == 0                                   # owner is optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ colours

@pytest.mark.parametrize("ssaa", [1, 2])
@pytest.mark.parametrize("T", (512, 777))
def test_colours_are_the_field(cuda, model, meshes, T, ssaa):
    """test_texture_gpu.py's test with atlas="adaptive": image[owner >= 0] == the quantised (mean of the) albedo the field
    gives at the kernels' positions, bitwise; unowned texels are 0."""
    import torch
    from mi3d import mesh
    v, t = meshes["collapsed"]
    dv, dt = torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)
    image, vt, owner = mesh.bake_texture(model, dv, dt, T, ssaa, atlas="adaptive")
    assert image.shape == (T, T, 3) and image.dtype == torch.uint8 and image.device == cuda
    assert vt.shape == (3 * len(t), 2) and vt.dtype == torch.float32 and owner.shape == (T, T) and owner.dtype == torch.int32
    k = run_adaptive(cuda, v, t, T, ssaa)
    image, vt, owner = image.cpu().numpy(), vt.cpu().numpy(), owner.cpu().numpy()
    assert k["bad"] == 0 and vt.tobytes() == k["vt"].tobytes() and np.array_equal(owner, k["owner"])
    owned = owner >= 0
    assert owned.any() and (~owned).any()
    assert (image[~owned] == 0).all()
    a = albedo_at(model, cuda, k["xyz"][owned].reshape(-1, 3)).reshape(-1, ssaa * ssaa, 3)
    mean = a[:, 0]
    for j in range(1, ssaa * ssaa):
        mean = mean + a[:, j]
    mean = mean * F(1.0 / (ssaa * ssaa))
    want = quantise(mean)
    got = image[owned]
    print(f"[atlas-adaptive] T {T} ssaa {ssaa}: {owned.sum()} owned texels, {(got != want).sum()} bytes differ, "
          f"{len(np.unique(got))} distinct byte values")
    assert np.array_equal(got, want)
    assert not np.array_equal(got[1:], want[:-1])
    image2, _, _ = mesh.bake_texture(model, dv, dt, T, ssaa, atlas="adaptive")
    assert image2.cpu().numpy().tobytes() == image.tobytes()


class Stripes:
    """A stub field: density(xyz)["albedo"] = 0.5 + 0.5 sin(2 pi 20 x), y and z likewise in the other channels."""
    calls = 0

    def density(self, xyz):
        import torch
        type(self).calls += 1
        return {"albedo": 0.5 + 0.5 * torch.sin(2.0 * np.pi * 20.0 * xyz)}


def test_sharper_where_it_matters(cuda, meshes):
    """The stripes baked into the graded plane at T = 256 under both atlases, read back by bilinear lookup through vt at
    area-weighted random surface points, in NumPy: the RMS error against the analytic albedo is lower for adaptive.
    The reasoning: about 9 texels per wavelength (176 to 192 texels per unit length, wavelength 0.05) against about 2
    (38 texels per unit length) on the large triangles that carry most of the area.  No ratio is asserted.
    Figures on an MI355X: 0.1829 uniform (c = 21), 0.0127 adaptive (profiles/atlas_adaptive.json)."""
    import torch
    from mi3d import mesh
    v, t = meshes["plane"]
    dv, dt = torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)
    tri, w, pts = M.surface_samples(v, t, 20000, seed=11)
    want = M.stripes(pts)
    rms = {}
    for atlas in ("uniform", "adaptive"):
        image, vt, _ = mesh.bake_texture(Stripes(), dv, dt, 256, atlas=atlas)
        got = M.bilinear_lookup(image.cpu().numpy(), vt.cpu().numpy(), tri, w)
        rms[atlas] = float(np.sqrt(np.mean((got - want) ** 2)))
    print(f"[atlas-adaptive] stripes on the graded plane at T 256, RMS error over {len(tri)} surface points: uniform "
          f"{rms['uniform']:.5f} (c = {mesh.atlas_cell(len(t), 256)}), adaptive {rms['adaptive']:.5f}")
    os.makedirs(os.path.dirname(REPORT_PATH), exist_ok=True)
    with open(REPORT_PATH, "w") as fp:
        json.dump({"sharpness": {"mesh": "graded plane, 252 triangles", "texture_size": 256, "points": len(tri),
                                 "rms_uniform": rms["uniform"], "rms_adaptive": rms["adaptive"]}}, fp, indent=1)
    assert rms["adaptive"] < rms["uniform"]


def test_a_mesh_that_does_not_fit_is_refused_before_the_field_is_evaluated(cuda, meshes):
    import torch
    from mi3d import _lib, mesh
    v, t = meshes["mc_sphere"]
    dv, dt = torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda)
    hist = M.measure(v, t)[1]
    fit = next(T for T in (1 << k for k in range(6, 15)) if M.plan(hist, T) is not None)
    assert fit == 512
    before = Stripes.calls
    with pytest.raises(_lib.Mi3dError) as e:
        mesh.bake_texture(Stripes(), dv, dt, 256, atlas="adaptive")
    msg = str(e.value)
    print(f"[atlas-adaptive] {msg}")
    assert str(len(t)) in msg and "256" in msg and str(fit) in msg and Stripes.calls == before
    for bad in ("Adaptive", None, 3):
        with pytest.raises(_lib.Mi3dError, match="atlas"):
            mesh.bake_texture(Stripes(), dv, dt, 512, atlas=bad)
    assert Stripes.calls == before


# ------------------------------------------------------------------------------------------------ through the files

R_EXPORT, COLLAPSE_TO = 64, 1600


@pytest.fixture()
def ball(cuda, model, monkeypatch):
    """export_mesh sees the radius-0.6 sphere instead of the random-weight field's own density (a noise surface on which
    a collapse stalls far above any target); the colours stay the field's.  About 13 000 triangles at 64^3."""
    import torch
    from mi3d import mesh
    thresh = float(min(model.mean_density, model.density_thresh) if model.cuda_ray else model.density_thresh)
    ax = torch.linspace(-1, 1, R_EXPORT, device=cuda)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.6 - torch.sqrt(x * x + y * y + z * z)).float() + thresh
    monkeypatch.setattr(mesh, "extract_volume", lambda m, R: vol)
    return vol


def check_files(out, result, T):
    v, f, col, vt, image = result[:5]
    nt = len(f)
    assert sorted(n for n in os.listdir(out) if not n.startswith("preview")) == ["albedo.png", "mesh.mtl", "mesh.obj"]
    assert vt.shape == (3 * nt, 2) and vt.dtype == F and image.shape == (T, T, 3) and image.dtype == np.uint8
    mtllib, pv, extra, pvt, pf, pft, usemtl = parse_textured_obj(out / "mesh.obj")
    assert mtllib == "mesh.mtl" and usemtl == "mat0" and extra == 0
    assert np.array_equal(pv.astype(F), v) and len(pvt) == 3 * nt and np.array_equal(pvt.astype(F), vt)
    assert np.array_equal(pf, f.astype(np.int64) + 1)
    assert np.array_equal(pft, np.arange(3 * nt).reshape(nt, 3) + 1)
    png = decode_png(out / "albedo.png")
    assert np.array_equal(png, image)
    return pv, pvt, pf, pft, png


def test_export_mesh_end_to_end(cuda, model, ball, tmp_path):
    """export_mesh(texture_size=512, collapse=, atlas="adaptive"): the files match the returned arrays, the arrays are
    bake_texture's, and - by the method and the tolerance of test_texture_gpu.py's
    test_exported_files_show_the_field_at_the_points_their_uvs_denote - the field's albedo at the points the files' UVs
    denote matches the decoded image: one code value plus twice the field's four-ulp sensitivity."""
    import torch
    from mi3d import mesh
    T = 512
    res = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT, texture_size=T, collapse=COLLAPSE_TO, atlas="adaptive")
    assert len(res) == 5
    pv, pvt, pf, pft, png = check_files(tmp_path / "a", res, T)
    v, f, _, vt, image = res
    nt = len(f)
    dv, df = torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda)
    plan = mesh.atlas_plan(dv, df, T)
    assert nt in (COLLAPSE_TO, COLLAPSE_TO - 1)
    print(f"[atlas-adaptive] export at 64^3 collapsed to nt {nt}: shift {plan['shift']}, rows {plan['rows']}, fill "
          f"{plan['fill']:.3f}, clamped legs {plan['clamped_small']} + {plan['clamped_large']}")
    img, kvt, _ = mesh.bake_texture(model, dv, df, T, atlas="adaptive")
    assert img.cpu().numpy().tobytes() == image.tobytes() and kvt.cpu().numpy().tobytes() == vt.tobytes()
    uni = model.export_mesh(str(tmp_path / "u"), resolution=R_EXPORT, texture_size=T, collapse=COLLAPSE_TO)
    assert uni[0].tobytes() == v.tobytes() and uni[1].tobytes() == f.tobytes() and uni[3].tobytes() != vt.tobytes()

    tri_px = np.stack([pvt[:, 0] * T - 0.5, (1.0 - pvt[:, 1]) * T - 0.5], -1)[pft - 1]      # [nt, 3, 2] float64
    rng = np.random.default_rng(7)
    pairs, want_pairs = [], 4096
    while sum(len(p[0]) for p in pairs) < want_pairs:
        tri = rng.integers(0, nt, 8192)
        w = rng.dirichlet(np.ones(3), size=len(tri))
        P = tri_px[tri]
        texel = np.rint(np.einsum("nb,nbd->nd", w, P))
        d1, d2, dp = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], texel - P[:, 0]
        det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
        b1 = (dp[:, 0] * d2[:, 1] - dp[:, 1] * d2[:, 0]) / det
        b2 = (d1[:, 0] * dp[:, 1] - d1[:, 1] * dp[:, 0]) / det
        bary = np.stack([1 - b1 - b2, b1, b2], -1)
        inside = (bary > 1e-3).all(1)
        pairs.append((tri[inside], texel[inside].astype(np.int64), bary[inside]))
    tri = np.concatenate([p[0] for p in pairs])
    texel = np.concatenate([p[1] for p in pairs])
    bary = np.concatenate([p[2] for p in pairs])
    assert len(tri) >= want_pairs and len(np.unique(tri)) > nt // 4
    pts32 = np.einsum("nb,nbd->nd", bary, pv[pf[tri] - 1]).astype(F)
    albedo = albedo_at(model, cuda, pts32).astype(np.float64)
    sens = 0.0
    for axis in range(3):
        for direction in (F(np.inf), F(-np.inf)):
            moved = pts32.copy()
            for _ in range(4):
                moved[:, axis] = np.nextafter(moved[:, axis], direction)
            sens = max(sens, float(np.abs(albedo_at(model, cuda, moved).astype(np.float64) - albedo).max()))
    margin = 2 * sens
    decoded = png[texel[:, 1], texel[:, 0]].astype(np.float64) / 255.0
    err = np.abs(decoded - albedo)
    print(f"[atlas-adaptive] files vs field over {len(tri)} (triangle, interior texel) pairs of {len(np.unique(tri))} "
          f"triangles: max |texel / 255 - albedo| {err.max():.6f}; four-ulp sensitivity {sens:.3e}, bound "
          f"{1 / 255 + margin:.6f}")
    assert (err <= 1.0 / 255.0 + margin).all()
    assert (np.abs(np.roll(decoded, 1, axis=0) - albedo) > 1.0 / 255.0 + margin).any()
    assert (decoded - albedo <= margin).all()


def test_export_mesh_with_views_and_preview(cuda, model, ball, tmp_path):
    import texture_views_model as V
    import torch
    from mi3d import mesh
    from test_texture_views_cpu import smooth_images
    T, H, W = 512, 48, 64
    c2w, K = V.orbit(4, 3.2, 0.4, 0.1), V.pinhole(1.6, H, W)
    views = dict(images=smooth_images(4, H, W, seed=9), c2w=c2w, K=K)
    preview = dict(c2w=c2w[:2], K=K, H=H, W=W)
    field = model.export_mesh(str(tmp_path / "f"), resolution=R_EXPORT, texture_size=T, collapse=COLLAPSE_TO, atlas="adaptive")
    both = model.export_mesh(str(tmp_path / "v"), resolution=R_EXPORT, texture_size=T, collapse=COLLAPSE_TO, atlas="adaptive",
                             views=views, preview=preview)
    check_files(tmp_path / "v", both, T)
    assert sorted(n for n in os.listdir(tmp_path / "v") if n.startswith("preview")) == ["preview_000.png", "preview_001.png"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(field[:4], both[:4]))         # the same mesh, the same vt
    dv, df = torch.from_numpy(both[0]).to(cuda), torch.from_numpy(both[1]).to(cuda)
    image, vt, owner, hits = mesh.bake_views(model, dv, df, T, atlas="adaptive", **views)
    assert image.cpu().numpy().tobytes() == both[4].tobytes() and vt.cpu().numpy().tobytes() == both[3].tobytes()
    seen = (hits[:, :, 0] > 0).cpu().numpy()
    owned = (owner >= 0).cpu().numpy()
    print(f"[atlas-adaptive] views: texels a view sees {seen.sum()} of {owned.sum()}")
    assert seen.sum() > 500 and (~seen & owned).sum() > 100
    assert (both[4][~seen] == field[4][~seen]).all() and (both[4][seen] != field[4][seen]).any()
    shown = decode_png(tmp_path / "v" / "preview_000.png")
    assert shown.shape == (H, W, 3) and len(np.unique(shown.reshape(-1, 3), axis=0)) > 16      # the textured mesh, not a blank


def test_the_uniform_atlas_is_untouched(cuda, model, ball, tmp_path, monkeypatch):
    """atlas="uniform" writes files byte-identical to the same call without the argument, and launches no kernel of
    Part 20."""
    from mi3d import _lib
    seen, launch = [], _lib.launch

    def spy(name, *a):
        seen.append(name)
        return launch(name, *a)
    monkeypatch.setattr(_lib, "launch", spy)
    a = model.export_mesh(str(tmp_path / "a"), resolution=R_EXPORT, texture_size=512, collapse=COLLAPSE_TO)
    plain = list(seen)
    del seen[:]
    b = model.export_mesh(str(tmp_path / "b"), resolution=R_EXPORT, texture_size=512, collapse=COLLAPSE_TO, atlas="uniform")
    assert seen == plain and "mi3d_atlas_uv" in seen and not any("adaptive" in name for name in seen)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for name in ("mesh.obj", "mesh.mtl", "albedo.png"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    with pytest.raises(_lib.Mi3dError, match="texture_size"):
        model.export_mesh(str(tmp_path / "c"), resolution=R_EXPORT, collapse=COLLAPSE_TO, atlas="adaptive")
    with pytest.raises(_lib.Mi3dError, match="atlas"):
        model.export_mesh(str(tmp_path / "c"), resolution=R_EXPORT, texture_size=512, atlas="charts")
    assert not os.path.exists(tmp_path / "c")
