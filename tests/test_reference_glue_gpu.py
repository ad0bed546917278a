"""GPU: the reference's OWN renderer / field Python (nerf/renderer.py:481-639, nerf/network_tcnn.py:94-205 - staged
verbatim under the git-ignored oracle/_ref/py by oracle/build_ref.py) running UNCHANGED on the product's drop-in
`raymarching` + `tinycudann` packages (the zero-change route: 13 encoder passes, torch
nn.Linear MLP, torch elementwise head, atomic scatter) against the product's fast route (mi3d.network.NeRFNetwork:
one stencil gather, MFMA MLP, fused head, binned scatter) - same weights, same seeds.

This pins the glue the kernels sit under - run_cuda's training branch with both normal regularisers and every
parameter gradient, update_extra_state's grid values / EMA / mean / bitfield, and the eval march-composite loop - on
the reference itself rather than on a restatement of it.  fp32 (no autocast): 1e-4 relative, as BASELINE.json states;
one autocast case checks the route under AMP the way main.py runs it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference sources not staged (oracle/build_ref.py runs in the build container)")
    ref_import.install()
    return ref_import


def _pair(ref, cuda, **opt_kw):
    """(reference network on the drop-ins, product network) with identical, lively parameters."""
    from mi3d.network import NeRFNetwork
    kw = dict(cuda_ray=True, lambda_smooth=1.0, max_steps=128)
    kw.update(opt_kw)
    opt = ref.default_opt(**kw)
    torch.manual_seed(0)
    ours = NeRFNetwork(opt).to(cuda)
    with torch.no_grad():
        ours.encoder.params.uniform_(-0.3, 0.3)
    theirs = ref.reference_network(opt, "dropin").to(cuda)
    assert set(theirs.state_dict().keys()) == set(ours.state_dict().keys())
    theirs.load_state_dict(ours.state_dict())
    return theirs, ours, opt


def _sphere_bits(model, r):
    from mi3d import sds_step
    sds_step.set_bitfield(model, r)


def _close(a, b, rtol=1e-4, atol=1e-6, what=""):
    a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


def _render_train(model, ro, rd, ds, seed, max_steps, autocast=False, dt_gamma=0):
    model.train()
    model.zero_grad()
    torch.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out = model.render(ro, rd, depth_scale=ds, bg_color=torch.full((3,), 0.7, device=ro.device), perturb=True,
                           ambient_ratio=1.0, shading="albedo", force_all_rays=True, dt_gamma=dt_gamma,
                           max_steps=max_steps)
        loss = ((out["image"] ** 2).mean() + (out["weights_sum"] ** 2).mean() + 0.1 * out["loss_orient"]
                + (out["loss_smooth"] if "loss_smooth" in out else 0))
    loss.backward()
    return out


@pytest.mark.parametrize("H,smooth", [(8, 1.0), (32, 0.0)])
def test_training_run_cuda_matches_the_reference_renderer(ref, cuda, H, smooth):
    """run_cuda, training branch.  8x8 rays = one marching wave, so both runs lay their samples out identically and
    the smoothness jitter (torch.randn_like(xyzs), drawn per ROW) lands on the same samples: loss_smooth and its
    gradients compare exactly.  32x32 rays (16 waves, slab order free): everything but the jitter term."""
    from mi3d import rays as R
    theirs, ours, opt = _pair(ref, cuda, lambda_smooth=smooth, max_steps=256)
    for m in (theirs, ours):
        _sphere_bits(m, 0.6)
    ro, rd, ds = R.view_rays(H, H, device=cuda)
    a = _render_train(theirs, ro, rd, ds, 123, 256)
    b = _render_train(ours, ro, rd, ds, 123, 256)
    assert int(theirs.step_counter[0, 0]) == int(ours.step_counter[0, 0]) > 64 * H
    for k in ("image", "depth", "weights_sum"):
        _close(b[k], a[k], what=k)
    assert torch.equal(a["mask"], b["mask"])
    _close(b["loss_orient"], a["loss_orient"], rtol=2e-4, what="loss_orient")
    if smooth > 0:
        _close(b["loss_smooth"], a["loss_smooth"], rtol=2e-4, what="loss_smooth")
    for (name, p), q in zip(theirs.named_parameters(), ours.parameters()):
        scale = float(p.grad.abs().max())
        assert scale > 0, name
        err = float((p.grad - q.grad).abs().max())
        # the normal regularisers differentiate safe_normalize of finite differences: conditioning ~1e3
        assert err <= 2e-3 * scale, (name, err, scale)


def _compare_training(theirs, ours, a, b, smooth_rtol=None):
    for k in ("image", "depth", "weights_sum"):
        _close(b[k], a[k], what=k)
    assert torch.equal(a["mask"], b["mask"])
    _close(b["loss_orient"], a["loss_orient"], rtol=2e-4, what="loss_orient")
    if smooth_rtol is not None:
        _close(b["loss_smooth"], a["loss_smooth"], rtol=smooth_rtol, what="loss_smooth")
    for (name, p), q in zip(theirs.named_parameters(), ours.parameters()):
        scale = float(p.grad.abs().max())
        assert scale > 0, name
        assert float((p.grad - q.grad).abs().max()) <= 2e-3 * scale, name


def test_training_at_baseline_size_pruned(ref, cuda):
    """BASELINE config 2's ray count and step budget with the pruned occupancy of SURVEY 8(d) (sphere 0.3: ~2.3 M
    samples, 13 x that many field evaluations on the reference route) - the size at which the binned scatter, the
    prefix backward and the planes kernels run as they do in the benchmark, against the reference's own Python.
    The smoothness jitter is drawn per ROW and the 256 marching waves' slabs arrive in a different order in each run,
    so that one term is left out of the loss here (its exact comparison is the 8 x 8 case above)."""
    from mi3d import rays as R
    theirs, ours, opt = _pair(ref, cuda, lambda_smooth=0.0, max_steps=1024)
    for m in (theirs, ours):
        _sphere_bits(m, 0.3)
    ro, rd, ds = R.view_rays(128, 128, device=cuda)
    a = _render_train(theirs, ro, rd, ds, 21, 1024)
    b = _render_train(ours, ro, rd, ds, 21, 1024)
    n = int(ours.step_counter[0, 0])
    assert n == int(theirs.step_counter[0, 0]) and 1_500_000 < n < 3_500_000
    _compare_training(theirs, ours, a, b)


def test_training_with_lambertian_shading(ref, cuda):
    """shading='lambertian' below the reference's 1e6-sample cut-off (network_tcnn.py:159): the normal enters the
    colour, so the image gradient reaches the six finite-difference neighbours - the 7-point backward of the fused
    field node - through the reference's own shading arithmetic."""
    from mi3d import rays as R
    theirs, ours, opt = _pair(ref, cuda, lambda_smooth=0.0, max_steps=1024)
    for m in (theirs, ours):
        _sphere_bits(m, 0.3)
    ro, rd, ds = R.view_rays(80, 80, device=cuda)
    outs = []
    for model in (theirs, ours):
        model.train()
        model.zero_grad()
        torch.manual_seed(5)
        out = model.render(ro, rd, depth_scale=ds, bg_color=torch.full((3,), 0.7, device=cuda), perturb=True,
                           ambient_ratio=0.3, shading="lambertian", force_all_rays=True, dt_gamma=0, max_steps=1024)
        ((out["image"] ** 2).mean() + (out["weights_sum"] ** 2).mean()).backward()   # the image term alone
        outs.append(out)
    n = int(ours.step_counter[0, 0])
    assert n == int(theirs.step_counter[0, 0]) and 300_000 < n < 1_000_000   # shading really applies (< 1e6 rows)
    for k in ("image", "depth", "weights_sum"):
        _close(outs[1][k], outs[0][k], what=k)
    for (name, p), q in zip(theirs.named_parameters(), ours.parameters()):
        scale = float(p.grad.abs().max())
        assert scale > 0, name
        assert float((p.grad - q.grad).abs().max()) <= 2e-3 * scale, name


def test_training_run_cuda_under_autocast(ref, cuda):
    """The same route under torch.autocast(float16), as nerf/utils.py:979 runs it: the reference's nn.Linear stack
    rounds where the MFMA kernel's binary16 mode rounds; rendered outputs agree to binary16 resolution."""
    from mi3d import rays as R
    theirs, ours, opt = _pair(ref, cuda, lambda_smooth=0.0, max_steps=256)
    for m in (theirs, ours):
        _sphere_bits(m, 0.6)
    ro, rd, ds = R.view_rays(32, 32, device=cuda)
    a = _render_train(theirs, ro, rd, ds, 7, 256, autocast=True)
    b = _render_train(ours, ro, rd, ds, 7, 256, autocast=True)
    for k in ("image", "depth", "weights_sum"):
        _close(b[k], a[k], rtol=2e-2, atol=2e-3, what=k)
    g_ref, g = theirs.encoder.params.grad, ours.encoder.params.grad
    assert float((g_ref - g).abs().max()) <= 5e-2 * float(g_ref.abs().max())


def test_update_extra_state_matches_the_reference(ref, cuda):
    """Density-grid refresh (renderer.py:586-639): same torch.rand jitter under a shared seed -> grid values, EMA-max
    over two refreshes, mean density, occupancy bitfield, mean_count."""
    from mi3d import rays as R
    theirs, ours, opt = _pair(ref, cuda, lambda_smooth=0.0, bound=2.0)   # two cascades
    for rnd in range(2):
        for m in (theirs, ours):
            torch.manual_seed(50 + rnd)
            m.update_extra_state()
        _close(ours.density_grid, theirs.density_grid, rtol=1e-4, atol=1e-6, what=f"density_grid round {rnd}")
        assert abs(ours.mean_density - theirs.mean_density) <= 1e-5 * abs(theirs.mean_density)
        # a bit may differ only where the density sits within rounding of the threshold
        thresh = min(theirs.mean_density, theirs.density_thresh)
        diff = (ours.density_bitfield ^ theirs.density_bitfield).cpu().numpy()
        if diff.any():
            bytes_ = np.nonzero(diff)[0]
            grid = theirs.density_grid.reshape(-1).cpu().numpy()
            for bidx in bytes_:
                for bit in range(8):
                    if (diff[bidx] >> bit) & 1:
                        assert abs(grid[bidx * 8 + bit] - thresh) <= 2e-4 * thresh
        assert diff.astype(bool).mean() < 1e-4
        assert ours.iter_density == theirs.iter_density and ours.local_step == theirs.local_step == 0
        # a training render in between so the next refresh also averages step counters
        ro, rd, ds = R.view_rays(16, 16, device=cuda)
        for m in (theirs, ours):
            _render_train(m, ro, rd, ds, 9, 128)
    assert ours.mean_count == theirs.mean_count


def test_eval_render_matches_the_reference(ref, cuda):
    """The inference branch (renderer.py:526-551 march_rays / composite_rays loop) on a refreshed occupancy grid:
    image, depth, weights, normal map."""
    from mi3d import rays as R
    theirs, ours, opt = _pair(ref, cuda, lambda_smooth=0.0)
    torch.manual_seed(3)
    ours.update_extra_state()
    theirs.density_grid.copy_(ours.density_grid)
    theirs.density_bitfield.copy_(ours.density_bitfield)
    theirs.mean_density = ours.mean_density
    ro, rd, ds = R.view_rays(48, 48, device=cuda)
    outs = []
    for m in (theirs, ours):
        m.eval()
        with torch.no_grad():
            torch.manual_seed(11)
            outs.append(m.render(ro, rd, depth_scale=ds, bg_color=torch.ones(3, device=cuda), perturb=False,
                                 ambient_ratio=1.0, shading="albedo", dt_gamma=0, max_steps=256))
    a, b = outs
    assert float(a["weights_sum"].max()) > 0.5
    for k in ("image", "depth", "weights_sum"):
        _close(b[k], a[k], what=k)
    # the normal map is a weighted sum of ratios of finite differences: compare in absolute terms
    _close(b["normal"], a["normal"], rtol=0, atol=2e-3, what="normal")


def _pair_two_cascades(ref, cuda, oracle):
    """bound = 2 (two cascades), max_steps = 256, the same analytic occupancy on both sides: a sphere of radius 1.6, so
    that samples lie inside the unit box (cascade 0) and outside it."""
    from conftest import sphere_bitfield
    theirs, ours, opt = _pair(ref, cuda, lambda_smooth=0.0, bound=2.0, max_steps=256)
    bits = torch.from_numpy(sphere_bitfield(oracle, 2, 128, 1.6)).to(cuda)
    for m in (theirs, ours):
        assert m.cascade == 2 and m.grid_size == 128 and m.density_bitfield.shape == bits.shape
        m.density_bitfield.copy_(bits)
    return theirs, ours


def test_training_with_two_cascades_and_cone_steps(ref, cuda, oracle):
    """run_cuda's training branch at bound = 2 and dt_gamma = 1/64 (every other training comparison here runs at
    bound = 1, dt_gamma = 0): bound, dt_gamma and the cascade count reach march_rays_train through the renderer as the
    reference passes them; outputs and every parameter gradient through _compare_training."""
    from mi3d import rays as R
    theirs, ours = _pair_two_cascades(ref, cuda, oracle)
    ro, rd, ds = R.view_rays(32, 32, device=cuda)
    a = _render_train(theirs, ro, rd, ds, 123, 256, dt_gamma=1 / 64)
    b = _render_train(ours, ro, rd, ds, 123, 256, dt_gamma=1 / 64)
    n = int(ours.step_counter[0, 0])
    print(f"{n} samples")
    assert n == int(theirs.step_counter[0, 0]) and n > 64 * 32
    _compare_training(theirs, ours, a, b)


# The eval jitter reaches one sample per ray: round 0 takes one step from near + dt * noise, and the composite's running t
# restarts every later round from near + dt (renderer.py docstring of _infer_loop), so the rest of the ray is the
# unperturbed one.  Under albedo shading the colour of that one sample hardly changes over a step of dt_min and the
# image moves by 9.4e-5 - two tolerances, too little to tell a jitter from none.  Under lambertian shading the sample's
# colour follows its normal, which varies at that scale: the image moves by 4.3e-3, eleven times the bar below
# (measured on an MI355X; textureless 8.3e-3, normal 1.3e-2; all of them pass the comparisons with the reference).
EVAL_JITTER_SHADING = dict(shading="lambertian", ambient_ratio=0.3)


def _eval_two_cascades(ref, cuda, oracle, shading, ambient_ratio):
    """The body of the test below for one shading; returns how far the jitter moved the product's image and the bar."""
    from mi3d import rays as R
    theirs, ours = _pair_two_cascades(ref, cuda, oracle)
    ro, rd, ds = R.view_rays(48, 48, device=cuda)
    light = torch.tensor([0.0, -0.6, 0.8], device=cuda)

    def render(m, perturb, dt_gamma):
        m.eval()
        with torch.no_grad():
            torch.manual_seed(11)
            return m.render(ro, rd, depth_scale=ds, bg_color=torch.ones(3, device=cuda), perturb=perturb, light_d=light,
                            ambient_ratio=ambient_ratio, shading=shading, dt_gamma=dt_gamma, max_steps=256)

    def compare(a, b, what):
        assert float(a["weights_sum"].max()) > 0.5
        for k in ("image", "depth", "weights_sum"):
            _close(b[k], a[k], what=f"{what}: {k}")
        _close(b["normal"], a["normal"], rtol=0, atol=2e-3, what=f"{what}: normal")

    compare(render(theirs, False, 1 / 64), render(ours, False, 1 / 64), "dt_gamma 1/64")
    plain = render(ours, False, 0)
    a, b = render(theirs, True, 0), render(ours, True, 0)
    first = dict(ours.infer_stats)
    assert first["schedule"] == "reference"
    compare(a, b, "perturb")
    moved = float((b["image"] - plain["image"]).abs().max())
    bar = 10 * 1e-4 * float(plain["image"].abs().max())
    print(f"{shading} {ambient_ratio}: the jitter moves the image by {moved:.3g} (ten times the tolerance: {bar:.3g})")
    again = render(ours, True, 0)
    assert ours.infer_stats["graphs_captured"] == 0 and ours.infer_stats["graph_replays"] >= 1
    for k in ("image", "depth", "weights_sum", "normal"):
        assert torch.equal(again[k], b[k]), k
    return moved, bar


def test_eval_render_with_two_cascades_cone_steps_and_jitter(ref, cuda, oracle):
    """The inference branch at bound = 2: (1) dt_gamma = 1/64, no jitter; (2) perturb=True at dt_gamma = 0, which the
    product runs on the reference's round structure with the jitter in round 0 only, drawn as the reference's march_rays
    draws it (one torch.rand(N) after the seed).  Both against the reference's own loop with the comparisons of
    test_eval_render_matches_the_reference; the jitter must be visible (more than ten times the tolerance away from the
    unperturbed image), and a second perturbed render - through the graphs the first one captured - must repeat it bit
    for bit after the same seed."""
    moved, bar = _eval_two_cascades(ref, cuda, oracle, **EVAL_JITTER_SHADING)
    assert moved > bar


def test_main_py_import_line_trains_on_the_fused_field(ref, cuda):
    """INTEGRATION.md section 2, on the GPU, in a fresh interpreter whose PYTHONPATH starts with make-it-3d_amd/autopatch (the
    zero-edit route): `from nerf.network_tcnn import NeRFNetwork` (main.py:104) hands out mi3d.network.NeRFNetwork, a
    training render + both backward passes of the reference schedule run on it (13-point fused field: ONE binned scatter
    call for the two passes), and its outputs equal the reference's own class on the same weights (1e-4)."""
    import subprocess
    import sys
    import textwrap
    from conftest import PKG, ROOT
    script = """
        import sys, torch
        from oracle import ref_import
        ref_import.install()
        from nerf.network_tcnn import NeRFNetwork            # main.py:104
        import mi3d.network, nerf.network_tcnn as m
        from mi3d import field_ops, rays as R, sds_step
        assert NeRFNetwork is mi3d.network.NeRFNetwork
        dev = torch.device("cuda:0")
        opt = ref_import.default_opt(cuda_ray=True, lambda_smooth=1.0, max_steps=256)
        torch.manual_seed(0)
        ours = NeRFNetwork(opt).to(dev)
        with torch.no_grad():
            ours.encoder.params.uniform_(-0.3, 0.3)
        theirs = m.NeRFNetwork_reference(opt).to(dev)
        theirs.load_state_dict(ours.state_dict())
        for net in (ours, theirs):
            sds_step.set_bitfield(net, 0.5)
        ro, rd, ds = R.view_rays(32, 32, device=dev)
        outs, calls = [], []
        real = field_ops.scatter_binned
        field_ops.scatter_binned = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        for net in (theirs, ours):
            net.train()
            calls.clear()
            torch.manual_seed(3)
            out = net.render(ro, rd, depth_scale=ds, bg_color=torch.full((3,), 0.7, device=dev), perturb=True,
                             ambient_ratio=1.0, shading="albedo", force_all_rays=True, dt_gamma=0, max_steps=256)
            out["image"].backward(torch.full_like(out["image"], 1e-3), retain_graph=True)     # nerf/sd.py:171
            (out["loss_orient"] + out["weights_sum"].mean()).backward()                         # nerf/utils.py:983
            assert net.encoder.params.grad.abs().sum() > 0
            outs.append(out)
        assert len(calls) == 1, calls      # the fused class: the first pass's point-0 planes rode along in ONE scatter
        for k in ("image", "depth", "weights_sum"):
            torch.testing.assert_close(outs[1][k], outs[0][k], rtol=1e-4, atol=1e-6)
        print("ok")
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(PKG, "autopatch"), PKG, ROOT])
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
