"""CPU: the reference-view loss of mi3d.sds_step (pearson_corrcoef, ref_view_loss), the options it needs and the op it
trains through.  No GPU: the loss is plain torch."""
import numpy as np
import torch
import torch.nn.functional as F


def _pearson(x, y):
    from mi3d.sds_step import pearson_corrcoef
    return float(pearson_corrcoef(torch.from_numpy(x), torch.from_numpy(y)))


def test_pearson_corrcoef_against_numpy():
    rng = np.random.default_rng(0)
    x = rng.normal(size=500)
    for y in (rng.normal(size=500), 0.7 * x + 0.3 * rng.normal(size=500), 3.0 - 2.0 * x + 1e-3 * rng.normal(size=500)):
        assert abs(_pearson(x, y) - np.corrcoef(x, y)[0, 1]) <= 1e-12
    assert abs(_pearson(x, 5.0 - 2.0 * x) + 1.0) <= 1e-12   # perfectly anti-correlated
    assert abs(_pearson(x + 7.0, 3.0 * x) - 1.0) <= 1e-12


def test_pearson_corrcoef_clamps():
    """Pairs whose unclamped quotient rounds past 1: only the clamp keeps the result inside [-1, 1]."""
    rng = np.random.default_rng(1)
    found = 0
    for _ in range(200):
        x = rng.normal(size=64) * 10.0 ** rng.uniform(-3, 3)
        y = 3.0 * x
        xm, ym = x - x.mean(), y - y.mean()
        raw = (xm * ym).sum() / np.sqrt((xm * xm).sum() * (ym * ym).sum())
        r = _pearson(x, y)
        assert -1.0 <= r <= 1.0 and abs(r - np.corrcoef(x, y)[0, 1]) <= 1e-12
        found += raw > 1.0
    assert found > 0


def _loss_inputs():
    g = torch.Generator().manual_seed(2)
    S, h = 12, 5
    pred_rgb = torch.rand(1, 3, h, h, generator=g, dtype=torch.float64)
    pred_depth = (torch.rand(1, 1, h, h, generator=g, dtype=torch.float64) * 3 + 1).requires_grad_(True)
    gt_rgb = torch.rand(1, 3, S, S, generator=g, dtype=torch.float64)
    ref_depth = torch.rand(S, S, generator=g, dtype=torch.float64)
    depth_mask = torch.rand(S, S, generator=g) < 0.3  # True = no prior there
    return pred_rgb, pred_depth, gt_rgb, ref_depth, depth_mask


def test_ref_view_loss_is_the_reference_formula():
    from mi3d.sds_step import make_opt, ref_view_loss
    opt = make_opt(lambda_img=1e3, lambda_depth=0.7)
    pred_rgb, pred_depth, gt_rgb, ref_depth, depth_mask = _loss_inputs()
    loss = ref_view_loss(pred_rgb, pred_depth, gt_rgb, ref_depth, depth_mask, opt)

    up_rgb = F.interpolate(pred_rgb, gt_rgb.shape[-2:], mode="bilinear", align_corners=True)
    up_d = F.interpolate(pred_depth.detach(), gt_rgb.shape[-2:], mode="bilinear", align_corners=True)
    valid = ~depth_mask.reshape(-1).numpy()
    co = np.corrcoef(up_d.reshape(-1).numpy()[valid], ref_depth.reshape(-1).numpy()[valid])[0, 1]
    want = 1e3 * float((up_rgb - gt_rgb).abs().mean()) + 0.7 * (1 - co)
    assert abs(float(loss.detach()) - want) <= 1e-9 * abs(want)

    loss.backward()
    assert float(pred_depth.grad.abs().max()) > 0


def test_ref_view_loss_mask_and_nan():
    """Masked-out pixels do not count; a NaN in a masked-in depth pixel is read as 0 (torch.nan_to_num in depth_loss)."""
    from mi3d.sds_step import make_opt, ref_view_loss
    opt = make_opt()
    pred_rgb, _, gt_rgb, ref_depth, depth_mask = _loss_inputs()
    S = gt_rgb.shape[-1]
    pred_depth = torch.rand(1, 1, S, S, generator=torch.Generator().manual_seed(4), dtype=torch.float64) + 1  # no resize
    base = ref_view_loss(pred_rgb, pred_depth, gt_rgb, ref_depth, depth_mask, opt)

    out_y, out_x = [int(v[0]) for v in torch.nonzero(depth_mask, as_tuple=True)]
    in_y, in_x = [int(v[0]) for v in torch.nonzero(~depth_mask, as_tuple=True)]
    moved, moved_ref = pred_depth.clone(), ref_depth.clone()
    moved[0, 0, out_y, out_x] = 1e6
    moved_ref[out_y, out_x] = float("nan")
    assert float(ref_view_loss(pred_rgb, moved, gt_rgb, moved_ref, depth_mask, opt)) == float(base)

    with_nan, with_zero = pred_depth.clone(), pred_depth.clone()
    with_nan[0, 0, in_y, in_x] = float("nan")
    with_zero[0, 0, in_y, in_x] = 0.0
    a = ref_view_loss(pred_rgb, with_nan, gt_rgb, ref_depth, depth_mask, opt)
    b = ref_view_loss(pred_rgb, with_zero, gt_rgb, ref_depth, depth_mask, opt)
    assert torch.isfinite(a) and float(a) == float(b) and float(a) != float(base)


def test_options_and_op_exist():
    import raymarching
    from mi3d import sds_step
    opt = sds_step.make_opt()
    assert (opt.lambda_img, opt.lambda_depth, opt.depth_grad) == (1e3, 1.0, False)
    assert callable(raymarching.composite_rays_train_depth)
    assert callable(sds_step.ref_view_train_step)
