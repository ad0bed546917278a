"""CPU: GroupNorm.forward(x, act=...) of mi3d/sd_standin.py off the fused route - CPU tensors never take it - equals
F.group_norm (+ F.silu) bit for bit, whatever the GN_FUSED switch says; and the Part 10 host query."""
import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_route_is_stock_group_norm_bit_for_bit(fused, dtype):
    from mi3d import sd_standin as S
    torch.manual_seed(0)
    m = S.GroupNorm(4, 8, eps=1e-6).to(dtype)
    with torch.no_grad():
        m.weight.normal_()
        m.bias.normal_()
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 8, 5, 7, dtype=dtype)
    old = S.GN_FUSED
    S.GN_FUSED = fused
    try:
        plain, act = m(x), m(x, act="silu")
    finally:
        S.GN_FUSED = old
    want = F.group_norm(x, 4, m.weight, m.bias, 1e-6)
    assert torch.equal(plain, want)
    assert torch.equal(act, F.silu(want))


def test_unknown_activation_is_refused():
    from mi3d import sd_standin as S
    with pytest.raises(ValueError):
        S.GroupNorm(4, 8)(torch.zeros(1, 8, 2, 2), act="relu")


def test_resblock_on_cpu_is_unchanged_by_the_switch():
    from mi3d import sd_standin as S
    torch.manual_seed(1)
    blk = S.ResBlock(32, 64)
    x = torch.randn(1, 32, 6, 6)
    want = blk.conv1(F.silu(F.group_norm(x, 32, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)))
    want = blk.conv2(F.silu(F.group_norm(want, 32, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)))
    want = blk.skip(x) + want
    assert torch.equal(blk(x), want)


def test_chunk_query_is_host_only():
    from mi3d import _lib
    q = _lib.lib().mi3d_groupnorm_chunks
    assert q(1) == 1 and q(8192) == 1 and q(8193) == 2 and q(9600) == 2 and q(512 * 512) == 32
