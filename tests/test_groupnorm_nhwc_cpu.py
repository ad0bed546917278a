"""CPU: routing of the channels-last GroupNorm kernels.  A CPU tensor, or one that is not channels-last, never reaches the
NHWC entry points; the host queries of the span decomposition; the stand-in's switches convert weights and nothing else."""
import pytest
import torch
import torch.nn.functional as F

CL = torch.channels_last


@pytest.fixture
def calls():
    """Names of every C-ABI call made while the fixture is active (none may launch: there is no GPU here)."""
    from mi3d import _lib as L
    seen, orig = [], L.call

    def spy(name, *a):
        seen.append(name)
        raise AssertionError(f"{name} reached on a machine without a GPU")
    L.call = spy
    try:
        yield seen
    finally:
        L.call = orig


@pytest.mark.parametrize("fused", [True, False])
def test_cpu_channels_last_input_takes_the_stock_route(calls, fused):
    from mi3d import sd_standin as S
    torch.manual_seed(0)
    m = S.GroupNorm(4, 16, eps=1e-6)
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 16, 5, 7).contiguous(memory_format=CL)
    old = S.GN_FUSED
    S.GN_FUSED = fused
    try:
        y = m(x, act="silu")
    finally:
        S.GN_FUSED = old
    assert torch.equal(y, F.silu(F.group_norm(x, 4, m.weight, m.bias, 1e-6)))
    assert calls == []


def test_layout_names_the_kernel_family():
    from mi3d import norm_ops
    x = torch.zeros(2, 16, 5, 7, dtype=torch.float16)
    assert norm_ops.layout(x, 4) == "nchw"
    assert norm_ops.layout(x.contiguous(memory_format=CL), 4) == "nhwc"
    assert norm_ops.layout(x.transpose(2, 3), 4) is None                         # neither format
    assert norm_ops.layout(x[:, :12].contiguous(memory_format=CL), 4) is None    # 12 channels: no multiple of 8
    assert norm_ops.layout(x.contiguous(memory_format=CL)[:, :8], 4) is None     # a channel slice: not dense
    assert norm_ops.layout(torch.zeros(2, 16, 35, dtype=torch.float16).transpose(1, 2), 4) is None  # not 4-D
    one = torch.zeros(2, 16, 1, 1, dtype=torch.float16)                          # both formats at once: NCHW by default
    assert norm_ops.layout(one, 4) == "nchw" and norm_ops.layout(one, 4, family="nhwc") == "nhwc"
    assert norm_ops.layout(x.contiguous(memory_format=CL), 4, family="nchw") is None


def test_a_cpu_or_non_channels_last_tensor_is_refused_before_any_launch(calls):
    from mi3d import _lib as L
    from mi3d import norm_ops
    w, b = torch.ones(16), torch.zeros(16)
    x = torch.zeros(2, 16, 5, 7, dtype=torch.float16)
    for bad in (x.contiguous(memory_format=CL), x, x.transpose(2, 3)):
        with pytest.raises(L.Mi3dError):
            norm_ops.forward(bad, w, b, 4, 1e-5)
        with pytest.raises(L.Mi3dError):
            norm_ops.forward(bad, w, b, 4, 1e-5, family="nhwc")
    assert calls == []


def test_span_queries_are_host_only():
    from mi3d import _lib
    lib = _lib.lib()
    span, spans = lib.mi3d_groupnorm_nhwc_span, lib.mi3d_groupnorm_nhwc_spans
    # 64 channels in 32 groups: one slab of 64 channels, spans of 8192 / 64 = 128 pixels
    assert (span(64, 1, 32), spans(64, 1, 32)) == (1, 1)
    assert (span(64, 128, 32), spans(64, 128, 32)) == (128, 1)
    assert (span(64, 129, 32), spans(64, 129, 32)) == (128, 2)
    # the VAE's largest activation: slabs of 64 channels = 16 groups; spans of sqrt(16 HW / 4) = 1024 pixels, so that a
    # workgroup merges 16 x 256 workspace entries for its 16 x as many elements
    assert (span(128, 512 * 512, 32), spans(128, 512 * 512, 32)) == (1024, 256)
    # 10 channels per group: slabs of lcm(10, 8) * 2 = 80 channels, spans of ceil(8192 / 80) = 103 pixels
    assert (span(320, 64 * 64, 32), spans(320, 64 * 64, 32)) == (103, 40)
    assert (span(256, 256 * 256, 32), spans(256, 256 * 256, 32)) == (363, 181)     # sqrt(16 * 65536 / 8) = 362.04
    for C, HW, G in ((12, 16, 4), (16, 16, 3), (0, 16, 4), (16, 0, 4), (16, 16, 0)):
        assert span(C, HW, G) == 0 and spans(C, HW, G) == 0          # refused: no multiple of 8, G does not divide C, null


def test_switches_convert_conv_weights_once_and_back():
    from mi3d import sd_standin as S
    torch.manual_seed(0)
    enc = S.VAEEncoderSD(ch=(32, 64))
    convs = [m for m in enc.modules() if isinstance(m, torch.nn.Conv2d)]
    before = [m.weight.detach().clone() for m in convs]
    assert not enc.channels_last
    enc.set_channels_last(True)
    assert enc.NHWC_EXCEPT == ("conv_in",) and enc.conv_in.weight.is_contiguous()     # the 3-channel layer stays NCHW
    assert enc.channels_last and all(m.weight.is_contiguous(memory_format=CL) for m in convs if m is not enc.conv_in)
    assert sum(not m.weight.is_contiguous() for m in convs) >= len(convs) - 4           # (1 x 1 weights are both)
    ptrs = [m.weight.data_ptr() for m in convs]
    enc.set_channels_last(True)                                      # no second conversion
    assert ptrs == [m.weight.data_ptr() for m in convs]
    x = torch.rand(1, 3, 16, 16)
    y_cl = enc(x)
    enc.set_channels_last(False)
    assert all(m.weight.is_contiguous() for m in convs)
    assert all(torch.equal(a, m.weight) for a, m in zip(before, convs))
    torch.testing.assert_close(y_cl, enc(x), rtol=1e-4, atol=1e-4)   # fp32 on the CPU: summation order only
