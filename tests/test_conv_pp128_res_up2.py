"""Half-resolution residual of the 128-channel ping-pong conv (csrc/kernels/conv_pp128.hip, epilogue
RES 2): the call that reads ``res[n, y >> 1, x >> 1]`` from an [N, H/2, W/2, 128] tensor against the
same call given that tensor expanded, bit for bit, and the 1x1 projection that feeds it at half
resolution against the one computed through the up2 input transform."""
import pytest
import torch

from bioengine_worker_amd.ops import conv as cv
from bioengine_worker_amd.ops.conv import PackedConv, fused_conv2d


def _expand(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()


def _conv(seed, cout=128, cin=128, ks=3):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    return PackedConv.from_weight(w, b)


def _inputs(seed, N, H, W):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, 128, generator=g).bfloat16()
    scale = (1 + 0.1 * torch.randn(128, generator=g)).float()
    shift = (0.1 * torch.randn(N, 384, generator=g)).float()  # per image, a column slice, as the style shifts
    res = torch.randn(N, H // 2, W // 2, 128, generator=g).bfloat16()
    return x, scale, shift, res


def test_cpu_up2_residual_is_the_expanded_residual():
    pc = _conv(5)
    x, scale, shift, res = _inputs(6, 2, 8, 12)
    sh = shift[:, 128:256]
    assert cv.pp128_takes_res_up2(pc, x)
    a = fused_conv2d(x, pc, scale=scale, shift=sh, relu=True, residual=res, residual_mode="up2")
    b = fused_conv2d(x, pc, scale=scale, shift=sh, relu=True, residual=_expand(res))
    assert torch.equal(a, b)
    with pytest.raises(AssertionError):
        fused_conv2d(x, pc, scale=scale, shift=sh, relu=True, residual=_expand(res), residual_mode="up2")


def _launches():
    from bioengine_worker_amd.ops import _native

    return int(_native.hip().be_conv_pp128_launches())


# (56, 56): the workload's size, every tile inside the image (the FULL epilogue); (20, 30): partial
# tiles in both directions (the per-pixel range checks), even but no multiple of the patch size
@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(56, 56), (20, 30)])
@pytest.mark.parametrize("relu", [False, True])
def test_up2_residual_equals_the_expanded_residual(gpu, hw, relu):
    """N = 3 on a forced grid of 5 workgroups (uneven ranges, a dummy tile): both calls run on
    conv_pp128_kernel and must give the same bits; at the default grid the native side declines."""
    from bioengine_worker_amd.ops import _native

    H, W = hw
    N = 3
    pc = _conv(51).to(gpu)
    x, scale, shift, res = (t.to(gpu) for t in _inputs(52, N, H, W))
    sh = shift[:, 128:256]
    assert not cv.pp128_takes_res_up2(pc, x), "no fragments yet: the call is not offered"
    pc.frag()
    assert not cv.pp128_takes_res_up2(pc, x), "42 tiles at most: the default grid keeps the per-layer kernel"
    n0 = _launches()
    try:
        _native.call("be_conv_pp128_set_grid", 5)
        assert cv.pp128_takes_res_up2(pc, x)
        assert not cv.pp128_takes_res_up2(pc, x[:, : H - 1]), "odd sizes have no half-resolution residual"
        full = fused_conv2d(x, pc, scale=scale, shift=sh, relu=relu, residual=_expand(res))
        half = fused_conv2d(x, pc, scale=scale, shift=sh, relu=relu, residual=res, residual_mode="up2")
        torch.cuda.synchronize()
    finally:
        _native.call("be_conv_pp128_set_grid", 0)
    assert _launches() - n0 == 2, "both calls must run on the ping-pong kernel"
    assert torch.isfinite(half.float()).all()
    assert (half != fused_conv2d(x, pc, scale=scale, shift=sh, relu=relu)).any(), "the residual must have been added"
    assert torch.equal(half, full)
    with pytest.raises(RuntimeError):  # default grid again: declined, and no other kernel has this mode
        fused_conv2d(x, pc, scale=scale, shift=sh, relu=relu, residual=res, residual_mode="up2")


@pytest.mark.gpu
def test_projection_at_half_resolution_expands_to_the_up2_projection(gpu):
    """up[2].proj: 1x1, 256 -> 128, no ReLU, 28^2 -> 56^2."""
    N = 3
    pc = _conv(61, 128, 256, 1).to(gpu)
    g = torch.Generator().manual_seed(62)
    x = torch.randn(N, 28, 28, 256, generator=g).bfloat16().to(gpu)
    scale = (1 + 0.1 * torch.randn(256, generator=g)).float().to(gpu)
    shift = (0.1 * torch.randn(256, generator=g)).float().to(gpu)
    lo = fused_conv2d(x, pc, scale=scale, shift=shift)
    hi = fused_conv2d(x, pc, scale=scale, shift=shift, inmode="up2")
    assert lo.shape == (N, 28, 28, 128) and hi.shape == (N, 56, 56, 128)
    assert torch.equal(_expand(lo), hi)
