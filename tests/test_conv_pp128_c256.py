"""256-channel build of the 128-channel ping-pong conv (csrc/kernels/conv_pp128.hip, C256): CPnet's
level-3 entry conv (3x3, 128 -> 256, post-activated for its consumer) on the source pooled once by
be_pool2_nhwc, bit for bit against the per-layer kernel reading the source through its pooled-input
loader; integer data against the float64 model; the host's per-half fragment order; the size rule and
the launch counters."""
import copy

import pytest
import torch

import conv_exact_cases as cx
from bioengine_worker_amd.ops import conv as cv
from bioengine_worker_amd.ops.conv import PackedConv, fused_conv2d


def _conv(seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(256, 128, 3, 3, generator=g) / (128 * 9) ** 0.5
    b = 0.1 * torch.randn(256, generator=g) if bias else None
    return PackedConv.from_weight(w, b), w


def test_pack_frag_c256_maps_every_weight_to_the_lane_that_reads_it():
    """Work item half h, wave cp, K-step (chunk, tap), ct in {0, 1}: 16 bytes per lane at element
    h * 4 * 9 * 4096 + ((chunk * 9 + tap) * 8 + 2 cp + ct) * 512 + lane * 8; lane kq * 16 + lrow supplies
    output channel 128 h + (2 cp + ct) * 16 + lrow, input channels chunk * 32 + kq * 8 + e."""
    pc, w = _conv(90)
    assert cv.frag_eligible_c256(pc) and not cv.frag_eligible(pc) and not cv.frag_eligible_pool(pc)
    assert (pc.ck, pc.tco, pc.cin_pad, pc.cout_pad) == (32, 64, 128, 256)
    wf = pc.frag()
    assert pc.frag() is wf and pc.frag_built() is wf
    assert wf.shape == (2, 4, 9, 8, 64, 8) and wf.is_contiguous() and wf.dtype == torch.bfloat16
    flat = wf.reshape(-1).float()
    co, ci, tap = torch.meshgrid(torch.arange(256), torch.arange(128), torch.arange(9), indexing="ij")
    half, c = co // 128, co % 128
    chunk, k = ci // 32, ci % 32
    kq, e = k // 8, k % 8
    cpair, ct, lrow = c // 32, (c // 16) % 2, c % 16
    idx = half * (4 * 9 * 8 * 512) + ((chunk * 9 + tap) * 8 + 2 * cpair + ct) * 512 + (kq * 16 + lrow) * 8 + e
    assert idx.unique().numel() == flat.numel()
    assert torch.equal(flat[idx], w.to(torch.bfloat16).float()[co, ci, tap // 3, tap % 3])
    # each half is the 128 -> 128 packing of its rows
    assert torch.equal(wf[1], cv.pack_frag(pc.wp[128:]))


#: the integer-data case: pooled 12 x 30 (partial tiles on both axes), shared post-activation, ReLU
EXACT = cx.Case("pp128_c256_pool_12x30", cin=128, cout=256, H=12, W=30, inmode="pool2", shift="strided", post="shared",
                post_relu=True, rounds=True, tmpl=(32, 64), seed=720)


def test_integer_case_is_exact_on_the_model():
    d = cx.make(EXACT)
    st = cx.check_exactness(d)
    print(f"{EXACT.name}: {st}")
    assert torch.equal(cx.run(d), cx.ref64(d)), "the CPU path on the same data"


# ---------------------------------------------------------------------------------------------- GPU


def _native():
    from bioengine_worker_amd.ops import _native as n

    return n


def _counts():
    lib = _native().hip()
    return (int(lib.be_conv_pp128_c256_launches()), int(lib.be_conv_pp128_launches()), int(lib.be_conv_pp128_pool_launches()))


class _Entry:
    def __init__(self, gpu, seed, bias):
        g = torch.Generator().manual_seed(seed)
        self.pc = _conv(seed + 1, bias)[0].to(gpu)
        self.pc.frag()
        self.bare = _conv(seed + 1, bias)[0].to(gpu)  # no fragments: always the per-layer kernel
        self.s0 = (1 + 0.2 * torch.randn(128, generator=g)).float().to(gpu)
        self.t0 = (0.3 * torch.randn(128, generator=g)).float().to(gpu)
        self.qs = (1 + 0.2 * torch.randn(256, generator=g)).float().to(gpu)
        self.qt = (0.3 * torch.randn(256, generator=g)).float().to(gpu)


@pytest.fixture(scope="module")
def entries(gpu):
    return {True: _Entry(gpu, 800, True), False: _Entry(gpu, 810, False)}


def _source(gpu, seed, N, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 2 * H, 2 * W, 128, generator=g).bfloat16().to(gpu)


# pooled sizes: CPnet's level 3 (four tile rows, the last with four valid rows); one exact tile; partial
# tiles on both axes.  N = 3 on 5 workgroups: uneven item ranges, odd ranges (an idle group's dummy item),
# a range that starts on the second half of a tile.
SIZES = [(28, 28), (8, 28), (12, 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_pool_then_c256_equals_the_pooled_input_per_layer_launch(gpu, entries, size, bias):
    H, W = size
    N = 3
    en = entries[bias]
    x = _source(gpu, 820 + H, N, H, W)
    kw = dict(scale=en.s0, shift=en.t0, relu=True, post_scale=en.qs, post_shift=en.qt, post_relu=True)
    c0 = _counts()
    old = fused_conv2d(x, en.bare, inmode="pool2", **kw)
    pooled = cv.pool2_nhwc(x)
    # at the default grid so small a call is not taken: the rule answers 0, asking anyway is an error
    assert not cv.pp128_takes_c256(en.pc, pooled) and not cv.pp128_takes_prepool(en.pc, x)
    with pytest.raises(RuntimeError):
        cv.fused_conv2d_c256(pooled, en.pc, **kw)
    assert _counts() == c0, "nothing launched, no counter moved"
    nat = _native()
    try:
        nat.call("be_conv_pp128_set_grid", 5)
        assert cv.pp128_takes_c256(en.pc, pooled) and cv.pp128_takes_prepool(en.pc, x)
        new = cv.fused_conv2d_c256(pooled, en.pc, **kw)
        assert _counts() == (c0[0] + 1, c0[1], c0[2]), "the launch counts on its own counter only"
        per_layer = fused_conv2d(pooled, en.pc, nw=8, **kw)  # the pre-pooled route without the new build
        assert _counts() == (c0[0] + 1, c0[1], c0[2])
        nat.call("be_conv_pp128_set_c256", 1, 0)
        assert not cv.pp128_takes_c256(en.pc, pooled) and cv.pp128_takes_prepool(en.pc, x)
        nat.call("be_conv_pp128_set_c256", 0, 1)
        assert not cv.pp128_takes_c256(en.pc, pooled) and not cv.pp128_takes_prepool(en.pc, x)
        torch.cuda.synchronize()
    finally:
        nat.call("be_conv_pp128_set_c256", 1, 1)
        nat.call("be_conv_pp128_set_grid", 0)
    assert new.shape == (N, H, W, 256) and new.dtype == torch.bfloat16
    assert torch.isfinite(new.float()).all() and (new.float() > 0).any() and (new.float() == 0).any()
    print(f"c256 {size} bias={bias}: differing {(new != old).sum().item()}, pre-pooled per-layer differing "
          f"{(per_layer != old).sum().item()}")
    assert torch.equal(new, old)
    assert torch.equal(per_layer, old)


@pytest.mark.gpu
def test_c256_integer_data_equals_the_float64_model(gpu):
    d = cx.make(EXACT)
    want = cx.ref64(d)
    assert torch.equal(cx.run(d, gpu), want), "the per-layer kernel on this case"
    pc = copy.copy(d.pc).to(gpu)
    pc.frag()
    shift = d.shift._base.to(gpu)[:, d.shift.shape[1]:2 * d.shift.shape[1]]  # stays a column slice
    assert not shift.is_contiguous()
    nat = _native()
    c0 = _counts()
    try:
        nat.call("be_conv_pp128_set_grid", 5)
        pooled = cv.pool2_nhwc(d.x.to(gpu))
        got = cv.fused_conv2d_c256(pooled, pc, scale=d.scale.to(gpu), shift=shift, relu=True,
                                   post_scale=d.post_scale.to(gpu), post_shift=d.post_shift.to(gpu), post_relu=True)
        torch.cuda.synchronize()
    finally:
        nat.call("be_conv_pp128_set_grid", 0)
    assert _counts() == (c0[0] + 1, c0[1], c0[2])
    cx.assert_exact(got.cpu(), want, EXACT.name, th=8)


@pytest.mark.gpu
def test_c256_size_rule(gpu):
    lib = _native().hip()
    # a 9-tile batch (one 512^2 image) at level 3: 9 x 28^2, 36 tiles of 8 x 28, 72 items; grid unforced
    assert lib.be_conv_pp128_takes_c256(9, 28, 28) == 0 and lib.be_conv_pp128_takes_prepool(9, 28, 28) == 0
    assert lib.be_conv_pp128_takes_c256(63, 28, 28) == 0  # 504 items
    assert lib.be_conv_pp128_takes_c256(64, 28, 28) == 1  # 512 items: two per group of 256 workgroups
    assert lib.be_conv_pp128_takes_c256(288, 28, 28) == 1 and lib.be_conv_pp128_takes_prepool(288, 28, 28) == 1
    assert lib.be_conv_pp128_takes_c256(64, 2048, 2048) == 0  # an image of 2^31 bytes and more
