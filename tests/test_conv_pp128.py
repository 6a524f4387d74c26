"""Two-group ping-pong 128 -> 128 3x3 conv (csrc/kernels/conv_pp128.hip): the host's fragment-order
weight packing and its caching, the kernel's LDS swizzle (modelled on the address formulas of the
source), and the kernel against the fp32 oracle and, bit for bit, against the per-layer kernel that
the same call takes at the default grid."""
import pytest
import torch

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine, to_nhwc_input
from bioengine_worker_amd.ops import conv as cv
from bioengine_worker_amd.ops.conv import PackedConv, fused_conv2d, fused_conv2d_ref

TH, TW, IW = 8, 28, 30  # the kernel's tile and the width of its LDS input image


def test_pack_frag_maps_every_weight_to_the_lane_the_kernel_reads():
    """The kernel's wave (channel-tile pair cp = 0..3) reads, for K-step (chunk, tap) and ct in {0, 1},
    16 bytes per lane at element ((chunk * 9 + tap) * 8 + 2 cp + ct) * 512 + lane * 8.  As the MFMA's
    A operand, lane kq * 16 + lrow supplies output channel (2 cp + ct) * 16 + lrow and K indices
    kq * 8 .. kq * 8 + 7 = input channels chunk * 32 + kq * 8 + e."""
    g = torch.Generator().manual_seed(128)
    w = torch.randn(128, 128, 3, 3, generator=g)
    pc = PackedConv.from_weight(w, None)
    assert cv.frag_eligible(pc)
    wf = cv.pack_frag(pc.wp)
    assert wf.shape == (4, 9, 8, 64, 8) and wf.is_contiguous() and wf.dtype == pc.wp.dtype
    flat = wf.reshape(-1).float()
    co, ci, tap = torch.meshgrid(torch.arange(128), torch.arange(128), torch.arange(9), indexing="ij")
    chunk, k = ci // 32, ci % 32
    kq, e = k // 8, k % 8
    cpair, ct, lrow = co // 32, (co // 16) % 2, co % 16
    lane = kq * 16 + lrow
    idx = ((chunk * 9 + tap) * 8 + 2 * cpair + ct) * 512 + lane * 8 + e
    assert idx.unique().numel() == flat.numel()  # a bijection onto the packed tensor
    want = w.to(torch.bfloat16).float()[co, ci, tap // 3, tap % 3]
    assert torch.equal(flat[idx], want)
    assert torch.equal(cv.unpack_frag(wf), pc.wp)


def test_pack_frag_agrees_with_the_pair_kernels_packing():
    from bioengine_worker_amd.ops import conv_pair as cp

    pc = PackedConv.from_weight(torch.randn(64, 64, 3, 3), None)
    assert torch.equal(cv.pack_frag(pc.wp), cp.pack_frag(pc.wp))


def test_fragments_are_packed_once_and_never_used_stale(monkeypatch):
    pc = PackedConv.from_weight(torch.randn(128, 128, 3, 3), None)
    assert pc.wf is None and pc.frag_built() is None  # nothing is packed behind a forward's back
    calls = []
    real = cv.pack_frag
    monkeypatch.setattr(cv, "pack_frag", lambda wp: calls.append(1) or real(wp))
    a = pc.frag()
    assert pc.frag() is a and pc.frag_built() is a and len(calls) == 1
    assert torch.equal(cv.unpack_frag(a), pc.wp)
    pc.to("cpu")
    assert pc.frag_built() is not None and len(calls) == 1
    pc.wp.mul_(2)  # the trainer rewrites wp in place: the fragments no longer describe it
    assert pc.frag_built() is None
    b = pc.frag()
    assert len(calls) == 2 and torch.equal(cv.unpack_frag(b), pc.wp)
    pc.refresh(torch.randn(128, 128, 3, 3))
    assert pc.wf is None and pc.frag_built() is None
    assert not cv.frag_eligible(PackedConv.from_weight(torch.randn(128, 64, 3, 3), None))
    assert not cv.frag_eligible(PackedConv.from_weight(torch.randn(128, 128, 1, 1), None))


def _commit_addr(y, x, c):
    """Byte address of 16-byte unit c of input-image pixel (y, x), as commit() writes it."""
    return (y * IW + x) * 64 + ((c ^ (((x >> 1) & 1) << 1)) << 4)


def _read_addr(lrow, kq, tap, j):
    """Byte address lane (lrow, kq) reads for fragment j at this tap, as mma_chunk() forms it."""
    dy, dx = tap // 3, tap % 3
    x = (lrow & 3) + dx
    a0 = ((lrow >> 2) * IW + x) * 64 + ((kq ^ (((x >> 1) & 1) << 1)) << 4)
    return a0 + ((4 * (j // 7) + dy) * IW + 4 * (j % 7)) * 64


def test_swizzle_reads_what_commit_wrote_without_bank_conflicts():
    """Every fragment read (14 fragments x 9 taps) addresses unit kq of pixel (4 fr + ly + dy,
    4 fc + lx + dx) where commit put it, stays inside the 10 x 30 image, and within each of the four
    ds_read_b128 lane groups the 16 lanes hit 16 distinct 16-byte bank slots."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]
    seen = set()
    for tap in range(9):
        for j in range(14):
            addr = {}
            for lane in range(64):
                lrow, kq = lane & 15, lane >> 4
                y, x = 4 * (j // 7) + (lrow >> 2) + tap // 3, 4 * (j % 7) + (lrow & 3) + tap % 3
                assert y < TH + 2 and x < TW + 2
                addr[lane] = _read_addr(lrow, kq, tap, j)
                assert addr[lane] == _commit_addr(y, x, kq)
                assert 0 <= addr[lane] and addr[lane] + 16 <= (TH + 2) * IW * 64
                seen.add((y, x))
            for g in groups:
                assert len({(addr[l] // 16) % 16 for l in g}) == 16, (tap, j)
    assert len(seen) == (TH + 2) * IW  # the reads cover the whole halo image
    # commit: the units of the image are a bijection onto its 16-byte slots
    slots = {_commit_addr(y, x, c) for y in range(TH + 2) for x in range(IW) for c in range(4)}
    assert len(slots) == (TH + 2) * IW * 4


def _conv(seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(128, 128, 3, 3, generator=g) / (128 * 9) ** 0.5
    b = 0.1 * torch.randn(128, generator=g)
    return PackedConv.from_weight(w, b)


def _launches():
    from bioengine_worker_amd.ops import _native

    return int(_native.hip().be_conv_pp128_launches())


def _run_both(gpu, pc, x, scale, shift, res, alias=False):
    """(per-layer kernel at the default grid, ping-pong kernel on a forced 5-workgroup grid)"""
    from bioengine_worker_amd.ops import _native

    d = lambda t: None if t is None else t.to(gpu)
    outs = []
    for grid in (0, 5):
        r = d(res)
        n0 = _launches()
        try:
            _native.call("be_conv_pp128_set_grid", grid)
            o = fused_conv2d(d(x), pc, scale=d(scale), shift=d(shift), relu=True, residual=r, out=r if alias else None)
        finally:
            _native.call("be_conv_pp128_set_grid", 0)
        assert _launches() - n0 == (1 if grid else 0), "the forced grid must reach the ping-pong kernel, the default not"
        outs.append(o.cpu())
    return outs


# (16, 56): exact tiles, the workload's width; (24, 60): an interior tile plus partial right-edge tiles;
# (12, 20): partial tiles in both directions only; (8, 8): narrower than one tile
SIZES = [(16, 56), (24, 60), (12, 20), (8, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_pp128_matches_reference_and_per_layer_kernel(gpu, hw, per_image, with_res):
    """N = 3 on a forced grid of 5 workgroups: uneven tile ranges, and a group without a tile runs its
    dummy tile.  The default grid routes the same call to conv2d_nhwc_kernel."""
    H, W = hw
    N = 3
    pc = _conv(31)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(N, H, W, 128, generator=g).bfloat16()
    scale = (1 + 0.1 * torch.randn(128, generator=g)).float()
    if per_image:  # a column slice of a wider tensor, as the style shifts arrive
        shift = (0.1 * torch.randn(N, 384, generator=g)).float()
    else:
        shift = (0.1 * torch.randn(128, generator=g)).float()
    res = torch.randn(N, H, W, 128, generator=g).bfloat16() if with_res else None
    sh_cpu = shift[:, 128:256] if per_image else shift
    ref = fused_conv2d_ref(x, pc, scale=scale, shift=sh_cpu, relu=True, residual=res).float()
    pc.to(gpu).frag()
    sh_gpu = shift.to(gpu)[:, 128:256] if per_image else shift.to(gpu)
    assert not per_image or not sh_gpu.is_contiguous()
    old, out = _run_both(gpu, pc, x, scale, sh_gpu, res)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - ref).abs()
    tol = 2e-2 * max(1.0, ref.abs().max().item())
    print(f"pp128 {hw} per_image={per_image} res={with_res}: max err {err.max().item():.4g} (tol {tol:.4g}), "
          f"differing from the per-layer kernel: {(out != old).sum().item()}")
    assert err.max().item() < tol, f"max err {err.max().item()} (tol {tol}); at {torch.nonzero(err == err.max())[0].tolist()}"
    assert torch.equal(out, old)


@pytest.mark.gpu
def test_pp128_out_may_alias_the_residual(gpu):
    H, W, N = 24, 60, 3
    pc = _conv(41)
    g = torch.Generator().manual_seed(42)
    x = torch.randn(N, H, W, 128, generator=g).bfloat16()
    scale = (1 + 0.1 * torch.randn(128, generator=g)).float()
    shift = (0.1 * torch.randn(128, generator=g)).float()
    res = torch.randn(N, H, W, 128, generator=g).bfloat16()
    ref = fused_conv2d_ref(x, pc, scale=scale, shift=shift, relu=True, residual=res).float()
    pc.to(gpu).frag()
    sep_old, sep_new = _run_both(gpu, pc, x, scale, shift.to(gpu), res)
    old, out = _run_both(gpu, pc, x, scale, shift.to(gpu), res, alias=True)
    assert torch.isfinite(out.float()).all()
    assert (out.float() - ref).abs().max().item() < 2e-2 * max(1.0, ref.abs().max().item())
    assert torch.equal(out, old) and torch.equal(out, sep_new) and torch.equal(sep_old, sep_new)


@pytest.mark.gpu
def test_cpnet_engine_pp128_equals_default_grid(gpu):
    """3 x 224^2: at the default grid the level-2 convs (56^2, 42 tiles) stay on the per-layer kernel;
    a 5-workgroup grid puts the six plain 128 -> 128 ones on the ping-pong kernel.  Same bits."""
    from bioengine_worker_amd.ops import _native

    torch.manual_seed(0)
    net = CPnet().randomize_(3).eval()
    xin = to_nhwc_input(torch.randn(3, 2, 224, 224), 8).to(gpu)
    eng = CPnetEngine(net, gpu)
    n0 = _launches()
    y0, s0 = eng(xin)
    y0, s0 = y0.cpu(), s0.cpu()
    assert _launches() == n0
    try:
        _native.call("be_conv_pp128_set_grid", 5)
        y1, s1 = eng(xin)
        y1, s1 = y1.cpu(), s1.cpu()
    finally:
        _native.call("be_conv_pp128_set_grid", 0)
    assert _launches() - n0 == 6
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
