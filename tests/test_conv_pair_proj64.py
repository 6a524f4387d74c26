"""Level-1 pool2 half-block with the block's 1x1 projection inside the CM = 64 ping-pong kernel
(csrc/kernels/conv_pair_pp64.inc, PROJ build): the host's projection fragment packing, an address
model of the projection's LDS image, the reference as a composition of the existing references, and
the fused launch against the two launches it replaces, bit for bit."""
import pytest
import torch

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine, to_nhwc_input
from bioengine_worker_amd.ops import conv_pair as cp
from bioengine_worker_amd.ops.conv import PackedConv, fused_conv2d_ref

CASE = (32, 64, "pool2", False, True, "none")
TS = 16  # the kernel's output tile edge: the projection's image is TS x TS pixels of 64 bytes


def test_the_configuration_is_registered_apart_from_the_fragment_ones():
    assert cp.PROJ_CONFIGS == {CASE}
    assert CASE in cp.SUPPORTED and CASE not in cp.FRAG_CONFIGS


def test_pack_proj_frag_maps_every_weight_to_the_lane_the_kernel_reads():
    """The kernel's wave (channel-tile pair cp) reads, for ct in {0, 1}, 16 bytes per lane at element
    (2 cp + ct) * 512 + lane * 8.  As the MFMA's A operand, lane kq * 16 + lrow supplies output channel
    (2 cp + ct) * 16 + lrow and K indices kq * 8 .. kq * 8 + 7 = input channels kq * 8 + e."""
    g = torch.Generator().manual_seed(7)
    w = torch.randn(64, 32, 1, 1, generator=g)
    pc = PackedConv.from_weight(w, None)
    assert pc.wp.shape == (64, 1, 32) and pc.ck == 32
    wf = cp.pack_proj_frag(pc.wp)
    assert wf.shape == (1, 4, 64, 8) and wf.is_contiguous() and wf.dtype == pc.wp.dtype
    flat = wf.reshape(-1).float()
    co, ci = torch.meshgrid(torch.arange(64), torch.arange(32), indexing="ij")
    kq, e = ci // 8, ci % 8
    cpair, ct, lrow = co // 32, (co // 16) % 2, co % 16
    lane = kq * 16 + lrow
    idx = (2 * cpair + ct) * 512 + lane * 8 + e
    assert idx.unique().numel() == flat.numel()  # a bijection onto the packed tensor
    assert torch.equal(flat[idx], w.to(torch.bfloat16).float()[co, ci, 0, 0])
    assert torch.equal(cp.unpack_proj_frag(wf), pc.wp)
    # one K-step of the 3x3 layout: the same lane order as pack_frag's
    w3 = torch.zeros(64, 32, 3, 3)
    w3[:, :, 0, 0] = w[:, :, 0, 0]
    assert torch.equal(cp.pack_frag(PackedConv.from_weight(w3, None).wp)[0, 0], wf[0])


def _p_commit_addr(y, x, c):
    """Byte address of 16-byte unit c of halo pixel (y, x), 2 <= y, x < 18, as commit() writes it to the
    projection's image (p_off(y - 2, x - 2, c))."""
    oy, ox = y - 2, x - 2
    return (oy * TS + ox) * 64 + ((c ^ ((((ox >> 2) ^ oy) & 1) << 1)) << 4)


def _p_read_addr(lrow, kq, ph, pt):
    """Byte address lane (lrow, kq) of pixel half ph reads for output row pt, as proj_res() forms it."""
    p0 = ((8 * ph * TS + lrow) * 64 + kq * 16) ^ (((lrow >> 2) & 1) << 5)
    return (p0 + pt * TS * 64) ^ ((pt & 1) << 5)


def test_projection_image_reads_what_commit_wrote_without_bank_conflicts():
    """Every fragment read (2 pixel halves x 8 rows) addresses unit kq of pixel (8 ph + pt, lrow) where
    commit put it and stays inside the 16 KB image; within each of the four ds_read_b128 lane groups
    the 16 lanes hit 16 distinct 16-byte bank slots; the commit's units are a bijection onto the image."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]
    seen = set()
    for ph in range(2):
        for pt in range(8):
            addr = {}
            for lane in range(64):
                lrow, kq = lane & 15, lane >> 4
                addr[lane] = _p_read_addr(lrow, kq, ph, pt)
                assert addr[lane] == _p_commit_addr(8 * ph + pt + 2, lrow + 2, kq)
                assert 0 <= addr[lane] and addr[lane] + 16 <= TS * TS * 64
                seen.add(addr[lane])
            for g in groups:
                assert len({(addr[l] // 16) % 16 for l in g}) == 16, (ph, pt)
    slots = {_p_commit_addr(y, x, c) for y in range(2, TS + 2) for x in range(2, TS + 2) for c in range(4)}
    assert len(slots) == TS * TS * 4 and slots == seen  # every commit store is read back, and nothing else


def _spec(seed, proj_bias=True):
    cin, cm = 32, 64
    g = torch.Generator().manual_seed(seed)
    wa = torch.randn(cm, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    wb = torch.randn(cm, cm, 3, 3, generator=g) / (cm * 9) ** 0.5
    wp = torch.randn(cm, cin, 1, 1, generator=g) / cin ** 0.5
    ba, bb, bp = (0.1 * torch.randn(cm, generator=g) for _ in range(3))
    sa, ta = 1 + 0.1 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    sb, tb = 1 + 0.1 * torch.randn(cm, generator=g), 0.1 * torch.randn(cm, generator=g)
    sp, tp = 1 + 0.1 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    spec = cp.PairSpec(pa=PackedConv.from_weight(wa, ba), pb=PackedConv.from_weight(wb, bb), sa=sa.float(),
                       ta=ta.float(), sb=sb.float(), tb=cp.fold_bias(tb, sb, ba).float(), bias=bb.float(),
                       inmode="pool2", pp=PackedConv.from_weight(wp, bp if proj_bias else None), sp=sp.float(),
                       tp=tp.float(), bias_p=(bp if proj_bias else torch.zeros(cm)).float())
    return spec, ba


def _inputs(seed, N, H, W, per_image, spec, ba):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 2 * H, 2 * W, 32, generator=g).bfloat16()
    ta = (0.1 * torch.randn(N, 32, generator=g)).float() if per_image else None
    tb = cp.fold_bias((0.1 * torch.randn(N, 64, generator=g)).float(), spec.sb, ba) if per_image else None
    return x, ta, tb


@pytest.mark.parametrize("proj_bias", [True, False])
def test_reference_is_the_composition_of_the_existing_references(proj_bias):
    spec, ba = _spec(11, proj_bias)
    assert spec.supports(False, "none") and spec.proj_rounded(False, "none")
    x, ta, tb = _inputs(12, 2, 10, 12, True, spec, ba)
    plain = cp.PairSpec(pa=spec.pa, pb=spec.pb, sa=spec.sa, ta=spec.ta, sb=spec.sb, tb=spec.tb, bias=spec.bias,
                        inmode="pool2")
    proj = fused_conv2d_ref(x, spec.pp, scale=spec.sp, shift=spec.tp, inmode="pool2")
    want = cp.conv_pair_ref(x, plain, ta=ta, tb=tb, res=proj, res_mode="full")
    assert torch.equal(cp.conv_pair_ref(x, spec, ta=ta, tb=tb), want)
    assert torch.equal(cp.conv_pair(x, spec, ta=ta, tb=tb), want)  # the CPU path
    assert not cp.proj_fused(x, spec)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(48, 64), (30, 44)])
@pytest.mark.parametrize("per_image", [False, True])
def test_fused_projection_equals_the_two_launches(gpu, hw, per_image):
    """N = 3 with a 5-workgroup grid (test_conv_pair_pp64.py's shapes: an interior tile, partial edge
    tiles only, uneven ranges with a dummy tile): one launch with the projection inside.  At the default
    grid the same call is the per-layer projection and the one-group pair kernel.  Same bits, and both
    within the pp64 test's tolerance of the oracle."""
    from bioengine_worker_amd.ops import _native

    H, W = hw
    N = 3
    spec, ba = _spec(21)
    x, ta, tb = _inputs(22, N, H, W, per_image, spec, ba)
    ref = cp.conv_pair_ref(x, spec, ta=ta, tb=tb).float()
    d = lambda t: None if t is None else t.to(gpu)
    gspec = cp.PairSpec(pa=spec.pa.to(gpu), pb=spec.pb.to(gpu), sa=d(spec.sa), ta=d(spec.ta), sb=d(spec.sb),
                        tb=d(spec.tb), bias=d(spec.bias), inmode="pool2", pp=spec.pp.to(gpu), sp=d(spec.sp),
                        tp=d(spec.tp), bias_p=d(spec.bias_p))
    xg = d(x)
    assert not cp.proj_fused(xg, gspec), "36 tiles at most: the default grid keeps the two launches"
    two = cp.conv_pair(xg, gspec, ta=d(ta), tb=d(tb)).cpu()
    try:
        _native.call("be_conv_pair_set_grid", 5)
        assert cp.proj_fused(xg, gspec)
        out = cp.conv_pair(xg, gspec, ta=d(ta), tb=d(tb)).cpu()
        _native.call("be_conv_pair_set_proj_fusion", 0)  # the A/B switch: the pair on pp64, the projection apart
        assert not cp.proj_fused(xg, gspec)
        off = cp.conv_pair(xg, gspec, ta=d(ta), tb=d(tb)).cpu()
    finally:
        _native.call("be_conv_pair_set_proj_fusion", 1)
        _native.call("be_conv_pair_set_grid", 0)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - ref).abs()
    tol = 1.5e-2 * max(1.0, ref.abs().max().item())
    print(f"proj64 {hw} per_image={per_image}: max err {err.max().item():.4g} (tol {tol:.4g}), "
          f"differing from the two launches: {(out != two).sum().item()}")
    assert err.max().item() < tol, f"max err {err.max().item()} (tol {tol}); at {torch.nonzero(err == err.max())[0].tolist()}"
    assert torch.equal(out, two)
    assert torch.equal(off, two)


@pytest.mark.gpu
def test_cpnet_engine_fused_projection_on_equals_off(gpu):
    """3 x 224^2 on a 5-workgroup grid: the level-1 pool2 half-block with the projection inside against
    the same forward with the fusion switched off."""
    from bioengine_worker_amd.ops import _native

    torch.manual_seed(0)
    net = CPnet().randomize_(3).eval()
    xin = to_nhwc_input(torch.randn(3, 2, 224, 224), 8).to(gpu)
    eng = CPnetEngine(net, gpu)
    assert eng.pair[("down", 1, 0)].bias_p is not None
    try:
        _native.call("be_conv_pair_set_grid", 5)
        assert int(_native.hip().be_conv_pair_proj_takes(3, 112, 112)) == 1
        y1, s1 = eng(xin)
        y1, s1 = y1.cpu(), s1.cpu()
        _native.call("be_conv_pair_set_proj_fusion", 0)
        assert int(_native.hip().be_conv_pair_proj_takes(3, 112, 112)) == 0
        y0, s0 = eng(xin)
        y0, s0 = y0.cpu(), s0.cpu()
    finally:
        _native.call("be_conv_pair_set_proj_fusion", 1)
        _native.call("be_conv_pair_set_grid", 0)
    assert torch.isfinite(y1).all()
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
