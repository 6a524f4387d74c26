"""CM = 64 two-group ping-pong half-block (csrc/kernels/conv_pair_pp64.inc): the host's
fragment-order weight packing, and the kernel against the fp32 oracle and, bit for bit, against the
one-group kernel that the same call takes at the default grid."""
import pytest
import torch

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine, to_nhwc_input
from bioengine_worker_amd.ops import conv_pair as cp
from bioengine_worker_amd.ops.conv import PackedConv

# configurations that run on the new kernel: Cin, CM, inmode, x2, proj, res
ENABLED = [
    (64, 64, "none", False, False, "full"),
    (32, 64, "pool2", False, False, "full"),
    (128, 64, "up2", True, False, "up2"),
]


def test_frag_configs_are_the_enabled_ones():
    assert sorted(cp.FRAG_CONFIGS) == sorted(ENABLED)
    assert all(c in cp.SUPPORTED for c in cp.FRAG_CONFIGS)


@pytest.mark.parametrize("cin", [32, 64, 128])
def test_pack_frag_maps_every_weight_to_the_lane_the_kernel_reads(cin):
    """The kernel's wave (channel-tile pair cp) reads, for K-step (chunk, tap) and ct in {0, 1},
    16 bytes per lane at element ((chunk * 9 + tap) * 4 + 2 cp + ct) * 512 + lane * 8.  As the MFMA's
    A operand, lane kq * 16 + lrow supplies output channel (2 cp + ct) * 16 + lrow and K indices
    kq * 8 .. kq * 8 + 7 = input channels chunk * 32 + kq * 8 + e."""
    g = torch.Generator().manual_seed(cin)
    w = torch.randn(64, cin, 3, 3, generator=g)
    pc = PackedConv.from_weight(w, None)
    wf = cp.pack_frag(pc.wp)
    assert wf.shape == (cin // 32, 9, 4, 64, 8) and wf.is_contiguous() and wf.dtype == pc.wp.dtype
    flat = wf.reshape(-1).float()
    co, ci, tap = torch.meshgrid(torch.arange(64), torch.arange(cin), torch.arange(9), indexing="ij")
    chunk, k = ci // 32, ci % 32
    kq, e = k // 8, k % 8
    cpair, ct, lrow = co // 32, (co // 16) % 2, co % 16
    lane = kq * 16 + lrow
    idx = ((chunk * 9 + tap) * 4 + 2 * cpair + ct) * 512 + lane * 8 + e
    assert idx.unique().numel() == flat.numel()  # a bijection onto the packed tensor
    want = w.to(torch.bfloat16).float()[co, ci, tap // 3, tap % 3]
    assert torch.equal(flat[idx], want)
    assert torch.equal(cp.unpack_frag(wf), pc.wp)


def test_spec_packs_fragments_once():
    pa = PackedConv.from_weight(torch.randn(64, 64, 3, 3), None)
    pb = PackedConv.from_weight(torch.randn(64, 64, 3, 3), None)
    z = torch.zeros(64)
    spec = cp.PairSpec(pa=pa, pb=pb, sa=z, ta=z, sb=z, tb=z, bias=z)
    assert spec.frag_cache is None
    a0, b0 = spec.frag(torch.device("cpu"))
    a1, b1 = spec.frag(torch.device("cpu"))
    assert a0 is a1 and b0 is b1
    assert torch.equal(cp.unpack_frag(a0), pa.wp) and torch.equal(cp.unpack_frag(b0), pb.wp)


def _spec(cin, cm, inmode, seed):
    g = torch.Generator().manual_seed(seed)
    wa = torch.randn(cm, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    wb = torch.randn(cm, cm, 3, 3, generator=g) / (cm * 9) ** 0.5
    ba, bb = 0.1 * torch.randn(cm, generator=g), 0.1 * torch.randn(cm, generator=g)
    sa, ta = 1 + 0.1 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    sb, tb = 1 + 0.1 * torch.randn(cm, generator=g), 0.1 * torch.randn(cm, generator=g)
    spec = cp.PairSpec(pa=PackedConv.from_weight(wa, ba), pb=PackedConv.from_weight(wb, bb), sa=sa.float(),
                       ta=ta.float(), sb=sb.float(), tb=cp.fold_bias(tb, sb, ba).float(), bias=bb.float(),
                       inmode=inmode)
    return spec, ba


@pytest.mark.gpu
@pytest.mark.parametrize("case", ENABLED)
@pytest.mark.parametrize("hw", [(48, 64), (30, 44)])
@pytest.mark.parametrize("per_image", [False, True])
def test_pp64_matches_reference_and_one_group_kernel(gpu, case, hw, per_image):
    """N = 3 with a 5-workgroup grid forces the ping-pong kernel (>= 2 tiles of 16 x 16 per workgroup)
    with uneven ranges, so an idle group's dummy tile runs; (48, 64) has a bounds-free interior tile,
    (30, 44) partial edge tiles only.  The default grid routes the same call to the one-group kernel."""
    from bioengine_worker_amd.ops import _native

    cin, cm, inmode, has_x2, proj, res = case
    assert not proj
    H, W = hw
    N = 3
    spec, ba = _spec(cin, cm, inmode, seed=21)
    g = torch.Generator().manual_seed(22)
    Hs, Ws = {"none": (H, W), "pool2": (2 * H, 2 * W), "up2": (H // 2, W // 2)}[inmode]
    x = torch.randn(N, Hs, Ws, cin, generator=g).bfloat16()
    x2 = torch.randn(N, H, W, cm, generator=g).bfloat16() if has_x2 else None
    r = torch.randn(*((N, H, W, cm) if res == "full" else (N, H // 2, W // 2, cm)), generator=g).bfloat16()
    ta = (0.1 * torch.randn(N, cin, generator=g)).float() if per_image else None
    tb = cp.fold_bias((0.1 * torch.randn(N, cm, generator=g)).float(), spec.sb, ba) if per_image else None
    ref = cp.conv_pair_ref(x, spec, ta=ta, tb=tb, x2=x2, res=r, res_mode=res).float()
    d = lambda t: None if t is None else t.to(gpu)
    gspec = cp.PairSpec(pa=spec.pa.to(gpu), pb=spec.pb.to(gpu), sa=d(spec.sa), ta=d(spec.ta), sb=d(spec.sb),
                        tb=d(spec.tb), bias=d(spec.bias), inmode=inmode)
    one = cp.conv_pair(d(x), gspec, ta=d(ta), tb=d(tb), x2=d(x2), res=d(r), res_mode=res).cpu()
    try:
        _native.call("be_conv_pair_set_grid", 5)
        out = cp.conv_pair(d(x), gspec, ta=d(ta), tb=d(tb), x2=d(x2), res=d(r), res_mode=res).cpu()
    finally:
        _native.call("be_conv_pair_set_grid", 0)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - ref).abs()
    tol = 1.5e-2 * max(1.0, ref.abs().max().item())
    print(f"pp64 {case} {hw} per_image={per_image}: max err {err.max().item():.4g} (tol {tol:.4g}), "
          f"differing from one-group: {(out != one).sum().item()}")
    assert err.max().item() < tol, f"max err {err.max().item()} (tol {tol}); at {torch.nonzero(err == err.max())[0].tolist()}"
    assert torch.equal(out, one)


@pytest.mark.gpu
def test_cpnet_engine_pp64_equals_default_grid(gpu):
    """3 x 224^2: at the default grid every pair call is too small for the ping-pong kernels; a
    5-workgroup grid puts the level-0 and level-1 pairs on them.  Same bits either way."""
    from bioengine_worker_amd.ops import _native

    torch.manual_seed(0)
    net = CPnet().randomize_(3).eval()
    xin = to_nhwc_input(torch.randn(3, 2, 224, 224), 8).to(gpu)
    eng = CPnetEngine(net, gpu)
    y0, s0 = eng(xin)
    y0, s0 = y0.cpu(), s0.cpu()
    try:
        _native.call("be_conv_pair_set_grid", 5)
        y1, s1 = eng(xin)
        y1, s1 = y1.cpu(), s1.cpu()
    finally:
        _native.call("be_conv_pair_set_grid", 0)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
