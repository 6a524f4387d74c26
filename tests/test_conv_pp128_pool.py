"""Pooled-input build of the 128-channel ping-pong conv (csrc/kernels/conv_pp128.hip, POOL / PROJ):
CPnet's level-2 entry conv (3x3, 64 -> 128, 2x2 max-pool in the loader) and the residual projection
of the same pooled pixels (1x1, 64 -> 128, no ReLU) in one launch, bit for bit against the two
launches of the per-layer kernel; the host's fragment order of both weight tensors; the size rule."""
import pytest
import torch

from bioengine_worker_amd.ops import conv as cv
from bioengine_worker_amd.ops.conv import PackedConv, fused_conv2d


def _conv(seed, cout, cin, ks):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    return PackedConv.from_weight(w, b), w


def test_pack_frag_of_the_two_chunk_conv():
    """The pooled build's wave (channel-tile pair cp) reads, for K-step (chunk, tap) and ct in {0, 1}, 16
    bytes per lane at element ((chunk * 9 + tap) * 8 + 2 cp + ct) * 512 + lane * 8; lane kq * 16 + lrow
    supplies output channel (2 cp + ct) * 16 + lrow, input channels chunk * 32 + kq * 8 + e."""
    pc, w = _conv(64, 128, 64, 3)
    assert cv.frag_eligible_pool(pc) and not cv.frag_eligible(pc) and not cv.frag_eligible_proj(pc)
    wf = pc.frag()
    assert wf.shape == (2, 9, 8, 64, 8) and wf.is_contiguous() and wf.dtype == torch.bfloat16
    flat = wf.reshape(-1).float()
    co, ci, tap = torch.meshgrid(torch.arange(128), torch.arange(64), torch.arange(9), indexing="ij")
    chunk, k = ci // 32, ci % 32
    kq, e = k // 8, k % 8
    cpair, ct, lrow = co // 32, (co // 16) % 2, co % 16
    idx = ((chunk * 9 + tap) * 8 + 2 * cpair + ct) * 512 + (kq * 16 + lrow) * 8 + e
    assert idx.unique().numel() == flat.numel()
    assert torch.equal(flat[idx], w.to(torch.bfloat16).float()[co, ci, tap // 3, tap % 3])


@pytest.mark.parametrize("ck1", ["64", "32"])
def test_pack_frag_1x1_of_the_projection(monkeypatch, ck1):
    """The projection's K-step s reads element (s * 8 + 2 cp + ct) * 512 + lane * 8 per lane; lane
    kq * 16 + lrow supplies output channel (2 cp + ct) * 16 + lrow, input channels s * 32 + kq * 8 + e,
    whichever chunk width the per-layer kernel's packing has."""
    monkeypatch.setenv("BE_CONV_CK1", ck1)
    pc, w = _conv(65, 128, 64, 1)
    assert pc.ck == int(ck1)
    assert cv.frag_eligible_proj(pc) and not cv.frag_eligible(pc) and not cv.frag_eligible_pool(pc)
    wf = pc.frag()
    assert pc.frag() is wf and pc.frag_built() is wf
    assert wf.shape == (2, 8, 64, 8) and wf.is_contiguous() and wf.dtype == torch.bfloat16
    flat = wf.reshape(-1).float()
    co, ci = torch.meshgrid(torch.arange(128), torch.arange(64), indexing="ij")
    s, k = ci // 32, ci % 32
    kq, e = k // 8, k % 8
    cpair, ct, lrow = co // 32, (co // 16) % 2, co % 16
    idx = (s * 8 + 2 * cpair + ct) * 512 + (kq * 16 + lrow) * 8 + e
    assert idx.unique().numel() == flat.numel()
    assert torch.equal(flat[idx], w.to(torch.bfloat16).float()[co, ci, 0, 0])


TH, TW = 8, 28


def _proj_commit_addr(y, x, u):
    """Byte address of 16-byte unit u (8 channels) of centre pixel (y, x), as commit_proj() writes it."""
    return (y * TW + x) * 128 + ((u ^ (((x >> 1) & 1) << 1) ^ ((y & 1) << 2)) << 4)


def _proj_read_addr(lrow, kq, s, j):
    """Byte address lane (lrow, kq) reads for fragment j of K-step s, as proj_mma() forms it."""
    ly, lx = lrow >> 2, lrow & 3
    p0 = (ly * TW + lx) * 128 + ((kq ^ (((lx >> 1) & 1) << 1) ^ ((ly & 1) << 2)) << 4)
    return (p0 ^ (s << 6)) + (4 * (j // 7) * TW + 4 * (j % 7)) * 128


def test_projection_image_reads_what_commit_wrote_without_bank_conflicts():
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]
    seen = set()
    for s in range(2):
        for j in range(14):
            addr = {}
            for lane in range(64):
                lrow, kq = lane & 15, lane >> 4
                y, x = 4 * (j // 7) + (lrow >> 2), 4 * (j % 7) + (lrow & 3)
                addr[lane] = _proj_read_addr(lrow, kq, s, j)
                assert addr[lane] == _proj_commit_addr(y, x, 4 * s + kq)
                assert 0 <= addr[lane] and addr[lane] + 16 <= TH * TW * 128
                seen.add((y, x, 4 * s + kq))
            for g in groups:
                assert len({(addr[l] // 16) % 16 for l in g}) == 16, (s, j)
    assert len(seen) == TH * TW * 8
    slots = {_proj_commit_addr(y, x, u) for y in range(TH) for x in range(TW) for u in range(8)}
    assert len(slots) == TH * TW * 8


# ---------------------------------------------------------------------------------------------- GPU


def _native():
    from bioengine_worker_amd.ops import _native as n

    return n


def _pool_launches():
    return int(_native().hip().be_conv_pp128_pool_launches())


def _launches():
    return int(_native().hip().be_conv_pp128_launches())


class _Level:
    """Random level-2 entry: c0 (3x3, ReLU), proj (1x1, no ReLU), c1 (3x3 128 -> 128), affines, biases."""

    def __init__(self, gpu, seed):
        g = torch.Generator().manual_seed(seed)
        self.c0 = _conv(seed + 1, 128, 64, 3)[0].to(gpu)
        self.pj = _conv(seed + 2, 128, 64, 1)[0].to(gpu)
        self.c1 = _conv(seed + 3, 128, 128, 3)[0].to(gpu)
        self.s0 = (1 + 0.2 * torch.randn(64, generator=g)).float().to(gpu)
        self.t0 = (0.3 * torch.randn(64, generator=g)).float().to(gpu)
        self.sp = (1 + 0.2 * torch.randn(64, generator=g)).float().to(gpu)
        self.tp = (0.3 * torch.randn(64, generator=g)).float().to(gpu)
        self.s1 = (1 + 0.2 * torch.randn(128, generator=g)).float().to(gpu)
        self.t1 = (0.3 * torch.randn(128, generator=g)).float().to(gpu)

    def frag(self):
        self.c0.frag(), self.pj.frag(), self.c1.frag()


def _source(gpu, seed, N, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 2 * H, 2 * W, 64, generator=g).bfloat16().to(gpu)  # negative values too


# output H x W (the source is twice that), N, forced grid, per-image shift rows on c0:
# one tile with every border, the other group on a dummy tile; partial tiles on both axes (the FULL =
# false epilogue, masked stores of both outputs); uneven tile ranges over 5 workgroups; per-image shifts
CASES = [(1, 8, 28, 5, False), (1, 10, 30, 5, False), (3, 56, 56, 5, False), (2, 16, 56, 3, True)]


@pytest.fixture(scope="module")
def level(gpu):
    lv = _Level(gpu, 700)
    lv.frag()
    return lv


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_g%d_%s" % (c[0], c[1], c[2], c[3], "rows" if c[4] else "shared"))
def test_pool_proj_launch_equals_the_two_per_layer_launches(gpu, level, case):
    N, H, W, grid, rows = case
    lv = level
    x = _source(gpu, 710 + H, N, H, W)
    if rows:  # a column slice of a wider tensor: pshift_ns != 0
        g = torch.Generator().manual_seed(720)
        t0 = (0.3 * torch.randn(N, 192, generator=g)).float().to(gpu)[:, 64:128]
        assert not t0.is_contiguous()
    else:
        t0 = lv.t0
    # today's launches, at the default grid: the per-layer kernel
    n0, p0 = _launches(), _pool_launches()
    assert not cv.pp128_takes_pool_proj(lv.c0, lv.pj, x) and not cv.pp128_takes_pool(lv.c0, x)
    h_old = fused_conv2d(x, lv.c0, scale=lv.s0, shift=t0, relu=True, inmode="pool2")
    p_old = fused_conv2d(x, lv.pj, scale=lv.sp, shift=lv.tp, inmode="pool2")
    y_old = fused_conv2d(h_old, lv.c1, scale=lv.s1, shift=lv.t1, relu=True, residual=p_old)
    assert (_launches(), _pool_launches()) == (n0, p0), "the default grid keeps these sizes on the per-layer kernel"
    nat = _native()
    try:
        nat.call("be_conv_pp128_set_grid", grid)
        assert cv.pp128_takes_pool_proj(lv.c0, lv.pj, x) and cv.pp128_takes_pool(lv.c0, x)
        h_new, p_new = cv.fused_conv2d_pool_proj(x, lv.c0, lv.pj, scale=lv.s0, shift=t0, relu=True, proj_scale=lv.sp,
                                                 proj_shift=lv.tp)
        assert _pool_launches() - p0 == 1 and _launches() == n0
        h_solo = fused_conv2d(x, lv.c0, scale=lv.s0, shift=t0, relu=True, inmode="pool2")  # the build without PROJ
        assert _pool_launches() - p0 == 2 and _launches() == n0
        y_new = fused_conv2d(h_new, lv.c1, scale=lv.s1, shift=lv.t1, relu=True, residual=p_new)
        assert _launches() - n0 == 1, "the 128 -> 128 path still takes the calls it took"
        torch.cuda.synchronize()
    finally:
        nat.call("be_conv_pp128_set_grid", 0)
    assert h_new.shape == p_new.shape == (N, H, W, 128)
    assert torch.isfinite(h_new.float()).all() and torch.isfinite(p_new.float()).all()
    assert (p_new.float() < 0).any() and (h_old != p_old).any()
    print(f"pool_proj {case}: c0 differing {(h_new != h_old).sum().item()}, proj differing {(p_new != p_old).sum().item()}, "
          f"c0 alone differing {(h_solo != h_old).sum().item()}, c1 differing {(y_new != y_old).sum().item()}")
    assert torch.equal(h_new, h_old)
    assert torch.equal(p_new, p_old)
    assert torch.equal(h_solo, h_old)
    assert torch.equal(y_new, y_old)


@pytest.mark.gpu
def test_size_rule_and_no_launch_when_it_says_no(gpu, level):
    lv = level
    nat = _native()
    lib = nat.hip()
    # a 9-tile batch (one 512^2 image) at level 2: 9 x 112^2 source, 126 tiles of 8 x 28, grid unforced
    assert lib.be_conv_pp128_takes_pool_proj(9, 112, 112) == 0 and lib.be_conv_pp128_takes_pool(9, 112, 112) == 0
    assert lib.be_conv_pp128_takes_pool_proj(37, 112, 112) == 1  # 518 tiles: two per group of 256 workgroups
    x = _source(gpu, 730, 2, 16, 28)
    assert not cv.pp128_takes_pool_proj(lv.c0, lv.pj, x)
    p0, n0 = _pool_launches(), _launches()
    h = fused_conv2d(x, lv.c0, scale=lv.s0, shift=lv.t0, relu=True, inmode="pool2")  # stays on the per-layer kernel
    with pytest.raises(RuntimeError):  # asked anyway: an error code, nothing launched
        cv.fused_conv2d_pool_proj(x, lv.c0, lv.pj, scale=lv.s0, shift=lv.t0, relu=True, proj_scale=lv.sp, proj_shift=lv.tp)
    assert (_pool_launches(), _launches()) == (p0, n0)
    try:
        nat.call("be_conv_pp128_set_grid", 4)
        assert cv.pp128_takes_pool_proj(lv.c0, lv.pj, x)
        for odd in (x[:, :31].contiguous(), x[:, :, :55].contiguous()):  # odd source height / width
            N, Hs, Ws, _ = odd.shape
            assert lib.be_conv_pp128_takes_pool_proj(N, Hs, Ws) == 0 and not cv.pp128_takes_pool_proj(lv.c0, lv.pj, odd)
            ho = fused_conv2d(odd, lv.c0, scale=lv.s0, shift=lv.t0, relu=True, inmode="pool2")
            assert ho.shape == (N, Hs // 2, Ws // 2, 128)
        assert (_pool_launches(), _launches()) == (p0, n0)
        # a conv without its fragments is not offered
        bare = _conv(741, 128, 64, 3)[0].to(gpu)
        assert not cv.pp128_takes_pool_proj(bare, lv.pj, x) and not cv.pp128_takes_pool(bare, x)
        hb = fused_conv2d(x, bare, scale=lv.s0, shift=lv.t0, relu=True, inmode="pool2")
        assert (_pool_launches(), _launches()) == (p0, n0) and hb.shape == h.shape
    finally:
        nat.call("be_conv_pp128_set_grid", 0)
