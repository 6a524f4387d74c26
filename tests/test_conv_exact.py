"""The CPU side of the exact integer-data conv tests (``conv_exact_cases``): the preconditions under
which equality may be demanded, the CPU path of every conv entry point against the independent float64
model, proof that the comparison catches local faults, and the tap map.

What the old rule of ``test_conv_gpu.py`` (``max|out - ref| < 2e-2 * max(1, max|ref|)``, Gaussian data,
N = 2, per-image shift, residual) makes of the same six faults, largest error against the tolerance:

    fault                  3x3 256->256 16x16   3x3 32->32 64x64   3x3 32->64 13x45
    tolerance              0.106                0.114              0.104
    truncate               0.031  passes        0.031  passes      0.031  passes
    corner_act0            0.086  passes        0.055  passes      0.066  passes
    drop_product           0.295 (*)            0.344 (*)          0.486 (*)
    shift_of_image0        0.454                0.355              0.395
    zero_channel_group     0.148                0.164              0.330
    residual_next_column   (one tile wide)      4.47               4.97

(*) the largest of the K products at that pixel; a typical one is about 0.02 and passes.  Truncation
and the padding slip pass everywhere; on the integer data below every one of the six breaks equality.
"""
import pytest
import torch

import conv_exact_cases as ce
from bioengine_worker_amd.ops.conv import fused_conv2d, fused_conv2d_concat
from bioengine_worker_amd.ops.conv3d import conv3d_ref, fused_conv3d, fused_conv3d_concat

NAMES = [c.name for c in ce.cases()]


def test_case_list_size_and_template_coverage():
    cs = ce.cases()
    assert 100 <= len(cs) <= 150
    for c in cs:
        assert c.H <= 40 and c.W <= 72
    seen = {(c.ks, ce.data(c.name).pc.ck, ce.data(c.name).pc.tco) for c in cs if not c.head}
    for ks, cks in ((3, (8, 32)), (1, (8, 32, 64))):
        for ck in cks:
            for tco in (16, 32, 64):
                assert (ks, ck, tco) in seen, (ks, ck, tco)
    for tco in (32, 64):
        for nw in (4, 8):
            for inmode in ("none", "up2", "pool2"):
                assert any(c.nw == nw and c.inmode == inmode and ce.data(c.name).pc.tco == tco for c in cs)
            assert any(c.nw == nw and c.x2 and ce.data(c.name).pc.tco == tco for c in cs)


def test_rounding_cases_reach_every_store_path():
    """Ties and halves go through the staged stores of both kernels, the unstaged stores at every tco,
    both casts of the post-affine path, and the persistent kernel's cross-tile loop."""
    r = [c for c in ce.cases() if c.rounds]
    tco = lambda c: ce.data(c.name).pc.tco
    for t in (32, 64):
        assert any(tco(c) == t and c.cout % 8 == 0 for c in r)
        assert any(tco(c) == t and c.post is not None for c in r)
    for t in (16, 32, 64):
        assert any(tco(c) == t and c.cout % 8 for c in r)
    assert any(c.persist and c.cin > 32 for c in r)
    assert any(c.cout % 8 and c.post is not None for c in r)
    ties = 0
    for c in r[:4]:
        y = ce.presum(ce.data(c.name))
        ties += int(((y.abs() > 128) & (y.abs() < 256) & (y != y.round())).sum())  # x.5 between 128 and 256: a tie
    assert ties > 100


@pytest.mark.parametrize("name", NAMES)
def test_preconditions_and_cpu_path(name):
    """check_exactness holds, and ``fused_conv2d`` on CPU bf16 tensors (``fused_conv2d_ref``) equals the
    float64 model bit for bit."""
    d = ce.data(name)
    ce.check_exactness(d)
    got = ce.run(d)
    if d.case.head:
        assert got.dtype == torch.float32 and d.want.dtype == torch.float64
    else:
        assert got.dtype == d.want.dtype == torch.bfloat16
    ce.assert_exact(got, d.want, name, th=ce.tile_rows(d), nchw=d.case.head, tco=d.pc.tco)


def test_fp32_in_another_order_is_still_exact():
    """The sum taken tap by tap in fp32, taps and channels reversed, equals the float64 value."""
    for name in ("cout256_cin256_rounds", "epi_residual_tco64"):
        d = ce.data(name)
        ap = ce.padded(ce.activated(d), 3).float()
        c = d.case
        y = torch.zeros(c.N, c.H, c.W, c.cout)
        for ty in (2, 1, 0):
            for tx in (2, 1, 0):
                for ci in range(c.cin - 1, -1, -1):
                    y += ap[:, ty:ty + c.H, tx:tx + c.W, ci, None] * d.w[:, ci, ty, tx]
        assert torch.equal(y.double(), ce.conv64(ap.double(), d.w))


MUTANT_CASES = ["epi_residual_tco32", "cout256_cin256_rounds", "persist7_nchunk4_cin128_cout32", "geom_17x65_tco64_nw8",
                "affine_scale_rows_shift_rows_tco64", "grid_ks1_cin8_ck8_tco16_nw8_up2"]


@pytest.mark.parametrize("mutant", sorted(ce.MUTANTS))
def test_every_mutant_breaks_equality(mutant):
    """The comparison has teeth: each fault, injected into the model, changes the answer of at least one
    case (and of every case that offers the fault at all, bar the ones named here)."""
    caught, offered = [], []
    for name in MUTANT_CASES:
        d = ce.data(name)
        bad = ce.MUTANTS[mutant](d, ce.tile_rows(d))
        if bad is None:
            continue
        offered.append(name)
        assert bad.shape == d.want.shape and bad.dtype == d.want.dtype
        if not torch.equal(bad, d.want):
            caught.append(name)
            with pytest.raises(AssertionError, match="outputs differ; first at"):
                ce.assert_exact(bad, d.want, name, th=ce.tile_rows(d))
    assert caught, f"{mutant}: no case notices it"
    if mutant == "truncate":  # only outputs that round can tell: the 1x1 case has none
        assert set(offered) - set(caught) <= {"grid_ks1_cin8_ck8_tco16_nw8_up2"}
    elif mutant == "drop_product":  # a product of 0.5 or 1 can vanish in the rounding of an output above 256
        assert set(offered) - set(caught) <= {n for n in offered if ce.by_name(n).rounds}
        assert len(caught) >= len(offered) - 1
    else:
        assert caught == offered, (mutant, set(offered) - set(caught))


def test_mismatch_report_points_at_the_tile():
    d = ce.data("geom_17x65_tco64_nw8")
    bad = d.want.clone()
    bad[2, 16, 33, 40] += 1
    with pytest.raises(AssertionError) as e:
        ce.assert_exact(bad, d.want, "x", th=16, tco=32)
    msg = str(e.value)
    assert "1 of" in msg and "(2, 16, 33, 40)" in msg and "= (1, 1)" in msg and "in-tile (0, 1)" in msg
    assert "channel block 1 (+8)" in msg


@pytest.mark.parametrize("cfg", ce.TAP_CONFIGS, ids=lambda c: "cin%d_cout%d_nw%d" % (c[0], c[2], c[3]))
def test_tap_map_cpu(cfg):
    x, pc, want = ce.tap_map(*cfg)
    got = fused_conv2d(x, pc)
    ce.assert_exact(got, want, "tap map", th=2 * cfg[3], tco=cfg[5])
    # the stamp is the flipped kernel: the output one pixel up-left of the 1 sees tap (2, 2)
    n = [i for i in range(x.shape[0]) if x[i, cfg[3] * 2, 32].any()][0]
    ci = int(x[n, cfg[3] * 2, 32].nonzero()[0])
    assert torch.equal(got[n, cfg[3] * 2 - 1, 31].float(), ce.tap_code(cfg[2], cfg[0])[:, ci, 2, 2])


@pytest.mark.parametrize("name", sorted(ce.CONCAT_CASES))
def test_concat_cpu(name):
    d = ce.concat_data(name)
    got = fused_conv2d_concat(d.xa, d.xb, d.pc, post_relu=d.post_relu, xb_d2s=d.d2s)
    ce.assert_exact(got, d.want, name, th=2 * d.nw, tco=d.pc.tco)


@pytest.mark.parametrize("name", sorted(ce.CONV3D_CASES))
def test_conv3d_cpu(name, monkeypatch):
    d = ce.conv3d_data(name, monkeypatch)
    ce.assert_exact(conv3d_ref(d.x, d.pc, d.post_relu), d.want, name)
    ce.assert_exact(fused_conv3d(d.x, d.pc, post_relu=d.post_relu), d.want, name)


@pytest.mark.parametrize("name", sorted(ce.CONV3D_CONCAT_CASES))
def test_conv3d_concat_cpu(name, monkeypatch):
    d = ce.conv3d_data(name, monkeypatch)
    xa, xb = d.x[..., : d.ca].contiguous(), d.x[..., d.ca:].contiguous()
    ce.assert_exact(fused_conv3d_concat(xa, xb, d.pc, post_relu=d.post_relu), d.want, name)


def test_some_3d_and_concat_outputs_round(monkeypatch):
    assert max(ce.concat_data(n).frac for n in ce.CONCAT_CASES) > 0.02
    assert max(ce.conv3d_data(n, monkeypatch).frac for n in ce.CONV3D_CASES) > 0.02


def test_a_16_channel_concatenation_is_fused_only_with_8_channel_chunks(monkeypatch):
    """``be_conv3d_ztaps_concat`` has no 16-channel-chunk build: with ``BE_CONV3D_CK16=1`` (the default)
    an 8 + 8 concatenation packs 16-channel chunks and must not be offered to it."""
    from bioengine_worker_amd.ops.conv3d import PackedConv3d, concat3d_fusible

    monkeypatch.setenv("BE_CONV3D", "ztaps")
    w = torch.zeros(16, 16, 3, 3, 3)
    monkeypatch.setenv("BE_CONV3D_CK16", "1")
    pc = PackedConv3d(w, None)
    assert pc.ztap.ck == 16 and not concat3d_fusible(pc, 8, 8)
    monkeypatch.setenv("BE_CONV3D_CK16", "0")
    pc = PackedConv3d(w, None)
    assert pc.ztap.ck == 8 and concat3d_fusible(pc, 8, 8)
    assert concat3d_fusible(PackedConv3d(torch.zeros(16, 64, 3, 3, 3), None), 32, 32)
