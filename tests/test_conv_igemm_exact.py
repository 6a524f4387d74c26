"""The CPU side of the exact integer-data tests of the level-3 implicit-GEMM convs (``conv_igemm_exact_cases``):
the preconditions under which equality may be demanded, the CPU paths of ``conv3_igemm`` and
``gemm_pp.conv3`` against the independent float64 model, ``IgemmConv.pack`` against its documented layout,
proof that the comparison catches local faults, the tap map, and the chained model of the two routes.

What the rule of ``test_conv_igemm.py`` (``max|out - y| < 0.02 max|y| + 1e-2`` on Gaussian data of its kind:
unit-variance input, residual, per-image shift; the same bound for ``aout``) makes of the same nine faults,
computed on the model alone: the larger of the errors of ``out`` and ``aout`` against the tolerance.  The
unmutated model itself is 0.016 away (the casts).

    fault                         3x28x28 64->128    2x28x28 256->256   2x13x17 32->128
    tolerance                     0.143              0.143              0.128
    truncate_first_cast           0.051  passes      0.053  passes      0.047  passes
    truncate_second_cast          0.031  passes      0.031  passes      0.031  passes
    aout_from_unrounded_y         0.029  passes      0.034  passes      0.030  passes
    pad_row_is_next_image         2.081              2.738              2.086
    shift_of_tiles_first_image    0.395              0.417              0.508
    halo_halves_swapped           1.044              0.532              1.046
    stale_k_chunk                 2.562              1.278              (two chunks)
    residual_of_next_pixel        3.985              5.895              3.240
    drop_product                  0.016  passes (*)  0.016  passes (*)  0.032  passes (*)

(*) the product in the middle of the list of K at that pixel; the median product is 0.008 .. 0.020, the largest
0.26 .. 0.52.  Both truncations, the activated copy taken from the unrounded sum and a typical dropped product
pass everywhere; on the integer data below every one of the nine breaks equality in every case that offers
it and can show it (``test_every_mutant_breaks_equality`` names the exceptions).
"""
import pytest
import torch

import conv_igemm_exact_cases as ic
from bioengine_worker_amd.ops import conv_igemm as ig

ALL = ic.cases() + ic.PP_EXTRA
NAMES = [c.name for c in ALL]


def test_case_list_covers_the_builds():
    cs = ic.cases()
    assert 40 <= len(cs) <= 80
    for c in cs:
        assert c.H <= 28 and c.W <= 28 or (c.H, c.W) in ((40, 1), (1, 40))
        assert c.bns, c.name
    for bn in ic.BNS:
        mine = [c for c in cs if bn in c.bns]
        # K chunks: one (the three-stage builds' guard), three, sixteen
        assert {c.cin // 16 for c in mine} >= {1, 2, 3, 4, 8, 16}
        # block counts tiles * cob: below 8, above 8 and no multiple of 8, a multiple of 8 (xcd_remap)
        nb = {-(-c.N * c.H * c.W // ic.bm_of(bn)) * (c.cout // ic.bnc_of(bn)) for c in mine}
        assert any(b < 8 for b in nb) and any(b > 8 and b % 8 for b in nb) and any(b % 8 == 0 for b in nb), (bn, nb)
        assert {c.cout for c in mine} >= ({64, 128, 192, 256} if ic.bnc_of(bn) == 64 else {128, 256})
        # a tile that crosses images with a per-image shift, a ragged last tile, one image with a 2-D shift
        assert any(c.N > 1 and c.H * c.W < ic.bm_of(bn) and c.ashift == "strided" for c in mine)
        assert any(c.N == 1 and c.ashift == "rows" for c in mine)
    r = [c for c in cs if c.rounds]
    assert {(c.cin, c.cout) for c in r} >= {(128, 128), (256, 256)}
    assert any(not c.want_out and c.res for c in r) and any(not c.want_out and not c.res for c in r)
    assert any(c.given for c in r) and any(c.post_relu for c in r) and any(not c.arelu for c in r)
    assert {c.ashift for c in r} == {None, "shared", "rows", "strided"}
    assert all(c.cin % 32 == 0 for c in ic.pp_cases()) and {c.cout for c in ic.PP_EXTRA} >= {68, 132}


@pytest.mark.parametrize("name", NAMES)
def test_preconditions_and_cpu_paths(name):
    """check_exactness holds, and ``conv3_igemm`` (and ``gemm_pp.conv3`` wherever Cin % 32 == 0) on CPU tensors
    equals the float64 model bit for bit: on this data the fp32 fallbacks are exact."""
    d = ic.data(name)
    c = d.case
    ic.check_exactness(d)
    if c.cout % 64 == 0:
        ic.assert_pair_exact(d, ic.run_igemm(d), f"{name} conv3_igemm (CPU)")
    if c.cin % 32 == 0:
        ic.assert_pair_exact(d, ic.run_pp(d), f"{name} gemm_pp.conv3 (CPU)")


@pytest.mark.parametrize("cout,cin", [(128, 32), (256, 48)])
@pytest.mark.parametrize("bn", [64, 128])
def test_pack_against_the_documented_layout(cout, cin, bn):
    """``[Cout/bnc][Cin/16][9][bnc/32][2][32][8]``: block, K chunk, tap, 32-channel fragment, channel half of
    the chunk, output channel of the fragment, input channel of the half."""
    w = ic.tap_code(cout, cin) + 0.5 * (torch.arange(cout)[:, None, None, None] % 3)  # every element differs nearby
    pk = ig.IgemmConv.from_weight(w, None, bn=bn)
    bnc = ic.bnc_of(bn)
    assert pk.bnc == bnc and pk.wp.dtype == torch.bfloat16 and pk.wp.numel() == w.numel()
    wp = pk.wp.view(cout // bnc, cin // 16, 9, bnc // 32, 2, 32, 8).float()
    back = torch.full_like(w, float("nan"))
    for b in range(cout // bnc):
        for k in range(cin // 16):
            for t in range(9):
                for f in range(bnc // 32):
                    for h in range(2):
                        for co in range(32):
                            for j in range(8):
                                back[b * bnc + f * 32 + co, k * 16 + h * 8 + j, t // 3, t % 3] = wp[b, k, t, f, h, co, j]
    assert torch.equal(back, w)


def _bm(name):  # tile sizes rotate through the cases: both occur with every kind of case
    return (256, 512)[NAMES.index(name) % 2]


@pytest.mark.parametrize("mutant", list(ic.MUTANTS))
def test_every_mutant_breaks_equality(mutant):
    """The comparison has teeth: each fault, injected into the model, changes what the launch returns in every
    case that offers it, bar those that cannot show it."""
    caught, offered = [], []
    for name in NAMES:
        d = ic.data(name)
        bad = ic.MUTANTS[mutant](d, _bm(name))
        if bad is None:
            continue
        offered.append(name)
        for b, w in zip(bad, d.want):
            assert (b is None) == (w is None) and (b is None or (b.shape == w.shape and b.dtype == w.dtype))
        if not ic.same(d, bad, d.want):
            caught.append(name)
            with pytest.raises(AssertionError, match="outputs differ; first at"):
                ic.assert_pair_exact(d, ic.returned(d, bad), name)
    missed = set(offered) - set(caught)
    rounding = {c.name for c in ALL if c.rounds}
    assert len(offered) >= 10, (mutant, offered)
    if mutant == "truncate_first_cast":  # only outputs that round can tell
        assert not missed & rounding
    elif mutant in ("truncate_second_cast", "aout_from_unrounded_y"):
        # a power of two commutes with the cast: the second cast rounds, and one cast differs from two,
        # only where a shift is added
        assert not missed & {n for n in rounding if ic.by_name(n).ashift is not None}
    elif mutant == "drop_product":
        # a product of 0.5 .. 2 can vanish in the rounding of an output above 128, and any product in a
        # negative value that a ReLU clamps (the output's own, or that of an activated copy which is all
        # the launch returns)
        assert missed <= rounding | {c.name for c in ALL if not c.want_out or c.post_relu}
        assert len(missed) <= len(offered) // 4, missed
    else:
        assert not missed, (mutant, missed)


def test_mutants_are_offered_where_the_kernel_can_have_the_fault():
    offers = lambda m, name, bm=256: ic.MUTANTS[m](ic.data(name), bm) is not None
    assert offers("shift_of_tiles_first_image", "geom_5x8x8_tile_spans_four_images")
    assert not offers("shift_of_tiles_first_image", "epi128_shift_shared")
    assert not offers("shift_of_tiles_first_image", "blocks_cout256_4x16x16")  # 256 pixels per image: no tile crosses
    assert offers("stale_k_chunk", "chunks3_cin48") and not offers("stale_k_chunk", "chunks2_cin32")
    assert not offers("halo_halves_swapped", "geom_1x1x1_rows_clamp_2d_shift_of_one_image")
    assert offers("halo_halves_swapped", "geom_1x40x1_one_column_2d_shift_of_one_image")
    assert not offers("truncate_second_cast", "epi256_no_activation")


def test_mismatch_report_points_at_the_tile():
    d = ic.data("geom_3x28x28_level3")
    out, _ = d.want
    bad = out.clone()
    bad[1, 5, 7, 100] += 1  # m = 784 + 147 = 931
    bad[2, 27, 27, 3] += 1
    with pytest.raises(AssertionError) as e:
        ic.assert_exact_linear(bad, out, "x", bm=256, bnc=64)
    msg = str(e.value)
    assert "2 of" in msg and "(1, 5, 7, 100)" in msg and "linear pixel m = 931" in msg and "tile m // 256 = 3" in msg
    assert "in-tile offset 163 (wave 2)" in msg and "channel block co // 64 = 1 (+36)" in msg
    assert "tiles hit: [3, 9] of 10" in msg
    assert "expected %s, got %s" % (out[1, 5, 7, 100].item(), bad[1, 5, 7, 100].item()) in msg
    with pytest.raises(AssertionError, match=r"tile m // 512 = 1, in-tile offset 419 \(wave 6\), channel block co // 128 = 0"):
        ic.assert_exact_linear(bad, out, "x", bm=512, bnc=128)
    with pytest.raises(AssertionError, match="aout is missing"):
        ic.assert_pair_exact(d, (out, None), "x")


def test_tap_map_cpu():
    x, w, want, items = ic.tap_map()
    H, W, cin, cout = ic.TAP_SHAPE
    assert all(int(x[n].sum()) == 1 for n, *_ in items) and int(x.sum()) == len(items) == 48
    assert {ci for *_, ci in items} == {0, 7, 8, 15, 16, cin - 1}
    ms = {(n * H + y) * W + xx for n, y, xx, _ in items}
    assert 255 in ms and 512 in ms
    for bm in (256, 512):  # both sides of a seam of either tile size
        assert {m % bm for m in ms} >= {bm - 1, 0}
    pos = {(y, xx) for _, y, xx, _ in items}
    assert pos >= {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    for bm in (256, 512):
        assert ic.tap_halo_parities(bm) == {0, 1}
    pk = ig.IgemmConv.from_weight(w, None)
    got, _ = ig.conv3_igemm(x, pk)
    ic.assert_exact_linear(got, want, "tap map (CPU)")
    # the stamp is the flipped kernel: the output one pixel up-left of the 1 sees tap (2, 2)
    n, y, xx, ci = next(i for i in items if (i[1], i[2]) == (6, 11))
    assert torch.equal(got[n, y - 1, xx - 1].float(), w[:, ci, 2, 2])
    # nothing leaks across the image seam: a 1 in a corner stamps four pixels of its own image and no other
    for n, y, xx, ci in items:
        if (y, xx) in ((0, 0), (H - 1, W - 1)):
            assert int((want[n] != 0).any(-1).sum()) == 4


def test_route_net_folds_to_powers_of_two_and_integers():
    net = ic.route_net()
    dn, up = net.downsample.down[3], net.upsample.up[3]
    bns = [dn.proj[0], up.proj[0], up.conv[0][0]] + [dn.conv[k][0] for k in range(4)]
    bns += [up.conv[k].conv[0] for k in (1, 2, 3)]
    for bn in bns:
        s, t = ic.bn64(bn)
        assert set(s.unique().tolist()) == {0.5, 1.0, 2.0} and torch.equal(t, t.round())
    for conv, dense in ((dn.conv[1][2], False), (dn.conv[3][2], True), (up.conv[0][2], False), (up.conv[3].conv[2], True)):
        w = conv.weight.detach()
        assert torch.equal(w, w.round()) and torch.equal(conv.bias.detach(), conv.bias.detach().round())
        per_out = (w != 0).sum((1, 2, 3)).float().mean().item()
        assert (per_out > 1500) if dense else (30 < per_out < 50), per_out


def test_route_models_are_exact_launch_by_launch():
    """Every launch of both chains passes its preconditions with its own quantum (asserted inside
    ``launch64``), stays below a fifth of ``2^22 q``, and the dense last convs round most of their outputs."""
    (Td, Ld), (Tu, Lu) = ic.route_models()
    for L in (Ld, Lu):
        for k, m in L.items():
            assert m.mag < 0.2, (k, m.mag)
        rounded = (L["c3"].out.double() != L["c3"].yr).double().mean().item()
        assert rounded > 0.85, rounded
    for T in (Td, Tu):
        for k, t in T.items():
            assert t.dtype == torch.bfloat16 and t.unique().numel() >= 100, k
    i = ic.route_inputs()
    assert not torch.equal(i.xcur, i.y) and not torch.equal(i.xcur, i.top_act) and not torch.equal(i.y, i.top_act)
    for k in (1, 2, 3):
        sh = i.shifts[(3, k)]
        assert not sh.is_contiguous() and torch.equal(sh, sh.round()) and len({tuple(r.tolist()) for r in sh}) == ic.ROUTE_N


@pytest.mark.parametrize("kind", ["1", "pp"])
def test_routes_cpu_path_equals_chained_model(kind):
    """``_down_ig`` / ``_up_ig`` on CPU tensors run the fp32 formulas of the same launches: the wiring (which
    tensor is a residual, which scale and shift feed which activated copy) against the chained model."""
    from bioengine_worker_amd.models.cpnet import CPnetEngine, CPnetEngineOptions

    net, i = ic.route_net(), ic.route_inputs()
    eng = CPnetEngine(net, "cpu", options=CPnetEngineOptions(igemm=kind))
    assert {("down", 3, k) for k in (1, 2, 3)} | {("up", 3, k) for k in range(4)} <= set(eng.ig)
    (Td, _), (Tu, _) = ic.route_models()
    xd, top_act = eng._down_ig(3, eng.down[3], i.src)
    ic.assert_exact_linear(xd, Td["xd"], f"down route {kind} (CPU): xd")
    ic.assert_exact_linear(top_act, Td["top_act"], f"down route {kind} (CPU): top_act")
    out = eng._up_ig(3, eng.up[3], i.xcur, i.y, i.shifts, i.top_act)
    ic.assert_exact_linear(out, Tu["out"], f"up route {kind} (CPU): out")
