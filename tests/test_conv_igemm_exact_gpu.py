"""The level-3 implicit-GEMM convs on the GPU -- ``conv3_igemm`` (csrc/kernels/conv_igemm.hip) in its five
builds and ``gemm_pp.conv3`` (csrc/kernels/gemm_pp.hip) in its three -- against the independent float64
model of ``conv_igemm_exact_cases`` on integer data whose answer does not depend on the order of summation,
and the engine's two level-3 routes against the same model chained launch by launch.  Every comparison is
``torch.equal`` through the linear-tile report (tile, wave, channel block).  The CPU half
(``test_conv_igemm_exact.py``) checks the preconditions of every case and that the comparison catches
local faults."""
import pytest
import torch

import conv_igemm_exact_cases as ic
from bioengine_worker_amd.ops import conv_igemm as ig
from bioengine_worker_amd.ops import gemm_pp as pp

pytestmark = pytest.mark.gpu

IG_ITEMS = [(c.name, bn) for c in ic.cases() for bn in c.bns]
PP_ITEMS = [(c.name, cfg) for c in ic.pp_cases() for cfg in sorted(ic.PP_TILES)]


@pytest.mark.parametrize("name,bn", IG_ITEMS, ids=[f"{n}-bn{b}" for n, b in IG_ITEMS])
def test_conv3_igemm_equals_model(gpu, name, bn):
    """Single launches: ``out`` and ``aout`` of every case on every build its Cout admits.  With
    ``want_out=False`` ``out`` is None; a given ``out=`` / ``aout=`` is the returned tensor and holds the
    answer, so none of the 77s it was filled with survives."""
    d = ic.data(name)
    c = d.case
    assert ig.supported(c.N, c.H, c.W, c.cout, bn)
    got = ic.run_igemm(d, gpu, bn)
    ic.assert_pair_exact(d, got, f"{name} bn {bn}", bm=ic.bm_of(bn), bnc=ic.bnc_of(bn))


@pytest.mark.parametrize("name,cfg", PP_ITEMS, ids=[f"{n}-cfg{c}" for n, c in PP_ITEMS])
def test_gemm_pp_conv3_equals_model(gpu, name, cfg):
    """The same data and the same model on the ping-pong kernel, plus three K-halves per tap (Cin 96) and
    ragged N (Cout 68, 132)."""
    d = ic.data(name)
    assert pp.conv3_supported(d.case.cin, d.case.cout)
    got = ic.run_pp(d, gpu, cfg)
    bm, bnc = ic.PP_TILES[cfg]
    ic.assert_pair_exact(d, got, f"{name} cfg {cfg}", bm=bm, bnc=bnc)


@pytest.mark.parametrize("bn", ic.TAP_BNS)
def test_tap_map(gpu, bn):
    """A single 1 per image at a corner, at either side of a tile seam, in either parity of the halo's
    half swap, in the first and last channel of an 8-channel half and of a K chunk, all images in one
    batch: the output is the flipped stamp of weight codes and zero elsewhere, other images included."""
    x, w, want, items = ic.tap_map()
    N, H, W, _ = x.shape
    assert ig.supported(N, H, W, w.shape[0], bn) and ic.tap_halo_parities(ic.bm_of(bn)) == {0, 1}
    pk = ig.IgemmConv.from_weight(w, None, bn=bn).to(gpu)
    got, aout = ig.conv3_igemm(x.to(gpu), pk)
    assert aout is None
    ic.assert_exact_linear(got.cpu(), want, f"tap map bn {bn}", bm=ic.bm_of(bn), bnc=ic.bnc_of(bn))


def _widths(bn):
    cout = ic.bnc_of(bn)
    return [W for W in range(1, 641) if ig.supported(2, 4, W, cout, bn)]


def _run_width(gpu, bn, W):
    d = ic.make(ic.widest_case(bn, W))
    c = d.case
    ic.check_exactness(d)
    assert ig.supported(c.N, c.H, W, c.cout, bn)
    ic.assert_pair_exact(d, ic.run_igemm(d, gpu, bn), c.name, bm=ic.bm_of(bn), bnc=ic.bnc_of(bn))


@pytest.mark.parametrize("bn", ic.BNS)
def test_widest_supported_image(gpu, bn):
    """2 x 4 x W at the largest W the host formula takes (W + 1 is refused): the host's worst-case count
    of halo rows must cover what the kernel stages, or the last halo DMAs are dropped."""
    ws = _widths(bn)
    assert ws and ws[-1] < 600 and not ig.supported(2, 4, ws[-1] + 1, ic.bnc_of(bn), bn)
    _run_width(gpu, bn, ws[-1])


@pytest.mark.parametrize("bn", ic.BNS)
def test_both_sides_of_a_gap_in_the_supported_widths(gpu, bn):
    """``be_conv3_igemm_lds`` is not monotonic in W: the 256 x 64 build refuses one width below its widest
    while it takes the next.  Both neighbours of every refused stretch run, on every build that has one."""
    ws = set(_widths(bn))
    gaps = [W for W in range(2, max(ws)) if W not in ws and W + 1 in ws]
    if bn == 64:
        assert gaps, "the formula became monotonic: revise this test's premise, not its cases"
    for above in gaps:
        _run_width(gpu, bn, max(W for W in ws if W < above))
        _run_width(gpu, bn, above + 1)


# ---- the two routes of both kinds


@pytest.fixture(scope="session")
def engines(gpu):
    from bioengine_worker_amd.models.cpnet import CPnetEngine, CPnetEngineOptions

    return {kind: CPnetEngine(ic.route_net(), gpu, options=CPnetEngineOptions(igemm=kind)) for kind in ("1", "pp")}


def _tile(kind):
    return (256, 64) if kind == "1" else ic.PP_TILES[pp.conv_cfg(ic.ROUTE_C)]


@pytest.mark.parametrize("kind", ["1", "pp"])
def test_engine_folds_the_integer_parameters_exactly(engines, kind):
    eng, net = engines[kind], ic.route_net()
    dn, up = net.downsample.down[3], net.upsample.up[3]
    pairs = [(eng.down[3]["proj"], dn.proj[0]), (eng.up[3]["proj"], up.proj[0]), (eng.up[3]["c0"], up.conv[0][0])]
    pairs += [(eng.down[3][f"c{k}"], dn.conv[k][0]) for k in range(4)]
    pairs += [(eng.up[3][f"c{k}"], up.conv[k].conv[0]) for k in (1, 2, 3)]
    for fc, bn in pairs:
        s, t = ic.bn64(bn)
        assert torch.equal(fc.scale.cpu().double(), s) and torch.equal(fc.shift.cpu().double(), t)
        assert set(s.unique().tolist()) == {0.5, 1.0, 2.0} and torch.equal(t, t.round())
    keys = {("down", 3, k) for k in (1, 2, 3)} | {("up", 3, k) for k in range(4)}
    assert set(eng.ig) == keys
    for key in keys:
        conv = dn.conv[key[2]][2] if key[0] == "down" else (up.conv[0][2] if key[2] == 0 else up.conv[key[2]].conv[2])
        pk = eng.ig[key]
        if kind == "1":
            assert isinstance(pk, ig.IgemmConv) and torch.equal(pk.w.cpu(), conv.weight.detach())
        else:
            assert torch.equal(pk.wp.cpu().float(), conv.weight.detach().permute(0, 2, 3, 1))


@pytest.mark.parametrize("kind", ["1", "pp"])
def test_down_route_equals_chained_model(gpu, engines, kind):
    """``_down_ig``: proj = P(pool(src)), ha = act_c1(c0(pool(src))), x1 = c1(ha) + proj, x1a = act_c2(x1),
    h2a = act_c3(c2(x1a)), xd = c3(h2a) + x1, top_act = act_up3c0(xd)."""
    eng, i = engines[kind], ic.route_inputs()
    (T, _), _ = ic.route_models()
    src = i.src.to(gpu)
    assert eng._down_route(3, src) == "ig"
    xd, top_act = eng._down_ig(3, eng.down[3], src)
    bm, bnc = _tile(kind)
    ic.assert_exact_linear(xd.cpu(), T["xd"], f"down route {kind}: xd", bm=bm, bnc=bnc)
    ic.assert_exact_linear(top_act.cpu(), T["top_act"], f"down route {kind}: top_act", bm=bm, bnc=bnc)


@pytest.mark.parametrize("kind", ["1", "pp"])
def test_up_route_equals_chained_model(gpu, engines, kind):
    """``_up_ig`` with different tensors for ``xcur``, ``y`` and ``top_act`` and per-image strided shifts:
    proj = P(xcur), h0a = act_c1(c0(top_act) + y), x1 = c1(h0a) + proj, x1a = act_c2(x1),
    h2a = act_c3(c2(x1a)), out = c3(h2a) + x1."""
    eng, i = engines[kind], ic.route_inputs()
    _, (T, _) = ic.route_models()
    xcur, y, top_act = i.xcur.to(gpu), i.y.to(gpu), i.top_act.to(gpu)
    wide = i.shifts_wide.to(gpu)
    shifts = {k: wide[:, v.storage_offset(): v.storage_offset() + v.shape[1]] for k, v in i.shifts.items()}
    for k, v in shifts.items():
        assert not v.is_contiguous() and torch.equal(v.cpu(), i.shifts[k])
    assert eng._up_route(3, xcur, top_act) == "ig"
    out = eng._up_ig(3, eng.up[3], xcur, y, shifts, top_act)
    bm, bnc = _tile(kind)
    ic.assert_exact_linear(out.cpu(), T["out"], f"up route {kind}: out", bm=bm, bnc=bnc)
