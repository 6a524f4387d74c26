"""The per-layer fused conv kernel (``conv2d_nhwc_kernel`` / ``conv2d_nhwc_persist``, csrc/kernels/
conv2d_nhwc.hip) against the independent float64 model of ``conv_exact_cases`` on integer data whose
answer does not depend on the order of summation: every comparison is ``torch.equal``.  The CPU half
(``test_conv_exact.py``) checks the preconditions of every case and that the comparison catches local
faults.  Block order is the default throughout (``BE_CONV_ORDER`` is read once per process)."""
import pytest
import torch

import conv_exact_cases as ce
from bioengine_worker_amd.ops import conv as cv
from bioengine_worker_amd.ops.conv import fused_conv2d, fused_conv2d_concat
from bioengine_worker_amd.ops.conv3d import fused_conv3d, fused_conv3d_concat

pytestmark = pytest.mark.gpu


def _native():
    from bioengine_worker_amd.ops import _native as n

    return n


def _pp128_launches():
    lib = _native().hip()
    return int(lib.be_conv_pp128_launches()), int(lib.be_conv_pp128_pool_launches())


@pytest.mark.parametrize("name", [c.name for c in ce.cases()])
def test_per_layer_kernel_equals_model(gpu, name):
    d = ce.data(name)
    n0 = _pp128_launches()
    got = ce.run(d, gpu)
    assert _pp128_launches() == n0, "the per-layer kernel is under test"
    ce.assert_exact(got, d.want, name, th=ce.tile_rows(d), nchw=d.case.head, tco=d.pc.tco)


@pytest.mark.parametrize("cfg", ce.TAP_CONFIGS, ids=lambda c: "cin%d_cout%d_nw%d" % (c[0], c[2], c[3]))
def test_tap_map(gpu, cfg):
    """A single 1 at a corner, at either side of the tile seams or at the last pixel, in the first and
    last channel of an 8-channel group and of a K chunk: the output is the flipped stamp of weight codes."""
    x, pc, want = ce.tap_map(*cfg)
    got = fused_conv2d(x.to(gpu), pc.to(gpu), nw=cfg[3]).cpu()
    assert pc.frag_built() is None
    ce.assert_exact(got, want, "tap map", th=2 * cfg[3], tco=cfg[5])


@pytest.mark.parametrize("name", sorted(ce.CONCAT_CASES))
def test_concat(gpu, name):
    d = ce.concat_data(name)
    import copy

    got = fused_conv2d_concat(d.xa.to(gpu), d.xb.to(gpu), copy.copy(d.pc).to(gpu), post_relu=d.post_relu, nw=d.nw,
                              xb_d2s=d.d2s).cpu()
    ce.assert_exact(got, d.want, name, th=2 * d.nw, tco=d.pc.tco)


@pytest.mark.parametrize("name", sorted(ce.CONV3D_CASES))
def test_conv3d_ztaps(gpu, name, monkeypatch):
    """D = 1, 2, 5: the first and last slice's depth taps fall outside the volume."""
    d = ce.conv3d_data(name, monkeypatch)
    got = fused_conv3d(d.x.to(gpu), d.pc.to(gpu), post_relu=d.post_relu).cpu()
    ce.assert_exact(got, d.want, name, tco=d.pc.ztap.tco)


@pytest.mark.parametrize("name", sorted(ce.CONV3D_CONCAT_CASES))
def test_conv3d_ztaps_concat(gpu, name, monkeypatch):
    d = ce.conv3d_data(name, monkeypatch)
    xa, xb = d.x[..., : d.ca].contiguous().to(gpu), d.x[..., d.ca:].contiguous().to(gpu)
    got = fused_conv3d_concat(xa, xb, d.pc.to(gpu), post_relu=d.post_relu).cpu()
    ce.assert_exact(got, d.want, name, tco=d.pc.ztap.tco)


# ---- the fused families: fragment weights built, the ping-pong kernels run, same data, same model


@pytest.mark.parametrize("case", ce.PP128_CASES, ids=lambda c: c.name)
def test_pp128_equals_model(gpu, case):
    d = ce.make(case)
    ce.check_exactness(d)
    want = ce.ref64(d)
    nat = _native()
    n0 = _pp128_launches()
    try:
        nat.call("be_conv_pp128_set_grid", 5)
        got = ce.run(d, gpu, frag=True)
    finally:
        nat.call("be_conv_pp128_set_grid", 0)
    assert _pp128_launches() == (n0[0] + 1, n0[1]), "the forced grid must reach the ping-pong kernel"
    ce.assert_exact(got, want, case.name, th=8, tco=128)


def test_pp128_pool_and_pool_proj_equal_model(gpu):
    import copy

    dc, dp = ce.pool_pair()
    ce.check_exactness(dc), ce.check_exactness(dp)
    pc, pp = copy.copy(dc.pc).to(gpu), copy.copy(dp.pc).to(gpu)
    pc.frag(), pp.frag()
    x = dc.x.to(gpu)
    shift = dc.shift._base.to(gpu)[:, 64:128]
    assert not shift.is_contiguous() and torch.equal(shift.cpu(), dc.shift)
    nat = _native()
    n0 = _pp128_launches()
    try:
        nat.call("be_conv_pp128_set_grid", 5)
        assert cv.pp128_takes_pool(pc, x) and cv.pp128_takes_pool_proj(pc, pp, x)
        solo = fused_conv2d(x, pc, scale=dc.scale.to(gpu), shift=shift, relu=True, inmode="pool2").cpu()
        assert _pp128_launches() == (n0[0], n0[1] + 1)
        h, p = cv.fused_conv2d_pool_proj(x, pc, pp, scale=dc.scale.to(gpu), shift=shift, relu=True,
                                         proj_scale=dp.scale.to(gpu), proj_shift=dp.shift.to(gpu))
        h, p = h.cpu(), p.cpu()
        assert _pp128_launches() == (n0[0], n0[1] + 2)
    finally:
        nat.call("be_conv_pp128_set_grid", 0)
    ce.assert_exact(solo, dc.want, "pooled build alone", th=8, tco=128)
    ce.assert_exact(h, dc.want, "pooled build, conv", th=8, tco=128)
    ce.assert_exact(p, dp.want, "pooled build, projection", th=8, tco=128)


@pytest.mark.parametrize("i", range(len(ce.PAIR_CASES)), ids=lambda i: "cin%d_cm%d_%s" % ce.PAIR_CASES[i][:3])
@pytest.mark.parametrize("grid", [0, 5], ids=["default_grid", "pingpong_grid5"])
def test_conv_pair_equals_model(gpu, i, grid):
    """Both kernels of the fused half-block: the default grid, and 5 workgroups (every workgroup has two
    tiles or more, which is what the ping-pong builds need)."""
    from bioengine_worker_amd.ops import conv_pair as cp

    d = ce.pair_data(i)
    s = d.spec
    g = lambda t: None if t is None else t.to(gpu)
    gspec = cp.PairSpec(pa=s.pa.to(gpu), pb=s.pb.to(gpu), sa=g(s.sa), ta=None, sb=g(s.sb), tb=None, bias=g(s.bias),
                        inmode=s.inmode, pp=None if s.pp is None else s.pp.to(gpu), sp=g(s.sp), tp=g(s.tp))
    nat = _native()
    try:
        nat.call("be_conv_pair_set_grid", grid)
        got = cp.conv_pair(g(d.x), gspec, ta=g(d.ta), tb=g(d.tb), x2=g(d.x2), res=g(d.res), res_mode=d.res_mode).cpu()
    finally:
        nat.call("be_conv_pair_set_grid", 0)
    ce.assert_exact(got, d.want, "conv_pair %s" % (ce.PAIR_CASES[i],), th=8, tco=64)
