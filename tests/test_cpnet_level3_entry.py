"""CPnetEngine with the level-3 entry on a source pooled once (be_pool2_nhwc) and its 3x3 conv on the
ping-pong kernel's 256-channel build: a whole forward on a forced grid under the three switch settings,
bit for bit, with the launches each makes; and a batch-1 request (9 tiles), whose launches stay what
they were."""
import pytest
import torch

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine, to_nhwc_input

#: (BE_CPNET_L3_PREPOOL, BE_CONV_PP128_C256) -> launches of the 256-channel build per forward
ARMS = {(1, 1): 1, (1, 0): 0, (0, 0): 0}


def _counts(lib):
    return int(lib.be_conv_pp128_c256_launches()), int(lib.be_conv_pp128_launches()), int(lib.be_conv_pp128_pool_launches())


@pytest.fixture(scope="module")
def engine(gpu):
    torch.manual_seed(0)
    return CPnetEngine(CPnet().randomize_(7).eval(), gpu)


def _forward(eng, xin, prepool, c256, grid):
    from bioengine_worker_amd.ops import _native

    try:
        _native.call("be_conv_pp128_set_grid", grid)
        _native.call("be_conv_pp128_set_c256", prepool, c256)
        y, s = eng(xin)
        return y.cpu(), s.cpu()
    finally:
        _native.call("be_conv_pp128_set_c256", 1, 1)
        _native.call("be_conv_pp128_set_grid", 0)


@pytest.mark.gpu
def test_forward_is_the_same_under_every_switch_setting(gpu, engine):
    """3 tiles of 224^2 on a grid of 5 workgroups: level 3 is 3 x 28^2, 12 tiles of 8 x 28, 24 items."""
    from bioengine_worker_amd.ops import _native

    lib = _native.hip()
    assert ("down", 3, 1) in engine.ig, "level 3 runs on the implicit-GEMM path, whose entry this is"
    xin = to_nhwc_input(torch.randn(3, 2, 224, 224, generator=torch.Generator().manual_seed(31)), 8).to(gpu)
    outs, plain = {}, {}
    for arm, want in ARMS.items():
        c0 = _counts(lib)
        outs[arm] = _forward(engine, xin, *arm, grid=5)
        c1 = _counts(lib)
        assert c1[0] - c0[0] == want, (arm, c0, c1)
        plain[arm] = (c1[1] - c0[1], c1[2] - c0[2])
    assert len(set(plain.values())) == 1, plain  # the other builds take the calls they took, in every arm
    assert plain[(0, 0)][0] == 6
    y, s = outs[(0, 0)]
    assert torch.isfinite(y).all() and torch.isfinite(s).all()
    for arm in ((1, 1), (1, 0)):
        print(f"arm {arm}: y differing {(outs[arm][0] != y).sum().item()}, style differing {(outs[arm][1] != s).sum().item()}")
        assert torch.equal(outs[arm][0], y) and torch.equal(outs[arm][1], s)


@pytest.mark.gpu
def test_batch1_request_makes_the_launches_it_made(gpu, engine):
    """One 512^2 image is 9 tiles of 224^2, 72 items at level 3: below the size rule at the default grid,
    so the level keeps its two pooled-input launches whatever the switches say."""
    from bioengine_worker_amd.ops import _native

    lib = _native.hip()
    assert lib.be_conv_pp128_takes_prepool(9, 28, 28) == 0 and lib.be_conv_pp128_takes_c256(9, 28, 28) == 0
    xin = to_nhwc_input(torch.randn(9, 2, 224, 224, generator=torch.Generator().manual_seed(9)), 8).to(gpu)
    c0 = _counts(lib)
    outs = [_forward(engine, xin, *arm, grid=0) for arm in ARMS]
    assert _counts(lib) == c0
    for y, s in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(s, outs[0][1])
