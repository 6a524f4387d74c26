"""CPnetEngine with the level-2 entry (pooled 3x3 conv + 1x1 projection) on the 128-channel ping-pong
kernel's pooled build: a whole forward with both switches on against both off, bit for bit, and the
launches of a batch-1 request (9 tiles), which stay what they were."""
import pytest
import torch

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine, to_nhwc_input


def _counts(lib):
    return int(lib.be_conv_pp128_launches()), int(lib.be_conv_pp128_pool_launches())


@pytest.fixture(scope="module")
def engine(gpu):
    torch.manual_seed(0)
    return CPnetEngine(CPnet().randomize_(5).eval(), gpu)


def _forward(eng, xin, pool, proj):
    from bioengine_worker_amd.ops import _native

    try:
        _native.call("be_conv_pp128_set_pool", pool, proj)
        y, s = eng(xin)
        return y.cpu(), s.cpu()
    finally:
        _native.call("be_conv_pp128_set_pool", 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [36, 37])
def test_forward_with_the_pooled_entry_equals_the_forward_without(gpu, engine, tiles):
    """36 tiles of 224^2 are 504 tiles of 8 x 28 at level 2 (56^2, 14 per image): eight short of the
    kernel's rule for an unforced grid (two per workgroup of 256), so the native rule answers 0 and
    the forward keeps the per-layer launches; 37 tiles (518) are the smallest batch it takes.  Both
    must give the bits of the forward with the switches off."""
    from bioengine_worker_amd.ops import _native

    lib = _native.hip()
    takes = bool(lib.be_conv_pp128_takes_pool_proj(tiles, 112, 112))
    assert takes == (tiles * 14 >= 512)
    assert bool(lib.be_conv_pp128_takes(tiles, 56, 56)) == takes  # one rule for every build of the kernel
    g = torch.Generator().manual_seed(tiles)
    xin = to_nhwc_input(torch.randn(tiles, 2, 224, 224, generator=g), 8).to(gpu)
    n0, p0 = _counts(lib)
    y_off, s_off = _forward(engine, xin, 0, 0)
    n1, p1 = _counts(lib)
    assert p1 == p0 and n1 - n0 == (6 if takes else 0)
    y_on, s_on = _forward(engine, xin, 1, 1)
    n2, p2 = _counts(lib)
    assert p2 - p1 == (1 if takes else 0) and n2 - n1 == n1 - n0
    y_c0, s_c0 = _forward(engine, xin, 1, 0)  # the projection as a launch of its own
    n3, p3 = _counts(lib)
    assert p3 - p2 == (1 if takes else 0) and n3 - n2 == n1 - n0
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_on, y_off) and torch.equal(s_on, s_off)
    assert torch.equal(y_c0, y_off) and torch.equal(s_c0, s_off)


@pytest.mark.gpu
def test_batch1_request_makes_the_launches_it_made(gpu, engine):
    """One 512^2 image is 9 tiles of 224^2: below the size rule, so no build of the ping-pong kernel
    runs, pooled or not, whatever the switches say."""
    from bioengine_worker_amd.ops import _native

    lib = _native.hip()
    assert lib.be_conv_pp128_takes_pool_proj(9, 112, 112) == 0 and lib.be_conv_pp128_takes_pool(9, 112, 112) == 0
    xin = to_nhwc_input(torch.randn(9, 2, 224, 224, generator=torch.Generator().manual_seed(9)), 8).to(gpu)
    c0 = _counts(lib)
    y_on, s_on = _forward(engine, xin, 1, 1)
    assert _counts(lib) == c0
    y_off, s_off = _forward(engine, xin, 0, 0)
    assert _counts(lib) == c0
    assert torch.equal(y_on, y_off) and torch.equal(s_on, s_off)
