"""2x2 max-pool of a bf16 NHWC tensor (csrc/kernels/pool2_nhwc.hip, ops/conv.py pool2_nhwc): bit for bit
against the CPU reference, on random data and on small integers with ties, negatives and both zeros."""
import pytest
import torch
import torch.nn.functional as F

from bioengine_worker_amd.ops import conv as cv

SHAPES = [(2, 6, 10, 128), (1, 56, 56, 128), (3, 4, 4, 8)]


def _random(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16()


def _integers(shape, seed):
    """Values in {-2, -1, -0.0, +0.0, 1, 2}: most 2x2 windows hold a tie; a fifth of them hold -0 only, and
    another fifth -0 and negatives with a single +0 at a random place of the window."""
    g = torch.Generator().manual_seed(seed)
    N, Hs, Ws, C = shape
    v = torch.randint(-2, 3, shape, generator=g).float()
    v = torch.where((v == 0) & (torch.rand(shape, generator=g) < 0.5), torch.full_like(v, -0.0), v)
    win = v.view(N, Hs // 2, 2, Ws // 2, 2, C)  # a view: writes below land in v
    mode = torch.rand(N, Hs // 2, 1, Ws // 2, 1, C, generator=g)
    place = torch.randint(0, 4, (N, Hs // 2, 1, Ws // 2, 1, C), generator=g)
    here = (torch.arange(2).view(1, 1, 2, 1, 1, 1) * 2 + torch.arange(2).view(1, 1, 1, 1, 2, 1)) == place
    nonpos = torch.where(win > 0, -win, win)
    win.copy_(torch.where(mode < 0.2, torch.full_like(win, -0.0), win))
    win.copy_(torch.where((mode >= 0.2) & (mode < 0.4), torch.where(here, torch.zeros_like(win), nonpos), win))
    return v.bfloat16()


def _bits(t):
    return t.contiguous().view(torch.int16)


def test_reference_orders_the_two_zeros_and_matches_max_pool2d():
    x = _integers((2, 6, 10, 16), 5)
    y = cv.pool2_nhwc(x)
    assert y.shape == (2, 3, 5, 16) and y.dtype == torch.bfloat16
    assert torch.equal(y.float(), F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
    win = torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]])
    all_neg0 = (_bits(win) == -32768).all(0)
    any_pos0 = ((_bits(win) == 0).any(0)) & (win.float() <= 0).all(0)
    assert all_neg0.any() and any_pos0.any(), "the data must hold windows of -0 only and windows whose maximum is +0"
    assert (_bits(y)[all_neg0] == -32768).all(), "a window of -0 only pools to -0"
    assert (_bits(y)[any_pos0] == 0).all(), "+0 beats -0 wherever it stands in the window"
    w = torch.tensor([[[[-0.0]], [[0.0]]], [[[-0.0]], [[-0.0]]]]).permute(2, 0, 1, 3).bfloat16()  # [1, 2, 2, 1]
    assert _bits(cv.pool2_nhwc(w)).item() == 0 and _bits(cv.pool2_nhwc(w.flip(2))).item() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("data", ["random", "integers"])
def test_pool2_kernel_equals_the_reference_bit_for_bit(gpu, shape, data):
    x = _random(shape, 11) if data == "random" else _integers(shape, 12)
    want = cv.pool2_nhwc(x)
    got = cv.pool2_nhwc(x.to(gpu))
    torch.cuda.synchronize()
    N, Hs, Ws, C = shape
    assert got.shape == (N, Hs // 2, Ws // 2, C) and got.dtype == torch.bfloat16 and got.is_contiguous()
    diff = (_bits(got.cpu()) != _bits(want)).sum().item()
    print(f"pool2 {shape} {data}: {diff} of {want.numel()} half-words differ")
    assert diff == 0
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(got.cpu().float(), ref)


@pytest.mark.gpu
def test_pool2_rejects_what_the_kernel_does_not_read(gpu):
    with pytest.raises(AssertionError):
        cv.pool2_nhwc(torch.zeros(1, 5, 4, 8, dtype=torch.bfloat16, device=gpu))
    with pytest.raises(AssertionError):
        cv.pool2_nhwc(torch.zeros(1, 4, 4, 4, dtype=torch.bfloat16, device=gpu))
    from bioengine_worker_amd.ops import _native

    x = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16, device=gpu)
    out = torch.empty(1, 2, 2, 8, dtype=torch.bfloat16, device=gpu)
    lib = _native.hip()
    st = _native.stream(gpu)
    assert lib.be_pool2_nhwc(_native.ptr(x), _native.ptr(out), 1, 3, 4, 8, st) == -40
    assert lib.be_pool2_nhwc(_native.ptr(x), _native.ptr(out), 1, 4, 4, 12, st) == -40
    assert lib.be_pool2_nhwc(_native.ptr(x), None, 1, 4, 4, 8, st) == -40
