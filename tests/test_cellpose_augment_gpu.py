"""Cellpose test-time augmentation on the GPU: the mirroring gathers (``be_tiles_gather_aug``,
``be_tiles_gather_norm_aug``) bit for bit against a torch formulation (slice the zero-padded image,
flip, permute, cast), the un-mirroring blend (``be_tiles_blend_aug``) against the oracle's
``unaugment_tiles`` + float64 ``average_tiles``, and the network stage of ``CellposeRunner`` under
``augment=True`` against the same composition built by hand."""
import copy

import numpy as np
import pytest
import torch

import cellpose_augment_cases as ac
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16)


def _plan(H, W, bsize, gpu):
    from bioengine_worker_amd.cellpose.gpu import TilePlan

    plan = TilePlan(H, W, bsize, 0.1, device=gpu, augment=True)
    assert plan.by == plan.bx == bsize and plan.nt == len(plan.ys) * len(plan.xs)
    assert (plan.Ly, plan.Lx) == (max(plan.Hp, bsize), max(plan.Wp, bsize))
    return plan


def _torch_tiles(plan, x, cpad, mirror=True):
    """The tiles of ``plan`` from torch ops: [B * nt, by, bx, cpad] bf16."""
    B, C, H, W = x.shape
    xp = torch.zeros(B, cpad, plan.Ly, plan.Lx, device=x.device)
    xp[:, :C, plan.pad_y: plan.pad_y + H, plan.pad_x: plan.pad_x + W] = x
    out = []
    for b in range(B):
        for j, y in enumerate(plan.ys):
            for i, x0 in enumerate(plan.xs):
                t = xp[b, :, y: y + plan.by, x0: x0 + plan.bx]
                if mirror and i % 2:
                    t = t.flip(1)
                if mirror and j % 2:
                    t = t.flip(2)
                out.append(t)
    return torch.stack(out).permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()


def _data(shape, kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "uint8":
        return (torch.rand(shape, generator=g) ** 3 * 255).round().to(torch.uint8)
    if kind == "uint16":
        return (torch.rand(shape, generator=g) ** 4 * 4000).round().to(torch.int32).to(torch.uint16)
    return torch.randn(shape, generator=g) * 100


GATHER_CASES = {
    "multi": ((3, 2, 70, 90), 32),  # all four mirror classes, both pads non-zero
    "short": ((1, 1, 20, 100), 64),  # padded height below the tile, equal starts along y
    "tiny": ((1, 2, 16, 16), 32),  # equal starts on both axes
    "rows30": ((2, 1, 50, 45), 30),  # tile height no multiple of the kernel's 4-row group
    "tile224": ((1, 2, 250, 230), 224),
}


@pytest.mark.parametrize("cpad", [8, 16])
@pytest.mark.parametrize("case", list(GATHER_CASES))
def test_gather_mirrors_bit_for_bit(gpu, case, cpad):
    shape, bsize = GATHER_CASES[case]
    B, C, H, W = shape
    plan = _plan(H, W, bsize, gpu)
    if case == "multi":
        assert len(plan.ys) >= 2 and len(plan.xs) >= 2 and plan.pad_y > 0 and plan.pad_x > 0
        assert (plan.ys, plan.xs) == tuple(ac.GEOMETRIES[(70, 90, 32)][1:])
    if case == "short":
        assert plan.Hp < bsize and plan.ys == [0, 0]
    if case == "tiny":
        assert plan.ys == [0, 0] and plan.xs == [0, 0]
    if case == "rows30":
        assert plan.by % 4
    x = _data(shape, "float32", seed=H).to(gpu)
    got = plan.gather(x, cpad)
    want = _torch_tiles(plan, x, cpad)
    assert got.shape == (B * plan.nt, bsize, bsize, cpad) and got.dtype == torch.bfloat16
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(got), _bits(_torch_tiles(plan, x, cpad, mirror=False)))  # the mirroring is in the comparison
    assert not got[..., C:].any()


@pytest.mark.parametrize("kind", ["uint8", "uint16", "float32"])
@pytest.mark.parametrize("case", ["multi", "tiny"])
def test_gather_normalized_mirrors_bit_for_bit(gpu, case, kind):
    from bioengine_worker_amd.cellpose.gpu import normalize99

    shape, bsize = GATHER_CASES[case]
    B, C, H, W = shape
    plan = _plan(H, W, bsize, gpu)
    x = _data(shape, kind, seed=W).to(gpu)
    for cpad in (8, 16):
        got = plan.gather_normalized(x, cpad)
        want = plan.gather(normalize99(x.float()), cpad)
        assert got.shape == want.shape == (B * plan.nt, bsize, bsize, cpad)
        assert torch.equal(_bits(got), _bits(want))
        assert got[..., :C].any() and not got[..., C:].any()  # the channel padding is zero
    # and the normalised image reaches the tiles mirrored
    assert torch.equal(_bits(want), _bits(_torch_tiles(plan, normalize99(x.float()), 16)))


def _oracle_blend(plan, yt_plain, B, H, W):
    """``yt_plain`` [B * nt, nout, by, bx] numpy, already un-mirrored -> (float64 ``average_tiles`` cropped
    to the image [B, nout, H, W], tolerance): four times the largest difference between ``average_tiles``
    accumulated in float32 and in float64 on the same tiles."""
    want, tol = [], 0.0
    for b in range(B):
        t = yt_plain[b * plan.nt: (b + 1) * plan.nt]
        a64 = ref.average_tiles(t, plan.ys, plan.xs, plan.Ly, plan.Lx, dtype=np.float64)
        a32 = ref.average_tiles(t, plan.ys, plan.xs, plan.Ly, plan.Lx)
        tol = max(tol, 4.0 * float(np.abs(a32 - a64).max()))
        want.append(a64[:, plan.pad_y: plan.pad_y + H, plan.pad_x: plan.pad_x + W])
    return np.stack(want), tol


BLEND_CASES = [(70, 90, 32), (20, 100, 64), (300, 260, 224)]


@pytest.mark.parametrize("H,W,bsize", BLEND_CASES)
def test_blend_unmirrors(gpu, H, W, bsize):
    """Independent random tiles (a different value in every tile) blended by the kernel against
    ``average_tiles`` in float64 over the oracle's ``unaugment_tiles``, cropped to the image."""
    plan = _plan(H, W, bsize, gpu)
    assert (plan.ys, plan.xs) == tuple(ac.GEOMETRIES[(H, W, bsize)][1:])
    B, nout = 2, 3
    yt = torch.randn(B * plan.nt, nout, bsize, bsize, generator=torch.Generator().manual_seed(W))
    plain = np.concatenate([ref.unaugment_tiles(yt[b * plan.nt: (b + 1) * plan.nt].numpy(), plan.ys, plan.xs)
                            for b in range(B)])
    want, tol = _oracle_blend(plan, plain, B, H, W)
    got = plan.blend(yt.to(gpu), B)
    assert got.shape == (B, nout, H, W) and got.dtype == torch.float32
    diff = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    # the same tiles blended without un-mirroring are far away: the comparison sees the mirroring
    far, _ = _oracle_blend(plan, yt.numpy(), B, H, W)
    print(f"augmented blend {H} x {W}: tiles {len(plan.ys)} x {len(plan.xs)} of {bsize}, tolerance {tol:.3e}, "
          f"largest difference {diff:.3e} (not un-mirrored: {float(np.abs(far - want).max()):.3e})")
    assert float(np.abs(far - want).max()) > 0.1
    assert 0 < tol < 1e-5 and diff <= tol
    again = plan.blend(yt.to(gpu), B)
    assert torch.equal(got, again)  # bit-deterministic


def _standin_torch(tiles):
    """:func:`cellpose_augment_cases.standin_net` on NHWC bf16 tiles, in torch: [T, 3, by, bx] fp32."""
    t = tiles[..., 0].float()
    p = torch.nn.functional.pad(t, (1, 1, 1, 1))
    return torch.stack([p[:, 2:, 1:-1] - p[:, :-2, 1:-1], p[:, 1:-1, 2:] - p[:, 1:-1, :-2], t], 1).contiguous()


@pytest.mark.parametrize("H,W,bsize", BLEND_CASES)
def test_equivariant_network_on_the_device(gpu, H, W, bsize):
    """Gather under ``augment``, an exactly mirror-equivariant stand-in network, blend under ``augment``:
    the same chain without any mirroring at the same starts must come out (the plain kernels run on a
    copy of the plan)."""
    plan = _plan(H, W, bsize, gpu)
    plain = copy.copy(plan)
    plain.augment, plain._sfx = False, ""
    B = 2
    x = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(H + W)).to(gpu)
    tiles = plan.gather(x, 8)
    tiles_plain = plain.gather(x, 8)
    assert torch.equal(_bits(tiles_plain), _bits(_torch_tiles(plan, x, 8, mirror=False)))
    got = plan.blend(_standin_torch(tiles), B)
    yt_plain = _standin_torch(tiles_plain)
    ref_dev = plain.blend(yt_plain, B)
    want, tol = _oracle_blend(plan, yt_plain.cpu().numpy(), B, H, W)
    d_dev = float((got - ref_dev).abs().max())
    d_orc = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"equivariance {H} x {W} / {bsize}: tolerance {tol:.3e}, against the plain chain {d_dev:.3e}, "
          f"against the float64 oracle {d_orc:.3e}")
    assert tol > 0 and d_dev <= tol and d_orc <= tol
    # channel 2 is the image itself (bf16-rounded): the blend of equal values gives it back
    assert float((got[:, 2] - x[:, 0].bfloat16().float()).abs().max()) <= 1e-5


# ------------------------------------------------------------------ network stage


@pytest.fixture(scope="module")
def runner(gpu):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    return CellposeRunner(device=gpu, seed=0)


def _spy_calls(monkeypatch):
    from bioengine_worker_amd.ops import _native

    names = []
    real = _native.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", call)
    return names


def test_run_net_equals_the_composition_by_hand(gpu, runner):
    from bioengine_worker_amd.cellpose.gpu import normalize99
    from bioengine_worker_amd.cellpose.pipeline import EvalParams, synthetic_cells

    B, H, W = 2, 256, 256
    x = normalize99(torch.from_numpy(synthetic_cells(B, H, W)).to(gpu).float())
    p = EvalParams(augment=True)
    y, style = runner.run_net(x, p)
    plan = runner._plan(H, W, p)
    assert plan.augment and plan.by == plan.bx == 224 and plan.nt == 9
    assert plan is not runner._plan(H, W, EvalParams()) and runner._plan(H, W, EvalParams()).nt == 4
    tiles = _torch_tiles(plan, x, runner.cin_pad)
    yt, st = runner._tile_queue(tiles, p)
    plain = np.concatenate([ref.unaugment_tiles(yt[b * plan.nt: (b + 1) * plan.nt].cpu().numpy(), plan.ys, plan.xs)
                            for b in range(B)])
    want, tol = _oracle_blend(plan, plain, B, H, W)
    diff = float(np.abs(y.cpu().numpy().astype(np.float64) - want).max())
    print(f"run_net(augment=True) {H} x {W}: tolerance {tol:.3e}, largest difference {diff:.3e}")
    assert y.shape == (B, 3, H, W) and 0 < tol and diff <= tol
    s = st.view(B, plan.nt, -1).sum(1)
    assert torch.equal(style, s / torch.sqrt((s * s).sum(1, keepdim=True)).clamp_min(1e-12))
    y0, _ = runner.run_net(x, EvalParams())
    assert not torch.equal(y, y0)
    with pytest.raises(ValueError, match="tile"):
        runner.run_net(x, EvalParams(augment=True, tile=False))


def test_eval_fused_front_equals_unfused(gpu, runner, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    raw = torch.from_numpy(synthetic_cells(2, 96, 128, ncells=12)).to(gpu)
    names = _spy_calls(monkeypatch)
    fused = runner.eval(raw, augment=True)
    assert "be_tiles_gather_norm_aug" in names and "be_tiles_blend_aug" in names
    assert not {"be_tiles_gather_norm", "be_tiles_gather", "be_tiles_blend", "be_pct_normalize"} & set(names)
    del names[:]
    monkeypatch.setattr(cg, "FUSED_FRONT", False)
    unfused = runner.eval(raw.float(), augment=True)
    assert "be_tiles_gather_aug" in names and "be_pct_normalize" in names and "be_tiles_gather_norm_aug" not in names
    assert fused[0].shape == (2, 96, 128) and torch.isfinite(fused[1]).all()
    for a, b in zip(fused, unfused):
        assert torch.equal(a, b)


def test_stack_and_volume_run_with_augment(gpu, runner):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    stack = synthetic_cells(3, 64, 80, ncells=8, seed=5)[:, 0]  # [3, 64, 80]
    m, f, s = runner.eval_stack(stack, augment=True, stitch_threshold=0.25)
    assert m.shape == (3, 64, 80) and f.shape == (3, 3, 64, 80) and s.shape[0] == 3 and torch.isfinite(f).all()
    vol = synthetic_cells(8, 64, 64, ncells=6, seed=6)[:, 0]  # [8, 64, 64]
    m, f, s = runner.eval_3d(vol, augment=True, niter=20)
    assert m.shape == (8, 64, 64) and f.shape == (4, 8, 64, 64) and s.dim() == 1 and torch.isfinite(f).all()


def test_cellpose_sam_with_augment(gpu, monkeypatch):
    """Cellpose-SAM under ``augment``: the network sees only 256 x 256 tiles (an image smaller than
    the tile gives equal starts on both axes: four tiles, one per mirror class), and the stage equals
    the composition by hand."""
    from bioengine_worker_amd.cellpose.gpu import normalize99
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, EvalParams
    from bioengine_worker_amd.models.cpsam import CPSAM

    r = CellposeRunner(CPSAM(dim=256, depth=2, heads=4).randomize_(0), device=gpu)
    assert r.is_sam and r.bsize == 256
    B, H, W = 2, 100, 120
    x = normalize99(_data((B, 3, H, W), "uint16", seed=7).to(gpu).float())
    seen = []
    real = r._sam_tiles
    monkeypatch.setattr(r, "_sam_tiles", lambda t: (seen.append(tuple(t.shape)), real(t))[1])
    p = EvalParams(augment=True)
    y, _ = r.run_net(x, p)
    plan = r._plan(H, W, p)
    assert plan.ys == [0, 0] and plan.xs == [0, 0] and seen == [(B * 4, 256, 256, r.cin_pad)]
    yt = real(_torch_tiles(plan, x, r.cin_pad))
    plain = np.concatenate([ref.unaugment_tiles(yt[b * 4: (b + 1) * 4].cpu().numpy(), plan.ys, plan.xs) for b in range(B)])
    want, tol = _oracle_blend(plan, plain, B, H, W)
    diff = float(np.abs(y.cpu().numpy().astype(np.float64) - want).max())
    print(f"Cellpose-SAM run_net(augment=True) {H} x {W}: tolerance {tol:.3e}, largest difference {diff:.3e}")
    assert y.shape == (B, 3, H, W) and torch.isfinite(y).all() and 0 < tol and diff <= tol
