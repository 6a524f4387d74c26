"""Per-image ``diameter`` on the GPU: the ragged tile plan (``gpu.ScaledTilePlan``) and its kernels
(``be_tiles_gather_scaled``, ``be_tiles_blend_scaled``, ``be_resize_bilinear_ragged``) against the
oracle's ``scaled_tiles`` / ``average_tiles`` / ``resize_bilinear_ref``, and ``CellposeRunner`` with a
list of diameters against its own one-image calls."""
import threading

import numpy as np
import pytest
import torch

import cellpose_augment_cases as ac
from bioengine_worker_amd.cellpose import reference as ref
from test_cellpose_augment_gpu import _data, _spy_calls, _standin_torch

pytestmark = pytest.mark.gpu

DYADIC = [None, 2.0, 0.5, 0.25]
GENERAL = [None, 30 / 17, 30 / 41, 2.0]
SETS = {"dyadic": DYADIC, "general": GENERAL}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _plan(H, W, scales, bsize, augment, gpu):
    from bioengine_worker_amd.cellpose.gpu import ScaledTilePlan

    plan = ScaledTilePlan(H, W, scales, bsize, 0.1, augment=augment, device=gpu)
    assert plan.B == len(scales) and sum(g[3] for g in plan.groups) == plan.nt_total
    if augment or all(min(im["Hs"], im["Ws"]) + 16 >= bsize for im in plan.images):
        assert len(plan.groups) == 1  # one launch of the network: the normal case
    return plan


def _oracle_tiles(plan, x, scales, bsize, augment, cpad, dtype):
    """The oracle's tiles of every image in the plan's order: one [tiles, by, bx, cpad] array per group."""
    per = []
    for b, r in enumerate(scales):
        out = ref.scaled_tiles(x[b], r, bsize, 0.1, augment, dtype)
        assert list(out[1]) == plan.images[b]["ys"] and list(out[2]) == plan.images[b]["xs"]
        per.append(out[0])
    groups = []
    for by, bx, first, n in plan.groups:
        t = np.concatenate([t for t in per if t.shape[2:] == (by, bx)])
        assert t.shape[0] == n
        t = np.pad(t, ((0, 0), (0, cpad - t.shape[1]), (0, 0), (0, 0)))
        groups.append(np.ascontiguousarray(t.transpose(0, 2, 3, 1)))
    return groups


def _image_tiles(plan, groups, b):
    """Rows of image ``b`` out of per-group arrays [tiles, ...]."""
    rows = [t for g in groups for t in g]
    t0 = int(plan.itab[b, 6])
    return np.stack(rows[t0: t0 + plan.images[b]["nt"]])


# ------------------------------------------------------------------ gather


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("cpad", [8, 16])
@pytest.mark.parametrize("bsize", [32, 64])
def test_gather_scaled_exact(gpu, bsize, cpad, augment):
    """Dyadic scales on 72 x 88 (every ``H * r`` an integer, weights 1/4, 1/2, 3/4) and integer pixels
    in [0, 255]: every product of the lerp is exact, so the tiles are bf16 of the oracle bit for bit --
    zero padding, channel padding, mirror flags and the second tile-shape group included."""
    B, C, H, W = 4, 2, 72, 88
    x = torch.randint(0, 256, (B, C, H, W), generator=torch.Generator().manual_seed(bsize + cpad)).float()
    plan = _plan(H, W, DYADIC, bsize, augment, gpu)
    assert [(im["Hs"], im["Ws"]) for im in plan.images] == [(72, 88), (144, 176), (36, 44), (18, 22)]
    if bsize == 64 and not augment:  # 18 x 22 pads to 48 x 48, below the tile: its own group
        assert [(g[0], g[1]) for g in plan.groups] == [(64, 64), (48, 48)]
    got = plan.gather(x.to(gpu), cpad)
    want = _oracle_tiles(plan, x.numpy(), DYADIC, bsize, augment, cpad, np.float32)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        w = torch.from_numpy(w).to(torch.bfloat16)
        assert g.shape == w.shape and g.dtype == torch.bfloat16
        assert torch.equal(_bits(g.cpu()), _bits(w))
        assert g[..., :C].any() and not g[..., C:].any()
    flags = set(plan.tiles_t[:, 3].tolist())
    assert flags == ({0, 1, 2, 3} if augment else {0})  # under augment all four mirror classes are in the comparison
    if augment:  # and a mirrored tile differs from the window it was cut from
        k = plan.tiles_t[:, 3].tolist().index(3)
        assert not torch.equal(got[0][k], got[0][k].flip(0, 1))


NORM_CASES = {
    "uint8": ("uint8", {}),
    "uint16": ("uint16", {}),
    "float32": ("float32", {}),
    "lowhigh": ("uint16", {"lowhigh": (50.0, 3000.0)}),
    "invert": ("float32", {"invert": True}),
    "percentile": ("uint8", {"percentile": (3.0, 97.0)}),
}


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("case", list(NORM_CASES))
def test_gather_scaled_fused_normalisation(gpu, case, augment):
    """General ratios from raw pixels.  Yardstick: the float64 oracle's tiles of the image normalised by
    the (separately tested) unfused kernels.  Bound per element: one bf16 rounding, ``2^-8 |want|``, plus
    four times the largest float32-vs-float64 difference of the oracle on the same image."""
    from bioengine_worker_amd.cellpose.gpu import normalize99, normalize_img_gpu
    from bioengine_worker_amd.cellpose.pipeline import norm_params

    kind, opts = NORM_CASES[case]
    B, C, H, W, bsize, cpad = 4, 2, 70, 90, 32, 8
    x = _data((B, C, H, W), kind, seed=len(case)).to(gpu)
    params = norm_params(opts) if opts else None
    xn = normalize99(x.float()) if params is None else normalize_img_gpu(x, params)
    plan = _plan(H, W, GENERAL, bsize, augment, gpu)
    got = plan.gather_normalized(x, cpad, params=params)
    pre = plan.gather(xn, cpad)  # the fp32, already normalised source form
    w64 = _oracle_tiles(plan, xn.cpu().numpy(), GENERAL, bsize, augment, cpad, np.float64)
    w32 = _oracle_tiles(plan, xn.cpu().numpy(), GENERAL, bsize, augment, cpad, np.float32)
    o_err = max(float(np.abs(a - b).max()) for a, b in zip(w32, w64))
    assert 0 < o_err < 1e-4
    for g, p, w in zip(got, pre, w64):
        assert torch.equal(_bits(g), _bits(p))
        bound = 2.0 ** -8 * np.abs(w) + 4 * o_err
        diff = np.abs(g.float().cpu().numpy().astype(np.float64) - w)
        print(f"scaled gather {case} augment={augment} tiles {g.shape}: bound {bound.max():.3e} (oracle part {4 * o_err:.3e}), "
              f"largest difference {diff.max():.3e}, largest difference / bound {(diff / bound).max():.3f}")
        assert (diff <= bound).all()
        assert g[..., :C].any() and not g[..., C:].any()


@pytest.mark.parametrize("augment", [False, True])
def test_gather_scaled_large_tile(gpu, augment):
    """300 x 260 with the network's 224 tile, general ratios, raw uint16."""
    from bioengine_worker_amd.cellpose.gpu import normalize99

    B, C, H, W, bsize, cpad = 4, 2, 300, 260, 224, 8
    x = _data((B, C, H, W), "uint16", seed=5).to(gpu)
    xn = normalize99(x.float())
    plan = _plan(H, W, GENERAL, bsize, augment, gpu)
    got = plan.gather_normalized(x, cpad)
    w64 = _oracle_tiles(plan, xn.cpu().numpy(), GENERAL, bsize, augment, cpad, np.float64)
    w32 = _oracle_tiles(plan, xn.cpu().numpy(), GENERAL, bsize, augment, cpad, np.float32)
    o_err = max(float(np.abs(a - b).max()) for a, b in zip(w32, w64))
    # 260 * 30 / 41 = 190 pads to 208, narrower than the tile: that image is a group of its own
    assert [(g[0], g[1]) for g in plan.groups] == ([(224, 224)] if augment else [(224, 224), (224, 208)]) and 0 < o_err < 1e-3
    for g, w in zip(got, w64):
        bound = 2.0 ** -8 * np.abs(w) + 4 * o_err
        diff = np.abs(g.float().cpu().numpy().astype(np.float64) - w)
        print(f"scaled gather 300 x 260 / 224 tiles {tuple(g.shape)}: oracle part of the bound {4 * o_err:.3e}, "
              f"largest difference {diff.max():.3e}")
        assert (diff <= bound).all()


# ------------------------------------------------------------------ blend and ragged resize

#: Standard deviation of the random tile outputs.  The tolerance below is the float32 rounding of the
#: oracle chain, which for general ratios is dominated by the source coordinate: half an ulp of a
#: coordinate near 530 (300 x 30 / 17) is 3e-5 of a pixel, times the step between neighbouring blended
#: values.  Unit-variance tiles put four times that at 1e-4 .. 6e-4; at 2^-7 it is below the 1e-5 the
#: test asserts, and a power of two changes no mantissa: the comparison is as tight relative to the data.
TILE_STD = 2.0 ** -7


def _oracle_chain(plan, yts, H, W, augment, dtype, unmirror=True):
    """Tile outputs (numpy, one array per group) -> [B, nout, H, W]: un-mirror, ``average_tiles``, crop
    to the scaled image, ``resize_bilinear_ref``, all in ``dtype``."""
    out = []
    for b, im in enumerate(plan.images):
        t = _image_tiles(plan, yts, b)
        if augment and unmirror:
            t = ref.unaugment_tiles(t, im["ys"], im["xs"])
        Ly = max(im["ys"]) + im["by"]
        Lx = max(im["xs"]) + im["bx"]
        a = ref.average_tiles(t, im["ys"], im["xs"], Ly, Lx, dtype=dtype)
        a = a[:, im["pad_y"]: im["pad_y"] + im["Hs"], im["pad_x"]: im["pad_x"] + im["Ws"]]
        out.append(a if (im["Hs"], im["Ws"]) == (H, W) else ref.resize_bilinear_ref(a, (H, W), dtype))
    return np.stack(out)


BLEND_CASES = [(72, 88, 32), (70, 90, 64), (300, 260, 224)]


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("scales", list(SETS))
@pytest.mark.parametrize("H,W,bsize", BLEND_CASES)
def test_blend_and_ragged_resize(gpu, H, W, bsize, scales, augment):
    """Independent random tiles against float64 ``average_tiles`` then float64 ``resize_bilinear_ref``.
    Tolerance: four times the float32-vs-float64 difference of that same chain."""
    sc = SETS[scales]
    plan = _plan(H, W, sc, bsize, augment, gpu)
    gen = torch.Generator().manual_seed(W + bsize)
    yts = [torch.randn(n, 3, by, bx, generator=gen) * TILE_STD for by, bx, _, n in plan.groups]
    ynp = [y.numpy() for y in yts]
    want = _oracle_chain(plan, ynp, H, W, augment, np.float64)
    tol = 4.0 * float(np.abs(_oracle_chain(plan, ynp, H, W, augment, np.float32) - want).max())
    dev = [y.to(gpu) for y in yts]
    flat = plan.blend(dev)
    got = plan.resize_back(flat, 3)
    assert got.shape == (len(sc), 3, H, W) and got.dtype == torch.float32
    diff = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"ragged blend + resize {H} x {W} / {bsize} {scales} augment={augment}: groups {[g[:2] for g in plan.groups]}, "
          f"tolerance {tol:.3e}, largest difference {diff:.3e}")
    assert 0 < tol < 1e-5 and diff <= tol
    assert torch.equal(plan.resize_back(plan.blend(dev), 3), got)  # bit-deterministic
    # an image that is not rescaled comes back as its blend, untouched by the resize
    assert torch.equal(got[0], plan.scaled_flow(flat, 0, 3))
    if augment:  # the same tiles blended without un-mirroring are far away
        far = plan.resize_back(plan.blend(dev, unmirror=False), 3).cpu().numpy()
        d_far = float(np.abs(far - want).max())
        print(f"  not un-mirrored: {d_far:.3e}")
        assert d_far > 0.1 * TILE_STD


# ------------------------------------------------------------------ round trip


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("scales", list(SETS))
@pytest.mark.parametrize("H,W,bsize", BLEND_CASES[:2])
def test_round_trip_with_a_standin_network(gpu, H, W, bsize, scales, augment):
    """Gather, the mirror-equivariant stand-in network, blend, resize, against the same chain of the
    oracle in float64.  The bound combines the two above: a tile element is off by at most ``e_g = 2^-8
    max|tile| + 4 max|oracle32 - oracle64|``; the stand-in's differences double that, blending and
    resampling are convex combinations and add the chain's own float32 rounding."""
    from bioengine_worker_amd.cellpose.gpu import normalize99

    sc = SETS[scales]
    B = len(sc)
    x = normalize99(_data((B, 1, H, W), "uint16", seed=H + bsize).to(gpu).float())
    xn = x.cpu().numpy()
    plan = _plan(H, W, sc, bsize, augment, gpu)
    tiles = plan.gather(x, 8)
    got = plan.resize_back(plan.blend([_standin_torch(t) for t in tiles]), 3).cpu().numpy().astype(np.float64)
    t64 = _oracle_tiles(plan, xn, sc, bsize, augment, 8, np.float64)
    t32 = _oracle_tiles(plan, xn, sc, bsize, augment, 8, np.float32)
    e_g = 2.0 ** -8 * max(float(np.abs(t).max()) for t in t64) + 4 * max(float(np.abs(a - b).max()) for a, b in zip(t32, t64))
    y64 = [ac.standin_net(t.transpose(0, 3, 1, 2)) for t in t64]
    want = _oracle_chain(plan, y64, H, W, augment, np.float64)
    y32 = [y.astype(np.float32) for y in y64]
    tol = 4.0 * float(np.abs(_oracle_chain(plan, y32, H, W, augment, np.float32) - _oracle_chain(plan, y32, H, W, augment, np.float64)).max())
    diff = np.abs(got - want).max(axis=(0, 2, 3))
    print(f"round trip {H} x {W} / {bsize} {scales} augment={augment}: tile bound {e_g:.3e}, chain tolerance {tol:.3e}, "
          f"largest differences per channel {diff}")
    assert tol > 0 and (diff[:2] <= 2 * e_g + tol).all() and diff[2] <= e_g + tol
    # channel 2 is the image itself: down and up again, within one bf16 rounding (and the chain's own)
    updown = np.stack([xn[b, 0] if r is None else ref.resize_bilinear_ref(
        ref.resize_bilinear_ref(xn[b, 0], (ref.scaled_size(H, r), ref.scaled_size(W, r)), np.float64), (H, W), np.float64)
        for b, r in enumerate(sc)])
    assert float(np.abs(got[:, 2] - updown).max()) <= e_g + tol


# ------------------------------------------------------------------ runner


@pytest.fixture(scope="module")
def runner(gpu):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    return CellposeRunner(device=gpu, seed=0)


@pytest.fixture(scope="module")
def cells(gpu):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    return torch.from_numpy(synthetic_cells(3, 160, 200)).to(gpu)


def test_eval_list_equals_one_image_calls(gpu, runner, cells, monkeypatch):
    from bioengine_worker_amd.cellpose.gpu import RAW_DTYPES
    from bioengine_worker_amd.ops import _native

    names = _spy_calls(monkeypatch)
    spied, gathers = _native.call, []
    monkeypatch.setattr(_native, "call", lambda name, *a: (gathers.append(a) if name == "be_tiles_gather_scaled" else None,
                                                         spied(name, *a))[1])
    m, y, s = runner.eval(cells, diameter=[15, None, 60])
    # 160 x 200 at r = 2, 1 and 0.5 is three tile shapes (two of them below the 224 tile): one gather each,
    # every one on the raw uint16 batch, normalising in the load
    assert len(gathers) == 3
    for g in gathers:
        assert g[0].value == cells.data_ptr() and g[1:4] == (RAW_DTYPES[torch.uint16], 1, 3)
    assert "be_tiles_gather_scaled" in names and "be_tiles_blend_scaled" in names and "be_resize_bilinear_ragged" in names
    assert not {"be_pct_normalize", "be_resize_bilinear", "be_tiles_gather", "be_tiles_gather_norm"} & set(names)
    assert cells.dtype == torch.uint16  # the gather ran on the raw batch
    assert m.shape == (3, 160, 200) and y.shape == (3, 3, 160, 200) and torch.isfinite(y).all()
    assert m.diameters.dtype == torch.float32 and not m.diameters.is_cuda and m.diameters.tolist() == [15.0, 0.0, 60.0]
    for b, d in enumerate([15, None, 60]):
        mb, yb, sb = runner.eval(cells[b: b + 1], diameter=[d])
        bound = 1e-2 * float(yb.abs().max())
        diff = float((y[b] - yb[0]).abs().max())
        print(f"image {b} diameter {d}: batch vs alone {diff:.3e} (bound {bound:.3e})")
        assert diff <= bound and mb.diameters.tolist() == [float(d or 0)]
    assert not torch.equal(y[0], y[1])


def test_niter_unset_recovers_masks_per_group(gpu, runner, cells):
    """With ``niter`` unset every image gets ``int(200 / r_b)`` steps: the masks of the batch are those
    of every image recovered alone from the same flows."""
    from bioengine_worker_amd.cellpose.pipeline import EvalParams, PerImageRescale

    diams = [15.0, None, 60.0, 15.0]
    x = torch.cat([cells, cells[1:2]])
    p = EvalParams(niter=0)
    m, y, _ = runner.eval(x, p, diameter=diams)
    rescale = PerImageRescale([2.0, 1.0, 0.5, 2.0], diams)
    assert [int(200 / r) for r in rescale] == [100, 200, 400, 100]
    assert torch.equal(runner.compute_masks(y, p, rescale), m) and m.diameters.tolist() == [15.0, 0.0, 60.0, 15.0]
    for b, r in enumerate(rescale):
        assert torch.equal(runner.compute_masks(y[b: b + 1].contiguous(), p, r), m[b: b + 1])
    assert int(m.max()) < m.label_bound


def test_eval_list_without_a_rescale_is_the_unscaled_path(gpu, runner, cells):
    m0, y0, s0 = runner.eval(cells)
    m, y, s = runner.eval(cells, diameter=[30 / 1.0005, None, 30.0])
    assert torch.equal(m, m0) and torch.equal(y, y0) and torch.equal(s, s0)
    assert m.diameters.tolist() == [0.0, 0.0, 0.0] and not hasattr(m0, "diameters")


def test_stream_and_eval_locked_carry_the_list(gpu, runner, cells):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams

    diams = [15, None, 60]
    m, y, s = runner.eval(cells, diameter=diams)
    st = runner.stream(EvalParams(diameter=diams))
    assert st.submit(cells) is None
    ms, ys, ss = st.flush()
    ml, yl, sl, ev = runner.eval_locked(cells, threading.Lock(), threading.Lock(), diameter=diams)
    ev.synchronize()
    for a, b, c in ((ms, ys, ss), (ml, yl, sl)):
        assert torch.equal(a, m) and torch.equal(b, y) and torch.equal(c, s) and a.diameters.tolist() == [15.0, 0.0, 60.0]
    # the pipelined form splits the diameters with the images
    mp, yp, _ = runner.eval(torch.cat([cells, cells[:1]]), diameter=diams + [15], pipeline_chunks=2, pipeline_min_chunk=2)
    assert mp.diameters.tolist() == [15.0, 0.0, 60.0, 15.0]
    assert float((yp[:3] - y).abs().max()) <= 1e-2 * float(y.abs().max())
    with pytest.raises(ValueError, match="diameter"):
        runner.eval(cells, diameter=[15, 30])


def test_auto_diameter_on_the_device(gpu, runner, cells):
    """``"auto"``: the estimate is the oracle's ``diameter_px`` of the pass-1 masks, and the images
    that need no second pass keep their pass-1 result."""
    m0, y0, _ = runner.eval(cells)
    want = np.array([t["diameter_px"] for t in runner.measure(m0)])
    assert np.array_equal(runner.estimate_diameters(m0).astype(np.float32), want.astype(np.float32))
    m, y, _ = runner.eval(cells, diameter="auto")
    assert torch.equal(m.diameters, torch.tensor(want, dtype=torch.float32))
    for b, d in enumerate(want):
        if not (d > 0 and abs(runner.diam_mean / d - 1) > 1e-3):
            assert torch.equal(m[b], m0[b]) and torch.equal(y[b], y0[b])
