"""Cellpose 2-D mask recovery on the GPU (``csrc/kernels/cellpose_dynamics.hip``) stage by stage against
the oracle, on the small ragged shapes of ``cellpose2d_cases``: ``be_cp_prep_flow`` bit for bit; every
flow-following launch against a float64 model after 0, 1 and 3 steps of random flows; on capped flows
(end points mid-bin) histogram, bins and final masks **equal** to ``reference``; ``get_masks_gpu`` equal
to ``reference.get_masks`` on every hand-built seeding / expansion rule, alone and stacked into a batch;
the run-length counters of ``be_cp_label_lookup``; and the tile gather / blend kernels against
``make_tiles`` / ``average_tiles``."""
import numpy as np
import pytest
import torch

import cellpose2d_cases as cc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu

#: (entry point, BE_FOLLOW_TILE or None): the five flow-following launches
ENTRIES = [("be_cp_follow_flows", None), ("be_cp_follow_flows_xcd", None), ("be_cp_follow_flows_xcd_pool", None),
           ("be_cp_follow_flows_lds", None), ("be_cp_follow_flows_lds", "32")]
ENTRY_IDS = ["plain", "xcd", "xcd_pool", "lds16", "lds32"]


def _follow(monkeypatch, y, entry, **kw):
    from bioengine_worker_amd.cellpose.gpu import follow_flows_gpu

    name, tile = entry
    if tile is None:
        monkeypatch.delenv("BE_FOLLOW_TILE", raising=False)
    else:
        monkeypatch.setenv("BE_FOLLOW_TILE", tile)
    return follow_flows_gpu(y, entry=name, **kw)


def _assert_hist_of_pos(hist, pos):
    """``hist`` [B, Hp, Wp] is exactly the histogram of the non-negative entries of ``pos`` [B, H, W]."""
    hist, pos = hist.cpu().numpy(), pos.cpu().numpy()
    for b in range(pos.shape[0]):
        want = np.bincount(pos[b][pos[b] >= 0], minlength=hist[b].size).reshape(hist[b].shape)
        assert np.array_equal(hist[b], want), b


# ------------------------------------------------------------------ 1. prep_flow


def test_prep_flow_is_exact(gpu):
    """``fg = cellprob > thr`` (strict; NaN is background), ``flow2 = float32(dP) * float32(0.2)`` on the
    foreground and 0 elsewhere, in (dy, dx) order -- bit for bit."""
    from bioengine_worker_amd.cellpose.gpu import follow_flows_gpu

    rng = np.random.default_rng(11)
    y = rng.standard_normal((2, 3, 37, 53)).astype(np.float32) * 3
    thr = np.float32(0.3)
    cp = y[:, 2].reshape(-1)  # a copy: written back below
    cp[::7] = thr  # exactly at the threshold: background
    cp[3::11] = np.nextafter(thr, np.float32(1))  # one ulp above: foreground
    y[:, 2] = cp.reshape(2, 37, 53)
    y[1, 2, 5, 6] = np.nan
    _, _, flow2, fg = follow_flows_gpu(torch.from_numpy(y).to(gpu), niter=0, cellprob_threshold=float(thr), with_flow=True)
    assert flow2.shape == (2, 37, 53, 2) and flow2.dtype == torch.float32 and fg.shape == (2, 37, 53) and fg.dtype == torch.uint8
    want_fg = y[:, 2] > thr
    assert not want_fg[1, 5, 6] and not want_fg[0, 0, 0] and want_fg[0, 0, 3] and 0.3 < want_fg.mean() < 0.6
    assert np.array_equal(fg.cpu().numpy(), want_fg.astype(np.uint8))
    want = np.where(want_fg[..., None], np.moveaxis(y[:, :2], 1, -1) * np.float32(0.2), np.float32(0)).astype(np.float32)
    assert np.array_equal(flow2.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ 2. short horizons against the float64 model


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
@pytest.mark.parametrize("niter", [0, 1, 3])
@pytest.mark.parametrize("shape", [(37, 53), (45, 77)])
def test_short_horizon_matches_float64_model(gpu, monkeypatch, shape, niter, entry):
    """Random flows, 80 % random foreground, three images (blocks of 256 and 1,024 pixels straddle
    them; ragged tiles; a block count that is no multiple of 8).  Every foreground pixel's bin equals
    the model's unless its pre-clamp end point is within 1e-3 of a bin edge.  Excluded share measured
    on the model: 0.23 % / 0.30 % of the foreground at 37 x 53 and 0.45 % / 0.42 % at 45 x 77 after
    1 / 3 steps (the cap is 2 %); nothing is excluded without a step."""
    want, excl, fg = cc.random_model(shape, niter)
    assert excl.sum() <= 0.02 * fg.sum() and (niter > 0 or not excl.any())
    y = torch.from_numpy(cc.random_flows(shape)).to(gpu)
    hist, pos = _follow(monkeypatch, y, entry, niter=niter)
    assert hist.shape == (3, shape[0] + 40, shape[1] + 40) and hist.dtype == pos.dtype == torch.int32
    got = pos.cpu().numpy()
    assert (got[~fg] == -1).all() and (got[fg] >= 0).all()
    bad = (got != want) & ~excl
    print(f"{shape} niter {niter}: excluded {excl.sum()} of {fg.sum()}, differing inside the excluded set "
          f"{int(((got != want) & excl).sum())}, outside {int(bad.sum())}")
    assert not bad.any()
    _assert_hist_of_pos(hist, pos)
    assert int(hist.sum()) == int(fg.sum())


# ------------------------------------------------------------------ 3. capped flows


@pytest.mark.parametrize("name", ["a", "big", "edge", "thin", "tiny"])
def test_capped_flows_exact(gpu, monkeypatch, name):
    from bioengine_worker_amd.cellpose.gpu import compute_masks_gpu

    v, o = cc.image(name, "capped"), cc.oracle(name, "capped")
    want_hist, want_pos = (torch.from_numpy(a)[None] for a in cc.hist_pos(o["bins"], o["inds"], v["shape"]))
    y = torch.from_numpy(v["y"])[None].to(gpu)
    for entry in ENTRIES:
        hist, pos = _follow(monkeypatch, y, entry)
        assert torch.equal(pos.cpu(), want_pos), entry  # every foreground pixel's bin, -1 elsewhere
        assert torch.equal(hist.cpu(), want_hist), entry
    monkeypatch.delenv("BE_FOLLOW_TILE", raising=False)
    m = compute_masks_gpu(y)
    assert m.dtype == torch.int32 and m.shape == (1,) + v["shape"] and m.device.type == "cuda"
    assert torch.equal(m[0].cpu(), torch.from_numpy(o["masks"]))
    assert int(m.max()) == (2 if name == "edge" else v["n"])


def test_capped_flows_exact_in_a_batch(gpu, monkeypatch):
    """Three layouts on 45 x 77, one without foreground: pixel blocks straddle the images, and one image
    has no seed while the batch's ``kmax`` is 4.  Each image equals its single-image result and the oracle."""
    from bioengine_worker_amd.cellpose.gpu import compute_masks_gpu, follow_and_label

    names = ["a", "empty", "a2"]
    vs, os_ = [cc.image(n, "capped") for n in names], [cc.oracle(n, "capped") for n in names]
    hp = [cc.hist_pos(o["bins"], o["inds"], v["shape"]) for v, o in zip(vs, os_)]
    want_hist, want_pos = (torch.from_numpy(np.stack([a[i] for a in hp])) for i in (0, 1))
    y = torch.from_numpy(np.stack([v["y"] for v in vs])).to(gpu)
    for entry in ENTRIES:
        hist, pos = _follow(monkeypatch, y, entry)
        assert torch.equal(pos.cpu(), want_pos) and torch.equal(hist.cpu(), want_hist), entry
    monkeypatch.delenv("BE_FOLLOW_TILE", raising=False)
    raw, nlab = follow_and_label(y, with_bound=True)
    assert nlab == 5 and raw.cpu().amax((1, 2)).tolist() == [4, 0, 3]
    m = compute_masks_gpu(y)
    for b, o in enumerate(os_):
        assert torch.equal(raw[b].cpu(), torch.from_numpy(o["raw"])), names[b]
        assert torch.equal(m[b].cpu(), torch.from_numpy(o["masks"])), names[b]
        assert torch.equal(m[b], compute_masks_gpu(y[b: b + 1])[0]), names[b]
    assert m.cpu().amax((1, 2)).tolist() == [4, 0, 3]


# ------------------------------------------------------------------ 4. unit flows at ragged shapes


@pytest.mark.parametrize("name", ["a", "big"])
def test_unit_flows_match(gpu, monkeypatch, name):
    from bioengine_worker_amd.cellpose.gpu import compute_masks_gpu

    v, o = cc.image(name, "unit"), cc.oracle(name, "unit")
    y = torch.from_numpy(v["y"])[None].to(gpu)
    m = compute_masks_gpu(y)[0].cpu().numpy()
    frac = cc.match_fraction(o["masks"], m)
    print(f"unit {name}: instances {int(m.max())} (oracle {int(o['masks'].max())}), match fraction {frac:.5f}")
    assert int(m.max()) == int(o["masks"].max()) == v["n"]
    assert frac > 0.99
    outs = [_follow(monkeypatch, y, entry) for entry in ENTRIES]
    assert int(outs[0][0].sum()) == int((v["truth"] > 0).sum())
    for hist, pos in outs[1:]:
        assert torch.equal(hist, outs[0][0]) and torch.equal(pos, outs[0][1])
    _assert_hist_of_pos(*outs[0])


# ------------------------------------------------------------------ 5. get_masks_gpu rules


def _hist_pos_t(shape, p, inds, gpu):
    hist, pos = cc.hist_pos(cc.end_bins(p, shape), inds, shape)
    return torch.from_numpy(hist)[None].to(gpu), torch.from_numpy(pos)[None].to(gpu)


def _check_get_masks(gpu, shape, p, inds, **kw):
    from bioengine_worker_amd.cellpose.gpu import get_masks_gpu

    want = ref.get_masks(p, inds, shape, **kw)
    hist, pos = _hist_pos_t(shape, p, inds, gpu)
    got = get_masks_gpu(hist, pos, shape, **kw)
    assert got.dtype == torch.int32 and tuple(got.shape) == (1,) + tuple(shape)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want))
    return want


@pytest.mark.parametrize("name", sorted(cc.RULES))
def test_get_masks_rules(gpu, name):
    shape, (p, inds) = cc.RULES[name]()
    want = _check_get_masks(gpu, shape, p, inds)
    assert want.any()
    if name == "oversize":
        assert (want > 0).sum() == 12
        assert (_check_get_masks(gpu, shape, p, inds, max_size_fraction=0.7) > 0).sum() == 50


def test_get_masks_rules_as_one_batch(gpu):
    """The rule cases of one shape stacked: images with 1 and 2 seeds side by side (the short rows' free
    key slots hold sort sentinels).  Each image equals its own single-image result and the oracle."""
    from bioengine_worker_amd.cellpose.gpu import get_masks_gpu

    names = [n for n in sorted(cc.RULES) if cc.RULES[n]()[0] == cc.SHAPE]
    assert len(names) == 8
    cases = [cc.RULES[n]() for n in names]
    hp = [_hist_pos_t(shape, p, inds, gpu) for shape, (p, inds) in cases]
    hist, pos = torch.cat([h for h, _ in hp]), torch.cat([q for _, q in hp])
    got, nlab = get_masks_gpu(hist, pos, cc.SHAPE, with_bound=True)
    assert nlab == 3 and sorted(set(got.cpu().amax((1, 2)).tolist())) == [1, 2]
    for b, (n, (shape, (p, inds))) in enumerate(zip(names, cases)):
        assert torch.equal(got[b].cpu(), torch.from_numpy(ref.get_masks(p, inds, shape))), n
        assert torch.equal(got[b], get_masks_gpu(hp[b][0], hp[b][1], shape)[0]), n


def test_get_masks_lattice_of_seeds(gpu):
    """225 seeds of equal count: more than one workgroup expands (four per workgroup), ordered by the
    raster tie-break alone."""
    shape, (p, inds) = cc.lattice()
    assert int(_check_get_masks(gpu, shape, p, inds).max()) == 225


# ------------------------------------------------------------------ 6. window at the histogram border


def test_get_masks_window_at_the_histogram_border(gpu):
    """Seeds in the first and last bins an end point can have: their windows end 15 bins inside the
    padded image; a hand-made histogram may also put one in the very corner, where the window is cut."""
    from bioengine_worker_amd.cellpose.gpu import get_masks_gpu

    shape = cc.SHAPE
    want = _check_get_masks(gpu, shape, *cc._points(shape, [((0, 0), 12), ((0, 1), 4), ((12, 28), 12), ((12, 27), 3)]))
    assert int(want.max()) == 2 and (want > 0).sum() == 31
    hist = torch.zeros(1, 53, 69, dtype=torch.int32)
    hist[0, 0, 0], hist[0, 0, 1], hist[0, 52, 68], hist[0, 51, 67] = 12, 3, 20, 3
    pos = torch.full((1,) + shape, -1, dtype=torch.int32)
    pos.view(-1)[:4] = torch.tensor([0, 1, 53 * 69 - 1, 51 * 69 + 67], dtype=torch.int32)
    got = get_masks_gpu(hist.to(gpu), pos.to(gpu), shape).cpu()
    assert got.view(-1)[:4].tolist() == [1, 1, 2, 2] and int((got > 0).sum()) == 4


# ------------------------------------------------------------------ 7. label_lookup counters


def test_label_lookup_counters(gpu):
    """``be_cp_label_lookup`` on its own: 37 pixels per image (four 8-pixel runs and a tail of 5), labels
    that change inside and across the runs, background gaps; ``M0`` and the per-label counts equal
    numpy and the background counter stays 0."""
    from bioengine_worker_amd.ops import _native

    B, HW, HWp, nlab = 2, 37, 50, 6
    M1 = np.zeros((B, HWp), np.int32)
    M1[0] = np.arange(HWp) % nlab
    M1[1] = (np.arange(HWp) // 3) % nlab
    runs = [(1, 3), (2, 5), (2, 3), (-1, 2), (3, 9), (0, 4), (5, 1), (4, 8), (1, 2)]  # (label or -1 = background, length)
    pos = np.full((B, HW), -1, np.int32)
    seq = np.concatenate([np.full(n, l) for l, n in runs])
    assert seq.size == HW
    for b in range(B):
        for q, l in enumerate(seq):
            if l >= 0:
                cand = np.nonzero(M1[b] == l)[0]
                pos[b, q] = cand[(q * 7 + b) % len(cand)]  # the same label through different bins
    pos[1] = pos[1][::-1]
    want_M0 = np.where(pos >= 0, np.take_along_axis(M1, np.maximum(pos, 0), 1), 0)
    want_counts = np.stack([np.bincount(want_M0[b], minlength=nlab) for b in range(B)])
    assert (want_counts[:, 0] > 0).all()  # background and label-0 bins occur ...
    want_counts[:, 0] = 0  # ... and are not counted
    assert (want_counts[:, 1:] > 0).all() and np.array_equal(want_M0[0], np.where(seq >= 0, seq, 0))
    pos_t, M1_t = torch.from_numpy(pos).to(gpu), torch.from_numpy(M1).to(gpu)
    M0 = torch.full((B, HW), -7, dtype=torch.int32, device=gpu)
    counts = torch.zeros(B, nlab, dtype=torch.int32, device=gpu)
    _native.call("be_cp_label_lookup", _native.ptr(pos_t), _native.ptr(M1_t), B, HW, HWp, _native.ptr(M0),
                 _native.ptr(counts), nlab, _native.stream(gpu))
    assert np.array_equal(M0.cpu().numpy(), want_M0)
    assert np.array_equal(counts.cpu().numpy(), want_counts)


# ------------------------------------------------------------------ 8. misfit shapes


@pytest.mark.parametrize("H,W", [(1, 9), (9, 1), (1, 1)])
def test_one_pixel_axes_are_rejected(gpu, H, W):
    from bioengine_worker_amd.cellpose.gpu import compute_masks_gpu, follow_flows_gpu, get_masks_gpu

    y = torch.ones(2, 3, H, W, device=gpu)
    with pytest.raises(ValueError, match="two rows and two columns"):
        follow_flows_gpu(y)
    with pytest.raises(ValueError, match="two rows and two columns"):
        compute_masks_gpu(y)
    hist = torch.zeros(2, H + 40, W + 40, dtype=torch.int32, device=gpu)
    pos = torch.full((2, H, W), -1, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="two rows and two columns"):
        get_masks_gpu(hist, pos, (H, W))
    with pytest.raises(ValueError, match="do not fit"):
        get_masks_gpu(torch.zeros(2, 49, 53, dtype=torch.int32, device=gpu),
                      torch.full((2, 9, 12), -1, dtype=torch.int32, device=gpu), (9, 13))


# ------------------------------------------------------------------ 9. tiles


def _plan_and_pads(H, W, gpu):
    from bioengine_worker_amd.cellpose.gpu import TilePlan

    plan = TilePlan(H, W, device=gpu)
    (ya, yb), (xa, xb) = ref.pad_amounts(H), ref.pad_amounts(W)
    assert (ya, xa) == (plan.pad_y, plan.pad_x) and (H + ya + yb, W + xa + xb) == (plan.Hp, plan.Wp)
    return plan, (ya, yb), (xa, xb)


@pytest.mark.parametrize("H,W", [(300, 260), (100, 500)])
def test_tiles_gather_equals_make_tiles(gpu, H, W):
    """Zero padding, channel padding, NHWC layout and the bf16 cast: ``gather`` equals ``make_tiles`` of the
    zero-padded image rounded to bf16 (round to nearest even, as ``Tensor.bfloat16``), bit for bit."""
    plan, py, px = _plan_and_pads(H, W, gpu)
    B, C = 2, 3
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H))
    x[0, 0, 0, :3] = torch.tensor([1.00390625, 1.01171875, -1.00390625])  # rounding ties: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    t = plan.gather(x.to(gpu), 8)
    assert t.shape == (B * plan.nt, plan.by, plan.bx, 8) and t.dtype == torch.bfloat16
    want = []
    for b in range(B):
        tiles, ys, xs = ref.make_tiles(np.pad(x[b].numpy(), ((0, 0), py, px)))
        assert (ys, xs) == (plan.ys, plan.xs) and tiles.shape[2:] == (plan.by, plan.bx)
        want.append(tiles)
    want = torch.from_numpy(np.concatenate(want)).bfloat16().permute(0, 2, 3, 1)  # [B * nt, by, bx, C]
    got = t.cpu()
    assert (want == 0).float().mean() > 0.01  # the padding is in the comparison
    assert torch.equal(got[..., :C].contiguous().view(torch.int16), want.contiguous().view(torch.int16))
    assert not got[..., C:].contiguous().view(torch.int16).any()


@pytest.mark.parametrize("H,W", [(300, 260), (100, 500)])
def test_tiles_blend_equals_average_tiles(gpu, H, W):
    """Independent random tiles (a different value in every tile, so the weights matter) blended by the
    kernel against ``average_tiles`` in float64, cropped by the padding.  Tolerance: four times the
    largest difference between ``average_tiles`` accumulated in float32 and in float64 on the same
    tiles (another summation order over the at most four tiles of a pixel); it comes to 1.8e-6 at
    300 x 260 and 1.6e-6 at 100 x 500."""
    plan, (ya, _), (xa, _) = _plan_and_pads(H, W, gpu)
    B, nout = 2, 3
    yt = torch.randn(B * plan.nt, nout, plan.by, plan.bx, generator=torch.Generator().manual_seed(W))
    want, tol = [], 0.0
    for b in range(B):
        tiles = yt[b * plan.nt: (b + 1) * plan.nt].numpy()
        a64 = ref.average_tiles(tiles, plan.ys, plan.xs, plan.Hp, plan.Wp, dtype=np.float64)
        a32 = ref.average_tiles(tiles, plan.ys, plan.xs, plan.Hp, plan.Wp)
        tol = max(tol, 4.0 * float(np.abs(a32 - a64).max()))
        want.append(a64[:, ya: ya + H, xa: xa + W])
    got = plan.blend(yt.to(gpu), B)
    assert got.shape == (B, nout, H, W) and got.dtype == torch.float32
    diff = float(np.abs(got.cpu().numpy().astype(np.float64) - np.stack(want)).max())
    print(f"blend {H} x {W}: tiles {len(plan.ys)} x {len(plan.xs)} of {plan.by} x {plan.bx}, tolerance {tol:.3e}, "
          f"largest difference {diff:.3e}")
    assert 0 < tol < 1e-5 and diff <= tol
