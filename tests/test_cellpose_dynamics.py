"""Cellpose 2-D dynamics, CPU: the oracle's side of every case in ``cellpose2d_cases`` -- the conditions
the exact GPU comparisons of ``test_cellpose_dynamics_gpu.py`` rest on -- and the tile oracles
(``make_tiles``, ``average_tiles``, the separable taper of ``TilePlan``) against formulas written out."""
import numpy as np
import pytest

import cellpose2d_cases as cc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.unit

CAPPED = ["a", "big", "edge", "thin", "tiny", "a2"]


# ------------------------------------------------------------------ capped / unit images


@pytest.mark.parametrize("name", CAPPED)
def test_capped_end_points_sit_mid_bin(name):
    """What :func:`cellpose2d_cases.oracle` asserts, spelled out: fixed points ``k + 0.5``, every
    fractional part in [0.25, 0.75], one bin per object, no flow error near the QC threshold."""
    v, o = cc.image(name, "capped"), cc.oracle(name, "capped")
    shape, specs = cc.IMAGES[name]
    frac = o["p"] - np.floor(o["p"])
    assert frac.min() >= 0.25 and frac.max() <= 0.75
    lab = v["truth"][o["inds"]]
    for i, s in enumerate(specs):
        want = np.array(s[:2], np.float32) + 0.5
        assert np.abs(o["p"][:, lab == i + 1] - want[:, None]).max() <= 0.25
        assert (o["bins"][:, lab == i + 1] == np.array(s[:2])[:, None] + cc.RPAD).all()
    assert len(o["err"]) == len(specs) and not ((o["err"] >= 0.3) & (o["err"] <= 0.5)).any()
    hist, pos = cc.hist_pos(o["bins"], o["inds"], shape)
    assert hist.sum() == (v["truth"] > 0).sum() and ((pos >= 0) == (v["truth"] > 0)).all()
    assert sorted(hist[hist > 0].tolist()) == sorted(np.bincount(v["truth"].ravel())[1:].tolist())


@pytest.mark.parametrize("name", ["a", "big", "thin", "tiny", "a2"])
def test_oracle_recovers_capped_objects_exactly(name):
    v, o = cc.image(name, "capped"), cc.oracle(name, "capped")
    m = o["masks"]
    assert m.dtype == np.int32 and int(m.max()) == v["n"]
    assert np.array_equal(m > 0, v["truth"] > 0) and cc.match_fraction(m, v["truth"]) == 1.0


def test_edge_outcome_is_pinned():
    """Three objects cut by the image borders: flow QC keeps the ones cut by one border (errors 0.165,
    0.171) and drops the corner one (0.75)."""
    v, o = cc.image("edge", "capped"), cc.oracle("edge", "capped")
    assert int(o["raw"].max()) == 3 and np.array_equal(o["raw"] > 0, v["truth"] > 0)
    err = {int(v["truth"][o["raw"] == l][0]): float(o["err"][l - 1]) for l in (1, 2, 3)}  # by object
    assert err[1] < 0.2 and err[3] < 0.2 and err[2] > 0.7
    m = o["masks"]
    assert int(m.max()) == 2 and np.array_equal(m > 0, (v["truth"] == 1) | (v["truth"] == 3))
    assert cc.match_fraction(m, np.where(v["truth"] == 2, 0, v["truth"])) == 1.0


def test_big_ellipse_sits_just_under_max_size_fraction():
    v = cc.image("big", "capped")
    n, total = int((v["truth"] == 1).sum()), v["truth"].size
    assert 0.38 * total < n <= 0.4 * total  # kept by an exact integer comparison ...
    m = ref.compute_masks(v["dP"], v["cellprob"], max_size_fraction=(n - 1) / total)  # ... and dropped one pixel lower
    assert int(m.max()) == 1 and np.array_equal(m > 0, v["truth"] == 2)


@pytest.mark.parametrize("name", ["a", "big"])
def test_oracle_finds_unit_flow_objects(name):
    v, o = cc.image(name, "unit"), cc.oracle(name, "unit")
    assert int(o["masks"].max()) == v["n"] and cc.match_fraction(o["masks"], v["truth"]) > 0.99


def test_empty_image_and_misfit_shapes():
    v, o = cc.image("empty", "capped"), cc.oracle("empty", "capped")
    assert o["p"].shape == (2, 0) and not o["masks"].any() and o["masks"].shape == v["shape"]
    for shape in ((1, 9), (9, 1), (1, 1), (0, 5)):
        with pytest.raises(ValueError, match="two rows and two columns"):
            ref.follow_flows(np.zeros((2,) + shape, np.float32), np.ones(shape, np.float32))
        with pytest.raises(ValueError, match="two rows and two columns"):  # also without any foreground
            ref.compute_masks(np.zeros((2,) + shape, np.float32), -np.ones(shape, np.float32))


# ------------------------------------------------------------------ float64 model


def test_model_single_steps_by_hand():
    """One step of a constant field: the interior moves by dP / 5, the border rows sample half a pixel
    outside (zeros there) and move less; positions are clamped to the image."""
    H, W = 5, 7
    dP = np.zeros((2, H, W), np.float32)
    dP[1] = 5.0  # one pixel per step along +x
    p, pre, inds = cc.follow_model(dP, np.ones((H, W), np.float32), 0.0, 1)
    k = int(np.nonzero((inds[0] == 2) & (inds[1] == 3))[0][0])  # samples y = 2 * 5 / 4 - 0.5 = 2, x = 3 exactly
    assert abs(p[0, k] - 2.0) < 1e-12 and abs(p[1, k] - (3.0 + float(np.float32(5.0) * np.float32(0.2)))) < 1e-12
    k = int(np.nonzero((inds[0] == 0) & (inds[1] == 3))[0][0])  # samples y = -0.5: half of the step
    assert abs(p[1, k] - 3.5) < 1e-6
    k = int(np.nonzero((inds[0] == 2) & (inds[1] == 6))[0][0])  # x = 6 samples 6.5: half a step, then the clamp
    assert abs(pre[1, k] - 6.5) < 1e-6 and p[1, k] == 6.0
    p, pre, inds = cc.follow_model(dP, np.ones((H, W), np.float32), 0.0, 0)
    assert np.array_equal(p, np.stack(inds).astype(np.float64))
    assert cc.follow_model(dP, np.ones((H, W), np.float32), 1.0, 3)[0].shape == (2, 0)  # strict threshold


def test_near_bin_edge_rule():
    pre = np.array([[0.0004, -3.0, 4.0005, 4.002, 3.9995, 2.5, 1.0002], [2.5] * 7])
    #                 at 0: safe; clamped to 0: safe; at L-1 = 4: in doubt; overshoot > eps: safe; below 4; mid-bin; at 1
    assert cc.near_bin_edge(pre, (5, 7), 1e-3).tolist() == [False, False, True, False, True, False, True]


@pytest.mark.parametrize("shape", [(37, 53), (45, 77)])
@pytest.mark.parametrize("niter", [0, 1, 3])
def test_model_agrees_with_oracle_outside_the_excluded_set(shape, niter):
    """The fp32 oracle and the float64 model bin every foreground pixel alike unless its pre-clamp end
    point is within 1e-3 of a bin edge; at most 2 % of the foreground may be excluded (measured:
    0.23 % / 0.30 % at 37 x 53 and 0.45 % / 0.42 % at 45 x 77 for 1 / 3 steps, none at 0)."""
    pos, excl, fg = cc.random_model(shape, niter)
    y = cc.random_flows(shape)
    assert 0.75 < fg.mean() < 0.85 and excl.sum() <= 0.02 * fg.sum() and not excl[~fg].any()
    assert (niter == 0) == (not excl.any())
    for b in range(y.shape[0]):
        p, inds = ref.follow_flows(y[b, :2], y[b, 2], 0.0, niter)
        want = cc.hist_pos(cc.end_bins(p, shape), inds, shape)[1]
        assert np.array_equal(want < 0, ~fg[b]) and np.array_equal(pos[b] < 0, ~fg[b])
        assert not ((want != pos[b]) & ~excl[b]).any()


# ------------------------------------------------------------------ get_masks rules


def _labels_at(shape, p, inds, bins, **kw):
    """Label of the pixels whose end point is in ``bins`` [(y, x), ...] (-1: several labels)."""
    m = ref.get_masks(p, inds, shape, **kw)
    pt = p.astype(np.int64)
    out = []
    for b in bins:
        labs = np.unique(m[inds][(pt[0] == b[0]) & (pt[1] == b[1])])
        out.append(int(labs[0]) if len(labs) == 1 else -1)
    return m, out


def test_rule_count_and_support_thresholds():
    shape, (p, inds) = cc.rule_count_10_vs_11()
    m, labs = _labels_at(shape, p, inds, [(6, 5), (6, 19)])
    assert labs == [0, 1] and int(m.max()) == 1  # 10 points: no seed; 11: a seed
    shape, (p, inds) = cc.rule_support_2_vs_3()
    m, labs = _labels_at(shape, p, inds, [(6, 10), (6, 9), (6, 11)])
    assert labs == [1, 0, 1]  # 2 points: outside the support; 3: inside


def test_rule_ties_and_overlaps():
    shape, (p, inds) = cc.rule_equal_maxima()
    m, labs = _labels_at(shape, p, inds, [(5, 10), (5, 11), (6, 12), (5, 9), (5, 8), (5, 7), (5, 6), (5, 5)])
    # both seed; the raster-later one (expanded last) owns everything it reaches, the other seed's bin included
    assert int(m.max()) == 2 and labs == [2, 2, 2, 2, 2, 2, 1, 1]
    shape, (p, inds) = cc.rule_unequal_overlap()
    m, labs = _labels_at(shape, p, inds, [(6, x) for x in range(8, 18)])
    # the seed of 20 is raster-earlier but larger: expanded last, it wins the bridge and both seed bins
    assert int(m.max()) == 2 and labs == [2, 2, 2, 2, 2, 2, 1, 1, 1, 1]
    shape, (p, inds) = cc.rule_non_maximum()
    m, labs = _labels_at(shape, p, inds, [(6, x) for x in range(8, 16)])
    # 12 points beside 20: no seed of its own, so nothing is labelled past the reach of the seed of 20
    assert int(m.max()) == 1 and labs == [1, 1, 1, 1, 1, 1, 0, 0]


def test_rule_dilation_connectivity_and_reach():
    shape, (p, inds) = cc.rule_gap()
    _, labs = _labels_at(shape, p, inds, [(6, 10), (6, 12), (6, 13)])
    assert labs == [1, 0, 0]  # a one-bin gap is not crossed
    shape, (p, inds) = cc.rule_diagonal()
    _, labs = _labels_at(shape, p, inds, [(6, 10), (7, 11), (8, 12), (8, 13)])
    assert labs == [1, 1, 1, 1]  # a corner contact (8-connectivity) is crossed
    shape, (p, inds) = cc.rule_far_reach()
    _, labs = _labels_at(shape, p, inds, [(6, 5 + d) for d in range(8)])
    assert labs == [1, 1, 1, 1, 1, 1, 0, 0]  # five dilations: five bins from the seed


def test_rule_oversize_and_empty():
    shape, (p, inds) = cc.rule_oversize()
    m = ref.get_masks(p, inds, shape)
    assert int(m.max()) == 1 and (m > 0).sum() == 12  # the 38-pixel object (60 % of 63) is dropped
    m = ref.get_masks(p, inds, shape, max_size_fraction=0.7)
    assert int(m.max()) == 2 and (m > 0).sum() == 50
    empty = ref.get_masks(np.zeros((2, 0), np.float32), (np.zeros(0, np.int64), np.zeros(0, np.int64)), (7, 9))
    assert empty.shape == (7, 9) and empty.dtype == np.int32 and not empty.any()


def test_lattice_every_bin_is_a_seed():
    shape, (p, inds) = cc.lattice()
    assert shape == (77, 78)
    m = ref.get_masks(p, inds, shape)
    assert int(m.max()) == 225
    # equal counts: numbered in raster order of the bins; every pixel carries its own bin's label
    pt = p.astype(np.int64)
    want = ((pt[0] - 2) // 5) * 15 + (pt[1] - 1) // 5 + 1
    assert np.array_equal(m[inds], want)


def test_hist_pos_layout():
    shape, (p, inds) = cc.rule_support_2_vs_3()
    hist, pos = cc.hist_pos(cc.end_bins(p, shape), inds, shape)
    assert hist.shape == (53, 69) and hist.dtype == pos.dtype == np.int32
    assert (hist[26, 30], hist[26, 29], hist[26, 31], int(hist.sum())) == (12, 2, 3, 17)
    assert pos.ravel()[:17].tolist() == [26 * 69 + 30] * 12 + [26 * 69 + 29] * 2 + [26 * 69 + 31] * 3
    assert (pos.ravel()[17:] == -1).all()


# ------------------------------------------------------------------ tiles


def test_make_and_average_tiles_against_direct_formulas():
    """One small plan (32-pixel tiles, 2 x 3 of them): ``make_tiles`` element by element, ``average_tiles``
    of independent random tiles against the per-pixel float64 formula."""
    rng = np.random.default_rng(5)
    C, Ly, Lx = 2, 40, 72
    img = rng.standard_normal((C, Ly, Lx)).astype(np.float32)
    tiles, ys, xs = ref.make_tiles(img, bsize=32)
    assert (ys, xs) == ([0, 8], [0, 20, 40]) and tiles.shape == (6, C, 32, 32)
    for t in range(6):
        for i in (0, 13, 31):
            for j in (0, 7, 31):
                assert (tiles[t, :, i, j] == img[:, ys[t // 3] + i, xs[t % 3] + j]).all()
    y = rng.standard_normal((6, 3, 32, 32)).astype(np.float32)  # a different value in every tile
    want = cc.average_tiles_direct(y, ys, xs, Ly, Lx)
    got64 = ref.average_tiles(y, ys, xs, Ly, Lx, dtype=np.float64)
    assert got64.dtype == np.float64 and np.abs(got64 - want).max() < 1e-12
    got32 = ref.average_tiles(y, ys, xs, Ly, Lx)
    # float32 sums of at most n = 4 weighted tiles, numerator and denominator: (2 n + 3) roundings of 2^-24
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 11 * 2.0 ** -24 * np.abs(y).max()
    # the centre crop of the taper is nearly flat at 32 pixels; a strip of full-width tiles (16 x 224, two
    # of them 36 columns apart) has the whole roll-off: there the blend is far from the plain mean
    y = rng.standard_normal((2, 1, 16, 224)).astype(np.float32)
    want = cc.average_tiles_direct(y, [0], [0, 36], 16, 260)
    assert np.abs(ref.average_tiles(y, [0], [0, 36], 16, 260, dtype=np.float64) - want).max() < 1e-12
    assert np.abs(ref.average_tiles(y, [0], [0, 36], 16, 260) - want).max() <= 7 * 2.0 ** -24 * np.abs(y).max()
    both = slice(36, 224)
    assert np.abs(0.5 * (y[0, :, :, both] + y[1, :, :, :188]) - want[:, :, both]).max() > 0.5
    m = ref.taper_mask(16, 224).astype(np.float64)
    assert m[8, 0] < 0.1 and m[8, 112] > 0.99  # 1 / (1 + exp((112 - 0.5 - 92) / 7.5)) = 0.069 at the rim


@pytest.mark.parametrize("H,W", [(300, 260), (100, 500)])
def test_tile_plan_taper_factors_rebuild_the_mask(H, W):
    from bioengine_worker_amd.cellpose.gpu import TilePlan

    plan = TilePlan(H, W)
    if (H, W) == (100, 500):
        assert (plan.by, plan.bx, len(plan.ys)) == (128, 224, 1) and len(plan.xs) > 1
    else:
        assert plan.by == plan.bx == 224 and len(plan.ys) > 1 and len(plan.xs) > 1
    m = ref.taper_mask(plan.by, plan.bx).astype(np.float64)
    got = np.outer(plan.wy.numpy().astype(np.float64), plan.wx.numpy().astype(np.float64))
    assert got.shape == m.shape and (np.abs(got - m) <= 1e-6 * m).all()
