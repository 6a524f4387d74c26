"""Synthetic images for the 2-D dynamics tests: non-touching ellipses with known radial flows, random
flows with a float64 model of the flow following, and hand-built end points for the seeding / expansion
rules of ``reference.get_masks``.  The 2-D twin of ``cellpose3d_cases``.

Shapes are no multiple of the 16- and 32-pixel tiles of the LDS launch, ``H * W`` is no multiple of the
256- and 1,024-pixel blocks of the other launches, and no image is square.

Two kinds of flow, both pointing at the ellipse's centre ``c`` (``v = c - pixel``):

* ``capped``: ``dP = 5 * v / |v| * min(|v|, 1)``.  Near ``c`` the followed field ``dP / 5`` is ``c - q``
  at sample position ``q``, so a step lands on ``p + c - q`` and every pixel of an ellipse ends on the
  fixed point ``p* = (c + 0.5) * (L - 1) / L`` per axis.  Centres are ``c = (k + 0.5) * L / (L - 1) - 0.5``,
  so every ``p*`` is ``k + 0.5``: the truncated end point sits mid-bin, and an implementation whose
  fp32 end points differ from the oracle's by far more than rounding still bins them identically.
  :func:`oracle` checks that on the oracle's own end points (all at least 0.25 from an integer, one bin
  per ellipse) and that no ellipse's flow error is near the QC threshold, so tests may demand equality.
* ``unit``: ``dP = 5 * v / |v|``.  Points hover around the centre and the histogram spreads over a few
  bins, as with real flows; tests compare instance counts and overlap fractions.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy import ndimage

from bioengine_worker_amd.cellpose import reference as ref
from cellpose3d_cases import match_fraction  # noqa: F401  (shared with the 3-D tests)

RPAD = 20

#: name -> (shape, [(ky, kx, ry, rx), ...]): centre ``c = (k + 0.5) * L / (L - 1) - 0.5`` per axis
IMAGES = {
    # ragged 16- and 32-pixel tiles; 45 * 77 is no multiple of 256
    "a": ((45, 77), [(10, 11, 7, 8), (12, 33, 9, 6), (31, 20, 8, 9), (30, 58, 10, 12)]),
    # rim pixels travel more than 16 px: they leave the LDS window (global fallback); the large ellipse
    # covers about 39 % of the image, just under max_size_fraction
    "big": ((61, 83), [(28, 30, 24, 26), (50, 70, 7, 8)]),
    # cut by three image borders: the clamps and the padded border of the histogram.  Flow QC drops the
    # corner object (oracle flow errors 0.165, 0.75, 0.171 against the threshold 0.4); one row and one
    # column further in, at (33, 49), its error is 0.444 -- too near the threshold to demand equality
    "edge": ((37, 53), [(2, 12, 6, 6), (34, 50, 6, 7), (20, 2, 7, 5)]),
    # the smallest legal height
    "thin": ((2, 67), [(0, 20, 5, 9)]),
    # smaller than one tile
    "tiny": ((9, 13), [(4, 6, 3, 4)]),
    # two more layouts on the shape of "a" (one of them without foreground) for batches
    "a2": ((45, 77), [(8, 15, 6, 9), (26, 48, 12, 10), (35, 12, 7, 8)]),
    "empty": ((45, 77), []),
}


def centre(k, L):
    return (k + 0.5) * L / (L - 1) - 0.5


@functools.lru_cache(maxsize=None)
def image(name: str, kind: str):
    """-> dict(dP [2,H,W] f32, cellprob [H,W] f32, y [3,H,W] f32 (dY, dX, cellprob), truth [H,W] int32, n)."""
    shape, specs = IMAGES[name]
    yy, xx = np.meshgrid(*[np.arange(L, dtype=np.float64) for L in shape], indexing="ij")
    truth = np.zeros(shape, np.int32)
    dP = np.zeros((2,) + shape, np.float64)
    for i, (ky, kx, ry, rx) in enumerate(specs):
        c = [centre(k, L) for k, L in zip((ky, kx), shape)]
        inside = ((yy - c[0]) / ry) ** 2 + ((xx - c[1]) / rx) ** 2 <= 1.0
        assert not (truth[inside] > 0).any()
        truth[inside] = i + 1
        v = np.stack([c[0] - yy, c[1] - xx])
        nrm = np.sqrt((v ** 2).sum(0))
        scale = np.minimum(nrm, 1.0) if kind == "capped" else np.ones_like(nrm)
        dP[:, inside] = (5.0 * v / np.maximum(nrm, 1e-12) * scale)[:, inside]
    ncomp = ndimage.label(truth > 0, structure=np.ones((3, 3), bool))[1]
    assert ncomp == len(specs), "ellipses touch"
    cellprob = np.where(truth > 0, 5.0, -5.0).astype(np.float32)
    dP = dP.astype(np.float32)
    out = {"dP": dP, "cellprob": cellprob, "y": np.concatenate([dP, cellprob[None]]), "truth": truth, "n": len(specs),
           "shape": shape}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def end_bins(p: np.ndarray, shape, rpad: int = RPAD) -> np.ndarray:
    """Truncated end points ``p`` [2, n] -> their (y, x) bins [2, n] int64 in the image padded by ``rpad``
    (clipped to ``[0, L + rpad - 1]`` per axis), as ``reference.get_masks`` bins them."""
    pt = p.astype(np.int64) + rpad  # truncation (p >= 0)
    for a in range(2):
        pt[a] = np.clip(pt[a], 0, shape[a] + rpad - 1)
    return pt


@functools.lru_cache(maxsize=None)
def oracle(name: str, kind: str, niter: int = 200):
    """The oracle's dynamics and masks of one image, computed once: dict(p, inds, bins, raw (labels of
    get_masks), err (flow error per raw label), masks (compute_masks))."""
    v = image(name, kind)
    p, inds = ref.follow_flows(v["dP"], v["cellprob"], 0.0, niter)
    bins = end_bins(p, v["shape"])
    raw = ref.get_masks(p, inds, v["shape"])
    err = ref.flow_errors(raw, v["dP"]) if raw.max() > 0 else np.zeros(0)
    if kind == "capped" and v["n"]:
        frac = p - np.floor(p)
        assert frac.min() >= 0.25 and frac.max() <= 0.75, (name, float(frac.min()), float(frac.max()))
        lab = v["truth"][inds]
        for i in range(1, v["n"] + 1):
            assert len(np.unique(bins[:, lab == i], axis=1).T) == 1, (name, i)
        # flow QC keeps err <= 0.4: no object may sit where rounding could decide it
        assert not ((err >= 0.3) & (err <= 0.5)).any(), (name, err.tolist())
    masks = ref.compute_masks(v["dP"], v["cellprob"], niter=niter)
    for a in (p, bins, raw, err, masks):
        a.setflags(write=False)
    return {"p": p, "inds": inds, "bins": bins, "raw": raw, "err": err, "masks": masks}


def hist_pos(bins: np.ndarray, inds, shape):
    """End-point bins [2, n] of the pixels ``inds`` -> (hist [H+40, W+40] int32, pos [H, W] int32: padded
    linear bin per pixel, -1 elsewhere) -- what the dynamics kernel hands to the seeding."""
    hs = tuple(L + 2 * RPAD for L in shape)
    hist = np.zeros(hs, np.int32)
    np.add.at(hist, (bins[0], bins[1]), 1)
    pos = np.full(shape, -1, np.int32)
    pos[inds] = (bins[0] * hs[1] + bins[1]).astype(np.int32)
    return hist, pos


# ------------------------------------------------------------------ float64 model of the flow following


def follow_model(dP: np.ndarray, cellprob: np.ndarray, thr: float = 0.0, niter: int = 200):
    """Plain float64 flow following (no ``grid_sample``) -> ``(p [2, n] final positions, pre [2, n] the
    last step's positions before the clamp, inds)``.  The followed field is the kernel's
    ``float32(dP) * float32(0.2)`` (the oracle divides by 5 in double, up to 1 ulp away) on
    ``cellprob > thr`` and zero elsewhere and outside the image; everything after that is float64."""
    fg = cellprob > thr
    H, W = cellprob.shape
    f = np.where(fg, np.asarray(dP, np.float32) * np.float32(0.2), np.float32(0)).astype(np.float64)
    f = np.pad(f, ((0, 0), (1, 2), (1, 2)))  # zeros outside: pixel (y, x) is f[:, y + 1, x + 1]
    inds = np.nonzero(fg)
    p = np.stack(inds).astype(np.float64)
    pre = p.copy()
    top = np.array([H - 1.0, W - 1.0])[:, None]
    for _ in range(niter):
        sy, sx = p[0] * H / (H - 1) - 0.5, p[1] * W / (W - 1) - 0.5
        y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
        wy, wx = sy - y0, sx - x0
        y0, x0 = np.clip(y0, -1, H) + 1, np.clip(x0, -1, W) + 1  # a sample beyond the pad ring reads zeros too
        d = (f[:, y0, x0] * ((1 - wy) * (1 - wx)) + f[:, y0, x0 + 1] * ((1 - wy) * wx)
             + f[:, y0 + 1, x0] * (wy * (1 - wx)) + f[:, y0 + 1, x0 + 1] * (wy * wx))
        pre = p + d
        p = np.clip(pre, 0.0, top)
    return p, pre, inds


def near_bin_edge(pre: np.ndarray, shape, eps: float) -> np.ndarray:
    """[n] bool: pre-clamp end points within ``eps`` of an integer in ``[1, L - 1]`` on either axis, where
    fp32 rounding may decide the bin.  A coordinate clamped to 0 is always safe, one clamped to ``L - 1``
    when it overshot by more than ``eps``."""
    out = np.zeros(pre.shape[1], bool)
    for a, L in enumerate(shape):
        r = np.round(pre[a])
        out |= (np.abs(pre[a] - r) < eps) & (r >= 1) & (r <= L - 1)
    return out


@functools.lru_cache(maxsize=None)
def random_flows(shape, B: int = 3, seed: int = 0):
    """-> y [B, 3, H, W] f32: uniform(-5, 5) flows, 80 % random foreground (cellprob +-1)."""
    rng = np.random.default_rng(seed + 1000 * shape[0] + shape[1])
    y = rng.uniform(-5, 5, (B, 3) + tuple(shape)).astype(np.float32)
    y[:, 2] = np.where(rng.random((B,) + tuple(shape)) < 0.8, 1.0, -1.0)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def random_model(shape, niter: int, eps: float = 1e-3, B: int = 3, seed: int = 0):
    """The float64 model on :func:`random_flows` -> (pos [B, H, W] int32 (-1 on background), excluded
    [B, H, W] bool, fg [B, H, W] bool).  Without a step every pixel bins itself: nothing is excluded."""
    y = random_flows(shape, B, seed)
    pos = np.full((B,) + tuple(shape), -1, np.int32)
    excl = np.zeros((B,) + tuple(shape), bool)
    for b in range(B):
        p, pre, inds = follow_model(y[b, :2], y[b, 2], 0.0, niter)
        pos[b] = hist_pos(end_bins(p, shape), inds, shape)[1]
        if niter > 0:
            excl[b][inds] = near_bin_edge(pre, shape, eps)
    return pos, excl, y[:, 2] > 0


# ------------------------------------------------------------------ hand-built end points (get_masks rules)
#
# A case is (shape, (p, inds)): ``count`` pixels of the image are given one end point.  Pixels are handed
# out in raster order.


def _points(shape, groups):
    """groups: [(bin (y, x), count)] -> (p [2, n] float32 mid-bin end points, inds)."""
    n = sum(c for _, c in groups)
    assert n <= int(np.prod(shape))
    inds = np.unravel_index(np.arange(n), shape)
    p = np.concatenate([np.repeat(np.asarray(b, np.float32)[:, None] + 0.5, c, axis=1) for b, c in groups], axis=1)
    return p.astype(np.float32), inds


SHAPE = (13, 29)


def rule_count_10_vs_11():
    # a bin of 10 end points is no seed, one of 11 is; they are 14 bins apart (no interaction)
    return SHAPE, _points(SHAPE, [((6, 5), 10), ((6, 19), 11)])


def rule_support_2_vs_3():
    # around a seed of 12: a neighbour with 2 points is outside the support, one with 3 inside
    return SHAPE, _points(SHAPE, [((6, 10), 12), ((6, 9), 2), ((6, 11), 3)])


def rule_equal_maxima():
    # two bins of 12 inside one 5x5 neighbourhood, joined by support: both are seeds, their windows
    # overlap, and the later one in raster order (x = 12) owns the overlap -- the earlier seed's own
    # bin included.  The earlier one keeps only what the later cannot reach in five steps (x = 5, 6).
    g = [((5, 10), 12), ((5, 11), 4), ((6, 12), 12)] + [((5, x), 3) for x in range(5, 10)]
    return SHAPE, _points(SHAPE, g)


def rule_unequal_overlap():
    # seeds of 20 (x = 8, earlier in raster order) and 12 (x = 12) joined by a support bridge: the
    # larger count is expanded last and wins the bridge and both seed bins; the smaller keeps the end
    # of its own chain (x = 14 .. 17), which the larger cannot reach
    g = [((6, 8), 20)] + [((6, x), 3) for x in (9, 10, 11)] + [((6, 12), 12)] + [((6, x), 3) for x in range(13, 18)]
    return SHAPE, _points(SHAPE, g)


def rule_non_maximum():
    # a bin of 12 beside one of 20: above the count threshold but no 5x5 maximum, so no seed of its own.
    # The chain of support is labelled as far as the seed of 20 reaches (x = 13) and no further; were
    # the 12 a seed too, it would keep x = 14
    return SHAPE, _points(SHAPE, [((6, 8), 20), ((6, 9), 12)] + [((6, x), 3) for x in range(10, 16)])


def rule_gap():
    # support at distance 2 from the seed with an empty bin between: dilation must not cross
    return SHAPE, _points(SHAPE, [((6, 10), 12), ((6, 12), 5), ((6, 13), 5)])


def rule_diagonal():
    # support touching the seed only through a corner (8-connected), then carrying on: crossed
    return SHAPE, _points(SHAPE, [((6, 10), 12), ((7, 11), 5), ((8, 12), 5), ((8, 13), 4)])


def rule_far_reach():
    # a chain of support 7 bins long: five dilations reach 5 bins from the seed and no further
    return SHAPE, _points(SHAPE, [((6, 5), 12)] + [((6, 5 + d), 3) for d in range(1, 8)])


def rule_oversize():
    # one object of 60 % of the pixels (dropped at max_size_fraction 0.4) beside a small one (kept)
    shape = (7, 9)
    return shape, _points(shape, [((3, 2), 38), ((3, 7), 12)])


RULES = {f.__name__[5:]: f for f in (rule_count_10_vs_11, rule_support_2_vs_3, rule_equal_maxima, rule_unequal_overlap,
                                     rule_non_maximum, rule_gap, rule_diagonal, rule_oversize, rule_far_reach)}


def lattice(n: int = 15, pitch: int = 5, count: int = 11):
    """``n`` x ``n`` bins of ``count`` end points on a lattice of ``pitch`` bins: every bin is a seed of its
    own (more seeds than one workgroup of four expands), equal counts so the raster tie-break orders them."""
    side = pitch * n
    shape = (side + 2, side + 3)  # (77, 78): not square, no multiple of 4
    assert count * n ** 2 <= int(np.prod(shape))
    g = [((2 + pitch * i, 1 + pitch * j), count) for i in range(n) for j in range(n)]
    return shape, _points(shape, g)


# ------------------------------------------------------------------ tiles


def average_tiles_direct(y: np.ndarray, ys, xs, Ly: int, Lx: int) -> np.ndarray:
    """The tapered blend written out per pixel in float64: ``sum_t m[Y - ys_t, X - xs_t] * y_t / sum_t m``
    over the tiles that cover ``(Y, X)``, ``m = taper_mask(by, bx)``."""
    nt, nout, by, bx = y.shape
    m = ref.taper_mask(by, bx).astype(np.float64)
    starts = [(a, b) for a in ys for b in xs]
    out = np.zeros((nout, Ly, Lx))
    for Y in range(Ly):
        for X in range(Lx):
            num, den = np.zeros(nout), 0.0
            for t, (a, b) in enumerate(starts):
                if 0 <= Y - a < by and 0 <= X - b < bx:
                    num += m[Y - a, X - b] * y[t, :, Y - a, X - b].astype(np.float64)
                    den += m[Y - a, X - b]
            out[:, Y, X] = num / den
    return out
