"""Synthetic volumes for the do_3D tests: non-touching ellipsoids with known radial flows, and hand-built
end points for the seeding / expansion rules of ``reference.get_masks3d``.

Volumes are non-cubic and no side is a multiple of 4, so axis mix-ups and ragged tails show.

Two kinds of flow, both pointing at the ellipsoid's centre ``c`` (``v = c - voxel``):

* ``capped``: ``dP = 5 * v / |v| * min(|v|, 1)``.  Near ``c`` the followed field ``dP / 5`` is ``c - q``
  at sample position ``q``, so a step lands on ``p + c - q`` and every voxel of an ellipsoid ends on
  the fixed point ``p* = (c + 0.5) * (L - 1) / L`` per axis.  Centres are chosen so that every ``p*``
  is ``k + 0.5``: the truncated end point then sits mid-bin, and an implementation whose fp32 end
  points differ from the oracle's by far more than rounding still bins them identically.  The
  generator checks that on the oracle's own end points (all at least 0.25 from an integer, one bin
  per ellipsoid), so tests may demand exact equality.
* ``unit``: ``dP = 5 * v / |v|``.  Points hover around the centre and the histogram spreads over a
  few bins, as with real flows; tests compare instance counts and overlap fractions.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy import ndimage

from bioengine_worker_amd.cellpose import reference as ref

RPAD = 20

#: name -> (shape, [(kz, ky, kx, rz, ry, rx), ...]): centre ``c = (k + 0.5) * L / (L - 1) - 0.5`` per axis
VOLUMES = {
    "a": ((24, 40, 56), [(11, 10, 10, 6, 6, 7), (12, 10, 28, 5, 6, 7), (11, 10, 45, 7, 6, 8), (12, 29, 18, 8, 6, 5),
                         (11, 29, 38, 6, 6, 8)]),
    "b": ((19, 33, 45), [(9, 10, 11, 5, 6, 7), (9, 22, 22, 6, 6, 5), (9, 11, 33, 7, 5, 8)]),
    "c": ((21, 37, 53), [(10, 10, 10, 6, 6, 6), (10, 26, 12, 7, 6, 8), (10, 11, 30, 5, 6, 7), (10, 25, 42, 8, 7, 7)]),
    # clamping and the padded border: one ellipsoid against the z = 0 face, one in the far corner
    "edge": ((19, 33, 45), [(2, 16, 12, 5, 6, 6), (16, 30, 42, 6, 6, 6)]),
    # one plane: the z axis has length 1 (sampled with weight 1, position fixed at 0)
    "flat": ((1, 5, 7), [(0, 2, 3, 10, 10, 10)]),
}


def centre(k, L):
    return (k + 0.5) * L / (L - 1) - 0.5 if L > 1 else 0.0


@functools.lru_cache(maxsize=None)
def volume(name: str, kind: str):
    """-> dict(dP [3,Z,H,W] f32, cellprob [Z,H,W] f32, truth [Z,H,W] int32, n)."""
    shape, specs = VOLUMES[name]
    zz, yy, xx = np.meshgrid(*[np.arange(L, dtype=np.float64) for L in shape], indexing="ij")
    truth = np.zeros(shape, np.int32)
    dP = np.zeros((3,) + shape, np.float64)
    for i, (kz, ky, kx, rz, ry, rx) in enumerate(specs):
        c = [centre(k, L) for k, L in zip((kz, ky, kx), shape)]
        inside = ((zz - c[0]) / rz) ** 2 + ((yy - c[1]) / ry) ** 2 + ((xx - c[2]) / rx) ** 2 <= 1.0
        assert not (truth[inside] > 0).any()
        truth[inside] = i + 1
        v = np.stack([c[0] - zz, c[1] - yy, c[2] - xx])
        nrm = np.sqrt((v ** 2).sum(0))
        scale = np.minimum(nrm, 1.0) if kind == "capped" else np.ones_like(nrm)
        dP[:, inside] = (5.0 * v / np.maximum(nrm, 1e-12) * scale)[:, inside]
    ncomp = ndimage.label(truth > 0, structure=np.ones((3, 3, 3), bool))[1]
    assert ncomp == len(specs), "ellipsoids touch"
    cellprob = np.where(truth > 0, 5.0, -5.0).astype(np.float32)
    out = {"dP": dP.astype(np.float32), "cellprob": cellprob, "truth": truth, "n": len(specs), "shape": shape}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name: str, kind: str, niter: int = 200):
    """The oracle's dynamics and masks of one volume, computed once: dict(p, inds, bins, masks)."""
    v = volume(name, kind)
    p, inds = ref.follow_flows3d(v["dP"], v["cellprob"], 0.0, niter)
    bins = ref.end_bins3d(p, v["shape"], RPAD)
    if kind == "capped":
        frac = p - np.floor(p)
        frac = frac[[L > 1 for L in v["shape"]]]  # an axis of length 1 stays at 0
        assert frac.min() >= 0.25 and frac.max() <= 0.75, (name, float(frac.min()), float(frac.max()))
        lab = v["truth"][inds]
        for i in range(1, v["n"] + 1):
            assert len(np.unique(bins[:, lab == i], axis=1).T) == 1, (name, i)
    # "flat" is one object filling its volume: keep it (max_size_fraction 1) so there is a mask to compare
    frac = 1.0 if name == "flat" else 0.4
    masks = ref.fill_holes_and_remove_small_masks3d(ref.get_masks3d(p, inds, v["shape"], max_size_fraction=frac), 15)
    for a in (p, bins, masks):
        a.setflags(write=False)
    return {"p": p, "inds": inds, "bins": bins, "masks": masks}


def hist_pos(bins: np.ndarray, inds, shape):
    """End-point bins [3, n] of the voxels ``inds`` -> (hist [Z+40, H+40, W+40] int32, pos [Z, H, W]
    int32: padded linear bin per voxel, -1 elsewhere) -- what the dynamics kernel hands to the seeding."""
    hs = tuple(L + 2 * RPAD for L in shape)
    hist = np.zeros(hs, np.int32)
    np.add.at(hist, (bins[0], bins[1], bins[2]), 1)
    pos = np.full(shape, -1, np.int32)
    pos[inds] = ((bins[0] * hs[1] + bins[1]) * hs[2] + bins[2]).astype(np.int32)
    return hist, pos


def match(masks: np.ndarray, truth: np.ndarray):
    """(instances found, smallest fraction of a true instance covered by its best label)."""
    worst = 1.0
    for i in range(1, int(truth.max()) + 1):
        sel = masks[truth == i]
        labs, cnt = np.unique(sel[sel > 0], return_counts=True)
        worst = min(worst, (cnt.max() / sel.size) if len(cnt) else 0.0)
    return int(masks.max()), worst


def match_fraction(a: np.ndarray, b: np.ndarray) -> float:
    """Fraction of the voxels on which two label volumes agree up to a renaming of the labels: every
    label of ``a`` is mapped to the label of ``b`` it overlaps most."""
    a, b = a.ravel(), b.ravel()
    pairs, cnt = np.unique(np.stack([a, b], 1), axis=0, return_counts=True)
    best: dict = {}
    for (la, lb), c in zip(pairs.tolist(), cnt.tolist()):
        if c > best.get(la, (0, None))[0]:
            best[la] = (c, lb)
    lut = np.zeros(int(a.max()) + 1, np.int64)
    for la, (_, lb) in best.items():
        lut[la] = lb
    return float((lut[a] == b).mean())


# ------------------------------------------------------------------ hand-built end points (get_masks3d rules)
#
# A case is (shape, [(voxels (z, y, x), bin (z, y, x) in unpadded coordinates), ...]): ``count`` voxels
# of the volume are given one end point.  Voxels are handed out in raster order.


def _points(shape, groups):
    """groups: [(bin (z, y, x), count)] -> (p [3, n] float32 mid-bin end points, inds)."""
    n = sum(c for _, c in groups)
    assert n <= int(np.prod(shape))
    inds = np.unravel_index(np.arange(n), shape)
    p = np.concatenate([np.repeat(np.asarray(b, np.float32)[:, None] + 0.5, c, axis=1) for b, c in groups], axis=1)
    return p.astype(np.float32), inds


def rule_count_10_vs_11():
    # a bin of 10 end points is no seed, one of 11 is; they are 12 bins apart (no interaction)
    return (9, 13, 29), _points((9, 13, 29), [((4, 6, 5), 10), ((4, 6, 19), 11)])


def rule_support_2_vs_3():
    # around a seed of 12: a neighbour with 2 points is outside the support, one with 3 inside
    return (9, 13, 29), _points((9, 13, 29), [((4, 6, 10), 12), ((4, 6, 9), 2), ((4, 6, 11), 3)])


def rule_equal_maxima():
    # two bins of 12 inside one 5^3 neighbourhood, joined by support: both are seeds, their windows
    # overlap, and the later one in raster order (x = 12) owns the overlap -- the earlier seed's own
    # bin included.  The earlier one keeps only what the later cannot reach in five steps (x = 5, 6).
    g = [((4, 5, 10), 12), ((4, 5, 11), 4), ((4, 6, 12), 12)] + [((4, 5, x), 3) for x in range(5, 10)]
    return (9, 13, 29), _points((9, 13, 29), g)


def rule_unequal_overlap():
    # seeds of 20 (x = 8, earlier in raster order) and 12 (x = 12) joined by a support bridge: the
    # larger count is expanded last and wins the bridge and both seed bins; the smaller keeps the end
    # of its own chain (x = 14 .. 17), which the larger cannot reach
    g = [((4, 6, 8), 20)] + [((4, 6, x), 3) for x in (9, 10, 11)] + [((4, 6, 12), 12)] + [((4, 6, x), 3) for x in range(13, 18)]
    return (9, 13, 29), _points((9, 13, 29), g)


def rule_gap():
    # support at distance 2 from the seed with an empty bin between: dilation must not cross
    return (9, 13, 29), _points((9, 13, 29), [((4, 6, 10), 12), ((4, 6, 12), 5), ((4, 6, 13), 5)])


def rule_diagonal():
    # support touching the seed only through a corner (26-connected), then carrying on: crossed
    g = [((4, 6, 10), 12), ((5, 7, 11), 5), ((6, 8, 12), 5), ((6, 8, 13), 4)]
    return (9, 13, 29), _points((9, 13, 29), g)


def rule_oversize():
    # one object of 60 % of the voxels (dropped at max_size_fraction 0.4) beside a small one (kept)
    shape = (5, 7, 9)
    return shape, _points(shape, [((2, 3, 2), 189), ((2, 3, 7), 30)])


def rule_far_reach():
    # a chain of support 7 bins long: five dilations reach 5 bins from the seed and no further
    g = [((4, 6, 5), 12)] + [((4, 6, 5 + d), 3) for d in range(1, 8)]
    return (9, 13, 29), _points((9, 13, 29), g)


RULES = {f.__name__[5:]: f for f in (rule_count_10_vs_11, rule_support_2_vs_3, rule_equal_maxima, rule_unequal_overlap,
                                     rule_gap, rule_diagonal, rule_oversize, rule_far_reach)}


def lattice(n: int = 9, pitch: int = 5, count: int = 11):
    """``n``^3 bins of ``count`` end points on a lattice of ``pitch`` bins: every bin is a seed of its
    own (more seeds than one workgroup expands), equal counts so the raster tie-break orders them."""
    side = pitch * n
    shape = (side, side + 1, side + 2)
    assert count * n ** 3 <= int(np.prod(shape))
    g = [((2 + pitch * i, 3 + pitch * j, 1 + pitch * k), count) for i in range(n) for j in range(n) for k in range(n)]
    return shape, _points(shape, g)
