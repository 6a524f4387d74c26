"""Label images for the per-cell measurement tests (``reference.measure_masks`` and its HIP kernel).

Every builder is cached and every oracle result is computed once and shared; tests must not write
into what they get.

* ``hand``    7 x 9, built by hand, expected raw values written out as literals (``HAND_RAW``).
* ``ragged``  B = 3 batch of 45 x 67 Voronoi labels with a zero background band; the width is no
              multiple of 64; K is 5, 40 and 0 (an all-zero image).
* ``big``     B = 2, 300 x 300: label 1 covers everything (``sum_yy`` is about 2.7e9 > 2^31); a
              one-pixel-wide spiral whose box is the whole image.  Both boxes are split into bands.
* ``many``    64 x 64 with one label per 2 x 2 block: 1,024 labels.
* ``nested``  64 x 64 with 40 interleaved diagonal labels: every box is the whole image, so the summed
              box area (40 images' worth) is what makes the kernel's plan enlarge its bands.
* ``vol``     5 x 17 x 33 volume of blobs, one of them spanning all planes; ``flat`` is a Z = 1 volume.

Intensities (``image(name, kind)``, 2 channels): ``int`` is integer valued float32 (a uint16 ramp
plus noise), where float64 sums are exact in any order; ``float`` is a field whose first channel is
positive everywhere and whose second is negative everywhere, so minima or maxima that start from
zero show.
"""
from __future__ import annotations

import functools

import numpy as np

from bioengine_worker_amd.cellpose import reference as ref

CASES_2D = ("hand", "ragged", "big", "many", "nested")
CASES_3D = ("vol", "flat")
KINDS = ("int", "float")

HAND = np.array([
    [2, 2, 0, 0, 0, 0, 0, 0, 0],
    [2, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 3, 3, 3, 0, 5, 5, 5, 6],
    [0, 3, 0, 3, 0, 5, 5, 5, 6],
    [0, 3, 3, 3, 0, 5, 5, 5, 6],
    [0, 0, 0, 0, 1, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0],
], np.int32)
#: label 1: one pixel; 2: touches the top and the left border; 3: a ring (the hole's inner edge is
#: boundary: all 8 pixels); 4: absent; 5 and 6 share an edge (5's right column is boundary against 6,
#: only its centre pixel is interior); 6 lies on the right border.
HAND_RAW = {
    "area": [1, 3, 8, 0, 9, 3],
    "sum_y": [5, 1, 24, 0, 27, 9],
    "sum_x": [4, 1, 16, 0, 54, 24],
    "sum_yy": [25, 1, 78, 0, 87, 29],
    "sum_xx": [16, 1, 38, 0, 330, 192],
    "sum_xy": [20, 0, 48, 0, 162, 72],
    "bbox": [[5, 4, 6, 5], [0, 0, 2, 2], [2, 1, 5, 4], [0, 0, 0, 0], [2, 5, 5, 8], [2, 8, 5, 9]],
    "boundary": [1, 3, 8, 0, 8, 3],
    # with the one-channel image 10 * y + x
    "int_sum": [[54.0], [11.0], [256.0], [0.0], [324.0], [114.0]],
    "int_sumsq": [[2916.0], [101.0], [8798.0], [0.0], [12270.0], [4532.0]],
    "int_min": [[54.0], [0.0], [21.0], [0.0], [25.0], [28.0]],
    "int_max": [[54.0], [10.0], [43.0], [0.0], [47.0], [48.0]],
}
HAND_IMAGE = (10.0 * np.arange(7)[:, None] + np.arange(9)[None, :]).astype(np.float32)[None]
HAND_OUTLINES = (HAND > 0) & ~((np.arange(7)[:, None] == 3) & (np.arange(9)[None, :] == 6))


def _voronoi(H, W, n, seed):
    """n labels, every one present: seeds lie outside the zero band (rows 20..24)."""
    out = np.zeros((H, W), np.int32)
    if n == 0:
        return out
    rng = np.random.default_rng(seed)
    ys = rng.choice(np.r_[0:20, 25:H], n)
    xs = rng.integers(0, W, n)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[None] - ys[:, None, None]) ** 2 + (xx[None] - xs[:, None, None]) ** 2
    out = (np.argmin(d, 0) + 1).astype(np.int32)
    out[20:25] = 0
    if len(np.unique(out)) != n + 1:  # two seeds on one pixel: draw again
        return _voronoi(H, W, n, seed + 100)
    return out


def _spiral(n):
    """One-pixel-wide square spiral (arms two pixels apart) from the corner inwards: label 1."""
    out = np.zeros((n, n), np.int32)
    y0, x0, y1, x1 = 0, 0, n - 1, n - 1
    while y1 - y0 >= 3 and x1 - x0 >= 3:
        out[y0, x0:x1 + 1] = 1
        out[y0:y1 + 1, x1] = 1
        out[y1, x0:x1 + 1] = 1
        out[y0 + 2:y1 + 1, x0] = 1
        out[y0 + 2, x0:x0 + 2] = 1  # on to the next ring
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return out


@functools.lru_cache(maxsize=None)
def masks(name: str) -> np.ndarray:
    """2-D cases -> [B, H, W] int32; 3-D cases -> [Z, H, W] int32."""
    if name == "hand":
        m = HAND[None].copy()
    elif name == "ragged":
        m = np.stack([_voronoi(45, 67, n, s) for n, s in ((5, 1), (40, 2), (0, 3))])
        assert [int(x.max()) for x in m] == [5, 40, 0]
        assert all(len(np.unique(x)) == int(x.max()) + 1 for x in m)
    elif name == "big":
        m = np.stack([np.ones((300, 300), np.int32), _spiral(300)])
        ys, xs = np.nonzero(m[1])
        assert (ys.min(), ys.max(), xs.min(), xs.max()) == (0, 299, 0, 299)
    elif name == "many":
        yy, xx = np.mgrid[0:64, 0:64]
        m = ((yy // 2) * 32 + xx // 2 + 1).astype(np.int32)[None]
    elif name == "nested":
        yy, xx = np.mgrid[0:64, 0:64]
        m = ((yy + xx) % 40 + 1).astype(np.int32)[None]
    elif name == "vol":
        Z, H, W = 5, 17, 33
        zz, yy, xx = np.mgrid[0:Z, 0:H, 0:W]
        m = np.zeros((Z, H, W), np.int32)
        m[((zz - 2) / 1.6) ** 2 + ((yy - 5) / 4.0) ** 2 + ((xx - 6) / 5.0) ** 2 <= 1] = 1
        m[((yy - 11) / 3.0) ** 2 + ((xx - 18) / 6.0) ** 2 <= 1] = 2          # spans all planes
        m[(zz >= 3) & (abs(yy - 4) <= 2) & (abs(xx - 28) <= 3)] = 3          # against the z = Z - 1 face
        m[(zz <= 1) & (yy >= 14) & (xx >= 29)] = 5                            # a corner; label 4 is absent
        assert set(np.unique(m[:, 11, 18])) == {2}
    elif name == "flat":
        m = np.ascontiguousarray(masks("ragged")[1][None, :17, :33])
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def image(name: str, kind: str) -> np.ndarray:
    """2-D cases -> [B, 2, H, W] float32; 3-D cases -> [Z, 2, H, W] float32 (planes first)."""
    m = masks(name)
    n, H, W = m.shape
    rng = np.random.default_rng(7)
    if kind == "int":
        ramp = ((np.arange(H)[:, None] * W + np.arange(W)[None, :]) * 13 % 60000).astype(np.float32)
        img = ramp[None, None] + rng.integers(0, 5000, (n, 2, H, W)).astype(np.float32)
        assert img.max() < 65536 and (img == np.round(img)).all()
    else:
        mag = np.abs(rng.standard_normal((n, 2, H, W))).astype(np.float32) * np.float32(1.7) + np.float32(0.25)
        img = mag * np.array([1.0, -1.0], np.float32)[None, :, None, None]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle(name: str, kind: str | None):
    """``reference.measure_masks`` with outlines: a list with one dict per image for the 2-D cases,
    one dict for the 3-D ones.  ``kind`` None: without intensities."""
    m = masks(name)
    if name in CASES_3D:
        im = None if kind is None else np.ascontiguousarray(image(name, kind).transpose(1, 0, 2, 3))
        return ref.measure_masks(m, im, outlines=True)
    return [ref.measure_masks(m[b], None if kind is None else image(name, kind)[b], outlines=True)
            for b in range(m.shape[0])]
