"""Polygon batches for the rasteriser tests (``reference.rasterize_rings`` and its HIP kernel).

A helper, not a test file.  Every builder is cached and every oracle result is computed once and
shared; tests must not write into what they get.  ``polys(name)`` is ``(polygons dict of the whole
batch, (B, H, W))``; the dict carries ``ring_image`` (``ragged``: ``image_rings`` instead), and
``oracle(name)`` is ``reference.rasterize_rings`` per image, int32 [B, H, W].

``rings:<case>`` for every case of ``cellpose_rings_cases`` (imported, not copied): the axis-parallel
integer rings of ``mask_rings``, whose raster is the mask they came from.  Built here, at the sizes
where the kernel changes path (a job is 64 rows x 256 columns, edges are walked 64 at a time):

* ``ties``        B = 3, 8 x 8: the square (0.5, 0.5) .. (2.5, 2.5), the triangle (0.5, 0.5), (0.5, 4.5),
                  (4.5, 0.5) and the bow tie (0, 0), (0, 8), (8, 0), (8, 8): centres on edges.
* ``partition``   40 x 40: a jittered 6 x 6 grid of quads on the half-pixel lattice, each split into
                  two triangles (72 labels); the shared edges pass through centres.
* ``overlap``     three overlapping polygons with labels 5, 2, 9 in that order: the maximum wins.
* ``outside``     20 x 24: vertices left of, above and beyond the image, one polygon wholly outside
                  on the right and one wholly at negative coordinates.
* ``sliver``      a polygon that contains no centre (its label is absent) beside an ordinary one.
* ``multi``       GeoJSON: a MultiPolygon with a hole and an island in the hole, given with both
                  orientations (labels 1 and 2).
* ``degenerate``  repeated vertices, collinear runs, a horizontal edge exactly on a centre line, a
                  two-vertex ring and an empty ring.
* ``edges``       groups of 63, 64, 65 and 129 edges, and one label of two 40-edge rings, the second
                  of which straddles the 64-edge block.
* ``bands``       B = 4, 132 x 600: boxes of 63 x 255, 64 x 256 and 65 x 257 pixels (one below, at
                  and one above a job's rows and columns) and a slanted quadrilateral of 131 x 599
                  pixels: three bands, three chunks, crossings left of the second and third chunk.
* ``gon``         a 1000-gon of 290 px diameter in 300 x 300.
* ``many``        1,024 small fractional pentagons in 256 x 256, labels shuffled.
* ``ragged``      B = 3, 33 x 47, the second image without polygons; ``image_rings`` form.
* ``stars``       B = 20, 24 x 24: random star-shaped polygons, every third snapped to the half-pixel
                  lattice (the Fraction test's inputs).
"""
from __future__ import annotations

import functools

import numpy as np

import cellpose_rings_cases as rc
from bioengine_worker_amd.cellpose import reference as ref

RINGS_CASES = tuple(f"rings:{n}" for n in rc.CASES)
CASES = RINGS_CASES + ("ties", "partition", "overlap", "outside", "sliver", "multi", "degenerate", "edges", "bands", "gon",
                       "many", "ragged", "stars")

SQUARE = [(0.5, 0.5), (0.5, 2.5), (2.5, 2.5), (2.5, 0.5)]
TRIANGLE = [(0.5, 0.5), (0.5, 4.5), (4.5, 0.5)]
BOW_TIE = [(0, 0), (0, 8), (8, 0), (8, 8)]


def batch(items, dtype=np.float64) -> dict:
    """``[(image, label, vertices (y, x)), ...]`` -> a polygons dict with ``ring_image``."""
    vs = [np.asarray(v, np.float64).reshape(-1, 2) for _, _, v in items]
    return {"verts": (np.concatenate(vs) if vs else np.zeros((0, 2))).astype(dtype),
            "ring_offsets": np.concatenate([[0], np.cumsum([v.shape[0] for v in vs])]).astype(np.int64),
            "ring_label": np.asarray([l for _, l, _ in items], np.int32),
            "ring_image": np.asarray([b for b, _, _ in items], np.int32)}


def ngon(n: int, cy: float, cx: float, r: float, phase: float = 0.1, reverse: bool = False) -> np.ndarray:
    a = phase + 2 * np.pi * np.arange(n) / n
    v = np.stack([cy + r * np.sin(a), cx + r * np.cos(a)], 1)
    return v[::-1] if reverse else v


@functools.lru_cache(maxsize=None)
def partition_triangles() -> tuple:
    """The 72 triangles of ``partition`` as [3, 2] arrays (y, x)."""
    rng = np.random.default_rng(11)
    g = np.round(np.arange(7) * 40 / 6 * 2) / 2  # 0, 6.5, 13.5, 20, 26.5, 33.5, 40
    py, px = np.meshgrid(g, g, indexing="ij")
    jy, jx = (rng.integers(-3, 4, (7, 7)) / 2 for _ in range(2))
    inner = np.zeros((7, 7), bool)
    inner[1:-1, 1:-1] = True
    py, px = py + jy * inner, px + jx * inner
    tris = []
    for i in range(6):
        for j in range(6):
            a, b, c, d = ((py[u, v], px[u, v]) for u, v in ((i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j)))
            tris += [np.asarray([a, b, c]), np.asarray([a, c, d])]
    return tuple(tris)


@functools.lru_cache(maxsize=None)
def star_polygons() -> tuple:
    rng = np.random.default_rng(5)
    out = []
    for i in range(20):
        n = int(rng.integers(5, 12))
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        r = rng.uniform(2.0, 10.0, n)
        v = np.stack([12 + r * np.sin(a), 12 + r * np.cos(a)], 1)
        if i % 3 == 0:
            v = np.round(v * 2) / 2  # vertices on the half-pixel lattice: centres sit on edges
        out.append(v)
    return tuple(out)


MULTI_GEOJSON = {"type": "FeatureCollection", "features": [
    {"type": "Feature", "properties": {"label": 1}, "geometry": {"type": "MultiPolygon", "coordinates": [
        [[[1.5, 1.5], [1.5, 14.5], [14.5, 14.5], [14.5, 1.5], [1.5, 1.5]],       # exterior, counter-clockwise in (x, y)
         [[4.25, 4.25], [11.75, 4.25], [11.75, 11.75], [4.25, 11.75], [4.25, 4.25]]],  # hole, clockwise
        [[[6.5, 6.5], [6.5, 9.5], [9.5, 9.5], [9.5, 6.5], [6.5, 6.5]]]]}},       # the island in the hole
    {"type": "Feature", "properties": {"label": 2}, "geometry": {"type": "MultiPolygon", "coordinates": [
        [[[17.5, 1.5], [30.5, 1.5], [30.5, 14.5], [17.5, 14.5], [17.5, 1.5]],    # the same, every ring reversed
         [[20.25, 4.25], [20.25, 11.75], [27.75, 11.75], [27.75, 4.25], [20.25, 4.25]]],
        [[[22.5, 6.5], [25.5, 6.5], [25.5, 9.5], [22.5, 9.5], [22.5, 6.5]]]]}}]}


@functools.lru_cache(maxsize=None)
def polys(name: str) -> tuple:
    if name.startswith("rings:"):
        case = name[6:]
        return rc.batch_oracle(case), tuple(rc.masks(case).shape)
    if name == "ties":
        return batch([(0, 1, SQUARE), (1, 1, TRIANGLE), (2, 1, BOW_TIE)]), (3, 8, 8)
    if name == "partition":
        return batch([(0, k + 1, t) for k, t in enumerate(partition_triangles())]), (1, 40, 40)
    if name == "overlap":
        return batch([(0, 5, [(2.2, 2.7), (2.2, 20.1), (19.6, 20.1), (19.6, 2.7)]),
                      (0, 2, [(8.4, 8.3), (8.4, 28.9), (27.7, 28.9), (27.7, 8.3)]),
                      (0, 9, ngon(7, 14.3, 15.8, 6.4))]), (1, 30, 31)
    if name == "outside":
        return batch([(0, 1, [(-3.2, -5.3), (7.4, 30.0), (26.1, 11.6)]),
                      (0, 2, [(3.0, 40.0), (3.0, 50.0), (12.0, 50.0), (12.0, 40.0)]),
                      (0, 3, [(-9.0, -9.0), (-9.0, -2.0), (-2.0, -2.0), (-2.0, -9.0)]),
                      (0, 4, [(15.2, -4.0), (15.2, 3.3), (22.9, 3.3), (22.9, -4.0)])]), (1, 20, 24)
    if name == "sliver":
        return batch([(0, 1, ngon(6, 9.1, 8.2, 4.3)),
                      (0, 2, [(2.6, 1.2), (2.9, 10.7), (2.7, 10.9), (2.55, 1.3)])]), (1, 16, 16)
    if name == "multi":
        return dict(ref.outlines_to_rings(MULTI_GEOJSON), ring_image=np.zeros(6, np.int32)), (1, 16, 32)
    if name == "degenerate":
        return batch([(0, 1, [(1.2, 1.2), (1.2, 1.2), (1.2, 9.7), (1.2, 9.7), (1.2, 9.7), (8.8, 9.7), (8.8, 1.2), (1.2, 1.2)]),
                      (0, 2, [(10.0, 2.0), (10.0, 5.0), (10.0, 8.0), (12.0, 8.0), (14.0, 8.0), (14.0, 2.0), (12.0, 2.0)]),
                      (0, 3, [(3.5, 12.0), (3.5, 19.0), (9.5, 19.0), (9.5, 12.0)]),  # top and bottom on centre lines
                      (0, 4, [(2.0, 2.0), (18.0, 18.0)]),
                      (0, 5, []),
                      (0, 6, [(15.1, 10.2), (18.7, 19.3), (18.7, 10.2)])]), (1, 20, 22)
    if name == "edges":
        return batch([(0, 1, ngon(63, 14.3, 14.6, 12.2)), (0, 2, ngon(64, 14.4, 44.1, 12.2)),
                      (0, 3, ngon(65, 44.2, 14.3, 12.2)), (0, 4, ngon(129, 44.6, 44.4, 12.2)),
                      (0, 5, ngon(40, 29.7, 74.2, 13.1)), (0, 5, ngon(40, 29.7, 74.2, 6.3, reverse=True))]), (1, 60, 90)
    if name == "bands":
        def box(rows, cols):  # a box of rows x cols centres, its right side pulled in at mid height
            return [(0.3, 0.2), (0.3, cols + 0.2), (rows / 2 + 0.1, cols - 4.3), (rows + 0.3, cols + 0.2), (rows + 0.3, 0.2)]
        return batch([(0, 1, box(63, 255)), (1, 2, box(64, 256)), (2, 3, box(65, 257)),
                      (3, 4, [(0.4, 0.3), (40.7, 599.4), (131.4, 520.6), (90.2, 10.8)])]), (4, 132, 600)
    if name == "gon":
        return batch([(0, 1, ngon(1000, 150.2, 149.7, 145.0))]), (1, 300, 300)
    if name == "many":
        rng = np.random.default_rng(3)
        labels = rng.permutation(1024) + 1
        return batch([(0, int(labels[k]), ngon(5, 8 * (k // 32) + 4 + rng.uniform(-0.5, 0.5), 8 * (k % 32) + 4 + rng.uniform(-0.5, 0.5),
                                              rng.uniform(2.0, 3.6), rng.uniform(0, 6.28))) for k in range(1024)]), (1, 256, 256)
    if name == "ragged":
        b = batch([(0, 1, ngon(9, 10.3, 11.8, 8.2)), (0, 3, ngon(5, 24.4, 33.1, 7.7)),
                   (2, 2, ngon(12, 16.6, 20.2, 14.9)), (2, 1, [(1.5, 30.5), (1.5, 46.5), (9.5, 46.5)])], np.float32)
        del b["ring_image"]
        return dict(b, image_rings=np.asarray([0, 2, 2, 4], np.int64)), (3, 33, 47)
    if name == "stars":
        return batch([(b, b + 1, v) for b, v in enumerate(star_polygons())]), (20, 24, 24)
    raise KeyError(name)


def ring_images(name: str) -> np.ndarray:
    p, (B, _, _) = polys(name)
    if "ring_image" in p:
        return np.asarray(p["ring_image"])
    return np.repeat(np.arange(B), np.diff(p["image_rings"]))


def image_polys(name: str, b: int) -> dict:
    """The polygons dict of image ``b`` alone."""
    p, _ = polys(name)
    rs = np.flatnonzero(ring_images(name) == b)
    off = np.asarray(p["ring_offsets"])
    vs = [np.asarray(p["verts"])[off[r]:off[r + 1]] for r in rs]
    return {"verts": np.concatenate(vs) if vs else np.zeros((0, 2)),
            "ring_offsets": np.concatenate([[0], np.cumsum([v.shape[0] for v in vs])]).astype(np.int64),
            "ring_label": np.asarray(p["ring_label"])[rs]}


@functools.lru_cache(maxsize=None)
def oracle(name: str) -> np.ndarray:
    _, (B, H, W) = polys(name)
    out = np.stack([ref.rasterize_rings(image_polys(name, b), (H, W)) for b in range(B)])
    out.setflags(write=False)
    return out


def invalid_inputs() -> list:
    """``(polygons dict, (B, H, W), a word of the message)`` of every input ``rasterize_rings_gpu`` refuses."""
    p, _ = polys("overlap")
    r, _ = polys("ragged")
    return [(dict(p, ring_offsets=p["ring_offsets"][:-1]), (1, 30, 31), "ring_offsets"),
            (dict(p, ring_label=np.asarray([1, 0, 2])), (1, 30, 31), "labels"),
            (dict(p, verts=p["verts"] * np.inf), (1, 30, 31), "finite"),
            (dict(p, verts=p["verts"] + 1e5), (1, 30, 31), "outside"),
            (dict(p, ring_image=np.asarray([0, 1, 0])), (1, 30, 31), "ring_image"),
            (dict(p, ring_image=np.asarray([0, -1, 0])), (1, 30, 31), "ring_image"),
            (dict(p, ring_image=np.asarray([0, 0])), (1, 30, 31), "ring_image"),
            ({k: v for k, v in p.items() if k != "ring_image"}, (1, 30, 31), "ring_image"),
            (dict(r, image_rings=np.asarray([0, 2, 4])), (3, 33, 47), "image_rings"),
            (dict(r, image_rings=np.asarray([0, 3, 2, 4])), (3, 33, 47), "image_rings"),
            (p, (1, 2 ** 15 + 1, 8), "too large"), (p, (1, 8, 2 ** 15 + 1), "too large"), (p, (2048, 1024, 1024), "too large")]
