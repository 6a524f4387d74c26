"""Label-image pairs for the average-precision tests (CPU: tests/test_cellpose_ap.py; GPU:
tests/test_cellpose_ap_gpu.py).  ``pair(name)`` is (true, predicted), each [B, ...] int32; built once
and never written to.  ``oracle(name, thresholds)`` is ``metrics.average_precision`` on it, computed
once per (case, thresholds) and shared.

The GPU scorer returns the edge count of the threshold graph wherever no label has two edges, and
sends an image to the host otherwise.  The tests rely on which cases are which, so the CPU suite
asserts it: ``NO_TWO_EDGE`` cases have no two-edge label at 0.5 / 0.75 / 0.9, ``TWO_EDGE`` maps a
case to thresholds at which it has one.
"""
from __future__ import annotations

import functools

import numpy as np

from bioengine_worker_amd.cellpose import metrics

ALL_THRESHOLDS = (0.1, 0.25, 0.5, 0.51, 0.75, 0.9)
HIGH_THRESHOLDS = (0.5, 0.75, 0.9)
DISK_SHAPE = (96, 120)
DISK_COUNTS = (40, 33, 25)  # labels painted per image of the "disks" batch


def _boxes(shape, boxes):
    m = np.zeros(shape, np.int32)
    for k, (y0, y1, x0, x1) in enumerate(boxes, start=1):
        m[y0:y1, x0:x1] = k
    return m


def _disks(n: int, seed: int):
    """About ``n`` disks on a jittered 5 x 8 grid, and a prediction of them: centres moved by up to a
    pixel, radii scaled by 0.85 .. 1.1, a tenth dropped, labels permuted."""
    H, W = DISK_SHAPE
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    t = np.zeros((H, W), np.int32)
    p = np.zeros((H, W), np.int32)
    perm = rng.permutation(n) + 1
    for i in range(n):
        cy = 10 + 19 * (i // 8) + rng.uniform(-2, 2)
        cx = 8 + 15 * (i % 8) + rng.uniform(-2, 2)
        r = rng.uniform(4.0, 6.5)
        t[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i + 1
        if rng.random() < 0.1:
            continue
        cy, cx, r = cy + rng.uniform(-1, 1), cx + rng.uniform(-1, 1), r * rng.uniform(0.85, 1.1)
        p[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = perm[i]
    return t, p


def _noise(nlab: int, seed: int):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, nlab, DISK_SHAPE).astype(np.int32), rng.integers(0, nlab, DISK_SHAPE).astype(np.int32))


def _exact_iou():
    """Four pairs, true a 1 x A strip and predicted its first ``ov`` pixels: IoU = ov / A exactly
    1/2, 3/4, 9/10 and 27/30."""
    t = np.zeros((8, 32), np.int32)
    p = np.zeros((8, 32), np.int32)
    for k, (ov, a) in enumerate([(1, 2), (3, 4), (9, 10), (27, 30)], start=1):
        t[2 * k - 2, :a] = k
        p[2 * k - 2, :ov] = k
    return t, p


def _grid1600():
    """1,600 labels of 5 x 5 pixels on 200 x 200 and the same grid moved by one pixel each way,
    labels reversed and some pixels cleared: a workgroup's 8,192 pixels (41 rows) meet ~360 labels with
    ~4 overlaps each, more distinct pairs than the 1,024 slots of its LDS table."""
    yy, xx = np.mgrid[:200, :200]
    t = ((yy // 5) * 40 + xx // 5 + 1).astype(np.int32)
    ys, xs = np.minimum(yy + 1, 199), np.minimum(xx + 1, 199)
    p = (1601 - ((ys // 5) * 40 + xs // 5 + 1)).astype(np.int32)
    p[::17, ::3] = 0
    return t, p


def _large():
    t = np.zeros((128, 160), np.int32)
    p = np.zeros((128, 160), np.int32)
    t[2:120, 3:150] = 1
    p[8:128, 0:140] = 1
    return t, p


def _volume():
    rng = np.random.default_rng(5)
    zz, yy, xx = np.mgrid[:5, :40, :40]
    t = np.zeros((5, 40, 40), np.int32)
    p = np.zeros((5, 40, 40), np.int32)
    for i in range(9):
        c = np.array([2, 7 + 13 * (i // 3), 7 + 13 * (i % 3)]) + rng.uniform(-1, 1, 3)
        r = rng.uniform(3.5, 5.5)
        t[(2 * (zz - c[0])) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r] = i + 1
        c, r = c + rng.uniform(-0.7, 0.7, 3), r * rng.uniform(0.9, 1.1)
        if i != 4:
            p[(2 * (zz - c[0])) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r] = 9 - i
    return t, p


def _stack(pairs):
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


def _build(name: str):
    if name == "boxes":  # the hand-built boxes of tests/test_metrics_cpu.py, four 50 x 50 pairs
        two = _boxes((50, 50), [(0, 10, 0, 10), (20, 30, 20, 30)])
        zero = np.zeros_like(two)
        shifted = _boxes((50, 50), [(0, 10, 2, 12), (20, 30, 20, 30), (40, 45, 40, 45)])
        return _stack([(two, two.copy()), (two, zero), (zero, zero), (two, shifted)])
    if name == "split":  # one true box split into two predictions (IoU 0.6 and 0.4)
        return _stack([(_boxes((20, 40), [(0, 20, 0, 20)]), _boxes((20, 40), [(0, 20, 0, 12), (0, 20, 12, 20)]))])
    if name == "exact_iou":
        return _stack([_exact_iou()])
    if name == "exact_half":  # a 2-pixel true mask split into two 1-pixel predictions: IoU 0.5 twice, tp 1
        t = np.zeros((1, 4, 6), np.int32)
        p = np.zeros((1, 4, 6), np.int32)
        t[0, 1, 2:4] = 1
        p[0, 1, 2], p[0, 1, 3] = 1, 2
        return t, p
    if name == "disks":
        return _stack([_disks(n, 10 + i) for i, n in enumerate(DISK_COUNTS)])
    if name == "noise":
        return _stack([_noise(4, 1), _noise(5, 2)])
    if name == "disks_noise":  # one batch of one shape: three fallback-free images and two that need it
        (t, p), (tn, pn) = pair("disks"), pair("noise")
        return np.concatenate([t, tn]), np.concatenate([p, pn])
    if name == "ragged37":
        rng = np.random.default_rng(3)
        t = np.repeat(np.repeat(rng.integers(0, 9, (2, 10, 14)), 4, 1), 4, 2)[:, :37, :53].astype(np.int32)
        p = np.roll(t, 1, 2) * (rng.random((2, 37, 53)) > 0.05)
        return t, p.astype(np.int32)
    if name == "ragged7":
        return np.array([[[1, 1, 1, 0, 2, 2, 2]]], np.int32), np.array([[[2, 2, 2, 0, 0, 1, 1]]], np.int32)
    if name == "grid1600":
        return _stack([_grid1600(), _grid1600()[::-1]])
    if name == "large":
        return _stack([_large()])
    if name == "empty":  # empty truth, empty prediction, both empty
        t, p = _disks(12, 4)
        z = np.zeros_like(t)
        return _stack([(z, p), (t, z), (z, z)])
    if name == "volume":
        t, p = _volume()
        return t[None], p[None]
    raise KeyError(name)


CASES = ("boxes", "split", "exact_iou", "exact_half", "disks", "noise", "disks_noise", "ragged37", "ragged7",
         "grid1600", "large", "empty", "volume")
NO_TWO_EDGE = ("disks",)
TWO_EDGE = {"noise": (0.1,), "exact_half": (0.5,), "disks_noise": (0.1,)}


@functools.lru_cache(maxsize=None)
def pair(name: str):
    t, p = _build(name)
    return np.ascontiguousarray(t, np.int32), np.ascontiguousarray(p, np.int32)


@functools.lru_cache(maxsize=None)
def oracle(name: str, thresholds: tuple = HIGH_THRESHOLDS):
    t, p = pair(name)
    return metrics.average_precision(list(t), list(p), list(thresholds))


def oracle_of(t: np.ndarray, p: np.ndarray, thresholds):
    return metrics.average_precision(list(np.asarray(t)), list(np.asarray(p)), list(thresholds))


def edges(t: np.ndarray, p: np.ndarray, th: float) -> np.ndarray:
    """The threshold graph of one image pair as a boolean [n_true, n_pred] matrix."""
    if int(t.max()) == 0 or int(p.max()) == 0:
        return np.zeros((int(t.max()), int(p.max())), bool)
    return metrics.intersection_over_union(t, p)[1:, 1:] >= th


def has_two_edge_label(t, p, th) -> bool:
    e = edges(t, p, th)
    return bool((e.sum(0) > 1).any() or (e.sum(1) > 1).any())


def max_matching(t, p, th) -> int:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching

    e = edges(t, p, th)
    if e.size == 0:
        return 0
    return int((maximum_bipartite_matching(csr_matrix(e.astype(np.int8)), perm_type="column") >= 0).sum())


def same(got, want) -> None:
    """(ap, tp, fp, fn) equal exactly: integers, and float32 ``ap`` bit for bit, NaN positions included."""
    for g, w, name in zip(got, want, ("ap", "tp", "fp", "fn")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        if name == "ap":
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, g, w)
        else:
            assert np.array_equal(g, w), (name, g, w)
