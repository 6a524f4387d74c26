"""Label volumes for the surface tests (``reference.label_surface`` and its HIP kernels).

A helper, not a test file.  Every builder is cached and every oracle result is computed once and
shared; tests must not write into what they get.  ``volume(name)`` is a [Z, H, W] int32 volume,
``nlab(name)`` the bound its oracle result was computed with (``None``: the maximum).  The shapes
are the smallest that still reach every code path:

* ``single``  3^3 with one voxel: 6 quads, 8 vertices, every ``ncross == 3``.
* ``diag``    2 x 2 x 3: label 1 at (0,0,0) and (1,1,1), label 2 at (0,0,1): a shared non-manifold
              corner and a two-label face; 18 quads, 23 vertices.
* ``full``    2 x 3 x 4, all one label: every quad lies on the border.
* ``line``    1 x 1 x 70: Z = 1 and a row longer than a wave.
* ``rand``    5 x 6 x 7, uniform labels 0..3, seed 0: ``ncross`` spans 3..12.
* ``ball6``   the 17^3 ball of radius 6 (F = 678, V = 680), ``ball10`` the 25^3 ball of radius 10
              (F = 1902, V = 1904).
* ``cells``   12 x 37 x 70 with 10 random ellipsoids, some touching, a gap in the label numbering
              (no label 4) and one label (12) above the deliberately low ``nlab`` of 12.
* ``tall``    3 x 130 x 300: more corners than one tile of 256 or one scan block.
* ``empty``   all zeros; ``nolab``: labels present but ``nlab = 1``.
"""
from __future__ import annotations

import functools

import numpy as np

from bioengine_worker_amd.cellpose import reference as ref

CASES = ("single", "diag", "full", "line", "rand", "ball6", "ball10", "cells", "tall", "empty", "nolab")
NLAB = {"cells": 12, "nolab": 1}

#: area / (4 pi r^2) of the surface-net mesh of the balls (numpy prototype of the rule)
BALL_RATIO = {"ball6": 1.030294, "ball10": 1.027151}
BALL_COUNTS = {"ball6": (678, 680), "ball10": (1902, 1904)}  # (F, V)


def ball(r: int) -> np.ndarray:
    n, c = 2 * r + 5, r + 2
    z, y, x = np.ogrid[:n, :n, :n]
    return ((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2 <= r * r).astype(np.int32)


def _cells() -> np.ndarray:
    rng = np.random.default_rng(7)
    Z, H, W = 12, 37, 70
    z, y, x = np.ogrid[:Z, :H, :W]
    L = np.zeros((Z, H, W), np.int32)
    labels = [1, 2, 3, 5, 6, 7, 8, 9, 10, 12]  # no 4; 12 is above nlab - 1 = 11
    for l in labels:
        cz, cy, cx = rng.uniform(1, Z - 1), rng.uniform(3, H - 3), rng.uniform(4, W - 4)
        rz, ry, rx = rng.uniform(2, 5), rng.uniform(3, 9), rng.uniform(4, 12)
        inside = ((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
        L[inside] = l  # later ellipsoids overwrite earlier ones: touching labels
    return L


def _tall() -> np.ndarray:
    rng = np.random.default_rng(3)
    L = np.zeros((3, 130, 300), np.int32)
    blocks = rng.integers(0, 6, (3, 13, 30)).astype(np.int32)  # 10 x 10 blocks of labels 0..5
    L[:] = np.kron(blocks, np.ones((1, 10, 10), np.int32))
    L[1, 64:66, :] = 6  # a thin bar through the middle plane, across the tiles of a row
    return L


@functools.lru_cache(maxsize=None)
def volume(name: str) -> np.ndarray:
    if name == "single":
        L = np.zeros((3, 3, 3), np.int32)
        L[1, 1, 1] = 1
    elif name == "diag":
        L = np.zeros((2, 2, 3), np.int32)
        L[0, 0, 0] = L[1, 1, 1] = 1
        L[0, 0, 1] = 2
    elif name == "full":
        L = np.ones((2, 3, 4), np.int32)
    elif name == "line":
        L = np.ones((1, 1, 70), np.int32)
        L[0, 0, 30:33] = (2, 0, 2)
    elif name == "rand":
        L = np.random.default_rng(0).integers(0, 4, (5, 6, 7)).astype(np.int32)
    elif name in ("ball6", "ball10"):
        L = ball(int(name[4:]))
    elif name == "cells":
        L = _cells()
    elif name == "tall":
        L = _tall()
    elif name == "empty":
        L = np.zeros((4, 5, 6), np.int32)
    elif name == "nolab":
        L = np.random.default_rng(1).integers(0, 3, (4, 5, 6)).astype(np.int32)
    else:
        raise KeyError(name)
    L.setflags(write=False)
    return L


def nlab(name: str):
    return NLAB.get(name)


@functools.lru_cache(maxsize=None)
def oracle(name: str, bound: int | None = -1) -> dict:
    """``reference.label_surface`` of the case (with its own ``nlab`` unless ``bound`` is given),
    computed once; read-only arrays."""
    res = ref.label_surface(volume(name), nlab(name) if bound == -1 else bound)
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def stats(name: str, spacing=(1.0, 1.0, 1.0)) -> dict:
    return ref.surface_stats(oracle(name), spacing)
