"""Label images for the outline tests (``reference.mask_rings`` and its HIP kernel).

A helper, not a test file.  Every builder is cached and every oracle result is computed once and
shared; tests must not write into what they get.  ``masks(name)`` is always a [B, H, W] int32 batch.

From ``cellpose_measure_cases``: ``hand`` (expected rings written out as literals, ``HAND_RINGS``),
``ragged`` (B = 3, width 67, one all-zero image), ``big`` (300 x 300: the full-image label and the
one-pixel spiral with 602 turn vertices; both boxes are beyond 64 x 64), ``many`` (1,024 labels of
2 x 2), ``nested`` (every pixel its own ring: 4,096 rings) and ``vol`` (the 5 x 17 x 33 volume read
as planes).  Built here, at the sizes where the kernel changes path:

* ``wide``    5 x 131 and ``tall`` 131 x 5: one label with a notch and a hole at columns / rows
              62..66 and 126..130, across the 64-bit word boundaries; the box is beyond 64 in one
              direction only.
* ``holes``   16 x 16: label 1 with two holes; one holds an island of label 2, the other an island
              of label 1 itself, which has a hole of its own (contained in two outer rings).
* ``saddle``  6 x 6: a ring through one corner twice, and two diagonal pixels of label 2 that stay
              separate rings.
* ``border``  4 x 70: labels on all four borders; label 1 is the whole first row.
"""
from __future__ import annotations

import functools

import numpy as np

import cellpose_measure_cases as mc
from bioengine_worker_amd.cellpose import reference as ref

CASES = ("hand", "ragged", "big", "many", "nested", "wide", "tall", "holes", "saddle", "border", "vol")

#: (label, vertices (y, x), area2) of every ring of ``hand``, in order
HAND_RINGS = [
    (1, [(5, 4), (5, 5), (6, 5), (6, 4)], 2),
    (2, [(0, 0), (0, 2), (1, 2), (1, 1), (2, 1), (2, 0)], 6),
    (3, [(2, 1), (2, 4), (5, 4), (5, 1)], 18),
    (3, [(4, 2), (4, 3), (3, 3), (3, 2)], -2),
    (5, [(2, 5), (2, 8), (5, 8), (5, 5)], 18),
    (6, [(2, 8), (2, 9), (5, 9), (5, 8)], 6),
]


def _wide() -> np.ndarray:
    m = np.ones((5, 131), np.int32)
    m[0, 63:66] = 0      # a notch in the top side, across column 64
    m[2, 62:67] = 0      # a hole across column 64
    m[2, 126:130] = 0    # a hole across column 128
    m[4, 127:131] = 0    # a notch that takes the bottom right corner
    m[0, 128] = 0
    return m


@functools.lru_cache(maxsize=None)
def masks(name: str) -> np.ndarray:
    if name in mc.CASES_2D or name == "vol":
        return mc.masks(name)
    if name == "wide":
        m = _wide()[None]
    elif name == "tall":
        m = np.ascontiguousarray(_wide().T)[None]
    elif name == "holes":
        m = np.zeros((16, 16), np.int32)
        m[1:15, 1:15] = 1
        m[3:8, 3:8] = 0
        m[5, 5] = 2          # an island of another label in the first hole
        m[9:14, 3:13] = 0
        m[10:13, 5:8] = 1    # an island of the same label in the second hole ...
        m[11, 6] = 0         # ... with a hole of its own
        m = m[None]
    elif name == "saddle":
        m = np.zeros((6, 6), np.int32)
        m[1:4, 1:4] = 1
        m[1, 1] = m[2, 2] = 0  # (1, 2) and (2, 1) meet at corner (2, 2) only; joined round the loop
        m[4, 4] = m[5, 5] = 2
        m = m[None]
    elif name == "border":
        m = np.zeros((4, 70), np.int32)
        m[0, :] = 1
        m[1:, 0] = 2
        m[3, 5:41] = 3
        m[1:, 69] = 4
        m = m[None]
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle(name: str) -> tuple:
    """``reference.mask_rings`` of every image of the case."""
    return tuple(ref.mask_rings(m) for m in masks(name))


def join(per_image) -> dict:
    """Per-image rings dicts -> the arrays of a whole batch, as ``gpu.mask_rings_gpu`` returns them."""
    nv = np.cumsum([0] + [r["verts"].shape[0] for r in per_image])
    nr = np.cumsum([0] + [r["ring_label"].shape[0] for r in per_image])
    return {
        "verts": np.concatenate([r["verts"] for r in per_image]).astype(np.int32).reshape(-1, 2),
        "ring_offsets": np.concatenate([r["ring_offsets"][:-1] + nv[b] for b, r in enumerate(per_image)]
                                       + [nv[-1:]]).astype(np.int64),
        "ring_label": np.concatenate([r["ring_label"] for r in per_image]).astype(np.int32),
        "ring_area2": np.concatenate([r["ring_area2"] for r in per_image]).astype(np.int64),
        "ring_image": np.concatenate([np.full(r["ring_label"].shape[0], b) for b, r in enumerate(per_image)]).astype(np.int32),
        "image_rings": nr.astype(np.int64),
    }


@functools.lru_cache(maxsize=None)
def batch_oracle(name: str) -> dict:
    return join(oracle(name))
