"""Inputs shared by the z-stack stitching tests (CPU oracle and HIP kernels): small label stacks
[Z, H, W] int32 whose per-plane ids are unrelated, each built to hit one rule of
``bioengine_worker_amd.cellpose.reference.stitch3d``."""
import numpy as np


def shuffle_ids(vol: np.ndarray, rng) -> np.ndarray:
    """Permute the non-zero ids of every plane independently."""
    n = int(vol.max())
    out = np.zeros_like(vol)
    for z in range(vol.shape[0]):
        lut = np.concatenate([[0], rng.permutation(n) + 1]).astype(vol.dtype)
        out[z] = lut[vol[z]]
    return out


def prisms(Z=6, H=48, W=64, side=9, pitch=12, seed=0):
    """Grid of ``side`` x ``side`` squares constant in z -> (truth, per-plane shuffled ids)."""
    truth = np.zeros((Z, H, W), np.int32)
    k = 0
    for y in range(1, H - side + 1, pitch):
        for x in range(1, W - side + 1, pitch):
            k += 1
            truth[:, y: y + side, x: x + side] = k
    return truth, shuffle_ids(truth, np.random.default_rng(seed))


def spheres(seed=0, Z=24, S=64, n=10):
    """``n`` random non-touching spheres (radius 5 to 8, real-valued centres) -> (truth, shuffled)."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.mgrid[0:Z, 0:S, 0:S]
    placed = []
    while len(placed) < n:
        r = rng.uniform(5, 8)
        c = np.array([rng.uniform(r, d - 1 - r) for d in (Z, S, S)])
        if any(np.linalg.norm(c - c2) < r + r2 + 1.5 for c2, r2 in placed):
            continue
        placed.append((c, r))
    truth = np.zeros((Z, S, S), np.int32)
    for i, (c, r) in enumerate(placed):
        truth[(zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r] = i + 1
    return truth, shuffle_ids(truth, rng)


def rect(shape, y0, x0, h, w, lab, into=None):
    m = np.zeros(shape, np.int32) if into is None else into
    m[y0: y0 + h, x0: x0 + w] = lab
    return m


def threshold_pair():
    """Two 4 x 5 rectangles shifted by 3 columns: ov = 8, u = 32, IoU exactly 0.25."""
    s = (8, 12)
    return np.stack([rect(s, 2, 1, 4, 5, 1), rect(s, 2, 4, 4, 5, 1)])


def tie_two_next():
    """Previous mask 1 (4 x 6) overlapped with identical IoU 8/16 by next masks 2 and 5 (4 x 2 each,
    inside it): the smaller id links, the other is new."""
    s = (8, 12)
    nxt = rect(s, 2, 2, 4, 2, 5)
    rect(s, 2, 6, 4, 2, 2, into=nxt)
    return np.stack([rect(s, 2, 2, 4, 6, 1), nxt])


def owns_two_unequal():
    """Next mask 1 (4 x 8) covers previous masks 3 (4 x 2, IoU 8/32) and 4 (4 x 5, IoU 20/32) and
    owns both: it links to the larger IoU (4); 3 ends."""
    s = (8, 14)
    prev = rect(s, 2, 1, 4, 2, 3)
    rect(s, 2, 4, 4, 5, 4, into=prev)
    return np.stack([prev, rect(s, 2, 1, 4, 8, 1)])


def equal_ratios():
    """Next mask 1 (area 6) owns previous masks 2 (area 2, ov 2: IoU 2/6) and 3 (area 10, ov 4: IoU
    4/12): different (ov, u) pairs, equal ratio -- treated as equal, so the smaller previous label
    (2) is the link.  Reversed in z it is the owner rule's tie: one previous mask, two next masks."""
    s = (6, 16)
    prev = np.zeros(s, np.int32)
    prev[1, 1:3] = 2          # area 2, both pixels inside b
    prev[1, 3:7] = 3          # 4 pixels inside b ...
    prev[2, 3:9] = 3          # ... + 6 outside: area 10
    nxt = np.zeros(s, np.int32)
    nxt[1, 1:7] = 1           # area 6
    return np.stack([prev, nxt])


def empty_leading():
    s = (8, 12)
    return np.stack([np.zeros(s, np.int32), rect(s, 1, 1, 4, 4, 2), rect(s, 1, 1, 4, 4, 1)])


def empty_middle():
    s = (8, 12)
    a = rect(s, 1, 1, 4, 4, 1)
    rect(s, 1, 7, 3, 3, 2, into=a)
    return np.stack([a, np.zeros(s, np.int32), a.copy(), a.copy()])


def gaps():
    """Labels {3, 7} only (ids with no pixels do not exist)."""
    s = (8, 12)
    a = rect(s, 1, 1, 4, 4, 3)
    rect(s, 1, 7, 3, 3, 7, into=a)
    b = rect(s, 1, 1, 4, 4, 7)
    rect(s, 1, 7, 3, 3, 3, into=b)
    return np.stack([a, b, a.copy()])


def many_labels(Z=5, S=200, side=3, pitch=5):
    """40 x 40 grid of 3 x 3 squares (1,600 labels per plane); odd planes shifted one pixel in x so
    that every IoU is 6/12."""
    base = np.zeros((S, S), np.int32)
    k = 0
    for y in range(0, S - pitch + 1, pitch):
        for x in range(0, S - pitch + 1, pitch):
            k += 1
            base[y + 1: y + 1 + side, x: x + side] = k
    rng = np.random.default_rng(1)
    vol = np.stack([np.roll(base, 1, axis=1) if z % 2 else base for z in range(Z)])
    return shuffle_ids(vol, rng)


def one_large(Z=4, S=200):
    """One 150 x 150 object in every plane (a single (b, a) key takes every workgroup's increments),
    with a small neighbour."""
    a = rect((S, S), 10, 20, 150, 150, 1)
    rect((S, S), 170, 5, 6, 9, 2, into=a)
    return np.stack([a] * Z)


def ragged(H, W, Z=4, seed=3):
    """Random blocky labels on an H x W plane whose size is no multiple of the vector width."""
    rng = np.random.default_rng(seed)
    out = np.zeros((Z, H, W), np.int32)
    for z in range(Z):
        coarse = rng.integers(0, 6, ((H + 3) // 4, (W + 3) // 4))
        out[z] = np.kron(coarse, np.ones((4, 4), np.int64))[:H, :W]
    return out


EDGE_CASES = {
    "threshold": threshold_pair,
    "tie_two_next": tie_two_next,
    "owns_two_unequal": owns_two_unequal,
    "equal_ratios": equal_ratios,
    "equal_ratios_owner": lambda: equal_ratios()[::-1].copy(),
    "empty_leading": empty_leading,
    "empty_middle": empty_middle,
    "all_empty": lambda: np.zeros((3, 8, 12), np.int32),
    "single_plane": lambda: gaps()[:1],
    "gaps": gaps,
}
