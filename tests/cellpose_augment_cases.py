"""Shared by the test-time augmentation tests (CPU and GPU): the geometries the rule was worked out
on, and a stand-in "network" that is mirror-equivariant exactly, so that un-mirroring its output on
the mirrored tiles must reproduce, bit for bit, its output on the plain tiles."""
import numpy as np

from bioengine_worker_amd.cellpose import reference as ref

#: (H, W, bsize) -> padded size, tile starts along y, along x
GEOMETRIES = {
    (70, 90, 32): ((96, 112), [0, 12, 25, 38, 51, 64], [0, 13, 26, 40, 53, 66, 80]),
    (20, 100, 64): ((48, 128), [0, 0], [0, 21, 42, 64]),
    (16, 16, 32): ((32, 32), [0, 0], [0, 0]),
    (300, 260, 224): ((320, 288), [0, 48, 96], [0, 32, 64]),
}


def padded(img: np.ndarray) -> np.ndarray:
    """img [C, H, W] -> zero-padded as the tiling pads it (multiple of 16 plus the 8-pixel margin)."""
    return np.pad(img, ((0, 0), ref.pad_amounts(img.shape[1]), ref.pad_amounts(img.shape[2])))


def plain_tiles(imgp: np.ndarray, ys, xs, bsize: int) -> np.ndarray:
    """Un-mirrored bsize x bsize tiles at the given starts of the canvas (end-padded to bsize)."""
    C, Ly, Lx = imgp.shape
    canvas = np.zeros((C, max(Ly, bsize), max(Lx, bsize)), imgp.dtype)
    canvas[:, :Ly, :Lx] = imgp
    return np.stack([canvas[:, y: y + bsize, x: x + bsize] for y in ys for x in xs])


def standin_net(tiles: np.ndarray) -> np.ndarray:
    """tiles [nt, C, by, bx] -> [nt, 3, by, bx]: channel 0 the central difference along y of the
    tile's first channel with zero padding (``t[y + 1] - t[y - 1]``), channel 1 the same along x,
    channel 2 the tile itself.  Mirroring an axis of the input mirrors the output and negates the
    difference along that axis, exactly (``a - b == -(b - a)`` in floating point)."""
    t = np.asarray(tiles)[:, 0]
    p = np.pad(t, ((0, 0), (1, 1), (1, 1)))
    return np.stack([p[:, 2:, 1:-1] - p[:, :-2, 1:-1], p[:, 1:-1, 2:] - p[:, 1:-1, :-2], t], 1)
