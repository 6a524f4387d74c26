"""CPU oracle of the Cellpose mask-recovery algorithm (numpy / torch-CPU).

Re-derived from the Cellpose algorithm (cellpose 3.x ``dynamics.compute_masks``, EXT — the
reference reaches it through ``model.eval(..., niter, flow_threshold, cellprob_threshold)`` in
``apps/cellpose-finetuning/main.py:3559-3567,4998-5027`` and the model-runner cellpose pin,
SURVEY.md §2.5 K2-K7).  The HIP kernels in ``csrc/kernels/cellpose_*.hip`` implement the same
semantics; this module is what their tests compare against.

Stages
------
normalize99      per-channel 1st/99th percentile scaling (linear-interpolated percentiles)
normalize_img    the options of cellpose's ``normalize`` dict (written from memory of cellpose 3's
                 ``transforms.normalize_img`` / ``normalize99_tile``; not compared with the library):
                 other percentiles, fixed ``lowhigh`` bounds, ``invert`` (1 - x), and tile normalisation:
                 tile_norm_raw_maps (percentiles of blocks overlapping by ~20 %) -> tile_norm_fill
                 (degenerate blocks take the nearest valid block) -> tile_norm_smooth (Gaussian, sigma 1)
                 -> normalize99_tile (maps enlarged bilinearly, (x - X01) / (X99 - X01) per pixel)
make_tiles       224x224 tiles with 10 % overlap over an image padded to a multiple of 16 (+8 margin)
average_tiles    tapered-mask weighted blend of tile outputs
augment          test-time augmentation (cellpose ``augment=True``, written from memory of cellpose 3's
                 ``make_tiles`` / ``unaugment_tiles``; not compared with the library):
                 tile_starts_augment / make_tiles(augment=True): bsize x bsize tiles overlapping by half,
                 tile (j, i) of the grid mirrored in y when i is odd and in x when j is odd;
                 unaugment_tiles: outputs mirrored back, dY / dX negated along a mirrored axis; then
                 average_tiles as usual
follow_flows     niter Euler steps along dP (bilinear, grid_sample align_corners=False semantics)
get_masks        histogram of end points -> 5x5 max seeds (count > 10) -> 5x 3x3 dilation in 11x11
                 windows over histogram support (> 2) -> per-pixel label, drop masks > 40 % of image
masks_to_flows   per-mask heat diffusion from the median-nearest pixel, gradient of log(1 + T)
flow QC          mean squared error between mask flows and dP/5 per mask; drop masks above threshold
fill_holes       drop masks smaller than min_size, fill holes, renumber
stitch3d         z-stacks: join the masks of adjacent planes by exact mutual-best IoU into 3-D labels
do_3D            volumes: combine_views3d (YX + ZX + ZY network outputs -> dZ, dY, dX, cellprob),
                 follow_flows3d / get_masks3d / fill_holes_and_remove_small_masks3d: the 2-D stages
                 with one more axis (trilinear sampling, 5x5x5 seeds, 11x11x11 windows, no flow QC)
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage

# ------------------------------------------------------------------ normalization / tiling


def normalize99(img: np.ndarray, lower: float = 1.0, upper: float = 99.0) -> np.ndarray:
    """img [C, H, W] -> float32, each channel mapped so its p1 -> 0 and p99 -> 1."""
    out = np.zeros(img.shape, np.float32)
    for c in range(img.shape[0]):
        x = img[c].astype(np.float32)
        lo, hi = np.percentile(x, lower), np.percentile(x, upper)
        if hi - lo > 1e-3:
            out[c] = (x - lo) / (hi - lo)
        else:
            out[c] = 0.0 if np.ptp(x) == 0 else x - lo
    return out


def pad_amounts(L: int, div: int = 16, extra: int = 1) -> tuple[int, int]:
    lpad = int(div * math.ceil(L / div) - L)
    a = extra * div // 2 + lpad // 2
    b = extra * div // 2 + lpad - lpad // 2
    return a, b


def tile_starts(L: int, bsize: int = 224, overlap: float = 0.1) -> list[int]:
    overlap = min(0.5, max(0.05, overlap))
    b = min(bsize, L)
    n = 1 if L <= bsize else int(math.ceil((1.0 + 2 * overlap) * L / bsize))
    return [int(v) for v in np.linspace(0, L - b, n).astype(int)]


def tile_norm_blocks(L: int, blocksize: int) -> tuple[list[int], int]:
    """Blocks of the tile normalisation along one axis: ``(starts, b)``, by the rule of
    ``tile_starts(L, blocksize, 0.1)`` (blocks of ``b = min(blocksize, L)`` overlapping by ~20 %)."""
    return tile_starts(int(L), int(blocksize), 0.1), min(int(blocksize), int(L))


def tile_norm_raw_maps(img: np.ndarray, blocksize: int, lower: float = 1.0, upper: float = 99.0, dtype=np.float32):
    """Per-block percentiles of ``img`` [C, H, W]: ``(x01, x99)``, each [C, ny, nx] float32
    (``np.percentile`` with linear interpolation on the block's pixels as float32).  ``dtype``
    (here and in the stages below): float64 runs the same rules in double precision, the yardstick
    the tests measure the float32 rounding of these stages with."""
    C, H, W = img.shape
    ys, bh = tile_norm_blocks(H, blocksize)
    xs, bw = tile_norm_blocks(W, blocksize)
    x01 = np.zeros((C, len(ys), len(xs)), dtype)
    x99 = np.zeros_like(x01)
    for c in range(C):
        for j, y0 in enumerate(ys):
            for i, x0 in enumerate(xs):
                blk = img[c, y0: y0 + bh, x0: x0 + bw].astype(dtype)
                x01[c, j, i], x99[c, j, i] = np.percentile(blk, lower), np.percentile(blk, upper)
    return x01, x99


def tile_norm_fill(x01: np.ndarray, x99: np.ndarray):
    """Degenerate blocks (``x99 - x01 < 1e-3``) take both values of the nearest non-degenerate block
    of their channel (squared distance in grid indices, the raster-first block on ties, as ``argmin``
    gives); a channel without any valid block gets ``x01 = 0``, ``x99 = 1``.  Returns copies."""
    x01, x99 = np.array(x01, copy=True), np.array(x99, copy=True)
    C, ny, nx = x01.shape
    gy, gx = np.mgrid[0:ny, 0:nx]
    for c in range(C):
        bad = (x99[c] - x01[c]) < np.asarray(1e-3, x01.dtype)
        if bad.all():
            x01[c], x99[c] = 0.0, 1.0
            continue
        vy, vx = gy[~bad], gx[~bad]  # raster order
        for j, i in zip(gy[bad], gx[bad]):
            k = int(np.argmin((vy - j) ** 2 + (vx - i) ** 2))
            x01[c, j, i], x99[c, j, i] = x01[c, vy[k], vx[k]], x99[c, vy[k], vx[k]]
    return x01, x99


def tile_norm_smooth(m: np.ndarray) -> np.ndarray:
    """Gaussian (sigma 1, scipy's reflect boundary and truncate 4: nine taps) along the grid's y
    axis, then along its x axis; the result keeps ``m``'s dtype."""
    return ndimage.gaussian_filter1d(ndimage.gaussian_filter1d(m, 1.0, axis=-2), 1.0, axis=-1)


def tile_norm_maps(img: np.ndarray, blocksize: int, lower: float = 1.0, upper: float = 99.0, dtype=np.float32):
    """Local percentile maps of ``img`` [C, H, W] (cellpose ``tile_norm_blocksize``): block
    percentiles -> degenerate-block fill -> smoothing.  ``(x01, x99)``, each [C, ny, nx] float32.
    Written from memory of cellpose 3's ``normalize99_tile``; not compared with the library."""
    x01, x99 = tile_norm_fill(*tile_norm_raw_maps(img, blocksize, lower, upper, dtype))
    return tile_norm_smooth(x01), tile_norm_smooth(x99)


def _map_axis(n: int, L: int, dtype=np.float32):
    """Bilinear source coordinates of an ``n``-cell map axis enlarged to ``L``: half-pixel centres,
    clamped (``F.interpolate(align_corners=False)``): cells ``i0``, ``i1`` and the weight of ``i1``."""
    s = (np.arange(L, dtype=dtype) + dtype(0.5)) * dtype(n / L) - dtype(0.5)
    s = np.clip(s, dtype(0), dtype(n - 1))
    i0 = s.astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), (s - i0.astype(dtype)).astype(dtype)


def enlarge_map(m: np.ndarray, H: int, W: int) -> np.ndarray:
    """[C, ny, nx] -> [C, H, W] bilinearly (:func:`_map_axis` along x, then along y), in ``m``'s dtype."""
    dt = m.dtype.type
    y0, y1, wy = _map_axis(m.shape[1], H, dt)
    x0, x1, wx = _map_axis(m.shape[2], W, dt)
    rows = m[:, :, x0] + wx * (m[:, :, x1] - m[:, :, x0])  # [C, ny, W]
    top, bot = rows[:, y0], rows[:, y1]
    return top + wy[None, :, None] * (bot - top)


def normalize99_tile(img: np.ndarray, blocksize: int, lower: float = 1.0, upper: float = 99.0, dtype=np.float32) -> np.ndarray:
    """img [C, H, W] -> float32, every pixel scaled between the local percentile maps of
    :func:`tile_norm_maps` enlarged to the image: ``(x - X01) / (X99 - X01)``.  The fill and the
    positive smoothing weights keep the denominator at about 1e-3 or more wherever a channel has a
    valid block; it is 1 where it has none."""
    C, H, W = img.shape
    x01, x99 = tile_norm_maps(img, blocksize, lower, upper, dtype)
    X01, X99 = enlarge_map(x01, H, W), enlarge_map(x99, H, W)
    return ((img.astype(dtype) - X01) / (X99 - X01)).astype(dtype)


def normalize_img(img: np.ndarray, params) -> np.ndarray:
    """img [C, H, W] -> float32 under the normalisation options ``params`` (a
    :class:`~bioengine_worker_amd.cellpose.pipeline.NormParams`; cellpose ``transforms.normalize_img``,
    written from memory of cellpose 3 and not compared with the library): fixed ``lowhigh`` bounds
    per channel, or tile normalisation, or :func:`normalize99` between the ``lower`` / ``upper``
    percentiles; ``invert`` maps the result to ``1 - x``.  ``normalize=False`` converts only."""
    x = np.asarray(img)
    if not params.normalize:
        return x.astype(np.float32)
    if params.lowhigh is not None:
        lh = params.lowhigh
        pairs = [lh] * x.shape[0] if np.isscalar(lh[0]) else list(lh)
        if len(pairs) < x.shape[0]:
            raise ValueError(f"lowhigh has {len(pairs)} pairs for {x.shape[0]} channels")
        out = np.stack([(x[c].astype(np.float32) - np.float32(lo)) / (np.float32(hi) - np.float32(lo))
                        for c, (lo, hi) in zip(range(x.shape[0]), pairs)])
    elif params.tile_blocksize > 0:
        out = normalize99_tile(x, params.tile_blocksize, params.lower, params.upper)
    else:
        out = normalize99(x, params.lower, params.upper)
    return (1.0 - out).astype(np.float32) if params.invert else out.astype(np.float32)


def taper_mask(ly: int = 224, lx: int = 224, sig: float = 7.5) -> np.ndarray:
    bsize = max(224, max(ly, lx))
    xm = np.arange(bsize)
    xm = np.abs(xm - xm.mean())
    mask = 1 / (1 + np.exp((xm - (bsize / 2 - 20)) / sig))
    mask = mask * mask[:, np.newaxis]
    return mask[bsize // 2 - ly // 2: bsize // 2 - ly // 2 + ly, bsize // 2 - lx // 2: bsize // 2 - lx // 2 + lx].astype(np.float32)


def tile_starts_augment(L: int, bsize: int = 224) -> list[int]:
    """Tile starts along one padded axis under ``augment``: the axis counts as ``L' = max(L, bsize)``
    long, ``n = max(2, ceil(2 L' / bsize))`` tiles of ``bsize`` overlap by about half, at
    ``linspace(0, L' - bsize, n)`` truncated.  Equal starts are kept (an axis of at most ``bsize``
    gives ``[0, 0]``: the same window twice, once of them mirrored)."""
    Lc = max(int(L), int(bsize))
    n = max(2, -(-2 * Lc // int(bsize)))
    return [int(v) for v in np.linspace(0, Lc - bsize, n).astype(int)]


def make_tiles(img: np.ndarray, bsize: int = 224, overlap: float = 0.1, augment: bool = False):
    """img [C, Ly, Lx] (already padded) -> tiles [nt, C, by, bx], ystart, xstart.

    ``augment`` (test-time augmentation; ``overlap`` is ignored): returns ``(tiles [nt, C, bsize,
    bsize], ystart, xstart, Lyc, Lxc)``.  An axis shorter than ``bsize`` is zero-padded at its end to
    ``bsize`` (the canvas ``Lyc x Lxc``), the starts are :func:`tile_starts_augment`, and the tile
    of grid row ``j``, grid column ``i`` (index ``j * len(xstart) + i``) has its rows reversed when
    ``i`` is odd and its columns reversed when ``j`` is odd."""
    C, Ly, Lx = img.shape
    if augment:
        Lyc, Lxc = max(Ly, bsize), max(Lx, bsize)
        canvas = np.zeros((C, Lyc, Lxc), img.dtype)
        canvas[:, :Ly, :Lx] = img
        ys, xs = tile_starts_augment(Ly, bsize), tile_starts_augment(Lx, bsize)
        tiles = []
        for j, y in enumerate(ys):
            for i, x in enumerate(xs):
                t = canvas[:, y: y + bsize, x: x + bsize]
                if i % 2:
                    t = t[:, ::-1]
                if j % 2:
                    t = t[:, :, ::-1]
                tiles.append(t)
        return np.stack(tiles), ys, xs, Lyc, Lxc
    ys, xs = tile_starts(Ly, bsize, overlap), tile_starts(Lx, bsize, overlap)
    by, bx = min(bsize, Ly), min(bsize, Lx)
    tiles = np.stack([img[:, y: y + by, x: x + bx] for y in ys for x in xs])
    return tiles, ys, xs


def scaled_size(L: int, r) -> int:
    """Length of an axis of ``L`` pixels rescaled by ``r`` (``None``: not rescaled), never below 8."""
    return int(L) if r is None else max(8, int(round(L * r)))


def _fma(a, b, c, dtype):
    """``a * b + c`` with one rounding for float32 (through float64, where the product is exact), as the
    kernels' ``fmaf`` and the fused multiply-adds of torch's CPU kernel; plain arithmetic otherwise."""
    if dtype is np.float32:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def _resize_axis(n_in: int, n_out: int, dtype):
    """Taps ``i0``, ``i1`` and the weight of ``i1`` for every output index of one axis: half-pixel
    centres, the source coordinate clamped at 0, the upper neighbour clamped at the edge."""
    ratio = dtype(n_in) / dtype(n_out)
    s = _fma(ratio, np.arange(n_out).astype(dtype) + dtype(0.5), dtype(-0.5), dtype)
    s = np.maximum(s, dtype(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (s - i0.astype(dtype)).astype(dtype)


def resize_bilinear_ref(img: np.ndarray, size, dtype=np.float32) -> np.ndarray:
    """img [..., H, W] -> [..., oh, ow] by the bilinear rule of the resize kernels (no antialiasing),
    coordinates, weights and the lerp ``ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)`` all
    in ``dtype``.  float64 is the yardstick of the float32 kernels.  With float32 the coordinate and
    the first product of each sum are fused multiply-adds, as in ``be_tiles_gather_scaled``.  That
    gives the taps and weights of ``F.interpolate(mode="bilinear", align_corners=False)`` on the CPU
    exactly, and its values bit for bit at many sizes; at others torch's CPU kernel, whose sums the
    compiler fuses as it sees fit, differs in the last bit or two."""
    dtype = np.dtype(dtype).type
    x = np.asarray(img).astype(dtype)
    oh, ow = int(size[0]), int(size[1])
    y0, y1, ly1 = _resize_axis(x.shape[-2], oh, dtype)
    x0, x1, lx1 = _resize_axis(x.shape[-1], ow, dtype)
    ly1 = ly1[:, None]
    ly0, lx0 = dtype(1) - ly1, dtype(1) - lx1
    top, bot = x[..., y0, :], x[..., y1, :]
    t = _fma(lx0, top[..., x0], lx1 * top[..., x1], dtype)
    b = _fma(lx0, bot[..., x0], lx1 * bot[..., x1], dtype)
    return _fma(ly0, t, ly1 * b, dtype)


def scaled_tiles(img: np.ndarray, r, bsize: int = 224, overlap: float = 0.1, augment: bool = False, dtype=np.float32):
    """The tiles the network sees of image ``img`` [C, H, W] rescaled by ``r`` (``None``: as it is):
    :func:`resize_bilinear_ref` to ``scaled_size`` of both axes, zero padding by :func:`pad_amounts`,
    then :func:`make_tiles`.  Returns what :func:`make_tiles` returns."""
    C, H, W = img.shape
    Hs, Ws = scaled_size(H, r), scaled_size(W, r)
    x = np.asarray(img).astype(dtype) if (Hs, Ws) == (H, W) else resize_bilinear_ref(img, (Hs, Ws), dtype)
    ya, yb = pad_amounts(Hs)
    xa, xb = pad_amounts(Ws)
    return make_tiles(np.pad(x, ((0, 0), (ya, yb), (xa, xb))), bsize, overlap, augment=augment)


def unaugment_tiles(y: np.ndarray, ys, xs) -> np.ndarray:
    """Network outputs ``y`` [nt, nout >= 3, by, bx] (dY, dX, cellprob, ...) of the tiles of
    ``make_tiles(..., augment=True)`` -> the same outputs mirrored back (a new array): tile
    ``(j, i)`` gets its rows reversed and channel 0 negated when ``i`` is odd, its columns reversed
    and channel 1 negated when ``j`` is odd; the other channels keep their sign."""
    y = np.asarray(y)
    nx = len(xs)
    if y.ndim != 4 or y.shape[0] != len(ys) * nx or y.shape[1] < 3:
        raise ValueError(f"unaugment_tiles expects [{len(ys) * nx}, nout >= 3, by, bx] tile outputs, got shape {y.shape}")
    out = y.copy()
    for j in range(len(ys)):
        for i in range(nx):
            k = j * nx + i
            t = y[k]
            if i % 2:
                t = t[:, ::-1]
            if j % 2:
                t = t[:, :, ::-1]
            out[k] = t
            if i % 2:
                out[k, 0] = -out[k, 0]
            if j % 2:
                out[k, 1] = -out[k, 1]
    return out


def average_tiles(y: np.ndarray, ys, xs, Ly: int, Lx: int, dtype=np.float32) -> np.ndarray:
    """y [nt, nout, by, bx] -> [nout, Ly, Lx] tapered weighted average, accumulated in ``dtype``
    (float64: the yardstick of the float32 blends; the taper itself stays the float32 mask)."""
    nt, nout, by, bx = y.shape
    acc = np.zeros((nout, Ly, Lx), dtype)
    nrm = np.zeros((Ly, Lx), dtype)
    mask = taper_mask(by, bx).astype(dtype)
    k = 0
    for yy in ys:
        for xx in xs:
            acc[:, yy: yy + by, xx: xx + bx] += y[k] * mask
            nrm[yy: yy + by, xx: xx + bx] += mask
            k += 1
    return acc / nrm


# ------------------------------------------------------------------ dynamics


def follow_flows(dP: np.ndarray, cellprob: np.ndarray, cellprob_threshold: float = 0.0, niter: int = 200):
    """Returns (p_final [2, npts] float32 (y, x), inds (y, x) arrays).  A 2-D image needs two rows
    and two columns (the sample position is ``p * L / (L - 1) - 0.5``): ``ValueError`` otherwise."""
    Ly, Lx = cellprob.shape
    if Ly < 2 or Lx < 2:
        raise ValueError(f"2-D dynamics need at least two rows and two columns, got an image of {Ly} x {Lx}")
    fg = cellprob > cellprob_threshold
    inds = np.nonzero(fg)
    flow = torch.from_numpy((dP * fg / 5.0).astype(np.float32))
    p = torch.from_numpy(np.stack(inds).astype(np.float32))  # [2, n] (y, x)
    if p.shape[1] == 0:
        return p.numpy(), inds
    # grid_sample with align_corners=False at normalised coords 2p/(L-1)-1 samples pixel
    # position p*L/(L-1) - 0.5; each step adds the sampled flow in pixel units, clamped to [0, L-1].
    im = flow[[1, 0]].unsqueeze(0)  # (x, y) channel order as grid_sample expects
    pt = torch.zeros(1, 1, p.shape[1], 2)
    for t in range(niter):
        pt[0, 0, :, 0] = 2 * p[1] / (Lx - 1) - 1
        pt[0, 0, :, 1] = 2 * p[0] / (Ly - 1) - 1
        d = F.grid_sample(im, pt, align_corners=False)[0, :, 0, :]  # [2 (x,y), n]
        p[1] = torch.clamp(p[1] + d[0], 0, Lx - 1)
        p[0] = torch.clamp(p[0] + d[1], 0, Ly - 1)
    return p.numpy(), inds


def get_masks(p: np.ndarray, inds, shape, rpad: int = 20, max_size_fraction: float = 0.4) -> np.ndarray:
    Ly, Lx = shape
    M0 = np.zeros(shape, np.int32)
    if p.shape[1] == 0:
        return M0
    pt = p.astype(np.int64) + rpad  # truncation (p >= 0)
    pt[0] = np.clip(pt[0], 0, Ly + rpad - 1)
    pt[1] = np.clip(pt[1], 0, Lx + rpad - 1)
    hs = (Ly + 2 * rpad, Lx + 2 * rpad)
    h1 = np.zeros(hs, np.int32)
    np.add.at(h1, (pt[0], pt[1]), 1)
    hmax = ndimage.maximum_filter(h1, size=5, mode="constant", cval=0)
    seeds = np.argwhere((h1 >= hmax) & (h1 > 10))
    if len(seeds) == 0:
        return M0
    npts = h1[seeds[:, 0], seeds[:, 1]]
    lin = seeds[:, 0] * hs[1] + seeds[:, 1]
    order = np.lexsort((lin, npts))  # ascending count, ties by raster index
    seeds = seeds[order]
    M1 = np.zeros(hs, np.int32)
    for k, (sy, sx) in enumerate(seeds):
        win = h1[sy - 5: sy + 6, sx - 5: sx + 6] > 2
        sm = np.zeros((11, 11), bool)
        sm[5, 5] = True
        for _ in range(5):
            sm = ndimage.binary_dilation(sm, structure=np.ones((3, 3), bool)) & win
        yy, xx = np.nonzero(sm)
        M1[yy + sy - 5, xx + sx - 5] = k + 1
    M0[inds] = M1[pt[0], pt[1]]
    # remove big masks, renumber
    big = Ly * Lx * max_size_fraction
    labels, counts = np.unique(M0, return_counts=True)
    for lab, c in zip(labels, counts):
        if lab != 0 and c > big:
            M0[M0 == lab] = 0
    return renumber(M0)


def renumber(M: np.ndarray) -> np.ndarray:
    labs = np.unique(M)
    labs = labs[labs != 0]
    lut = np.zeros(int(M.max()) + 1 if M.size else 1, np.int32)
    lut[labs] = np.arange(1, len(labs) + 1)
    return lut[M]


def mask_centers(masks: np.ndarray) -> np.ndarray:
    """Per-mask pixel nearest the (y, x) median, padded coordinates (+1).  [nmask, 2]"""
    n = int(masks.max())
    centers = np.zeros((n, 2), np.int64)
    for i, sl in enumerate(ndimage.find_objects(masks)):
        if sl is None:
            continue
        yi, xi = np.nonzero(masks[sl] == i + 1)
        ymed, xmed = np.median(yi), np.median(xi)
        imin = np.argmin((xi - xmed) ** 2 + (yi - ymed) ** 2)
        centers[i] = (yi[imin] + sl[0].start + 1, xi[imin] + sl[1].start + 1)
    return centers


def masks_to_flows(masks: np.ndarray, niter: int | None = None) -> np.ndarray:
    """Unit flow field [2, Ly, Lx] (dy, dx) from heat diffusion inside each mask."""
    Ly, Lx = masks.shape
    mu0 = np.zeros((2, Ly, Lx), np.float32)
    if masks.max() == 0:
        return mu0
    mp = np.pad(masks, 1)
    slices = ndimage.find_objects(masks)
    ext = [(sl[0].stop - sl[0].start + 1) + (sl[1].stop - sl[1].start + 1) for sl in slices if sl is not None]
    n_iter = 2 * max(ext) if niter is None else niter
    centers = mask_centers(masks)
    y, x = np.nonzero(mp)
    dy9 = np.array([0, -1, 1, 0, 0, -1, -1, 1, 1])
    dx9 = np.array([0, 0, 0, -1, 1, -1, 1, -1, 1])
    ny = y[None, :] + dy9[:, None]
    nx = x[None, :] + dx9[:, None]
    isn = mp[ny, nx] == mp[y, x][None, :]
    T = np.zeros(mp.shape, np.float64)
    valid = centers[:, 0] > 0
    cy, cx = centers[valid, 0], centers[valid, 1]
    for _ in range(n_iter):
        T[cy, cx] += 1
        Tn = T[ny, nx] * isn
        T[y, x] = Tn.mean(axis=0)
    T = np.log(1.0 + T)
    dy = T[y + 1, x] - T[y - 1, x]
    dx = T[y, x + 1] - T[y, x - 1]
    mu = np.stack([dy, dx])
    mu /= 1e-60 + np.sqrt((mu ** 2).sum(0))
    mu0[:, y - 1, x - 1] = mu
    return mu0


def flow_errors(masks: np.ndarray, dP: np.ndarray) -> np.ndarray:
    mu = masks_to_flows(masks)
    n = int(masks.max())
    err = np.zeros(n, np.float64)
    for c in range(2):
        err += ndimage.mean((mu[c] - dP[c] / 5.0) ** 2, masks, index=np.arange(1, n + 1))
    return err


def remove_bad_flow_masks(masks: np.ndarray, dP: np.ndarray, threshold: float = 0.4) -> np.ndarray:
    err = flow_errors(masks, dP)
    bad = 1 + np.nonzero(err > threshold)[0]
    out = masks.copy()
    out[np.isin(out, bad)] = 0
    return out


def fill_holes_and_remove_small_masks(masks: np.ndarray, min_size: int = 15) -> np.ndarray:
    out = np.zeros_like(masks)
    j = 0
    for i, sl in enumerate(ndimage.find_objects(masks)):
        if sl is None:
            continue
        msk = masks[sl] == i + 1
        npix = msk.sum()
        if min_size > 0 and npix < min_size:
            continue
        if npix > 0:
            filled = ndimage.binary_fill_holes(msk)
            # hole pixels are claimed only where no other mask lives (order-independent form)
            claim = filled & ((masks[sl] == 0) | msk)
            out[sl][claim] = j + 1
            j += 1
    return out


def compute_masks(dP, cellprob, niter=200, cellprob_threshold=0.0, flow_threshold=0.4, min_size=15,
                  max_size_fraction=0.4) -> np.ndarray:
    p, inds = follow_flows(dP, cellprob, cellprob_threshold, niter)
    mask = get_masks(p, inds, cellprob.shape, max_size_fraction=max_size_fraction)
    if mask.max() > 0 and flow_threshold is not None and flow_threshold > 0:
        mask = remove_bad_flow_masks(mask, dP, flow_threshold)
    return fill_holes_and_remove_small_masks(mask, min_size)


# ------------------------------------------------------------------ z-stacks: stitch 2-D masks into 3-D labels


def stitch3d(masks: np.ndarray, stitch_threshold: float = 0.25, min_size: int = 0) -> np.ndarray:
    """Join per-plane label images ``masks`` [Z, H, W] (0 = background, labels of different planes
    unrelated, gaps allowed) into volumetric labels, int32 [Z, H, W] numbered ``1..K``.

    For adjacent planes ``z-1``, ``z``: ``ov(b, a)`` common pixels of label ``b`` (plane ``z``) and
    ``a`` (plane ``z-1``), ``u = A[b] + A_prev[a] - ov``, IoU the rational ``ov / u``.

    * candidate: ``ov > 0`` and ``float64(ov) >= float64(stitch_threshold) * float64(u)`` (equality links);
    * owner: every ``a`` is owned by its candidate ``b`` of largest IoU, ratios compared exactly by
      integer cross-multiplication, the smaller ``b`` on equal ratios;
    * link: every ``b`` links to the ``a`` it owns of largest IoU, the smaller ``a`` on equal ratios;
      a ``b`` that owns nothing starts a new instance;
    * global ids in order of plane, then ascending local label: a linked label takes its link's id,
      any other label with pixels the next unused id;
    * ``min_size > 0`` drops instances of fewer voxels over the whole stack;
    * the result is numbered ``1..K`` in order of first appearance (plane, then local label).

    This is the mutual-best rule of cellpose's ``utils.stitch3D`` (threshold, best row per column,
    argmax per row) with two deliberate departures: on an exact IoU tie the library lets two masks
    take one id, here the smaller label wins and the other starts a new instance; and across empty
    leading planes the library can hand out ids that are already taken, here an unlinked label
    always gets a fresh id."""
    M = np.asarray(masks)
    if M.ndim != 3:
        raise ValueError(f"stitch3d expects [Z, H, W] masks, got shape {M.shape}")
    Z = M.shape[0]
    thr = float(stitch_threshold)
    planes = []  # per plane: (labels ascending, dense index image, areas)
    gids: list[np.ndarray] = []
    vol = [0]  # voxels per global id (index 0 unused)
    for z in range(Z):
        cur = M[z].ravel()
        labs, inv = np.unique(cur, return_inverse=True)
        inv = inv.ravel()
        area = np.bincount(inv, minlength=labs.size)
        fg = labs > 0
        link = {}
        if z > 0 and fg.any():
            plabs, pinv, parea, pgid = planes[-1]
            both = (cur > 0) & (M[z - 1].ravel() > 0)
            if both.any():
                pk, ov = np.unique(inv[both].astype(np.int64) * plabs.size + pinv[both], return_counts=True)
                best_a: dict = {}  # a -> (ov, u, b): the owner so far
                cand = []
                for k, o in zip(pk.tolist(), ov.tolist()):
                    bi, ai = divmod(k, plabs.size)
                    u = int(area[bi]) + int(parea[ai]) - o
                    if not (o > 0 and float(o) >= thr * float(u)):
                        continue
                    cand.append((bi, ai, o, u))
                    cur_best = best_a.get(ai)
                    # pairs come in ascending b, so a strict improvement keeps the smaller b on ties
                    if cur_best is None or o * cur_best[1] > cur_best[0] * u:
                        best_a[ai] = (o, u, bi)
                best_b: dict = {}  # b -> (ov, u, a)
                for bi, ai, o, u in cand:  # ascending (b, a): strict improvement keeps the smaller a
                    if best_a[ai][2] != bi:
                        continue
                    cur_best = best_b.get(bi)
                    if cur_best is None or o * cur_best[1] > cur_best[0] * u:
                        best_b[bi] = (o, u, ai)
                link = {bi: v[2] for bi, v in best_b.items()}
        gid = np.zeros(labs.size, np.int64)
        for bi in range(labs.size):
            if not fg[bi]:
                continue
            if bi in link:
                gid[bi] = planes[-1][3][link[bi]]
            else:
                gid[bi] = len(vol)
                vol.append(0)
            vol[gid[bi]] += int(area[bi])
        planes.append((labs, inv, area, gid))
        gids.append(gid[inv].reshape(M.shape[1:]))
    volume = np.asarray(vol, np.int64)
    keep = volume > 0
    if min_size > 0:
        keep &= volume >= int(min_size)
    lut = (np.cumsum(keep) * keep).astype(np.int32)
    if Z == 0:
        return np.zeros(M.shape, np.int32)
    return lut[np.stack(gids)]


# ------------------------------------------------------------------ do_3D: orthogonal views + 3-D dynamics
#
# The 2-D stages above with one more axis, after cellpose 3.x ``_run_3D`` / ``dynamics.compute_masks``
# with ``do_3D=True``.  cellpose is not installed where this was written, so nothing below could be
# compared with the library: the semantics are the ones spelled out in the docstrings.


def combine_views3d(y_yx: np.ndarray, y_zx: np.ndarray, y_zy: np.ndarray):
    """Network outputs of the three orthogonal plane families of one volume -> ``(dP [3, Z, H, W]
    (dZ, dY, dX), cellprob [Z, H, W])`` float32.

    ``y_yx`` [Z, 3, H, W] (one plane per z), ``y_zx`` [H, 3, Z, W] (one per y), ``y_zy`` [W, 3, Z, H]
    (one per x); each view's channels are (flow along the plane's rows, flow along its columns,
    cellprob).  ``dZ = zx[0] + zy[0]``, ``dY = yx[0] + zy[1]``, ``dX = yx[1] + zx[1]``, ``cellprob =
    (yx[2] + zx[2]) + zy[2]``: sums, not means, as cellpose 3.x ``_run_3D`` adds them (not compared
    with the library, see above).  The order of the float additions is part of the definition."""
    yx = np.asarray(y_yx, np.float32).transpose(1, 0, 2, 3)  # [3, Z, H, W]
    zx = np.asarray(y_zx, np.float32).transpose(1, 2, 0, 3)  # [3, Z, H, W] from [H, 3, Z, W]
    zy = np.asarray(y_zy, np.float32).transpose(1, 2, 3, 0)  # [3, Z, H, W] from [W, 3, Z, H]
    dP = np.stack([zx[0] + zy[0], yx[0] + zy[1], yx[1] + zx[1]])
    cellprob = (yx[2] + zx[2]) + zy[2]
    return np.ascontiguousarray(dP), np.ascontiguousarray(cellprob)


def follow_flows3d(dP: np.ndarray, cellprob: np.ndarray, cellprob_threshold: float = 0.0, niter: int = 200):
    """:func:`follow_flows` with one more axis.  ``dP`` [3, Z, H, W] (dZ, dY, dX); returns
    ``(p_final [3, npts] float32 (z, y, x), inds (z, y, x) arrays)``.

    ``niter`` Euler steps of ``dP * fg / 5`` sampled trilinearly with 5-D ``grid_sample(
    align_corners=False)`` semantics: the sample position along an axis of length ``L`` is
    ``p * L / (L - 1) - 0.5`` (an axis of length 1 samples its only plane with weight 1), zeros
    outside the volume; positions are clamped to ``[0, L - 1]`` per axis after every step.  Not
    compared with cellpose (see above)."""
    fg = cellprob > cellprob_threshold
    inds = np.nonzero(fg)
    Lz, Ly, Lx = cellprob.shape
    flow = torch.from_numpy((dP * fg / 5.0).astype(np.float32))
    p = torch.from_numpy(np.stack(inds).astype(np.float32))  # [3, n] (z, y, x)
    n = p.shape[1]
    if n == 0:
        return p.numpy(), inds
    im = flow[[2, 1, 0]].unsqueeze(0)  # (x, y, z) channel order as grid_sample expects
    pt = torch.zeros(1, 1, 1, n, 3)
    L = (Lx, Ly, Lz)
    for t in range(niter):
        for a in range(3):  # grid axis a (x, y, z) is position row 2 - a
            pt[0, 0, 0, :, a] = 2 * p[2 - a] / (L[a] - 1) - 1 if L[a] > 1 else 0.0
        d = F.grid_sample(im, pt, align_corners=False)[0, :, 0, 0, :]  # [3 (x, y, z), n]
        for a in range(3):
            p[2 - a] = torch.clamp(p[2 - a] + d[a], 0, L[a] - 1)
    return p.numpy(), inds


def end_bins3d(p: np.ndarray, shape, rpad: int = 20) -> np.ndarray:
    """Truncated end points ``p`` [3, n] -> their (z, y, x) bins [3, n] int64 in the volume padded by
    ``rpad`` on every side (clipped to ``[0, L + rpad - 1]`` per axis)."""
    pt = p.astype(np.int64) + rpad  # truncation (p >= 0)
    for a in range(3):
        pt[a] = np.clip(pt[a], 0, shape[a] + rpad - 1)
    return pt


def get_masks3d(p: np.ndarray, inds, shape, rpad: int = 20, max_size_fraction: float = 0.4) -> np.ndarray:
    """:func:`get_masks` with one more axis: histogram of the end points in the padded volume, seeds
    where ``h > 10`` and ``h >=`` its 5x5x5 maximum (zero outside) ordered by ascending count (ties by
    raster index), per seed five 3x3x3 dilations from the centre of its 11x11x11 window and-ed with
    ``h > 2`` (later seeds overwrite earlier ones), every voxel labelled by its end point's bin,
    labels of more than ``max_size_fraction`` of the voxels dropped, renumbered.  Not compared with
    cellpose (see above)."""
    Lz, Ly, Lx = shape
    M0 = np.zeros(shape, np.int32)
    if p.shape[1] == 0:
        return M0
    pt = end_bins3d(p, shape, rpad)
    hs = (Lz + 2 * rpad, Ly + 2 * rpad, Lx + 2 * rpad)
    h1 = np.zeros(hs, np.int32)
    np.add.at(h1, (pt[0], pt[1], pt[2]), 1)
    hmax = ndimage.maximum_filter(h1, size=5, mode="constant", cval=0)
    seeds = np.argwhere((h1 >= hmax) & (h1 > 10))
    if len(seeds) == 0:
        return M0
    npts = h1[seeds[:, 0], seeds[:, 1], seeds[:, 2]]
    lin = (seeds[:, 0] * hs[1] + seeds[:, 1]) * hs[2] + seeds[:, 2]
    order = np.lexsort((lin, npts))  # ascending count, ties by raster index
    seeds = seeds[order]
    M1 = np.zeros(hs, np.int32)
    struct = np.ones((3, 3, 3), bool)
    for k, (sz, sy, sx) in enumerate(seeds):
        win = h1[sz - 5: sz + 6, sy - 5: sy + 6, sx - 5: sx + 6] > 2
        sm = np.zeros((11, 11, 11), bool)
        sm[5, 5, 5] = True
        for _ in range(5):
            sm = ndimage.binary_dilation(sm, structure=struct) & win
        zz, yy, xx = np.nonzero(sm)
        M1[zz + sz - 5, yy + sy - 5, xx + sx - 5] = k + 1
    M0[inds] = M1[pt[0], pt[1], pt[2]]
    big = Lz * Ly * Lx * max_size_fraction
    labels, counts = np.unique(M0, return_counts=True)
    for lab, c in zip(labels, counts):
        if lab != 0 and c > big:
            M0[M0 == lab] = 0
    return renumber(M0)


def fill_holes_and_remove_small_masks3d(masks: np.ndarray, min_size: int = 15) -> np.ndarray:
    """Volumetric labels [Z, H, W] -> holes filled plane by plane in z (the 2-D rule of
    :func:`fill_holes_and_remove_small_masks`: a hole voxel is claimed only where no other mask
    lives; where two masks claim one background voxel the larger id takes it), then instances of
    fewer than ``min_size`` voxels over the whole volume (counted after the fill) dropped and the
    rest numbered ``1..K`` in id order.  A cavity that no single plane closes stays open.  Not
    compared with cellpose (see above)."""
    masks = np.asarray(masks)
    out = np.zeros(masks.shape, np.int32)
    for z in range(masks.shape[0]):
        pl = masks[z]
        for i, sl in enumerate(ndimage.find_objects(pl)):
            if sl is None:
                continue
            msk = pl[sl] == i + 1
            filled = ndimage.binary_fill_holes(msk)
            claim = filled & ((pl[sl] == 0) | msk)
            out[z][sl][claim] = i + 1
    counts = np.bincount(out.ravel(), minlength=1)
    keep = counts > 0
    if min_size > 0:
        keep &= counts >= min_size
    keep[0] = False
    lut = (np.cumsum(keep) * keep).astype(np.int32)
    return lut[out]


def compute_masks3d(dP, cellprob, niter=200, cellprob_threshold=0.0, min_size=15, max_size_fraction=0.4) -> np.ndarray:
    """3-D mask recovery: :func:`follow_flows3d` -> :func:`get_masks3d` ->
    :func:`fill_holes_and_remove_small_masks3d`.  No flow QC: cellpose documents ``flow_threshold``
    as unused in 3-D."""
    p, inds = follow_flows3d(dP, cellprob, cellprob_threshold, niter)
    mask = get_masks3d(p, inds, cellprob.shape, max_size_fraction=max_size_fraction)
    return fill_holes_and_remove_small_masks3d(mask, min_size)


# ------------------------------------------------------------------ per-label measurements


def measure_masks(masks, image=None, outlines: bool = False) -> dict:
    """Raw per-label measurements of a label image: the specification of
    ``csrc/kernels/cellpose_measure.hip``, which the GPU tests compare with exactly.  (cellpose and
    scikit-image are not installed: the rules below are this project's own.)

    ``masks``: [H, W] or [Z, H, W] integer labels (0 = background); ``image``: [C, H, W] or
    [C, Z, H, W] float32 intensities on the same grid, or None.  ``K = masks.max()``; every array
    has one row per label ``1..K`` (row ``l - 1`` is label ``l``) and a label without pixels has
    zeros everywhere.  Coordinates are array indices.

    ``area``                        int64    pixels (voxels) of the label
    ``sum_y``, ``sum_x``            int64    coordinate sums (3-D: also ``sum_z``)
    ``sum_yy``, ``sum_xx``, ``sum_xy``  int64    second coordinate sums, 2-D only
    ``bbox``                        int32    half-open box: ``(y0, x0, y1, x1)`` in 2-D,
                                             ``(z0, y0, x0, z1, y1, x1)`` in 3-D
    ``boundary``                    int64    pixels of the label with at least one 4-neighbour
                                             (6-neighbour in 3-D) that lies outside the array or
                                             carries a different label (background included)
    ``int_sum``, ``int_sumsq``      float64  [K, C]: sum of ``x`` and of ``x * x`` over the label,
                                             both taken in float64 (the square of a float32 is exact)
    ``int_min``, ``int_max``        float32  [K, C], exact

    The intensity fields exist only with an ``image``.  ``outlines=True`` adds ``outlines``: a bool
    array of the masks' shape, true at exactly the pixels that ``boundary`` counts."""
    m = np.asarray(masks)
    if m.ndim not in (2, 3):
        raise ValueError(f"measure_masks expects [H, W] or [Z, H, W] labels, got shape {m.shape}")
    m = m.astype(np.int64)
    nd = m.ndim
    K = max(int(m.max()), 0) if m.size else 0
    # boundary pixels: compare with each axis neighbour; outside the array counts as different
    pad = np.pad(m, 1, constant_values=-1)
    edge = np.zeros(m.shape, bool)
    for ax in range(nd):
        for start in (0, 2):
            sl = [slice(1, -1)] * nd
            sl[ax] = slice(start, start + m.shape[ax])
            edge |= pad[tuple(sl)] != m
    edge &= m > 0
    idx = np.nonzero(m > 0)
    row = m[idx] - 1

    def total(values, dtype=np.int64):
        out = np.zeros(K, dtype)
        np.add.at(out, row, np.asarray(values, dtype))
        return out

    raw = {"area": total(np.ones(row.shape, np.int64))}
    names = ("z", "y", "x")[3 - nd:]
    for name, c in zip(names, idx):
        raw["sum_" + name] = total(c)
    if nd == 2:
        y, x = idx
        raw["sum_yy"], raw["sum_xx"], raw["sum_xy"] = total(y * y), total(x * x), total(x * y)
    present = raw["area"] > 0
    lo = np.full((K, nd), np.iinfo(np.int64).max)
    hi = np.full((K, nd), -1)
    for d, c in enumerate(idx):
        np.minimum.at(lo[:, d], row, c)
        np.maximum.at(hi[:, d], row, c)
    raw["bbox"] = np.where(present[:, None], np.concatenate([lo, hi + 1], 1), 0).astype(np.int32)
    raw["boundary"] = total(edge[idx])
    if image is not None:
        img = np.asarray(image)
        if img.ndim != nd + 1 or img.shape[1:] != m.shape:
            raise ValueError(f"measure_masks: image {img.shape} does not match masks {m.shape} (channels first)")
        img = img.astype(np.float32)
        C = img.shape[0]
        raw["int_sum"], raw["int_sumsq"] = np.zeros((K, C)), np.zeros((K, C))
        raw["int_min"], raw["int_max"] = np.zeros((K, C), np.float32), np.zeros((K, C), np.float32)
        for c in range(C):
            v = img[c][idx]
            v64 = v.astype(np.float64)
            raw["int_sum"][:, c] = total(v64, np.float64)
            raw["int_sumsq"][:, c] = total(v64 * v64, np.float64)
            mn, mx = np.full(K, np.inf, np.float32), np.full(K, -np.inf, np.float32)
            np.minimum.at(mn, row, v)
            np.maximum.at(mx, row, v)
            raw["int_min"][:, c] = np.where(present, mn, 0)
            raw["int_max"][:, c] = np.where(present, mx, 0)
    if outlines:
        raw["outlines"] = edge
    return raw


def derive_measurements(raw: dict) -> dict:
    """Raw fields of :func:`measure_masks` (one image) -> the measurement table.  The only place
    where derived values are computed: the CPU and the GPU path both end here.  All in float64;
    a label without pixels has zeros everywhere.

    ``label`` ``1..K``; ``area``, ``bbox``, ``boundary`` (and ``int_min``, ``int_max``, and
    ``outlines`` when present) are passed through.  ``centroid`` [K, 2] (y, x) or [K, 3] (z, y, x)
    ``= sum / area``; ``equivalent_diameter = sqrt(4 area / pi)`` in 2-D, ``cbrt(6 area / pi)`` in
    3-D.  2-D only, from the central moments ``myy = sum_yy / area - cy^2`` (``mxx``, ``mxy``
    likewise) and the eigenvalues ``l1 >= l2 >= 0`` (clamped at 0) of ``[[myy, mxy], [mxy, mxx]]``:
    ``axis_major = 4 sqrt(l1)``, ``axis_minor = 4 sqrt(l2)``, ``eccentricity = sqrt(1 - l2 / l1)``
    (0 when ``l1 = 0``), ``orientation = 0.5 atan2(2 mxy, mxx - myy)``.  With intensities:
    ``int_mean = int_sum / area``, ``int_std = sqrt(max(int_sumsq / area - int_mean^2, 0))``.
    Image level: ``n_cells`` = labels with ``area > 0``; ``diameter_px`` = the median over those
    labels of ``sqrt(area)``, times ``2 / sqrt(pi)`` (0.0 without labels) -- the definition
    cellpose's ``utils.diameters`` uses, i.e. the value its ``diameter`` argument expects."""
    area_i = np.asarray(raw["area"]).astype(np.int64)
    K = area_i.shape[0]
    present = area_i > 0
    area = area_i.astype(np.float64)
    a = np.where(present, area, 1.0)
    vol = "sum_z" in raw
    out = {"label": np.arange(1, K + 1, dtype=np.int32), "area": area_i, "bbox": np.asarray(raw["bbox"]),
           "boundary": np.asarray(raw["boundary"]).astype(np.int64)}
    names = ("z", "y", "x") if vol else ("y", "x")
    cen = [np.asarray(raw["sum_" + n]).astype(np.float64) / a for n in names]
    out["centroid"] = np.stack(cen, 1) if K else np.zeros((0, len(names)))
    if vol:
        out["equivalent_diameter"] = np.cbrt(6.0 * area / np.pi)
    else:
        out["equivalent_diameter"] = np.sqrt(4.0 * area / np.pi)
        cy, cx = cen
        myy = np.asarray(raw["sum_yy"]).astype(np.float64) / a - cy * cy
        mxx = np.asarray(raw["sum_xx"]).astype(np.float64) / a - cx * cx
        mxy = np.asarray(raw["sum_xy"]).astype(np.float64) / a - cx * cy
        half = 0.5 * (myy + mxx)
        root = np.sqrt((0.5 * (myy - mxx)) ** 2 + mxy * mxy)
        l1, l2 = np.maximum(half + root, 0.0), np.maximum(half - root, 0.0)
        out["axis_major"], out["axis_minor"] = 4.0 * np.sqrt(l1), 4.0 * np.sqrt(l2)
        out["eccentricity"] = np.where(l1 > 0, np.sqrt(np.maximum(1.0 - l2 / np.where(l1 > 0, l1, 1.0), 0.0)), 0.0)
        out["orientation"] = np.where(present, 0.5 * np.arctan2(2.0 * mxy, mxx - myy), 0.0)
    if "int_sum" in raw:
        mean = np.asarray(raw["int_sum"], np.float64) / a[:, None]
        out["int_mean"] = mean
        out["int_std"] = np.sqrt(np.maximum(np.asarray(raw["int_sumsq"], np.float64) / a[:, None] - mean * mean, 0.0))
        out["int_min"], out["int_max"] = np.asarray(raw["int_min"]), np.asarray(raw["int_max"])
    if "outlines" in raw:
        out["outlines"] = np.asarray(raw["outlines"])
    out["n_cells"] = int(present.sum())
    out["diameter_px"] = float(np.median(np.sqrt(area[present])) * 2.0 / np.sqrt(np.pi)) if present.any() else 0.0
    return out


# ------------------------------------------------------------------ outlines: polygon rings

#: direction codes of the crack-following tracer: 0 = +x (top edge), 1 = +y (right edge),
#: 2 = -x (bottom edge), 3 = -y (left edge); (dy, dx) per code.  Turning right is ``d + 1``, left ``d - 1``.
_RING_DIRS = ((0, 1), (1, 0), (0, -1), (-1, 0))
#: tail vertex of a pixel's edge, relative to the pixel, per direction
_RING_TAIL = ((0, 0), (0, 1), (1, 1), (1, 0))


def _empty_rings() -> dict:
    return {"verts": np.zeros((0, 2), np.int32), "ring_offsets": np.zeros(1, np.int64),
            "ring_label": np.zeros(0, np.int32), "ring_area2": np.zeros(0, np.int64)}


def mask_rings(masks) -> dict:
    """Outlines of a label image as closed rings of pixel-corner coordinates: the specification of
    ``csrc/kernels/cellpose_rings.hip``, which the GPU tests compare with exactly.  (cellpose's
    ``utils.outlines_list``, OpenCV and scikit-image are not installed and not compared against: the
    rules below are this project's own.)

    ``masks``: [H, W] integer labels (0 = background; negative values are background too).  The
    outline of a label is the exact boundary of its pixel set (crack following), not a chain of
    pixel centres, so the polygon *is* the mask: :func:`rings_to_labels` inverts it.

    Directed edges.  A pixel ``(y, x)`` of label ``l`` owns one unit edge per side whose 4-neighbour
    lies outside the array or carries another label.  Edges run clockwise on screen (x right, y
    down), the label on the right hand: top ``+x`` from ``(y, x)``, right ``+y`` from ``(y, x+1)``,
    bottom ``-x`` from ``(y+1, x+1)``, left ``-y`` from ``(y+1, x)``.

    Successor.  At the head of an edge of pixel ``P`` with direction ``d``, with ``A = P + d`` and
    ``B = A + left(d)``: if ``A`` is not ``l`` turn right and stay on ``P``; else if ``B`` is ``l``
    turn left onto ``B``; else go straight onto ``A``.  ``A`` is tested first, so labels are
    4-connected: pixels that touch only diagonally are separate rings, and a ring may pass through
    one corner twice (a saddle whose two pixels are joined elsewhere).

    Rings.  Only turn vertices are kept (the tail of every edge whose predecessor has another
    direction).  A ring starts at the tail of its raster-first top edge; the rings of an image are
    ordered by label, then by the raster position of that edge.  ``area2 = sum(x_i * y_{i+1} -
    x_{i+1} * y_i)`` in int64: positive for outer rings, negative for holes, and a label's rings sum
    to twice its area.

    Returns ``verts`` int32 [V, 2] as (y, x), ``ring_offsets`` int64 [R + 1], ``ring_label`` int32
    [R] and ``ring_area2`` int64 [R]."""
    m = np.asarray(masks)
    if m.ndim != 2:
        raise ValueError(f"mask_rings expects [H, W] labels, got shape {m.shape}")
    H, W = m.shape
    P = np.zeros((H + 2, W + 2), np.int64)
    P[1:-1, 1:-1] = m
    P[P < 0] = 0
    top = (P[1:-1, 1:-1] > 0) & (P[1:-1, 1:-1] != P[:-2, 1:-1])
    ys, xs = np.nonzero(top)
    if ys.size == 0:
        return _empty_rings()
    seen = np.zeros((H, W), bool)
    Pl = P.tolist()  # plain ints: the walk is a Python loop
    rings = []  # (label, start raster index, vertices, area2)
    for y0, x0 in zip(ys.tolist(), xs.tolist()):
        if seen[y0, x0]:
            continue
        lab = Pl[y0 + 1][x0 + 1]
        py, px, d = y0, x0, 0
        verts = [(y0, x0)]
        while True:
            if d == 0:
                seen[py, px] = True
            dy, dx = _RING_DIRS[d]
            ay, ax = py + dy, px + dx
            nd = d
            if Pl[ay + 1][ax + 1] != lab:
                nd = (d + 1) & 3
            else:
                ly, lx = _RING_DIRS[(d + 3) & 3]
                if Pl[ay + ly + 1][ax + lx + 1] == lab:
                    py, px, nd = ay + ly, ax + lx, (d + 3) & 3
                else:
                    py, px = ay, ax
            if (py, px, nd) == (y0, x0, 0):
                break
            if nd != d:
                ty, tx = _RING_TAIL[nd]
                verts.append((py + ty, px + tx))
            d = nd
        v = np.asarray(verts, np.int64)
        nxt = np.roll(v, -1, 0)
        rings.append((lab, y0 * W + x0, v, int((v[:, 1] * nxt[:, 0] - nxt[:, 1] * v[:, 0]).sum())))
    rings.sort(key=lambda r: (r[0], r[1]))
    return {"verts": np.concatenate([r[2] for r in rings]).astype(np.int32),
            "ring_offsets": np.concatenate([[0], np.cumsum([len(r[2]) for r in rings])]).astype(np.int64),
            "ring_label": np.asarray([r[0] for r in rings], np.int32),
            "ring_area2": np.asarray([r[3] for r in rings], np.int64)}


def ring_vertex_counts(masks) -> np.ndarray:
    """Turn vertices per label ``1..K`` of :func:`mask_rings`, int64 [K], counted locally: at each of
    the ``(H + 1)(W + 1)`` pixel corners a label with one or three members in the corner's 2 x 2
    block has one vertex there, with two diagonal members two, otherwise none.  This is what sizes
    every label's segment of ``verts`` on the GPU before anything is traced."""
    m = np.asarray(masks)
    H, W = m.shape
    K = max(int(m.max()), 0) if m.size else 0
    P = np.zeros((H + 2, W + 2), np.int64)
    P[1:-1, 1:-1] = m
    a, b, c, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    out = np.zeros(K + 1, np.int64)
    for q in (a, b, c, d):  # every member of the block votes for its own label
        n = (q == a).astype(np.int64) + (q == b) + (q == c) + (q == d)
        diag = (n == 2) & (((q == a) & (q == d)) | ((q == b) & (q == c)))
        # a label with n members in the block is seen n times: in sixths of a vertex, each sighting
        # adds 6 / n of the corner's count (1 vertex for n = 1 or 3, 2 for a diagonal pair)
        np.add.at(out, q[(n == 1) & (q > 0)], 6)
        np.add.at(out, q[(n == 3) & (q > 0)], 2)
        np.add.at(out, q[diag & (q > 0)], 6)
    return out[1:] // 6


def _ring_list(rings: dict):
    off = np.asarray(rings["ring_offsets"]).astype(np.int64)
    v = np.asarray(rings["verts"]).astype(np.int64).reshape(-1, 2)
    labs = np.asarray(rings["ring_label"]).astype(np.int64)
    if off.shape[0] != labs.shape[0] + 1 or (off.size and (off[0] != 0 or off[-1] != v.shape[0])):
        raise ValueError("rings: ring_offsets does not fit verts / ring_label")
    return [(int(labs[r]), v[off[r]:off[r + 1]]) for r in range(labs.shape[0])]


def rings_to_labels(rings: dict, shape) -> np.ndarray:
    """The exact inverse of :func:`mask_rings`: int32 labels of ``shape`` (H, W) from a rings dict, by
    a signed scanline over the vertical edges of each label's rings (an edge running ``-y`` opens the
    label at its column, one running ``+y`` closes it).  Raises ``ValueError`` when the rings of two
    labels cover one pixel, a winding other than 0 / 1 appears, or a vertex lies outside the shape."""
    H, W = int(shape[0]), int(shape[1])
    out = np.zeros((H, W), np.int32)
    by_label: dict = {}
    for lab, v in _ring_list(rings):
        if lab <= 0:
            raise ValueError(f"rings_to_labels: ring label {lab} is not positive")
        if v.shape[0] and (v.min() < 0 or v[:, 0].max() > H or v[:, 1].max() > W):
            raise ValueError(f"rings_to_labels: a vertex of label {lab} lies outside {H} x {W}")
        by_label.setdefault(lab, []).append(v)
    for lab in sorted(by_label):
        vs = by_label[lab]
        allv = np.concatenate(vs)
        y0, x0, y1, x1 = allv[:, 0].min(), allv[:, 1].min(), allv[:, 0].max(), allv[:, 1].max()
        D = np.zeros((y1 - y0, x1 - x0 + 1), np.int64)
        for v in vs:
            nxt = np.roll(v, -1, 0)
            for (ya, xa), (yb, xb) in zip(v.tolist(), nxt.tolist()):
                if xa != xb and ya != yb:
                    raise ValueError(f"rings_to_labels: label {lab} has an edge that is not axis-parallel")
                if ya < yb:
                    D[ya - y0:yb - y0, xa - x0] -= 1
                elif yb < ya:
                    D[yb - y0:ya - y0, xa - x0] += 1
        wind = np.cumsum(D, 1)[:, :-1]
        if wind.size and (wind.min() < 0 or wind.max() > 1 or D.sum(1).any()):
            raise ValueError(f"rings_to_labels: label {lab} has a winding other than 0 / 1")
        sub = out[y0:y1, x0:x1]
        inside = wind == 1
        if (sub[inside] != 0).any():
            raise ValueError(f"rings_to_labels: label {lab} covers a pixel of another label")
        sub[inside] = lab
    return out


def _ring_contains2(v: np.ndarray, py2: int, px2: int) -> bool:
    """Even-odd test of the point (py2 / 2, px2 / 2), both odd, against the closed ring ``v`` (y, x):
    crossings of the ray towards +x with the ring's vertical edges, in doubled integer coordinates."""
    nxt = np.roll(v, -1, 0)
    vert = v[:, 1] == nxt[:, 1]
    lo, hi = 2 * np.minimum(v[:, 0], nxt[:, 0]), 2 * np.maximum(v[:, 0], nxt[:, 0])
    return bool((vert & (2 * v[:, 1] > px2) & (lo < py2) & (py2 < hi)).sum() & 1)


def rings_to_geojson(rings: dict, z: int | None = None) -> dict:
    """A rings dict of :func:`mask_rings` as a GeoJSON ``FeatureCollection`` (plain Python values):
    one ``Feature`` per label with ``properties`` ``{label, area, n_rings}`` (plus ``z`` when given),
    geometry ``Polygon`` when the label has one outer ring and ``MultiPolygon`` otherwise.
    Coordinates are ``[x, y]`` pixel corners, every ring closed by repeating its first vertex.  A hole
    belongs to the outer ring of its label that contains it, to the one of smallest ``area2`` when
    several do; the test point is the centre of the hole pixel above the hole ring's first top edge
    (even-odd crossings in doubled integers, no floats).  The rings' orientation is already RFC
    7946's: exteriors counter-clockwise in the numeric (x, y) plane, holes clockwise.  (No GIS
    library is installed or compared against; the tests check the structure and the containment.)"""
    area2 = np.asarray(rings["ring_area2"]).astype(np.int64)
    by_label: dict = {}
    for r, (lab, v) in enumerate(_ring_list(rings)):
        by_label.setdefault(lab, []).append((int(area2[r]), v))
    feats = []
    for lab in sorted(by_label):
        rs = by_label[lab]
        outers = [(a, v, []) for a, v in rs if a > 0]
        for a, v in rs:
            if a > 0:
                continue
            py2, px2 = 2 * int(v[0, 0]) - 1, 2 * int(v[0, 1]) + 1
            inside = [o for o in outers if _ring_contains2(o[1], py2, px2)]
            if not inside:
                raise ValueError(f"rings_to_geojson: a hole of label {lab} lies in none of its outer rings")
            min(inside, key=lambda o: o[0])[2].append(v)
        polys = []
        for _, v, holes in outers:
            polys.append([[[int(x), int(y)] for y, x in np.concatenate([q, q[:1]]).tolist()] for q in [v] + holes])
        props = {"label": int(lab), "area": int(sum(a for a, _ in rs) // 2), "n_rings": len(rs)}
        if z is not None:
            props["z"] = int(z)
        geom = {"type": "Polygon", "coordinates": polys[0]} if len(polys) == 1 else \
            {"type": "MultiPolygon", "coordinates": polys}
        feats.append({"type": "Feature", "properties": props, "geometry": geom})
    return {"type": "FeatureCollection", "features": feats}


# ------------------------------------------------------------------ polygons -> labels

#: sub-pixel steps per pixel of the rasteriser's integer lattice
RASTER_SUBPIX = 256
#: quantised coordinates must lie in [RASTER_QMIN, RASTER_QMAX] (-32,768 to 65,536 px): differences
#: then stay below 2^25 and every product of the inside test below 2^50
RASTER_QMIN, RASTER_QMAX = -(2 ** 23), 2 ** 24


def quantize_verts(verts) -> np.ndarray:
    """Vertices (any integer or float dtype, pixel-corner units) on the rasteriser's lattice:
    ``floor(c * 256 + 0.5)`` in float64, as int64 of the same shape.  Raises ``ValueError`` on a
    non-finite coordinate and on one outside ``[-2^23, 2^24]`` after quantisation."""
    f = np.asarray(verts).astype(np.float64)
    if not np.isfinite(f).all():
        raise ValueError("quantize_verts: a coordinate is not finite")
    q = np.floor(f * RASTER_SUBPIX + 0.5)
    if q.size and (q.min() < RASTER_QMIN or q.max() > RASTER_QMAX):
        raise ValueError(f"quantize_verts: a coordinate lies outside [{RASTER_QMIN // RASTER_SUBPIX}, "
                         f"{RASTER_QMAX // RASTER_SUBPIX}] pixels")
    return q.astype(np.int64)


def polygon_arrays(polys: dict, what: str = "rasterize_rings"):
    """The checked arrays of a polygons dict: quantised ``verts`` int64 [V, 2], ``ring_offsets``
    int64 [R + 1] and ``ring_label`` int64 [R].  Raises ``ValueError`` when the offsets do not fit
    (the check of the rings dicts, plus: they must not decrease), a label is not positive or a
    coordinate cannot be quantised."""
    off = np.asarray(polys["ring_offsets"]).astype(np.int64).reshape(-1)
    v = np.asarray(polys["verts"])
    if v.dtype.kind not in "iuf":
        raise ValueError(f"{what}: verts must be integers or floats, got {v.dtype}")
    v = v.reshape(-1, 2)
    labs = np.asarray(polys["ring_label"]).astype(np.int64).reshape(-1)
    if off.shape[0] != labs.shape[0] + 1 or off[0] != 0 or off[-1] != v.shape[0] or (np.diff(off) < 0).any():
        raise ValueError(f"{what}: ring_offsets does not fit verts / ring_label")
    if labs.size and (labs.min() <= 0 or labs.max() >= 2 ** 31 - 1):
        raise ValueError(f"{what}: ring labels must be positive and below 2^31 - 1, got "
                         f"{int(labs.min())} .. {int(labs.max())}")
    return quantize_verts(v), off, labs


def _first_centre(lo: np.ndarray) -> np.ndarray:
    """The first pixel whose centre ``256 p + 128`` is at or beyond the lattice coordinate ``lo``."""
    return -((RASTER_SUBPIX // 2 - lo) // RASTER_SUBPIX)


def rasterize_rings(polys: dict, shape) -> np.ndarray:
    """Label image int32 ``shape`` (H, W) of a polygons dict: the specification of
    ``csrc/kernels/cellpose_raster.hip``, which the GPU tests compare with exactly.  (PIL's
    ``ImageDraw.polygon`` truncates vertices to integers and is no yardstick; no other rasteriser is
    installed.  The rule is this project's own.)

    Polygons dict: the rings dict of :func:`mask_rings` with the vertex dtype freed -- ``verts``
    [V, 2] (y, x) of any integer or float dtype in pixel-corner units (pixel ``(y, x)`` is the square
    ``[y, y + 1) x [x, x + 1)``, its centre ``(y + 0.5, x + 0.5)``), ``ring_offsets`` int64 [R + 1],
    ``ring_label`` int32 [R]; ``ring_area2`` is ignored.

    The rule is in integers only.  Vertices are quantised by :func:`quantize_verts` to 1/256 pixel.
    Pixel ``(y, x)`` has the centre ``C = (256 y + 128, 256 x + 128)``.  For a label, every directed
    edge ``(Y0, X0) -> (Y1, X1)`` between consecutive vertices of each of its rings (the closing edge
    included) *crosses* the pixel's row when ``(Y0 <= Cy) != (Y1 <= Cy)``, and a crossing edge
    *counts* when its crossing lies at or left of the centre: ``(Cy - Y0)(X1 - X0) <= (Cx - X0)(Y1 -
    Y0)`` if ``Y1 > Y0``, ``>=`` if ``Y1 < Y0``.  The pixel is inside the label when the number of
    counting edges is odd: even-odd over all the rings of a label, so holes work whatever their
    orientation, a self-intersecting ring follows even-odd, and two overlapping parts of one label
    cancel where they overlap.  Horizontal and zero-length edges never cross and a ring of fewer
    than three vertices cancels itself.  Ties are top-left: a centre on a left or top edge is
    inside, one on a right or bottom edge outside, so polygons that share an edge never both claim a
    pixel and never leave one out.  A pixel takes the largest label whose polygon contains its
    centre.  Vertices may lie outside the image; the result is the part inside ``H x W``.

    Raises ``ValueError`` when the offsets do not fit, a label is not positive or a coordinate is
    not finite or out of range."""
    H, W = int(shape[0]), int(shape[1])
    q, off, labs = polygon_arrays(polys)
    out = np.zeros((H, W), np.int32)
    n = np.diff(off)
    S = RASTER_SUBPIX
    for lab in np.unique(labs).tolist():
        rs = np.nonzero((labs == lab) & (n > 0))[0]
        if rs.size == 0:
            continue
        a = np.concatenate([q[off[r]:off[r + 1]] for r in rs])
        b = np.concatenate([np.roll(q[off[r]:off[r + 1]], -1, 0) for r in rs])
        # rows and columns whose centre lies inside the vertex range: a row outside it is crossed by
        # no edge, a column left of it has no crossing at or left of it, one right of it has all of
        # them, an even number
        y_lo, x_lo = np.maximum(_first_centre(a.min(0)), 0).tolist()
        y_hi, x_hi = np.minimum(_first_centre(a.max(0)) - 1, (H - 1, W - 1)).tolist()
        if y_lo > y_hi or x_lo > x_hi:
            continue
        cx = (np.arange(x_lo, x_hi + 1, dtype=np.int64) * S + S // 2)[None, :]
        par = np.zeros((y_hi - y_lo + 1, x_hi - x_lo + 1), bool)
        for (Y0, X0), (Y1, X1) in zip(a.tolist(), b.tolist()):
            if Y0 == Y1:
                continue
            # rows with min(Y0, Y1) <= Cy < max(Y0, Y1): exactly those the edge crosses
            r0 = max(int(_first_centre(np.int64(min(Y0, Y1)))), y_lo)
            r1 = min(int(_first_centre(np.int64(max(Y0, Y1)))) - 1, y_hi)
            if r0 > r1:
                continue
            cy = (np.arange(r0, r1 + 1, dtype=np.int64) * S + S // 2)[:, None]
            lhs, rhs = (cy - Y0) * (X1 - X0), (cx - X0) * (Y1 - Y0)
            par[r0 - y_lo:r1 - y_lo + 1] ^= (lhs <= rhs) if Y1 > Y0 else (lhs >= rhs)
        sub = out[y_lo:y_hi + 1, x_lo:x_hi + 1]
        sub[par] = np.maximum(sub[par], lab)
    return out


def _empty_polygons() -> dict:
    return {"verts": np.zeros((0, 2), np.float64), "ring_offsets": np.zeros(1, np.int64),
            "ring_label": np.zeros(0, np.int32)}


def _geojson_ring(ring, where: str) -> np.ndarray:
    try:
        v = np.asarray([[float(p[1]), float(p[0])] for p in ring], np.float64).reshape(-1, 2)
    except (TypeError, ValueError, IndexError, KeyError) as e:
        raise ValueError(f"outlines_to_rings: {where}: positions must be [x, y] or [x, y, z] numbers") from e
    if v.shape[0] > 1 and (v[0] == v[-1]).all():
        v = v[:-1]
    if v.shape[0] < 3:
        raise ValueError(f"outlines_to_rings: {where}: a ring needs at least three vertices")
    return v


def _geojson_features(doc):
    """The features of a GeoJSON document as (properties, geometry) pairs, or None when ``doc`` is
    not GeoJSON."""
    if isinstance(doc, dict):
        t = doc.get("type")
        if t == "FeatureCollection":
            feats = doc.get("features")
            if not isinstance(feats, (list, tuple)):
                raise ValueError("outlines_to_rings: a FeatureCollection needs a list of features")
            for i, f in enumerate(feats):
                if not isinstance(f, dict) or f.get("type") != "Feature":
                    raise ValueError(f"outlines_to_rings: feature {i} is not a GeoJSON Feature")
            return [(f.get("properties") or {}, f.get("geometry")) for f in feats]
        if t == "Feature":
            return [(doc.get("properties") or {}, doc.get("geometry"))]
        if isinstance(t, str):
            return [({}, doc)]
        return None
    if isinstance(doc, (list, tuple)) and doc and all(isinstance(f, dict) and f.get("type") == "Feature" for f in doc):
        return [(f.get("properties") or {}, f.get("geometry")) for f in doc]
    return None


def outlines_to_rings(doc) -> dict:
    """One image's polygon annotation in any accepted form -> a polygons dict (see
    :func:`rasterize_rings`).

    * A polygons dict (``verts``, ``ring_offsets``, ``ring_label``): validated and returned.
    * The app's ``"rings"`` form, a list of ``{label, rings: [[[x, y], ...], ...]}``: the inverse of
      the app's ``outline_items``.
    * GeoJSON: a ``FeatureCollection``, a list of ``Feature`` s, one ``Feature`` or a bare geometry.
      ``Polygon`` and ``MultiPolygon`` only; any other geometry type, a ``null`` geometry and
      ``GeometryCollection`` raise ``ValueError`` naming the feature's index.  Positions are
      ``[x, y]`` or ``[x, y, z]`` (the third value is ignored); a ring's closing vertex, equal to its
      first, is dropped, and a ring with fewer than three vertices after that is a ``ValueError``.
      Labels are ``properties.label`` when every feature has it (a positive integer below 2^31 - 1;
      the same label on several features means several parts of one label), the feature's position
      + 1 when none has it; a mixture is a ``ValueError``.

    ``verts`` comes back as float64 (y, x) for the two parsed forms."""
    if isinstance(doc, dict) and "verts" in doc:
        if "ring_offsets" not in doc or "ring_label" not in doc:
            raise ValueError("outlines_to_rings: a polygons dict needs verts, ring_offsets and ring_label")
        polygon_arrays(doc, "outlines_to_rings")
        return doc
    rings, labels = [], []
    if isinstance(doc, (list, tuple)) and (not doc or all(isinstance(it, dict) and "rings" in it for it in doc)):
        for i, it in enumerate(doc):
            if "label" not in it:
                raise ValueError(f"outlines_to_rings: item {i} has no label")
            for ring in it["rings"]:
                rings.append(_geojson_ring(ring, f"item {i}"))
                labels.append(it["label"])
    else:
        feats = _geojson_features(doc)
        if feats is None:
            raise ValueError("outlines_to_rings expects a polygons dict, a list of {label, rings} or GeoJSON, got "
                             f"{type(doc).__name__}")
        has = [isinstance(p, dict) and p.get("label") is not None for p, _ in feats]
        if any(has) and not all(has):
            raise ValueError("outlines_to_rings: some features have properties.label and some do not")
        for i, (props, geom) in enumerate(feats):
            t = geom.get("type") if isinstance(geom, dict) else None
            if t not in ("Polygon", "MultiPolygon"):
                raise ValueError(f"outlines_to_rings: feature {i}: geometry {t!r} is not a Polygon or MultiPolygon")
            coords = geom.get("coordinates")
            if not isinstance(coords, (list, tuple)):
                raise ValueError(f"outlines_to_rings: feature {i}: no coordinates")
            for poly in ([coords] if t == "Polygon" else coords):
                for ring in poly:
                    rings.append(_geojson_ring(ring, f"feature {i}"))
                    labels.append(props["label"] if has[i] else i + 1)
    labs = []
    for lab in labels:
        if isinstance(lab, bool) or not isinstance(lab, (int, np.integer, float)) or lab != int(lab) \
                or not 0 < int(lab) < 2 ** 31 - 1:
            raise ValueError(f"outlines_to_rings: label {lab!r} is not a positive integer below 2^31 - 1")
        labs.append(int(lab))
    if not rings:
        return _empty_polygons()
    verts = np.concatenate(rings)
    if not np.isfinite(verts).all():
        raise ValueError("outlines_to_rings: a coordinate is not finite")
    return {"verts": verts, "ring_offsets": np.concatenate([[0], np.cumsum([r.shape[0] for r in rings])]).astype(np.int64),
            "ring_label": np.asarray(labs, np.int32)}


def unwrap_outlines(doc):
    """The annotation document of one image or plane: the app wraps a plane's ``"rings"`` outlines as
    ``{z, outlines}``; everything else is returned as it is."""
    if isinstance(doc, dict) and "outlines" in doc and "verts" not in doc and "type" not in doc:
        return doc["outlines"]
    return doc


def is_outline_document(doc) -> bool:
    """Whether ``doc`` looks like a polygon annotation of one image (any form
    :func:`outlines_to_rings` accepts) and not like an array of labels."""
    doc = unwrap_outlines(doc)
    if isinstance(doc, dict):
        return "verts" in doc or isinstance(doc.get("type"), str)
    return isinstance(doc, (list, tuple)) and all(isinstance(it, dict) for it in doc)


# ------------------------------------------------------------------ label surfaces: quad meshes of a volume

# corner offsets (in the next two axes b, c of the cycle z -> y -> x -> z) of a quad on the high
# (s = 1) and the low (s = 0) side of its voxel: outward winding, see :func:`label_surface`
_QUAD_BC = {1: ((0, 0), (1, 0), (1, 1), (0, 1)), 0: ((0, 0), (0, 1), (1, 1), (1, 0))}


def _surface_result(corner, verts, vlab, quads, qlab, lverts, lquads, faces, voxels) -> dict:
    return {"corner": corner, "verts": verts, "vert_label": vlab, "quads": quads, "quad_label": qlab,
            "label_verts": lverts, "label_quads": lquads, "faces": faces, "voxels": voxels}


def _empty_surface(K: int) -> dict:
    return _surface_result(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32),
                           np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros(K + 1, np.int64),
                           np.zeros(K + 1, np.int64), np.zeros((K, 3), np.int64), np.zeros(K, np.int64))


def surface_net_offsets(inside: np.ndarray):
    """Naive surface nets at lattice corners.  ``inside`` bool [V, 8]: whether each of the 8 voxels
    around the corner (index ``4 dz + 2 dy + dx``, ``d = 0`` the voxel below the corner along that
    axis) carries the vertex's label.  Returns ``nsum`` int32 [V, 3], the per-axis sum over the
    crossing edges of the 2 x 2 x 2 block of voxel centres of the edge midpoint's offset from the
    corner in half-voxel units, and ``ncross`` int32 [V], the number of crossing edges."""
    ins = np.asarray(inside, bool).reshape(-1, 2, 2, 2)
    nsum = np.zeros((ins.shape[0], 3), np.int32)
    ncross = np.zeros(ins.shape[0], np.int32)
    for a in range(3):
        lo, hi = np.take(ins, 0, axis=1 + a), np.take(ins, 1, axis=1 + a)  # [V, 2, 2] over the other two axes
        cross = lo != hi
        ncross += cross.reshape(-1, 4).sum(1).astype(np.int32)
        others = [ax for ax in range(3) if ax != a]
        for j, ax in enumerate(others):
            sign = np.array([-1, 1], np.int32).reshape((1, 2, 1) if j == 0 else (1, 1, 2))
            nsum[:, ax] += (cross * sign).reshape(-1, 4).sum(1).astype(np.int32)
    return nsum, ncross


def label_surface(L, nlab: int | None = None) -> dict:
    """The surface of every label of a volume as an indexed quad mesh (numpy only; the oracle of
    :func:`gpu.label_surface_gpu`, which is compared with it exactly).

    ``L`` [Z, H, W] integer labels; everything outside the array counts as 0.  ``K = nlab - 1``
    (default ``L.max()``): labels outside ``1..K`` are never meshed but still bound their neighbours.
    Coordinates are ``(z, y, x)`` on the corner lattice ``[0..Z] x [0..H] x [0..W]``; voxel
    ``(z, y, x)`` spans the corners ``(z, y, x)..(z + 1, y + 1, x + 1)``.

    Quads.  A voxel of label ``l`` owns one quad per side whose 6-neighbour is outside the array or
    carries another value (two touching labels each get a quad on the shared face, with opposite
    winding).  A side is (axis ``a``: 0 = z, 1 = y, 2 = x; ``s``: 0 = low, 1 = high); with ``(b, c)``
    the next two axes in the cycle z -> y -> x -> z the quad lies in the plane ``a = v_a + s`` with
    corners at the ``(b, c)`` offsets (0,0),(1,0),(1,1),(0,1) for ``s = 1`` and (0,0),(0,1),(1,1),(1,0)
    for ``s = 0``.  With this winding the sum of ``det(p0,p1,p2) + det(p0,p2,p3)`` over a label's quads
    is ``+6 x`` its voxel count and the directed edges of a label cancel in pairs.  Quads are ordered
    by (label, voxel raster index, ``2a + s``).

    Vertices.  One per (label ``l``, corner) where ``l`` holds between 1 and 7 of the 8 voxels around
    the corner, ordered by (label, corner raster index over ``(Z+1, H+1, W+1)``).  Two voxels of one
    label that meet only at an edge or corner share the vertex there (non-manifold by design).

    Returns ``corner`` int32 [V, 3] (the lattice corner: this mesh is the voxel set exactly),
    ``verts`` float32 [V, 3] (naive surface nets: ``float32(float64(corner) + float64(nsum) /
    float64(2 ncross))``, see :func:`surface_net_offsets`), ``vert_label`` int32 [V], ``quads`` int32
    [F, 4], ``quad_label`` int32 [F], ``label_verts`` / ``label_quads`` int64 [K + 1] (label ``l`` owns
    ``[l - 1]:[l]``), ``faces`` int64 [K, 3] (quads per axis z, y, x) and ``voxels`` int64 [K], computed
    from the mesh as the sum over the x-axis quads of +-(x of the quad's plane), + for ``s = 1``."""
    L = np.asarray(L)
    if L.ndim != 3:
        raise ValueError(f"label_surface expects a [Z, H, W] label volume, got shape {L.shape}")
    if L.dtype.kind not in "iub":
        raise ValueError(f"label_surface expects integer labels, got dtype {L.dtype}")
    Z, H, W = L.shape
    if nlab is None:
        nlab = int(L.max(initial=0)) + 1
    K = max(int(nlab) - 1, 0)
    if L.size == 0 or K == 0:
        return _empty_surface(K)
    dt = np.int64 if L.dtype.itemsize > 4 or L.dtype == np.uint32 else np.int32
    P = np.zeros((Z + 2, H + 2, W + 2), dt)
    P[1:-1, 1:-1, 1:-1] = L
    C = P[1:-1, 1:-1, 1:-1]
    valid = (C >= 1) & (C <= K)
    shape = (Z, H, W)
    NC = (Z + 1) * (H + 1) * (W + 1)

    # quads: (label, voxel, side)
    parts = []
    for a in range(3):
        for s in range(2):
            sl = [slice(1, -1)] * 3
            sl[a] = slice(2, None) if s else slice(0, -2)
            vox = np.flatnonzero(valid & (P[tuple(sl)] != C))
            parts.append((vox, np.full(vox.shape[0], 2 * a + s, np.int64)))
    qvox = np.concatenate([p[0] for p in parts])
    qside = np.concatenate([p[1] for p in parts])
    qlab = C.reshape(-1)[qvox].astype(np.int64)
    order = np.lexsort((qside, qvox, qlab))
    qvox, qside, qlab = qvox[order], qside[order], qlab[order]

    # vertices: (label, corner) at the corners whose 8 voxels are not all equal
    views = [P[dz:dz + Z + 1, dy:dy + H + 1, dx:dx + W + 1] for dz in range(2) for dy in range(2) for dx in range(2)]
    mixed = np.zeros((Z + 1, H + 1, W + 1), bool)
    for v in views[1:]:
        mixed |= v != views[0]
    cidx = np.flatnonzero(mixed)
    around = np.stack([v[mixed] for v in views], 1).astype(np.int64)  # [n, 8]
    ok = (around >= 1) & (around <= K)
    keys = np.unique((around * NC + cidx[:, None])[ok])
    vlab, vcorner = keys // NC, keys % NC
    row = np.searchsorted(cidx, vcorner)
    inside = around[row] == vlab[:, None]
    nsum, ncross = surface_net_offsets(inside)
    corner = np.stack(np.unravel_index(vcorner, (Z + 1, H + 1, W + 1)), 1).astype(np.int32)
    verts = (corner.astype(np.float64) + nsum.astype(np.float64) / (2 * ncross).astype(np.float64)[:, None]).astype(np.float32)

    # quad corners -> vertex indices
    vz, vy, vx = np.unravel_index(qvox, shape)
    base = np.stack([vz, vy, vx], 1).astype(np.int64)
    qa, qs = qside // 2, qside % 2
    quads = np.zeros((qvox.shape[0], 4), np.int64)
    strides = np.array([(H + 1) * (W + 1), W + 1, 1], np.int64)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for s in range(2):
            sel = np.flatnonzero((qa == a) & (qs == s))
            for k, (ob, oc) in enumerate(_QUAD_BC[s]):
                p = base[sel].copy()
                p[:, a] += s
                p[:, b] += ob
                p[:, c] += oc
                key = qlab[sel] * NC + p @ strides
                idx = np.searchsorted(keys, key)
                if not np.array_equal(keys[np.minimum(idx, keys.shape[0] - 1)], key):
                    raise AssertionError("label_surface: a quad corner has no vertex")
                quads[sel, k] = idx
    lbl = np.arange(1, K + 2)
    lverts = np.concatenate([[0], np.searchsorted(vlab, lbl[:-1], side="right")]).astype(np.int64)
    lquads = np.concatenate([[0], np.searchsorted(qlab, lbl[:-1], side="right")]).astype(np.int64)
    faces = np.bincount((qlab - 1) * 3 + qa, minlength=3 * K).reshape(K, 3).astype(np.int64)
    xs = qa == 2
    plane = base[xs, 2] + qs[xs]
    voxels = np.zeros(K, np.int64)
    np.add.at(voxels, qlab[xs] - 1, np.where(qs[xs] == 1, plane, -plane))
    return _surface_result(corner, verts, vlab.astype(np.int32), quads.astype(np.int32), qlab.astype(np.int32), lverts,
                           lquads, faces, voxels)


def _check_spacing(spacing, what: str):
    try:
        sp = tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: spacing must be three positive finite numbers, got {spacing!r}") from None
    if len(sp) != 3 or not all(np.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"{what}: spacing must be three positive finite numbers, got {spacing!r}")
    return sp


def _quad_triangles(pts: np.ndarray, quads: np.ndarray):
    p = pts[quads]  # [F, 4, 3]
    return p[:, 0], p[:, 1], p[:, 2], p[:, 3]


def _segment_sums(values: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    return np.array([values[a:b].sum(dtype=np.float64) for a, b in zip(offsets[:-1], offsets[1:])], np.float64)


def surface_stats(surf: dict, spacing=(1.0, 1.0, 1.0)) -> dict:
    """Per-label surface measurements of a :func:`label_surface` mesh, float64, one row per label.

    ``area_voxel = fz sy sx + fy sz sx + fx sz sy`` from ``faces`` (the voxel-face area, about 1.5 x a
    smooth surface's); ``area``: the ``verts`` mesh scaled by ``spacing`` (sz, sy, sx), every quad as
    the triangles (p0, p1, p2) and (p0, p2, p3); ``mesh_volume``: the sum of ``det / 6`` over the same
    triangles; ``volume = voxels sz sy sx``; ``sphericity = pi^(1/3) (6 volume)^(2/3) / area`` (NaN
    where ``area == 0``); ``n_verts``; ``n_quads``."""
    sz, sy, sx = sp = _check_spacing(spacing, "surface_stats")
    faces = np.asarray(surf["faces"], np.float64).reshape(-1, 3)
    K = faces.shape[0]
    lq, lv = np.asarray(surf["label_quads"], np.int64), np.asarray(surf["label_verts"], np.int64)
    pts = np.asarray(surf["verts"], np.float64).reshape(-1, 3) * np.asarray(sp, np.float64)
    p0, p1, p2, p3 = _quad_triangles(pts, np.asarray(surf["quads"], np.int64).reshape(-1, 4))
    n1, n2 = np.cross(p1 - p0, p2 - p0), np.cross(p2 - p0, p3 - p0)
    qarea = 0.5 * np.sqrt((n1 * n1).sum(1)) + 0.5 * np.sqrt((n2 * n2).sum(1))
    qvol = ((p0 * n1).sum(1) + (p0 * n2).sum(1)) / 6.0  # det(p0, p1, p2) = p0 . ((p1 - p0) x (p2 - p0))
    area, mesh_volume = _segment_sums(qarea, lq), _segment_sums(qvol, lq)
    volume = np.asarray(surf["voxels"], np.float64).reshape(-1) * (sz * sy * sx)
    with np.errstate(divide="ignore", invalid="ignore"):
        sph = np.where(area > 0, np.pi ** (1.0 / 3.0) * (6.0 * volume) ** (2.0 / 3.0) / area, np.nan)
    return {"label": np.arange(1, K + 1, dtype=np.float64),
            "area_voxel": faces[:, 0] * sy * sx + faces[:, 1] * sz * sx + faces[:, 2] * sz * sy,
            "area": area, "mesh_volume": mesh_volume, "volume": volume, "sphericity": sph,
            "n_verts": np.diff(lv).astype(np.float64), "n_quads": np.diff(lq).astype(np.float64)}


def surface_to_obj(surf: dict, spacing=(1.0, 1.0, 1.0), labels=None, smooth: bool = True) -> str:
    """Wavefront OBJ text of a :func:`label_surface` mesh: one ``o label_<l>`` group per label (all
    with quads, or the given ``labels``), ``v x y z`` lines (the reverse of the stored order, scaled by
    ``spacing`` (sz, sy, sx), written with ``repr`` of the Python float; ``smooth=False`` writes the
    lattice corners instead of the surface-net vertices) and 1-based ``f`` lines with every quad's
    vertex order reversed, so that normals point outward in the ``(x, y, z)`` frame."""
    sz, sy, sx = _check_spacing(spacing, "surface_to_obj")
    lv, lq = np.asarray(surf["label_verts"], np.int64), np.asarray(surf["label_quads"], np.int64)
    K = lv.shape[0] - 1
    if labels is None:
        labels = [l for l in range(1, K + 1) if lq[l] > lq[l - 1]]
    labels = [int(l) for l in labels]
    if any(l < 1 or l > K for l in labels):
        raise ValueError(f"surface_to_obj: labels must lie in 1..{K}, got {labels}")
    pts = np.asarray(surf["verts" if smooth else "corner"]).astype(np.float64).reshape(-1, 3)
    quads = np.asarray(surf["quads"], np.int64).reshape(-1, 4)
    lines, base = [], 1
    for l in labels:
        v0, v1 = int(lv[l - 1]), int(lv[l])
        lines.append(f"o label_{l}")
        for z, y, x in pts[v0:v1].tolist():
            lines.append(f"v {x * sx!r} {y * sy!r} {z * sz!r}")
        for q in (quads[int(lq[l - 1]):int(lq[l])] - v0 + base).tolist():
            lines.append(f"f {q[3]} {q[2]} {q[1]} {q[0]}")
        base += v1 - v0
    return "\n".join(lines) + ("\n" if lines else "")
