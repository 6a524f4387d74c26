"""GPU (HIP) implementation of Cellpose pre/post-processing on batches of images.

Every heavy step is a kernel in ``csrc/kernels/{tiles,cellpose_dynamics,cellpose_dynamics3d,cellpose_masks,cellpose_stitch,cellpose_measure,cellpose_ap,cellpose_rings,cellpose_raster,label_surface}.hip``;
torch is only used for tiny bookkeeping (sorting the seed keys, prefix sums over labels, building
per-mask job lists).  The semantics are those of :mod:`bioengine_worker_amd.cellpose.reference`
(the CPU oracle), which the GPU tests compare against.
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
import enum
import math
import os

import numpy as np
import torch

from ..ops import _native
from . import reference as ref

RPAD = 20
LDS_DIFFUSE_BYTES = 156 * 1024  # one mask per CU up to ~95 x 95 boxes; larger ones run tiled
LDS_FILL_BYTES = 32 * 1024


# ------------------------------------------------------------------ percentiles / tiles


_pct_ws: dict = {}

#: element type codes of ``be_tiles_gather_norm`` (csrc/kernels/percentile.h)
RAW_DTYPES = {torch.float32: 0, torch.uint16: 1, torch.uint8: 2}

#: ``BE_CELLPOSE_FUSED_FRONT=0`` (A/B): convert to fp32, normalise into an fp32 image and gather
#: that, instead of the percentile select on the raw pixels + normalising gather
FUSED_FRONT = os.environ.get("BE_CELLPOSE_FUSED_FRONT", "1") != "0"


def _pct_workspace(device, sptr, rows: int) -> torch.Tensor:
    """The percentile kernels' workspace for ``rows`` rows on stream ``sptr``."""
    key = (device, getattr(sptr, "value", sptr))  # one workspace per stream: concurrent streams never share histograms
    ws = _pct_ws.get(key)
    need = rows * 6 * 258 * 4
    if ws is None or ws.numel() < need:  # hist part must start zeroed; every call leaves it zeroed
        ws = _pct_ws[key] = torch.zeros(max(need, 64 * 6 * 258 * 4), dtype=torch.uint8, device=device)
    return ws


def takes_fused_front(x) -> bool:
    """Whether ``x`` can go to :meth:`TilePlan.gather_normalized` as it is: a contiguous
    [B, C, H, W] device tensor of uint8, uint16 or float32."""
    return (FUSED_FRONT and torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in RAW_DTYPES
            and x.is_contiguous())


def normalize99(x: torch.Tensor, lower: float = 1.0, upper: float = 99.0) -> torch.Tensor:
    """x [B, C, H, W] -> float32 normalised per (image, channel) with np.percentile 'linear' semantics.

    On the GPU: radix-select HIP kernel (``csrc/kernels/percentile.hip``; six order statistics per
    row in four digit passes, no sort).  :func:`normalize99_sort` is the torch formulation it is
    tested against."""
    if x.device.type != "cuda":
        return normalize99_sort(x, lower, upper)
    B, C, H, W = x.shape
    xf = x.float().contiguous()
    rows = B * C
    sptr = _native.stream(x.device)
    ws = _pct_workspace(x.device, sptr, rows)
    out = torch.empty_like(xf)
    _native.call("be_pct_normalize", _native.ptr(xf), rows, H * W, float(lower), float(upper), _native.ptr(out),
                 _native.ptr(ws), ws.numel() // 4 * 4, sptr)
    return out


#: largest block grid (ny * nx) of the tile normalisation (csrc/kernels/percentile.h kMaxCells)
TILE_NORM_MAX_CELLS = 4096

#: small device constants of the options (block starts per image shape, ``lowhigh`` bounds), least
#: recently used first; both come from requests, so each cache holds at most ``_CONST_CACHE_MAX``
#: entries.  An evicted tensor lives on while something else refers to it: eager launches are ordered
#: on the stream that frees it, a captured graph holds :func:`norm_constants`.
_CONST_CACHE_MAX = 64
_tile_norm_grids: "collections.OrderedDict" = collections.OrderedDict()
_lowhigh_consts: "collections.OrderedDict" = collections.OrderedDict()


def _cached_const(cache, key, make):
    v = cache.get(key)
    if v is None:
        v = cache[key] = make()
        while len(cache) > _CONST_CACHE_MAX:
            cache.popitem(last=False)
    else:
        cache.move_to_end(key)
    return v


def _gauss9() -> list[float]:
    """Weights at distance 0..4 of scipy's ``gaussian_filter1d(sigma=1)`` kernel (truncate 4)."""
    w = np.exp(-0.5 * np.arange(-4, 5, dtype=np.float64) ** 2)
    w /= w.sum()
    return [float(v) for v in w[4:]]


def _tile_norm_grid(H: int, W: int, blocksize: int, device):
    """Block starts of the tile normalisation on ``device``: ``(ys_t, xs_t, ny, nx, bh, bw)``.  Raises
    ``ValueError`` before anything is launched when the grid has more cells than the maps kernel holds."""
    if int(blocksize) <= 0:
        raise ValueError(f"tile normalisation needs a positive blocksize, got {blocksize}")
    ys, bh = ref.tile_norm_blocks(H, blocksize)
    xs, bw = ref.tile_norm_blocks(W, blocksize)
    if len(ys) * len(xs) > TILE_NORM_MAX_CELLS:
        raise ValueError(f"tile_norm_blocksize={blocksize} on a {H} x {W} image gives a {len(ys)} x {len(xs)} block grid; "
                         f"at most {TILE_NORM_MAX_CELLS} blocks are supported")
    key = (H, W, int(blocksize), torch.device(device))
    return _cached_const(_tile_norm_grids, key, lambda: (torch.tensor(ys, dtype=torch.int32, device=device),
                                                         torch.tensor(xs, dtype=torch.int32, device=device),
                                                         len(ys), len(xs), bh, bw))


def _check_raw(x_raw: torch.Tensor, what: str) -> None:
    if x_raw.dim() != 4 or x_raw.dtype not in RAW_DTYPES or not x_raw.is_contiguous():
        raise ValueError(f"{what} takes a contiguous [B, C, H, W] uint8, uint16 or float32 tensor, got "
                         f"{x_raw.dtype} {tuple(x_raw.shape)}")


def tile_block_percentiles_gpu(x_raw: torch.Tensor, blocksize: int, lower: float = 1.0, upper: float = 99.0,
                               c_use: int | None = None):
    """Percentiles of the overlapping blocks (:func:`reference.tile_norm_raw_maps`) of the first
    ``c_use`` channels of raw ``x_raw`` [B, C, H, W]: ``(x01, x99)``, each [B, c_use, ny, nx] float32."""
    _check_raw(x_raw, "tile_block_percentiles_gpu")
    B, C, H, W = x_raw.shape
    c_use = C if c_use is None else min(int(c_use), C)
    ys_t, xs_t, ny, nx, bh, bw = _tile_norm_grid(H, W, blocksize, x_raw.device)
    lo = torch.empty(B, c_use, ny, nx, dtype=torch.float32, device=x_raw.device)
    hi = torch.empty_like(lo)
    _native.call("be_pct_block_select", _native.ptr(x_raw), RAW_DTYPES[x_raw.dtype], B, C, c_use, H, W, _native.ptr(ys_t),
                 _native.ptr(xs_t), ny, nx, bh, bw, float(lower), float(upper), _native.ptr(lo), _native.ptr(hi),
                 _native.stream(x_raw.device))
    return lo, hi


def tile_maps_fill_smooth_gpu(x01: torch.Tensor, x99: torch.Tensor):
    """Block percentiles [B, C, ny, nx] -> the maps the apply samples (:func:`reference.tile_norm_fill`,
    then :func:`reference.tile_norm_smooth`), in place; returns its arguments."""
    B, C, ny, nx = x01.shape
    if ny * nx > TILE_NORM_MAX_CELLS:
        raise ValueError(f"a {ny} x {nx} block grid has more than {TILE_NORM_MAX_CELLS} blocks")
    if not (x01.is_contiguous() and x99.is_contiguous() and x01.dtype == x99.dtype == torch.float32):
        raise ValueError("tile_maps_fill_smooth_gpu takes contiguous float32 maps")
    _native.call("be_pct_tile_maps", _native.ptr(x01), _native.ptr(x99), B * C, ny, nx, *_gauss9(), _native.stream(x01.device))
    return x01, x99


def tile_norm_maps_gpu(x_raw: torch.Tensor, blocksize: int, lower: float = 1.0, upper: float = 99.0,
                       c_use: int | None = None):
    """:func:`reference.tile_norm_maps` of every image of raw ``x_raw`` [B, C, H, W] (uint8, uint16
    or float32, first ``c_use`` channels): ``(x01, x99)``, each [B, c_use, ny, nx] float32.  Two
    launches (block select, fill + smoothing), no workspace and no host read."""
    return tile_maps_fill_smooth_gpu(*tile_block_percentiles_gpu(x_raw, blocksize, lower, upper, c_use))


def _lowhigh_tensor(lowhigh, c_use: int, device) -> torch.Tensor:
    """``NormParams.lowhigh`` as a [c_use, 2] float32 device tensor (one small upload per value)."""
    pairs = [lowhigh] * c_use if not isinstance(lowhigh[0], tuple) else list(lowhigh)
    if len(pairs) < c_use:
        raise ValueError(f"normalize: lowhigh has {len(pairs)} pairs for {c_use} channels")
    key = (tuple(pairs[:c_use]), torch.device(device))
    return _cached_const(_lowhigh_consts, key, lambda: torch.tensor(pairs[:c_use], dtype=torch.float32, device=device))


def norm_constants(params, C: int, H: int, W: int, device) -> tuple:
    """The cached device tensors that normalising [*, C, H, W] images by ``params`` reads (block
    starts of the tile normalisation, ``lowhigh`` bounds), the very objects the caches hold now.
    The caches evict; whoever records kernel arguments for later (a captured HIP graph) keeps this
    tuple alive next to the recording."""
    out = ()
    if params.normalize and params.tile_blocksize > 0:
        out += tuple(_tile_norm_grid(H, W, params.tile_blocksize, device)[:2])
    if params.normalize and params.lowhigh is not None:
        out += (_lowhigh_tensor(params.lowhigh, C, device),)
    return out


def _plain_percentile(params) -> bool:
    """Whether ``params`` is the percentile rule alone, which the entry points from before the
    options existed compute."""
    return params.lowhigh is None and not params.invert and params.tile_blocksize == 0


def normalize_img_gpu(x: torch.Tensor, params=None, c_use: int | None = None) -> torch.Tensor:
    """:func:`reference.normalize_img` of every image of ``x`` [B, C, H, W] on the GPU -> float32
    [B, c_use, H, W].  The default rule (and other percentiles alone) is :func:`normalize99`; fixed
    bounds, inversion and tile normalisation run the unfused kernels that share their per-pixel
    function with :meth:`TilePlan.gather_normalized`, so both give the same bits."""
    from .pipeline import NormParams

    params = NormParams() if params is None else params
    C = x.shape[1]
    c_use = C if c_use is None else min(int(c_use), C)
    if not params.normalize:
        return x[:, :c_use].float()
    if _plain_percentile(params):
        return normalize99(x[:, :c_use], params.lower, params.upper)
    if x.device.type != "cuda":
        return torch.stack([torch.from_numpy(ref.normalize_img(x[b, :c_use].numpy(), params)) for b in range(x.shape[0])])
    if x.dtype not in RAW_DTYPES:
        x = x.float()
    x = x.contiguous()
    B, C, H, W = x.shape
    out = torch.empty(B, c_use, H, W, dtype=torch.float32, device=x.device)
    sptr = _native.stream(x.device)
    if params.tile_blocksize > 0:
        lo, hi = tile_norm_maps_gpu(x, params.tile_blocksize, params.lower, params.upper, c_use)
        _native.call("be_pct_normalize_tile", _native.ptr(x), RAW_DTYPES[x.dtype], B, C, c_use, H, W, _native.ptr(lo),
                     _native.ptr(hi), lo.shape[2], lo.shape[3], int(params.invert), _native.ptr(out), sptr)
        return out
    lh = _lowhigh_tensor(params.lowhigh, c_use, x.device) if params.lowhigh is not None else None
    ws = _pct_workspace(x.device, sptr, B * c_use)
    _native.call("be_pct_normalize_ext", _native.ptr(x), RAW_DTYPES[x.dtype], B, C, c_use, H, W, float(params.lower),
                 float(params.upper), _native.ptr(lh), int(params.invert), _native.ptr(out), _native.ptr(ws),
                 ws.numel() // 4 * 4, sptr)
    return out


def normalize99_sort(x: torch.Tensor, lower: float = 1.0, upper: float = 99.0) -> torch.Tensor:
    """Sort-based torch formulation of :func:`normalize99` (CPU path and test oracle)."""
    B, C, H, W = x.shape
    xf = x.float().reshape(B * C, H * W)
    srt, _ = torch.sort(xf, dim=1)
    n = H * W

    def pct(q):
        pos = q / 100.0 * (n - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, n - 1)
        frac = pos - lo
        return srt[:, lo] * (1 - frac) + srt[:, hi] * frac

    p1, p99 = pct(lower), pct(upper)
    rng = (p99 - p1)
    ok = rng > 1e-3
    scale = torch.where(ok, 1.0 / torch.where(ok, rng, torch.ones_like(rng)), torch.ones_like(rng))
    const = (srt[:, -1] - srt[:, 0]) == 0
    out = (xf - p1[:, None]) * scale[:, None]
    out = torch.where(const[:, None], torch.zeros_like(out), out)
    return out.reshape(B, C, H, W)


class TilePlan:
    """Cellpose tiling of an (H, W) image: pad to a multiple of 16 (+8 margin), 224 tiles, 10 % overlap.

    ``augment`` (test-time augmentation, :func:`reference.make_tiles` with ``augment=True``): tiles
    are always ``bsize x bsize`` and overlap by half (``overlap`` is ignored), an axis shorter than
    the tile is zero-padded at its end (canvas ``Ly x Lx``), and tile ``(j, i)`` of the grid goes to
    the network mirrored in y when ``i`` is odd and in x when ``j`` is odd.  The gathers write the
    mirrored tiles and :meth:`blend` takes the network's outputs as they come and mirrors them back
    (:func:`reference.unaugment_tiles`) as it reads: the ``*_aug`` entry points of ``tiles.hip``."""

    def __init__(self, H: int, W: int, bsize: int = 224, overlap: float = 0.1, device="cpu", augment: bool = False):
        self.H, self.W = H, W
        self.augment = bool(augment)
        ya, yb = ref.pad_amounts(H)
        xa, xb = ref.pad_amounts(W)
        self.pad_y, self.pad_x = ya, xa
        self.Hp, self.Wp = H + ya + yb, W + xa + xb
        if self.augment:
            self.ys = ref.tile_starts_augment(self.Hp, bsize)
            self.xs = ref.tile_starts_augment(self.Wp, bsize)
            self.by = self.bx = int(bsize)
        else:
            self.ys = ref.tile_starts(self.Hp, bsize, overlap)
            self.xs = ref.tile_starts(self.Wp, bsize, overlap)
            self.by, self.bx = min(bsize, self.Hp), min(bsize, self.Wp)
        self.Ly, self.Lx = max(self.Hp, self.by), max(self.Wp, self.bx)  # the canvas the tiles cover
        self._sfx = "_aug" if self.augment else ""
        self.nt = len(self.ys) * len(self.xs)
        m = ref.taper_mask(self.by, self.bx)
        # the 2-D taper is separable: recover the 1-D factors from its centre row/col
        cy, cx = self.by // 2, self.bx // 2
        wy = m[:, cx] / np.sqrt(m[cy, cx])
        wx = m[cy, :] / np.sqrt(m[cy, cx])
        dev = torch.device(device)
        self.ys_t = torch.tensor(self.ys, dtype=torch.int32, device=dev)
        self.xs_t = torch.tensor(self.xs, dtype=torch.int32, device=dev)
        self.wy = torch.tensor(wy, dtype=torch.float32, device=dev)
        self.wx = torch.tensor(wx, dtype=torch.float32, device=dev)

    def gather(self, img: torch.Tensor, cpad: int) -> torch.Tensor:
        B, C, H, W = img.shape
        out = torch.empty(B * self.nt, self.by, self.bx, cpad, dtype=torch.bfloat16, device=img.device)
        img = img.float().contiguous()
        _native.call("be_tiles_gather" + self._sfx, _native.ptr(img), B, C, H, W, self.pad_y, self.pad_x, _native.ptr(self.ys_t),
                     _native.ptr(self.xs_t), len(self.ys), len(self.xs), self.by, self.bx, cpad, _native.ptr(out),
                     _native.stream(img.device))
        return out

    def gather_normalized(self, x_raw: torch.Tensor, cpad: int, c_use: int | None = None, lower: float = 1.0,
                          upper: float = 99.0, params=None) -> torch.Tensor:
        """``gather(normalize99(x_raw[:, :c_use].float(), lower, upper), cpad)`` bit for bit, from
        the raw pixels in one native call: ``x_raw`` is a contiguous [B, C, H, W] uint8, uint16 or
        float32 device tensor (:func:`takes_fused_front`); channels from ``c_use`` on are ignored.

        ``params`` (a :class:`~.pipeline.NormParams`; ``None`` is exactly the call above): the
        gather of ``normalize_img_gpu(x_raw, params, c_use)`` bit for bit.  Its percentiles replace
        ``lower`` / ``upper``; fixed bounds skip the select, tile normalisation runs the block
        select and the maps kernel first and the gather samples the maps per pixel."""
        B, C, H, W = x_raw.shape
        if x_raw.dtype not in RAW_DTYPES or not x_raw.is_contiguous():
            raise ValueError(f"gather_normalized takes a contiguous uint8, uint16 or float32 tensor, got {x_raw.dtype}")
        c_use = C if c_use is None else min(int(c_use), C)
        if params is not None:
            if not params.normalize:
                raise ValueError("gather_normalized needs normalisation on; use gather() for the pixels as they are")
            lower, upper = params.lower, params.upper
        out = torch.empty(B * self.nt, self.by, self.bx, cpad, dtype=torch.bfloat16, device=x_raw.device)
        sptr = _native.stream(x_raw.device)
        tail = (self.pad_y, self.pad_x, _native.ptr(self.ys_t), _native.ptr(self.xs_t), len(self.ys), len(self.xs), self.by,
                self.bx, cpad, _native.ptr(out))
        if params is not None and params.tile_blocksize > 0:
            lo, hi = tile_norm_maps_gpu(x_raw, params.tile_blocksize, lower, upper, c_use)
            _native.call("be_tiles_gather_tilenorm" + self._sfx, _native.ptr(x_raw), RAW_DTYPES[x_raw.dtype], B, C, c_use, H, W,
                         _native.ptr(lo), _native.ptr(hi), lo.shape[2], lo.shape[3], int(params.invert), *tail, sptr)
            return out
        ws = _pct_workspace(x_raw.device, sptr, B * c_use)
        if params is not None and not _plain_percentile(params):
            lh = _lowhigh_tensor(params.lowhigh, c_use, x_raw.device) if params.lowhigh is not None else None
            _native.call("be_tiles_gather_normx" + self._sfx, _native.ptr(x_raw), RAW_DTYPES[x_raw.dtype], B, C, c_use, H, W,
                         float(lower), float(upper), _native.ptr(lh), int(params.invert), *tail, _native.ptr(ws),
                         ws.numel() // 4 * 4, sptr)
            return out
        _native.call("be_tiles_gather_norm" + self._sfx, _native.ptr(x_raw), RAW_DTYPES[x_raw.dtype], B, C, c_use, H, W, float(lower),
                     float(upper), self.pad_y, self.pad_x, _native.ptr(self.ys_t), _native.ptr(self.xs_t), len(self.ys),
                     len(self.xs), self.by, self.bx, cpad, _native.ptr(out), _native.ptr(ws), ws.numel() // 4 * 4, sptr)
        return out

    def blend(self, yt: torch.Tensor, B: int) -> torch.Tensor:
        nout = yt.shape[1]
        out = torch.empty(B, nout, self.H, self.W, dtype=torch.float32, device=yt.device)
        _native.call("be_tiles_blend" + self._sfx, _native.ptr(yt), B, nout, self.H, self.W, self.pad_y, self.pad_x,
                     _native.ptr(self.ys_t), _native.ptr(self.xs_t), len(self.ys), len(self.xs), self.by, self.bx,
                     _native.ptr(self.wy), _native.ptr(self.wx), _native.ptr(out), _native.stream(yt.device))
        return out


def _taper_factors(by: int, bx: int):
    """The 1-D factors ``(wy, wx)`` of the separable taper mask of a ``by x bx`` tile."""
    m = ref.taper_mask(by, bx)
    cy, cx = by // 2, bx // 2
    return m[:, cx] / np.sqrt(m[cy, cx]), m[cy, :] / np.sqrt(m[cy, cx])


class ScaledTilePlan:
    """Cellpose tiling of a batch of (H, W) images that each have their own scale (per-image
    ``diameter``): image ``b`` is resampled to ``(Hs_b, Ws_b) = scaled_size(H | W, scales[b])``
    (``None``: not rescaled), padded and tiled as :class:`TilePlan` tiles an image of that size, and
    its blended flows are resampled back to (H, W).  The resampling happens in the loads of the
    gather and of the last kernel (``csrc/kernels/tiles_scaled.hip``): no resized image exists.

    The network takes tiles of one shape per call, so the tiles are grouped by their shape
    ``(by, bx)``: ``groups`` lists ``(by, bx, first tile, tiles)``.  Whenever every scaled, padded
    image is at least ``bsize`` on both axes -- always under ``augment`` -- that is one group.  The
    tile table (image, y0, x0, mirror flags per tile; the flags replace the ``_aug`` entry points)
    and the per-image table are uploaded once, here; every offset in them is 64-bit."""

    N_FIELDS = 16  # int64 fields per row of the image table (tiles_scaled.hip kI)

    def __init__(self, H: int, W: int, scales, bsize: int = 224, overlap: float = 0.1, augment: bool = False, device="cpu"):
        self.H, self.W, self.B = int(H), int(W), len(scales)
        self.augment = bool(augment)
        if self.B == 0:
            raise ValueError("ScaledTilePlan needs at least one image")
        per = []
        for r in scales:
            Hs, Ws = ref.scaled_size(H, r), ref.scaled_size(W, r)
            ya, yb = ref.pad_amounts(Hs)
            xa, xb = ref.pad_amounts(Ws)
            Hp, Wp = Hs + ya + yb, Ws + xa + xb
            if self.augment:
                ys, xs = ref.tile_starts_augment(Hp, bsize), ref.tile_starts_augment(Wp, bsize)
                by = bx = int(bsize)
            else:
                ys, xs = ref.tile_starts(Hp, bsize, overlap), ref.tile_starts(Wp, bsize, overlap)
                by, bx = min(bsize, Hp), min(bsize, Wp)
            per.append(dict(Hs=Hs, Ws=Ws, pad_y=ya, pad_x=xa, ys=ys, xs=xs, by=by, bx=bx, nt=len(ys) * len(xs)))
        self.images = per
        shapes = []
        for im in per:
            if (im["by"], im["bx"]) not in shapes:
                shapes.append((im["by"], im["bx"]))
        taper, taper_off = [], {}
        for by, bx in shapes:
            taper_off[(by, bx)] = sum(len(t) for t in taper)
            taper.extend(_taper_factors(by, bx))
        tiles, flat_ys, flat_xs = [], [], []
        itab = np.zeros((self.B, self.N_FIELDS), np.int64)
        self.groups = []
        flow_pix = yt_pix = 0
        order = []  # images in tile-table order
        for by, bx in shapes:
            first = len(tiles)
            for b, im in enumerate(per):
                if (im["by"], im["bx"]) != (by, bx):
                    continue
                order.append(b)
                itab[b, :14] = (im["Hs"], im["Ws"], im["pad_y"], im["pad_x"], len(im["ys"]), len(im["xs"]), len(tiles),
                                len(flat_ys), len(flat_xs), 0, by, bx, taper_off[(by, bx)], yt_pix)
                for j, y0 in enumerate(im["ys"]):
                    for i, x0 in enumerate(im["xs"]):
                        tiles.append((b, y0, x0, ((i & 1) | ((j & 1) << 1)) if self.augment else 0))
                flat_ys.extend(im["ys"])
                flat_xs.extend(im["xs"])
                yt_pix += im["nt"] * by * bx
            self.groups.append((by, bx, first, len(tiles) - first))
        for b, im in enumerate(per):  # the flat scaled-flow buffer holds the images in batch order
            itab[b, 9] = flow_pix
            flow_pix += im["Hs"] * im["Ws"]
        self.itab = itab  # host copy; column 6 is an image's first row of the tile table
        self.nt_total, self.flow_pix, self.yt_pix = len(tiles), flow_pix, yt_pix
        self.max_pix = max(im["Hs"] * im["Ws"] for im in per)
        # rows of the tile outputs that belong to each image, padded with one past the end (a zero row)
        ntmax = max(im["nt"] for im in per)
        rows = np.full((self.B, ntmax), len(tiles), np.int64)
        for b, im in enumerate(per):
            rows[b, : im["nt"]] = int(itab[b, 6]) + np.arange(im["nt"])
        dev = torch.device(device)
        self.tiles_t = torch.tensor(np.asarray(tiles, np.int32).reshape(-1, 4), device=dev)
        self.itab_t = torch.tensor(itab, device=dev)
        self.ys_t = torch.tensor(flat_ys, dtype=torch.int32, device=dev)
        self.xs_t = torch.tensor(flat_xs, dtype=torch.int32, device=dev)
        self.taper_t = torch.tensor(np.concatenate(taper), dtype=torch.float32, device=dev)
        self.rows_t = torch.tensor(rows, device=dev)

    def _gather(self, img: torch.Tensor, cpad: int, mode: int, c_use: int, lower=1.0, upper=99.0, lh=None, invert=False):
        B, C, H, W = img.shape
        if (B, H, W) != (self.B, self.H, self.W):
            raise ValueError(f"this plan tiles [{self.B}, C, {self.H}, {self.W}] batches, got {tuple(img.shape)}")
        sptr = _native.stream(img.device)
        ws = _pct_workspace(img.device, sptr, B * c_use) if mode and lh is None else None
        out = []
        for by, bx, first, n in self.groups:
            t = torch.empty(n, by, bx, cpad, dtype=torch.bfloat16, device=img.device)
            _native.call("be_tiles_gather_scaled", _native.ptr(img), RAW_DTYPES[img.dtype], mode, B, C, c_use, H, W, float(lower),
                         float(upper), _native.ptr(lh), int(invert), _native.ptr(self.tiles_t), _native.ptr(self.itab_t), first, n,
                         by, bx, cpad, _native.ptr(t), _native.ptr(ws), ws.numel() // 4 * 4 if ws is not None else 0, sptr)
            out.append(t)
        return out

    def gather(self, img: torch.Tensor, cpad: int) -> list:
        """img [B, C, H, W], already normalised (or to be taken as it is) -> one NHWC bf16 tile
        tensor [tiles, by, bx, cpad] per group: each tile pixel is the bilinear sample of the image at
        its scaled coordinate, zero outside the scaled image, rounded once."""
        return self._gather(img.float().contiguous(), cpad, 0, img.shape[1])

    def gather_normalized(self, x_raw: torch.Tensor, cpad: int, c_use: int | None = None, params=None) -> list:
        """``gather(normalize_img_gpu(x_raw, params, c_use), cpad)`` bit for bit from the raw pixels
        (contiguous uint8, uint16 or float32): the percentile select runs on them and each of the
        four taps is normalised with its row's constants before the lerp.  ``params``: a
        :class:`~.pipeline.NormParams` of a global rule (``None``: the default percentiles); tile
        normalisation has no fused form here -- normalise first and use :meth:`gather`."""
        _check_raw(x_raw, "ScaledTilePlan.gather_normalized")
        C = x_raw.shape[1]
        c_use = C if c_use is None else min(int(c_use), C)
        if params is None or _plain_percentile(params):
            lower, upper = (1.0, 99.0) if params is None else (params.lower, params.upper)
            return self._gather(x_raw, cpad, 1, c_use, lower, upper)
        if not params.normalize or params.tile_blocksize > 0:
            raise ValueError("ScaledTilePlan.gather_normalized takes the global normalisation rules only")
        lh = _lowhigh_tensor(params.lowhigh, c_use, x_raw.device) if params.lowhigh is not None else None
        return self._gather(x_raw, cpad, 2, c_use, params.lower, params.upper, lh, params.invert)

    def blend(self, yts, unmirror: bool = True) -> torch.Tensor:
        """Tile outputs (one [tiles, nout, by, bx] fp32 tensor per group, as the gathers return the
        tiles) -> the flat fp32 buffer that holds image ``b``'s ``[nout, Hs_b, Ws_b]`` blend at
        ``itab[b, 9] * nout``.  Output-centric, no atomics: bit-deterministic."""
        yts = [yts] if torch.is_tensor(yts) else list(yts)
        nout = yts[0].shape[1]
        for yt, (by, bx, _, n) in zip(yts, self.groups):
            if tuple(yt.shape) != (n, nout, by, bx) or yt.dtype != torch.float32:
                raise ValueError(f"blend: expected float32 tile outputs {(n, nout, by, bx)}, got {yt.dtype} {tuple(yt.shape)}")
        if len(yts) != len(self.groups) or nout > 4:
            raise ValueError("blend: one tile-output tensor per group with at most 4 channels")
        flat = yts[0].contiguous().view(-1) if len(yts) == 1 else torch.cat([y.reshape(-1) for y in yts])
        out = torch.empty(self.flow_pix * nout, dtype=torch.float32, device=flat.device)
        _native.call("be_tiles_blend_scaled", _native.ptr(flat), _native.ptr(self.tiles_t), _native.ptr(self.itab_t),
                     _native.ptr(self.ys_t), _native.ptr(self.xs_t), _native.ptr(self.taper_t), self.B, nout, self.max_pix,
                     int(bool(unmirror)), _native.ptr(out), _native.stream(flat.device))
        return out

    def resize_back(self, flat: torch.Tensor, nout: int) -> torch.Tensor:
        """The buffer of :meth:`blend` -> [B, nout, H, W] fp32, each image resampled bilinearly from
        its own ``(Hs_b, Ws_b)``."""
        if flat.numel() != self.flow_pix * nout or flat.dtype != torch.float32 or not flat.is_contiguous():
            raise ValueError("resize_back takes the flat float32 buffer blend() returned")
        out = torch.empty(self.B, nout, self.H, self.W, dtype=torch.float32, device=flat.device)
        _native.call("be_resize_bilinear_ragged", _native.ptr(flat), _native.ptr(self.itab_t), self.B, nout, self.H, self.W,
                     _native.ptr(out), _native.stream(flat.device))
        return out

    def scaled_flow(self, flat: torch.Tensor, b: int, nout: int) -> torch.Tensor:
        """Image ``b``'s ``[nout, Hs_b, Ws_b]`` view of the buffer of :meth:`blend`."""
        im = self.images[b]
        o = sum(i["Hs"] * i["Ws"] for i in self.images[:b]) * nout
        return flat[o: o + nout * im["Hs"] * im["Ws"]].view(nout, im["Hs"], im["Ws"])

    def sum_styles(self, sts) -> torch.Tensor:
        """Per-tile style vectors (one [tiles, S] tensor per group) -> their sum per image [B, S]."""
        sts = [sts] if torch.is_tensor(sts) else list(sts)
        st = torch.cat(sts + [torch.zeros(1, sts[0].shape[1], dtype=sts[0].dtype, device=sts[0].device)])
        return st[self.rows_t].sum(1)


# ------------------------------------------------------------------ mask recovery


def _jobs_tensor(b, lab, y0, x0, ly, lx, scratch) -> torch.Tensor:
    """Pack MaskJob structs {int b, lab, y0, x0, ly, lx; int64 scratch} as int64 words."""
    w0 = (b.long() & 0xFFFFFFFF) | (lab.long() << 32)
    w1 = (y0.long() & 0xFFFFFFFF) | (x0.long() << 32)
    w2 = (ly.long() & 0xFFFFFFFF) | (lx.long() << 32)
    return torch.stack([w0, w1, w2, scratch.long()], 1).contiguous()


def _plan_jobs(bbox_valid, labs_b, labs_l, lds_fn, caps, scratch_fn, valid=None):
    """Bucket masks by their LDS need with ONE host sync.

    Bucket k < len(caps) holds masks with caps[k-1] < need <= caps[k]; bucket len(caps) holds the
    masks too big for LDS, which get scratch offsets.  Jobs are sorted by bucket on the device and
    only the per-bucket counts (+ the scratch total) come back to the host, so the slices below
    are views -- replacing one boolean-index gather (a nonzero + sync, ~75 us) per field and bucket.
    ``valid`` (optional bool per row) drops rows without a separate nonzero (and its sync).
    Returns ``(jobs_by_bucket: list of [n_k, 4] int64 views, scratch_total)``."""
    y0, y1, x0, x1 = bbox_valid.unbind(1)
    ly, lx = y1 - y0 + 1, x1 - x0 + 1
    need = lds_fn(ly, lx)
    dev = bbox_valid.device
    edges = torch.tensor(caps, dtype=need.dtype, device=dev)
    bucket = torch.bucketize(need, edges)  # need <= caps[k]  ->  k
    nb = len(caps) + 1
    if valid is not None:
        bucket = torch.where(valid, bucket, torch.full_like(bucket, nb))  # dropped rows sort last
    order = torch.argsort(bucket, stable=True)
    counts = torch.bincount(bucket, minlength=nb + 1)[:nb]
    big = bucket[order] == len(caps)
    ly_s, lx_s = ly[order], lx[order]
    sz = torch.where(big, scratch_fn(ly_s, lx_s), torch.zeros_like(ly_s)).long()
    off = torch.cumsum(sz, 0) - sz
    scr = torch.where(big, off, torch.full_like(off, -1))
    jobs = _jobs_tensor(labs_b[order], labs_l[order], y0[order], x0[order], ly_s, lx_s, scr)
    host = torch.cat([counts.long(), sz.sum().view(1)]).cpu().tolist()  # the one sync
    out, start = [], 0
    for k in range(nb):
        out.append(jobs[start:start + host[k]])
        start += host[k]
    return out, int(host[nb])


class PlanKind(enum.IntEnum):
    """``kind`` of ``be_cp_plan_masks``: what a mask needs for the flow-QC diffusion or the hole filling."""
    DIFFUSE = 0
    FILL = 1
    DIFFUSE_QUEUE = 2  # DIFFUSE with the compact work-queue buckets in front (needs pixel counts)
    FILL_WAVE = 3      # FILL with the one-wave buckets in front


#: (kind, pixel counts given) -> the kernel's bucket order, as the fields of :class:`MaskPlan`
#: (``lds`` = one bucket per LDS cap of the kind); what is not listed cannot be planned
PLAN_LAYOUT = {
    (PlanKind.DIFFUSE, False): ("lds", "big"),
    (PlanKind.DIFFUSE, True): ("lds", "sparse_big", "big"),
    (PlanKind.DIFFUSE_QUEUE, True): ("queue_wave", "queue_group", "lds", "sparse_big", "big"),
    (PlanKind.FILL, False): ("lds", "big"),
    (PlanKind.FILL_WAVE, False): ("wave_small", "wave_big", "lds", "big"),
}


@dataclasses.dataclass
class MaskPlan:
    """Jobs of one ``be_cp_plan_masks`` launch by bucket, each [n, 4] int64 (MaskJob rows, order
    inside a bucket arbitrary); a bucket the kind does not have is empty ([0, 4])."""
    kind: PlanKind
    scratch_total: int
    niter_img: torch.Tensor   # [B] int32, diffusion kinds
    lds: list                 # one workgroup per mask in LDS: one bucket per cap, smallest first
    big: torch.Tensor         # beyond LDS, with scratch offsets: tiled diffusion / global-scratch fill
    sparse_big: torch.Tensor  # diffusion with counts: beyond LDS but sparse, heat field in scratch
    queue_wave: torch.Tensor  # diffusion queue: wave jobs (<= 256 pixels)
    queue_group: torch.Tensor  # diffusion queue: workgroup jobs
    wave_small: torch.Tensor  # one-wave fill: box + ring <= 64 x 64
    wave_big: torch.Tensor    # one-wave fill: box + ring <= 256 x 128


def _plan_finish(launched: list) -> list:
    """Read back the bucket sizes of several :func:`_plan_launch` plans (each one ``be_cp_plan_masks``
    launch, the device-side :func:`_plan_jobs`) with ONE host sync: a :class:`MaskPlan` for each."""
    host = torch.cat([torch.cat([nk.long(), tot]) for _, nk, tot, _, _ in launched]).cpu().tolist()
    out, o = [], 0
    for jobs, nk, _, niter_img, (kind, split) in launched:
        layout, nb = PLAN_LAYOUT[kind, split], nk.shape[0]
        e = jobs[0, :0]  # every bucket without jobs: a slice is ~4 us of host time, and most buckets are empty
        plan = MaskPlan(kind, int(host[o + nb]), niter_img, lds=[], big=e, sparse_big=e, queue_wave=e, queue_group=e,
                        wave_small=e, wave_big=e)
        names = [name for name in layout for _ in range(nb - len(layout) + 1 if name == "lds" else 1)]
        for k, name in enumerate(names):
            rows = jobs[k, :host[o + k]] if host[o + k] else e
            if name == "lds":
                plan.lds.append(rows)
            else:
                setattr(plan, name, rows)
        out.append(plan)
        o += nb + 1
    return out


def _plan_launch(bbox: torch.Tensor, valid: torch.Tensor | None, kind: PlanKind, counts: torch.Tensor | None = None):
    """``counts`` (diffusion kinds): per-label pixel counts [B, nlab] int32, which split the too-big-for-LDS masks
    into big-sparse and tiled.  Returns ``(jobs, bucket_n, scratch_total, niter_img, (kind, counts given))``."""
    B, nlab = bbox.shape[:2]
    dev = bbox.device
    kind, split = PlanKind(kind), counts is not None
    # the kernel would write queue buckets that are not there (no counts), or put fill jobs
    # through the diffusion queue's test (FILL_WAVE with counts)
    if (kind, split) not in PLAN_LAYOUT:
        raise ValueError(f"no {kind.name} plan {'with' if split else 'without'} pixel counts")
    assert not split or (counts.shape == (B, nlab) and counts.dtype == torch.int32)
    caps = [LDS_FILL_BYTES] if kind in (PlanKind.FILL, PlanKind.FILL_WAVE) else DIFFUSE_CAPS
    nb = len(PLAN_LAYOUT[kind, split]) - 1 + len(caps)
    jobs = torch.empty(nb, max(B * nlab, 1), 4, dtype=torch.int64, device=dev)
    bucket_n = torch.zeros(nb, dtype=torch.int32, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    niter_img = torch.zeros(B, dtype=torch.int32, device=dev)
    carr = (ctypes.c_int * len(caps))(*[int(c) for c in caps])
    vptr = _native.ptr(valid.contiguous().view(torch.uint8)) if valid is not None else None
    cptr = _native.ptr(counts.contiguous()) if split else None
    _native.call("be_cp_plan_masks", _native.ptr(bbox.contiguous()), vptr, cptr, B, nlab, int(kind), ctypes.addressof(carr),
                 len(caps), _native.ptr(jobs), _native.ptr(bucket_n), _native.ptr(tot), _native.ptr(niter_img),
                 _native.stream(dev))
    return jobs, bucket_n, tot, niter_img, (kind, split)


#: compact work-queue diffusion (be_cp_diffuse_q) for the masks it can take; 0 = the LDS-box buckets
DIFFUSE_QUEUE = os.environ.get("BE_DIFFUSE_QUEUE", "1") != "0"


def _diffuse_plan_kind() -> PlanKind:
    return PlanKind.DIFFUSE_QUEUE if DIFFUSE_QUEUE else PlanKind.DIFFUSE


#: one-wave hole filling (be_cp_fill_holes_wave) for boxes up to 64 x 64 with the ring; 0 = LDS kernel only
FILL_WAVE = os.environ.get("BE_FILL_WAVE", "1") != "0"


def _fill_plan_kind() -> PlanKind:
    return PlanKind.FILL_WAVE if FILL_WAVE else PlanKind.FILL


def _diffuse_lds_bytes(ly, lx):
    R = (ly + 2) * (lx + 2)
    return 16 * R + 4 * (ly + 2 + lx + 2) + R + 16


def _diffuse_scratch_doubles(ly, lx):
    R = (ly + 2) * (lx + 2)
    return 2 * R + (ly + 2 + lx + 2 + 1) // 2 + (R + 7) // 8 + 2


#: (LDS bytes, threads) buckets of the one-workgroup-per-mask diffusion: a block reserves only its
#: bucket's LDS, so small masks run many blocks per CU (one 48 KiB reservation per mask allowed 3).
DIFFUSE_BUCKETS = ((6 * 1024, 64), (12 * 1024, 128), (24 * 1024, 256), (48 * 1024, 256), (80 * 1024, 512),
                   (LDS_DIFFUSE_BYTES, 512))
DIFFUSE_CAPS = [c for c, _ in DIFFUSE_BUCKETS]
#: rows per work item of the diffusion sweep (``BE_DIFFUSE_DV``): a smaller DV gives every mask
#: proportionally more threads (buckets scale up to 1024) and a shorter serial LDS chain per sweep
DIFFUSE_DV = 4


_DEBUG_STATS = os.environ.get("BIOENGINE_MASK_STATS", "0") == "1"


#: flow-following launch: LDS-staged flow window per 32 x 32 tile (default), XCD-ordered +
#: block-compacted L2 gathers, or the plain pixel-per-lane one (all bit-identical)
FOLLOW_FLOWS_ENTRY = os.environ.get("BIOENGINE_FOLLOW_ENTRY", "be_cp_follow_flows_lds")

_SIDE_STREAMS: dict = {}
#: LDS buckets run on their own HIP streams so their launch tails (a few CUs finishing the
#: largest masks of a bucket) overlap the next bucket instead of idling the rest of the chip.
N_SIDE_STREAMS = 3


def _side_streams(dev):
    key = (dev.type, dev.index)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(dev) for _ in range(N_SIDE_STREAMS)]
    return _SIDE_STREAMS[key]


def _bucket_small(plan: MaskPlan, L, scratch, dv: int) -> list:
    """``(entry, jobs, arguments after niter_img)`` of the non-empty one-workgroup-per-mask launches in
    queue order: the big sparse masks (global-scratch heat field; ``niter`` sweeps of the largest boxes,
    the longest-running launches), then the LDS buckets, largest first (they set the critical path)."""
    out = [("be_cp_diffuse_nt", jobs, (_native.ptr(L), cap, min(1024, threads * (8 // dv)), dv))
           for jobs, (cap, threads) in zip(plan.lds, DIFFUSE_BUCKETS) if jobs.shape[0]]
    if plan.sparse_big.shape[0]:
        out.append(("be_cp_diffuse_sparse_big", plan.sparse_big, (_native.ptr(scratch), _native.ptr(L))))
    if _DEBUG_STATS:
        print(f"[diffuse_small] buckets={[x.shape[0] for x in plan.lds]} sparse_big={plan.sparse_big.shape[0]} "
              f"big={plan.big.shape[0]}", flush=True)
    return out[::-1]


def _diffuse_small(Mc, launches, niter_img, L, scratch, st, ready=None) -> None:
    """Queues :func:`_bucket_small`'s ``launches``.  ``ready``: event recorded on the current stream once the inputs
    exist; the buckets start from it instead of from the stream's tail, so they run alongside the big-mask kernel.

    Every bucket kernel runs ``niter`` dependent sweeps, so its time grows with its mask size and a
    stream's tail is the sum of its buckets: the buckets (largest first) go to the queues in snake
    order (0, 1, .., n-1, n-1, .., 0), and without a big-mask kernel the main stream is one of the
    queues (4 hardware queues per process: main + 3 side streams)."""
    B, H, W = Mc.shape
    concurrent = Mc.is_cuda and N_SIDE_STREAMS > 0
    if concurrent:
        main = torch.cuda.current_stream(Mc.device)
        sides = _side_streams(Mc.device)
        for sd in sides:
            if ready is not None:
                sd.wait_event(ready)
            else:
                sd.wait_stream(main)
        queues = sides if ready is not None else [None] + sides  # None = the main stream itself
        nq = len(queues)
    for k, (entry, jobs, tail) in enumerate(launches):
        sptr = st
        if concurrent:
            r = k % (2 * nq)
            sd = queues[r if r < nq else 2 * nq - 1 - r]
            if sd is not None:
                for t in (jobs, Mc, niter_img, L, scratch):
                    t.record_stream(sd)
                sptr = ctypes.c_void_p(sd.cuda_stream)
        _native.call(entry, _native.ptr(Mc), _native.ptr(jobs), jobs.shape[0], H, W, _native.ptr(niter_img), *tail, sptr)
    if concurrent:
        for sd in sides:
            main.wait_stream(sd)


_TILE_PARAMS: tuple | None = None
#: "tiled" = multi-workgroup time-blocked diffusion for masks larger than LDS (default);
#: "block" = one workgroup per mask on a global scratch slab (kept as a cross-check).
BIG_MASK_MODE = "tiled"


def _diffuse_big(Mc, bj, niter_img, scratch, L, st, between=None) -> torch.Tensor | None:
    """Diffusion of masks too large for one workgroup's LDS (see diffuse_tiled_kernel).
    ``between()`` runs after the short per-mask centre kernel is queued and before the long
    cooperative sweep (the caller releases its other streams there)."""
    global _TILE_PARAMS
    B, H, W = Mc.shape
    if BIG_MASK_MODE == "block":
        if between is not None:
            between()
        _native.call("be_cp_diffuse", _native.ptr(Mc), _native.ptr(bj), bj.shape[0], H, W, _native.ptr(niter_img),
                     _native.ptr(scratch), _native.ptr(L), 0, st)
        return None
    if _TILE_PARAMS is None:
        buf = (ctypes.c_int * 3)()
        _native.call("be_cp_diffuse_tile_params", ctypes.addressof(buf))
        _TILE_PARAMS = (buf[0], buf[1], buf[2])
    core = _TILE_PARAMS[0]
    w2 = bj[:, 2].cpu()
    ly, lx = (w2 & 0xFFFFFFFF), (w2 >> 32)
    nty = (ly + 2 + core - 1) // core
    ntx = (lx + 2 + core - 1) // core
    per = (nty * ntx)
    job = torch.repeat_interleave(torch.arange(bj.shape[0]), per)
    start = torch.cumsum(per, 0) - per
    k = torch.arange(int(per.sum())) - start[job]
    ty = (k // ntx[job]) * core
    tx = (k % ntx[job]) * core
    tiles = torch.stack([job, ty, tx, torch.zeros_like(job)], 1).to(torch.int32).to(Mc.device)
    if _DEBUG_STATS:
        print(f"[diffuse_big] masks={bj.shape[0]} tiles={tiles.shape[0]} box_ly={ly.tolist()} box_lx={lx.tolist()} "
              f"niter={niter_img.tolist()}", flush=True)
    centers = torch.empty(bj.shape[0], dtype=torch.int32, device=Mc.device)
    ws = torch.zeros(4, dtype=torch.int32, device=Mc.device)
    args = (_native.ptr(Mc), _native.ptr(bj), bj.shape[0], _native.ptr(tiles), tiles.shape[0], H, W,
            _native.ptr(niter_img), _native.ptr(scratch), _native.ptr(L), _native.ptr(centers), _native.ptr(ws))
    _native.call("be_cp_diffuse_tiled", *args, 1, st)
    if between is not None:
        between()
    _native.call("be_cp_diffuse_tiled", *args, 2, st)
    return ws  # ws[1] != 0 <=> the grid barrier timed out; checked by the caller after queuing the rest


def _check_tiled(ws) -> None:
    if ws is not None and int(ws[1].item()) != 0:
        raise RuntimeError("diffuse_tiled_kernel: grid barrier timed out (workgroups not co-resident)")


def label_counts(M: torch.Tensor, nlab: int) -> torch.Tensor:
    """Pixels per label [B, nlab] (label 0 not counted)."""
    B = M.shape[0]
    counts = torch.zeros(B, nlab, dtype=torch.int32, device=M.device)
    Mc = M.contiguous()
    _native.call("be_label_counts", _native.ptr(Mc), B, Mc[0].numel(), nlab, _native.ptr(counts), _native.stream(M.device))
    return counts


def mask_bboxes(M: torch.Tensor, nlab: int) -> torch.Tensor:
    B, H, W = M.shape
    bbox = torch.empty(B, nlab, 4, dtype=torch.int32, device=M.device)
    bbox[..., 0] = 2 ** 31 - 1
    bbox[..., 1] = -1
    bbox[..., 2] = 2 ** 31 - 1
    bbox[..., 3] = -1
    _native.call("be_cp_bbox", _native.ptr(M), B, H, W, nlab, _native.ptr(bbox), _native.stream(M.device))
    return bbox


def masks_to_flows_gpu(M: torch.Tensor, dp: torch.Tensor | None = None, niter: int | None = None,
                       nlab: int | None = None, counts: torch.Tensor | None = None, plan=None, want_mu: bool = True):
    """Heat-diffusion flows of label images M [B, H, W] int32 (labels 1..n, contiguous per image).

    Returns (mu [B, 2, H, W] fp32, err_sum [B, nlab] fp32 or None, counts [B, nlab]).  When ``dp``
    ([B, >=2, H, W] network output) is given, err_sum[b, l] = sum over mask l of |mu - dp/5|^2.
    ``counts`` / ``plan`` (label_counts and a diffusion plan of the same labels) skip recomputing them;
    ``want_mu=False`` (flow QC: only the errors are used) returns ``mu=None`` and skips its writes.
    """
    B, H, W = M.shape
    dev = M.device
    if nlab is None:  # an upper bound on the labels + 1 is enough (absent labels have no pixels)
        nlab = _label_bound(M)
    mu = torch.zeros(B, 2, H, W, dtype=torch.float32, device=dev) if (want_mu or dp is None) else None
    if counts is None:
        counts = label_counts(M, nlab)
    if nlab <= 1:
        return mu, (torch.zeros(B, nlab, device=dev) if dp is not None else None), counts
    if plan is None:
        plan = _plan_finish([_plan_launch(mask_bboxes(M, nlab), None, _diffuse_plan_kind(), counts)])[0]
    niter_img = plan.niter_img if niter is None else torch.full((B,), niter, dtype=torch.int32, device=dev)
    bj, qw, qg = plan.big, plan.queue_wave, plan.queue_group
    L = torch.zeros(B, H, W, dtype=torch.float64, device=dev)
    scratch = torch.empty(max(plan.scratch_total, 1), dtype=torch.float64, device=dev)
    st = _native.stream(dev)
    Mc = M.contiguous()
    dv = int(os.environ.get("BE_DIFFUSE_DV", DIFFUSE_DV))  # read per call: benchmarks switch it between variants
    buckets = _bucket_small(plan, L, scratch, dv)
    ws = ready = release = None
    if bj.shape[0] and Mc.is_cuda and buckets:
        ready = torch.cuda.Event()

        def release():  # the buckets start once the big masks' centre kernel is done
            ready.record(torch.cuda.current_stream(dev))
    if qw.shape[0] or qg.shape[0]:
        # one persistent launch over every mask the compact kernel takes (nearly all of them),
        # queued first: the box-bucket kernels below then only see the rare leftovers
        qws = torch.empty(2, dtype=torch.int32, device=dev)
        _native.call("be_cp_diffuse_q", _native.ptr(Mc), _native.ptr(qw), qw.shape[0], _native.ptr(qg), qg.shape[0], H, W,
                     _native.ptr(niter_img), _native.ptr(L), _native.ptr(qws), st)
    if bj.shape[0]:
        # first, on an idle device: the centre kernel runs alone (~0.07 ms instead of ~0.36 ms
        # among the bucket kernels), then the cooperative tiled sweep -- the critical path -- is
        # queued right behind it; its few workgroups are resident before the bucket kernels
        # (which never wait on it) fill the remaining CUs, so its grid barrier cannot starve
        ws = _diffuse_big(Mc, bj, niter_img, scratch, L, st, between=release)
    if buckets:
        _diffuse_small(Mc, buckets, niter_img, L, scratch, st, ready=ready)
    err, dpp, bstride = None, None, 0
    if dp is not None:
        dpp = dp.float().contiguous()
        bstride = dpp.shape[1] * H * W
        err = torch.zeros(B, nlab, dtype=torch.float32, device=dev)
    _native.call("be_cp_flow_grad", _native.ptr(Mc), _native.ptr(L), B, H, W, _native.ptr(mu), _native.ptr(dpp),
                 bstride, _native.ptr(err), nlab, st)
    _check_tiled(ws)
    return mu, err, counts


def _renumber(M: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """keep [B, nlab] bool (index 0 ignored) -> M (B images; B = 1: any shape) relabelled 1..k per
    image, dropped labels -> 0."""
    return torch.gather(_rank_lut(keep), 1, M.reshape(keep.shape[0], -1).long()).reshape(M.shape)


def _label_bound(M: torch.Tensor) -> int:
    """The labels + 1 of ``M``, by a host read of ``M.max()``."""
    return int(M.max().item()) + 1 if M.numel() else 1


def _present_keep(counts: torch.Tensor, min_size: int) -> torch.Tensor:
    """counts [B, nlab] -> bool: the labels (never 0) that occur, with at least ``min_size`` pixels."""
    keep = counts > 0
    if min_size > 0:
        keep &= counts >= min_size
    keep[:, 0] = False
    return keep


def fill_holes_gpu(M: torch.Tensor, min_size: int = 15, nlab: int | None = None) -> torch.Tensor:
    """``nlab``: optional upper bound on the labels + 1 (saves the host sync on ``M.max()``)."""
    if nlab is None:
        nlab = _label_bound(M)
    if nlab <= 1:
        return M.clone()
    keep = _present_keep(label_counts(M, nlab), min_size)
    plan = _plan_finish([_plan_launch(mask_bboxes(M, nlab), keep, _fill_plan_kind())])[0]
    return _fill_run(M, _rank_lut(keep), nlab, plan)


def _rank_lut(keep: torch.Tensor) -> torch.Tensor:
    """keep [B, nlab] bool -> int32 lut: kept label -> its rank 1..k (id order), dropped -> 0."""
    keep = keep.clone()
    keep[:, 0] = False
    return (torch.cumsum(keep.int(), dim=1) * keep.int()).to(torch.int32).contiguous()


def _fill_run(M: torch.Tensor, lut: torch.Tensor, nlab: int, plan: MaskPlan) -> torch.Tensor:
    """Hole filling of the planned jobs (a fill plan); jobs whose lut entry is 0 write nothing."""
    B, H, W = M.shape
    out = torch.zeros_like(M)
    wjs = (plan.wave_small, plan.wave_big)
    (sj,), bj = plan.lds, plan.big
    if sj.shape[0] + bj.shape[0] + sum(w.shape[0] for w in wjs) == 0:
        return out
    scratch = torch.empty(max(plan.scratch_total, 1), dtype=torch.uint8, device=M.device)
    st = _native.stream(M.device)
    Mc = M.contiguous()
    for big, wj in enumerate(wjs):
        if wj.shape[0]:
            _native.call("be_cp_fill_holes_wave", _native.ptr(Mc), _native.ptr(wj), wj.shape[0], H, W, _native.ptr(lut), nlab,
                         _native.ptr(out), big, st)
    for jobs, lds_bytes in ((sj, LDS_FILL_BYTES), (bj, 0)):  # 0: the flood fill runs in global scratch
        if jobs.shape[0]:
            _native.call("be_cp_fill_holes", _native.ptr(Mc), _native.ptr(jobs), jobs.shape[0], H, W, _native.ptr(lut), nlab,
                         _native.ptr(scratch), _native.ptr(out), lds_bytes, st)
    return out


def _check_image2d(H: int, W: int) -> None:
    """The flow sampler maps position ``p`` to ``p * L / (L - 1) - 0.5``: an axis needs two pixels."""
    if H < 2 or W < 2:
        raise ValueError(f"2-D dynamics need at least two rows and two columns, got an image of {H} x {W}")


def follow_flows_gpu(y: torch.Tensor, niter: int = 200, cellprob_threshold: float = 0.0, entry: str | None = None,
                     with_flow: bool = False):
    """Network output ``y`` [B, 3, H, W] (dY, dX, cellprob) -> ``(hist [B, H+40, W+40] int32, pos
    [B, H, W] int32)``: the histogram of the end points of :func:`reference.follow_flows` in the
    padded image and every foreground pixel's padded linear bin index (-1 for background).
    ``be_cp_prep_flow`` then one flow-following launch: ``entry`` names it (``be_cp_follow_flows``,
    ``_xcd``, ``_xcd_pool`` or ``_lds``; identical results), None = :data:`FOLLOW_FLOWS_ENTRY`.
    ``with_flow`` also returns prep_flow's outputs ``(flow2 [B, H, W, 2] fp32 (dy, dx) / 5 on the
    foreground, fg [B, H, W] uint8)``.  No host sync."""
    B, _, H, W = y.shape
    _check_image2d(H, W)
    dev = y.device
    st = _native.stream(dev)
    y = y.float().contiguous()
    flow2 = torch.empty(B, H, W, 2, dtype=torch.float32, device=dev)
    fg = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    _native.call("be_cp_prep_flow", _native.ptr(y), B, H, W, float(cellprob_threshold), _native.ptr(flow2),
                 _native.ptr(fg), st)
    Hp, Wp = H + 2 * RPAD, W + 2 * RPAD
    hist = torch.zeros(B, Hp, Wp, dtype=torch.int32, device=dev)
    pos = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    _native.call(FOLLOW_FLOWS_ENTRY if entry is None else entry, _native.ptr(flow2), _native.ptr(fg), _native.ptr(hist),
                 _native.ptr(pos), B, H, W, int(niter), st)
    return (hist, pos, flow2, fg) if with_flow else (hist, pos)


def _lookup_labels(pos, M1, M0, B: int, nlab: int, max_size_fraction: float, st) -> torch.Tensor:
    """Tail of :func:`get_masks_gpu` / :func:`get_masks3d_gpu`: per-pixel lookup in the expanded seeds ``M1``
    into the zeroed ``M0`` (``B`` images or one volume), big-mask removal and renumber."""
    N, Np = M0.numel() // B, M1.numel() // B
    counts = torch.zeros(B, nlab, dtype=torch.int32, device=M0.device)
    _native.call("be_cp_label_lookup", _native.ptr(pos), _native.ptr(M1), B, N, Np, _native.ptr(M0), _native.ptr(counts),
                 nlab, st)
    keep = (counts > 0) & (counts <= N * max_size_fraction)
    return _renumber(M0, keep)


def get_masks_gpu(hist: torch.Tensor, pos: torch.Tensor, shape=None, max_size_fraction: float = 0.4,
                  with_bound: bool = False):
    """The stages of :func:`reference.get_masks` after the histogram, for a batch: ``hist``
    [B, H+40, W+40] int32 and ``pos`` [B, H, W] int32 (padded linear bin of every foreground pixel, -1
    elsewhere) -> raw labels [B, H, W] int32 numbered ``1..k`` per image (before QC / fill); with
    ``with_bound`` also an upper bound on its labels + 1 (known from the seed count).  5x5 seeds
    (``be_cp_seeds``), ``torch.sort`` of the seed keys, 11x11 window expansion (``be_cp_expand``),
    per-pixel lookup, big-mask removal and renumber.  One host sync (the seed count)."""
    B = pos.shape[0]
    H, W = tuple(pos.shape[1:]) if shape is None else tuple(int(v) for v in shape)
    _check_image2d(H, W)
    Hp, Wp = H + 2 * RPAD, W + 2 * RPAD
    if tuple(hist.shape) != (B, Hp, Wp) or tuple(pos.shape) != (B, H, W):
        raise ValueError(f"get_masks_gpu: hist {tuple(hist.shape)} / pos {tuple(pos.shape)} do not fit {B} images of "
                         f"{H} x {W} padded by {RPAD}")
    if hist.dtype != torch.int32 or pos.dtype != torch.int32:
        raise TypeError(f"get_masks_gpu expects int32 hist and pos, got {hist.dtype} and {pos.dtype}")
    dev = pos.device
    st = _native.stream(dev)
    hist, pos = hist.contiguous(), pos.contiguous()
    cap = H * W // 11 + 1
    keys = torch.full((B, cap), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
    nseeds = torch.zeros(B, dtype=torch.int32, device=dev)
    _native.call("be_cp_seeds", _native.ptr(hist), B, Hp, Wp, _native.ptr(keys), _native.ptr(nseeds), cap, st)
    kmax = int(nseeds.max().item()) if B else 0  # host sync: sizes the sort and the expansion grid
    kmax = min(kmax, cap)
    M1 = torch.zeros(B, Hp, Wp, dtype=torch.int32, device=dev)
    M0 = torch.zeros(B, H, W, dtype=torch.int32, device=dev)
    if kmax == 0:
        return (M0, 1) if with_bound else M0
    # seeds are compacted at the front of each row: sort only the first kmax slots (a few hundred)
    # instead of the whole cap-wide buffer of sentinels
    keys_sorted, _ = torch.sort(keys[:, :kmax].contiguous(), dim=1)
    _native.call("be_cp_expand", _native.ptr(hist), _native.ptr(keys_sorted), _native.ptr(nseeds), B, Hp, Wp, kmax, kmax,
                 _native.ptr(M1), st)
    nlab = kmax + 1
    M = _lookup_labels(pos, M1, M0, B, nlab, max_size_fraction, st)
    return (M, nlab) if with_bound else M


def follow_and_label(y: torch.Tensor, niter: int = 200, cellprob_threshold: float = 0.0,
                     max_size_fraction: float = 0.4, with_bound: bool = False):
    """Network output y [B, 3, H, W] -> raw masks M0 [B, H, W] int32 (before QC / fill); with
    ``with_bound`` also an upper bound on its labels + 1 (known from the seed count, no extra sync):
    :func:`follow_flows_gpu` then :func:`get_masks_gpu`."""
    hist, pos = follow_flows_gpu(y, niter, cellprob_threshold)
    return get_masks_gpu(hist, pos, tuple(y.shape[2:]), max_size_fraction, with_bound)


def compute_masks_gpu(y: torch.Tensor, niter: int = 200, cellprob_threshold: float = 0.0, flow_threshold: float = 0.4,
                      min_size: int = 15, max_size_fraction: float = 0.4) -> torch.Tensor:
    """Full Cellpose mask recovery for a batch: y [B, 3, H, W] -> masks [B, H, W] int32."""
    M, nlab = follow_and_label(y, niter, cellprob_threshold, max_size_fraction, with_bound=True)
    if nlab <= 1:
        return M
    # Label counts, boxes and BOTH job plans (QC diffusion, hole filling) come from the raw labels,
    # read back with one host sync.  QC only drops labels: the fill then runs on the raw ids with
    # QC-dropped masks zeroed (identical geometry to renumbering first) and a lut that ranks the
    # labels kept by QC and min_size in id order (= QC renumber followed by the fill's renumber).
    counts = label_counts(M, nlab)
    bbox = mask_bboxes(M, nlab)
    fill_keep = _present_keep(counts, min_size)
    qc = flow_threshold is not None and flow_threshold > 0
    # masks below min_size are dropped whatever their flow error: the QC diffusion skips them (the
    # plan still takes cellpose's per-image niter over ALL masks, so the kept masks' flows are
    # unchanged)
    *qc_plan, fill_plan = _plan_finish(([_plan_launch(bbox, fill_keep, _diffuse_plan_kind(), counts)] if qc else [])
                                       + [_plan_launch(bbox, fill_keep, _fill_plan_kind())])
    if qc:
        _, err, _ = masks_to_flows_gpu(M, dp=y, nlab=nlab, counts=counts, plan=qc_plan[0], want_mu=False)
        qc_keep = (counts > 0) & ~(err / counts.clamp(min=1).float() > flow_threshold)
        qc_keep[:, 0] = False
        M = torch.gather(qc_keep.to(torch.int32), 1, M.reshape(M.shape[0], -1).long()).reshape(M.shape) * M
        fill_keep &= qc_keep
    out = _fill_run(M.contiguous(), _rank_lut(fill_keep), nlab, fill_plan)
    out.label_bound = nlab  # labels + 1 never exceed it: measure_masks_gpu(nlab=...) then plans without a sync
    return out


# ------------------------------------------------------------------ z-stacks


def _stitch_capacity(nlab: int, HW: int) -> int:
    """Hash slots per plane pair.  A label of plane z overlaps a handful of labels of plane z-1 (its
    own continuation plus the neighbours it grazes), so 8 slots per possible label keep the load
    factor under ~1/2; never below 1024, and never above the first power of two >= 2 * H * W (a
    pair has at most H * W distinct overlaps, so that size cannot overflow).  Always a power of two."""
    cap = 1 << max(10, (8 * max(nlab, 1) - 1).bit_length())
    return min(cap, 1 << max(1, (2 * HW - 1).bit_length()))


def stitch3d_gpu(M: torch.Tensor, stitch_threshold: float = 0.25, min_size: int = 0, nlab: int | None = None,
                 capacity: int | None = None) -> torch.Tensor:
    """Stitch per-plane label images M [Z, H, W] int32 into volumetric labels ``1..K`` (same shape and
    dtype): HIP implementation of :func:`reference.stitch3d` (``csrc/kernels/cellpose_stitch.hip``),
    exactly equal to it.  ``nlab``: optional upper bound on the labels + 1 (saves the ``M.max()``
    sync; it must be a true bound, the per-label tables are sized by it); ``capacity``: hash slots per plane pair, a power of two (default :func:`_stitch_capacity`).
    One host read (the overflow word of the overlap launch; a set word re-runs that launch with twice
    the capacity).  CPU tensors run the oracle."""
    if M.dim() != 3:
        raise ValueError(f"stitch3d_gpu expects [Z, H, W] masks, got shape {tuple(M.shape)}")
    if M.device.type != "cuda":
        out = ref.stitch3d(M.numpy(), stitch_threshold, min_size)
        return torch.from_numpy(out).to(M.dtype)
    if M.dtype != torch.int32:
        raise TypeError(f"stitch3d_gpu expects int32 masks, got {M.dtype}")
    Z, H, W = M.shape
    HW = H * W
    dev = M.device
    if Z == 0 or HW == 0:
        return torch.zeros_like(M)
    if HW >= 2 ** 31:
        raise ValueError("stitch3d_gpu: planes of 2^31 pixels or more are not supported")
    if nlab is None:
        nlab = int(M.max().item()) + 1
    nlab = max(int(nlab), 1)
    Mc = M.contiguous()
    st = _native.stream(dev)
    counts = label_counts(Mc, nlab)
    n = Z * nlab
    # one zero-filled block: bestA, bestB, vol (64-bit), then owner, link (32-bit) and the two flag words
    ws = torch.zeros(2 * n + (n + 1) + n + 1, dtype=torch.int64, device=dev)
    best_a, best_b, vol = ws[:n], ws[n: 2 * n], ws[2 * n: 3 * n + 1]
    w32 = ws[3 * n + 1:].view(torch.int32)
    owner, link, flags = w32[:n], w32[n: 2 * n], w32[2 * n: 2 * n + 2]
    if Z > 1 and nlab > 1:
        max_cap = 1 << max(1, (2 * HW - 1).bit_length())
        cap = _stitch_capacity(nlab, HW) if capacity is None else int(capacity)
        if cap < 1 or cap & (cap - 1):
            raise ValueError("capacity must be a power of two")
        while True:
            keys = torch.zeros(Z - 1, cap, dtype=torch.int64, device=dev)
            vals = torch.zeros(Z - 1, cap, dtype=torch.int32, device=dev)
            _native.call("be_cp_stitch_overlap", _native.ptr(Mc), Z, HW, nlab, _native.ptr(keys), _native.ptr(vals), cap,
                         _native.ptr(flags), st)
            if int(flags[0].item()) == 0:  # host read: did every increment find a slot?
                break
            if cap >= max_cap:
                raise RuntimeError("stitch3d_gpu: overlap table overflowed at its maximum size")
            cap *= 2  # sizing retry of a launch that completed normally; bounded by the pixel count
            flags[0] = 0
        _native.call("be_cp_stitch_match", _native.ptr(keys), _native.ptr(vals), Z, cap, _native.ptr(counts), nlab,
                     float(stitch_threshold), _native.ptr(best_a), _native.ptr(owner), _native.ptr(best_b),
                     _native.ptr(link), st)
    gid = torch.empty(Z, nlab, dtype=torch.int32, device=dev)
    lut = torch.empty(n + 1, dtype=torch.int32, device=dev)
    _native.call("be_cp_stitch_number", _native.ptr(counts), _native.ptr(link), Z, nlab, int(min_size), _native.ptr(gid),
                 _native.ptr(vol), _native.ptr(lut), _native.ptr(flags), st)
    out = torch.empty_like(Mc)
    _native.call("be_cp_stitch_relabel", _native.ptr(Mc), Z, HW, nlab, _native.ptr(gid), _native.ptr(lut), _native.ptr(out),
                 st)
    return out


# ------------------------------------------------------------------ do_3D: orthogonal views + 3-D dynamics


def _check_volume(Z: int, H: int, W: int) -> None:
    """The padded histogram is indexed with 32-bit integers."""
    if min(Z, H, W) < 0 or (Z + 2 * RPAD) * (H + 2 * RPAD) * (W + 2 * RPAD) >= 2 ** 31:
        raise ValueError(f"3-D dynamics: volume {Z} x {H} x {W} is too large ((Z+40)*(H+40)*(W+40) must be below 2^31)")


def accum_view3d(acc: torch.Tensor, y: torch.Tensor, view: int, p0: int) -> None:
    """Add one chunk of one view's network output into the accumulator ``acc`` [4, Z, H, W] fp32
    (dZ, dY, dX, cellprob), in place.  ``y`` [n, 3, h, w] are planes ``p0 .. p0 + n - 1`` of ``view``:
    0 = YX ([n, 3, H, W], planes along z; *writes* dY, dX, cellprob and zeroes dZ), 1 = ZX
    ([n, 3, Z, W], planes along y; adds dZ, dX, cellprob), 2 = ZY ([n, 3, Z, H], planes along x; adds
    dZ, dY, cellprob).  Running all YX chunks, then ZX, then ZY gives the sums of
    :func:`reference.combine_views3d` bit for bit (``be_cp_accum_view3d``)."""
    _, Z, H, W = acc.shape
    _check_volume(Z, H, W)
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.shape[0] != 4:
        raise ValueError("accum_view3d: acc must be a contiguous [4, Z, H, W] float32 tensor")
    want = ((Z, H, W), (H, Z, W), (W, Z, H))[view]
    n = y.shape[0]
    if y.dim() != 4 or y.shape[1] != 3 or tuple(y.shape[2:]) != want[1:] or p0 < 0 or p0 + n > want[0]:
        raise ValueError(f"accum_view3d: view {view} chunk of shape {tuple(y.shape)} at plane {p0} does not fit "
                         f"a {Z} x {H} x {W} volume")
    y = y.float().contiguous()
    _native.call("be_cp_accum_view3d", _native.ptr(y), int(view), int(p0), n, Z, H, W, _native.ptr(acc),
                 _native.stream(acc.device))


def combine_views3d_gpu(y_yx: torch.Tensor, y_zx: torch.Tensor, y_zy: torch.Tensor, chunk: int = 32) -> torch.Tensor:
    """The three whole view outputs -> accumulator [4, Z, H, W] (dZ, dY, dX, cellprob), fed to
    :func:`accum_view3d` in chunks of ``chunk`` planes.  CPU tensors run the oracle."""
    if y_yx.device.type != "cuda":
        dP, cp = ref.combine_views3d(y_yx.numpy(), y_zx.numpy(), y_zy.numpy())
        return torch.from_numpy(np.concatenate([dP, cp[None]]))
    Z, _, H, W = y_yx.shape
    _check_volume(Z, H, W)
    acc = torch.empty(4, Z, H, W, dtype=torch.float32, device=y_yx.device)
    for view, y in enumerate((y_yx, y_zx, y_zy)):
        for i in range(0, y.shape[0], max(1, int(chunk))):
            accum_view3d(acc, y[i: i + chunk], view, i)
    return acc


def _as_flow4(flow, cellprob=None) -> torch.Tensor:
    """``flow`` [4, Z, H, W] or (dP [3, Z, H, W], cellprob [Z, H, W]) -> contiguous fp32 [4, Z, H, W]."""
    if isinstance(flow, (tuple, list)):
        flow, cellprob = flow
    if cellprob is not None:
        flow = torch.cat([flow.float(), cellprob.float()[None]])
    if flow.dim() != 4 or flow.shape[0] != 4:
        raise ValueError(f"3-D dynamics expect a [4, Z, H, W] field (dZ, dY, dX, cellprob), got shape {tuple(flow.shape)}")
    return flow.float().contiguous()


def follow_flows3d_gpu(flow: torch.Tensor, niter: int = 200, cellprob_threshold: float = 0.0, variant: int = 0):
    """Accumulator ``flow`` [4, Z, H, W] -> ``(hist [Z+40, H+40, W+40] int32, pos [Z, H, W] int32)``:
    the histogram of the end points of :func:`reference.follow_flows3d` in the padded volume and every
    foreground voxel's padded linear bin index (-1 for background).  ``variant`` 0 = XCD-ordered,
    block-compacted launch, 1 = plain one-lane-per-voxel launch; identical results."""
    _, Z, H, W = flow.shape
    _check_volume(Z, H, W)
    dev = flow.device
    st = _native.stream(dev)
    flow4 = torch.empty(Z, H, W, 4, dtype=torch.float32, device=dev)
    fg = torch.empty(Z, H, W, dtype=torch.uint8, device=dev)
    _native.call("be_cp_prep_flow3d", _native.ptr(flow), Z, H, W, float(cellprob_threshold), _native.ptr(flow4),
                 _native.ptr(fg), st)
    hist = torch.zeros(Z + 2 * RPAD, H + 2 * RPAD, W + 2 * RPAD, dtype=torch.int32, device=dev)
    pos = torch.empty(Z, H, W, dtype=torch.int32, device=dev)
    _native.call("be_cp_follow_flows3d", _native.ptr(flow4), _native.ptr(fg), _native.ptr(hist), _native.ptr(pos), Z, H, W,
                 int(niter), int(variant), st)
    return hist, pos


def get_masks3d_gpu(hist: torch.Tensor, pos: torch.Tensor, shape=None, max_size_fraction: float = 0.4,
                    with_bound: bool = False):
    """The stages of :func:`reference.get_masks3d` after the histogram: ``hist`` [Z+40, H+40, W+40]
    int32 and ``pos`` [Z, H, W] int32 (padded linear bin of every foreground voxel, -1 elsewhere) ->
    raw labels [Z, H, W] int32 numbered ``1..k`` (before the hole fill); with ``with_bound`` also an
    upper bound on its labels + 1.  5x5x5 seeds (``be_cp_seeds3d``), ``torch.sort`` of the seed keys,
    11^3 window expansion (``be_cp_expand3d``), per-voxel lookup.  One host sync (the seed count).
    CPU tensors run the oracle."""
    Z, H, W = tuple(pos.shape) if shape is None else tuple(int(v) for v in shape)
    _check_volume(Z, H, W)
    Zp, Hp, Wp = Z + 2 * RPAD, H + 2 * RPAD, W + 2 * RPAD
    if tuple(hist.shape) != (Zp, Hp, Wp) or tuple(pos.shape) != (Z, H, W):
        raise ValueError(f"get_masks3d_gpu: hist {tuple(hist.shape)} / pos {tuple(pos.shape)} do not fit a "
                         f"{Z} x {H} x {W} volume padded by {RPAD}")
    N = Z * H * W
    if pos.device.type != "cuda":
        pn = pos.numpy()
        inds = np.nonzero(pn >= 0)
        bins = np.stack(np.unravel_index(pn[inds].astype(np.int64), (Zp, Hp, Wp))) if N else np.zeros((3, 0), np.int64)
        M = torch.from_numpy(ref.get_masks3d((bins - RPAD).astype(np.float32), inds, (Z, H, W), RPAD, max_size_fraction))
        return (M, int(M.max()) + 1 if N else 1) if with_bound else M
    dev = pos.device
    st = _native.stream(dev)
    hist = hist.to(torch.int32).contiguous()
    pos = pos.to(torch.int32).contiguous()
    M0 = torch.zeros(Z, H, W, dtype=torch.int32, device=dev)
    if N == 0:
        return (M0, 1) if with_bound else M0
    cap = N // 11 + 1  # a seed holds more than 10 of the at most N end points
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    nseeds = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call("be_cp_seeds3d", _native.ptr(hist), Zp, Hp, Wp, _native.ptr(keys), _native.ptr(nseeds), cap, st)
    k = min(int(nseeds.item()), cap)  # host sync: sizes the sort and the expansion grid
    if k == 0:
        return (M0, 1) if with_bound else M0
    keys_sorted, _ = torch.sort(keys[:k])
    M1 = torch.zeros(Zp, Hp, Wp, dtype=torch.int32, device=dev)
    _native.call("be_cp_expand3d", _native.ptr(hist), _native.ptr(keys_sorted), k, Zp, Hp, Wp, _native.ptr(M1), st)
    nlab = k + 1
    M = _lookup_labels(pos, M1, M0, 1, nlab, max_size_fraction, st)
    return (M, nlab) if with_bound else M


def follow_and_label3d(flow, niter: int = 200, cellprob_threshold: float = 0.0, max_size_fraction: float = 0.4,
                       with_bound: bool = False, variant: int = 0):
    """``flow`` [4, Z, H, W] (dZ, dY, dX, cellprob) or ``(dP [3, Z, H, W], cellprob [Z, H, W])`` -> raw
    3-D labels [Z, H, W] int32 (before the hole fill): :func:`follow_flows3d_gpu` then
    :func:`get_masks3d_gpu`.  CPU tensors run the oracle."""
    flow = _as_flow4(flow)
    _, Z, H, W = flow.shape
    _check_volume(Z, H, W)
    if flow.device.type != "cuda":
        f = flow.numpy()
        p, inds = ref.follow_flows3d(f[:3], f[3], cellprob_threshold, niter)
        M = torch.from_numpy(ref.get_masks3d(p, inds, (Z, H, W), RPAD, max_size_fraction))
        return (M, int(M.max()) + 1 if M.numel() else 1) if with_bound else M
    hist, pos = follow_flows3d_gpu(flow, niter, cellprob_threshold, variant)
    return get_masks3d_gpu(hist, pos, (Z, H, W), max_size_fraction, with_bound)


def fill_holes3d_gpu(M: torch.Tensor, min_size: int = 15, nlab: int | None = None) -> torch.Tensor:
    """:func:`reference.fill_holes_and_remove_small_masks3d` on the device: the 2-D fill kernels with
    one image per plane and a lut that keeps the ids (``lut[z, l] = l`` where label ``l`` occurs in
    plane ``z``), then the volume ``min_size`` on the per-plane counts summed over z and a renumber in
    id order.  ``nlab``: optional upper bound on the labels + 1."""
    Z, H, W = M.shape
    if M.device.type != "cuda":
        return torch.from_numpy(ref.fill_holes_and_remove_small_masks3d(M.numpy(), min_size))
    if nlab is None:
        nlab = _label_bound(M)
    if nlab <= 1 or M.numel() == 0:
        return torch.zeros_like(M)
    M = M.to(torch.int32).contiguous()
    present = _present_keep(label_counts(M, nlab), 0)
    lut = (present.int() * torch.arange(nlab, dtype=torch.int32, device=M.device)[None]).contiguous()
    plan = _plan_finish([_plan_launch(mask_bboxes(M, nlab), present, _fill_plan_kind())])[0]
    out = _fill_run(M, lut, nlab, plan)
    keep = _present_keep(label_counts(out, nlab).sum(0, keepdim=True), min_size)
    return _renumber(out, keep)


def compute_masks3d_gpu(dP, cellprob=None, niter: int = 200, cellprob_threshold: float = 0.0, min_size: int = 15,
                        max_size_fraction: float = 0.4) -> torch.Tensor:
    """3-D Cellpose mask recovery: ``dP`` [3, Z, H, W] (dZ, dY, dX) and ``cellprob`` [Z, H, W] (or one
    [4, Z, H, W] field with ``cellprob=None``) -> masks [Z, H, W] int32 numbered ``1..K``.  HIP
    implementation of :func:`reference.compute_masks3d` (``csrc/kernels/cellpose_dynamics3d.hip`` plus
    the 2-D lookup and fill kernels); no flow QC in 3-D.  CPU tensors run the oracle."""
    flow = _as_flow4(dP, cellprob)
    if flow.device.type != "cuda":
        f = flow.numpy()
        return torch.from_numpy(ref.compute_masks3d(f[:3], f[3], niter, cellprob_threshold, min_size, max_size_fraction))
    M, nlab = follow_and_label3d(flow, niter, cellprob_threshold, max_size_fraction, with_bound=True)
    if nlab <= 1:
        return M
    return fill_holes3d_gpu(M, min_size, nlab)


# ------------------------------------------------------------------ per-label measurements

MEASURE_BAND_PX = 1024  # BAND_PX of cellpose_measure.hip
_MEASURE_INT_FIELDS = ("area", "sum_z", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy", "boundary")


def _check_measure(B: int, Z: int, H: int, W: int, volume: bool) -> None:
    """The second coordinate sums are 64-bit: ``y * y * area`` stays below 2^63 up to 2^15 rows and
    columns.  Offsets inside one volume are 32-bit."""
    if volume:
        if Z * H * W >= 2 ** 31:
            raise ValueError(f"measure_masks_gpu: volume {Z} x {H} x {W} is too large (Z*H*W must be below 2^31)")
    elif max(H, W) > 2 ** 15:
        raise ValueError(f"measure_masks_gpu: image {H} x {W} is too large (H and W must not exceed 2^15)")


def _measure_oracle(M, img, K: int, volume: bool, outlines: bool) -> dict:
    """CPU tensors: :func:`reference.measure_masks` per image, rows padded to ``K``."""
    Ms = [M] if volume else list(M)
    rows = []
    for b, m in enumerate(Ms):
        im = None
        if img is not None:
            im = (img.permute(1, 0, 2, 3) if volume else img[b]).numpy()
        raw = ref.measure_masks(m.numpy(), im, outlines)
        out = {}
        for k, v in raw.items():
            t = torch.from_numpy(np.ascontiguousarray(v))
            if k != "outlines":
                t = t[:K]
                t = torch.cat([t, torch.zeros((K - t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype)])
            out[k] = t
        rows.append(out)
    return rows[0] if volume else {k: torch.stack([r[k] for r in rows]) for k in rows[0]}


def measure_masks_gpu(M: torch.Tensor, img: torch.Tensor | None = None, nlab: int | None = None, volume: bool = False,
                      outlines: bool = False) -> dict:
    """Raw per-label measurements of label images on the device: HIP implementation of
    :func:`reference.measure_masks` (``csrc/kernels/cellpose_measure.hip``), exactly equal to it in
    every integer field, box, minimum, maximum and outline, and bit-identical from run to run in
    every field.

    ``M`` [B, H, W] labels with ``img`` [B, C, H, W] or None; with ``volume=True`` ``M`` is one
    [Z, H, W] volume and ``img`` [Z, C, H, W].  Returns the oracle's fields as device tensors
    [B, K, ...] ([K, ...] for a volume; ``outlines`` [B, H, W] / [Z, H, W] bool), with ``K`` the
    largest label of the batch; rows above an image's own maximum are zero.  ``nlab``: optional
    upper bound on the labels + 1, as the sibling wrappers take it (``K = nlab - 1``; saves the
    ``M.max()`` sync -- nothing else is read back; labels above the bound are not measured).
    Runs on the current stream.  CPU tensors run the oracle."""
    if M.dim() != 3:
        raise ValueError(f"measure_masks_gpu expects [B, H, W] masks (or one [Z, H, W] volume), got {tuple(M.shape)}")
    (B, Z), (H, W) = ((1, M.shape[0]) if volume else (M.shape[0], 1)), M.shape[1:]
    _check_measure(B, Z, H, W, volume)
    C = 0
    if img is not None:
        if img.dim() != 4 or img.shape[0] != M.shape[0] or tuple(img.shape[2:]) != (H, W):
            raise ValueError(f"measure_masks_gpu: image {tuple(img.shape)} does not fit masks {tuple(M.shape)}")
        C = img.shape[1]
    dev = M.device
    if nlab is None:
        nlab = _label_bound(M)
    K = max(int(nlab) - 1, 0)
    if dev.type != "cuda":
        return _measure_oracle(M, img.float() if img is not None else None, K, volume, outlines)
    Mc = M.to(torch.int32).contiguous()
    imc = img.float().contiguous() if img is not None and C > 0 else None
    lead = () if volume else (B,)
    out_i = torch.empty(B, K, len(_MEASURE_INT_FIELDS), dtype=torch.int64, device=dev)
    out_box = torch.empty(B, K, 6, dtype=torch.int32, device=dev)
    out_f = torch.empty(B, K, C, 2, dtype=torch.float64, device=dev)
    out_m = torch.empty(B, K, C, 2, dtype=torch.float32, device=dev)
    edge = torch.zeros(Mc.shape, dtype=torch.uint8, device=dev) if outlines else None
    if K > 0 and Mc.numel() > 0:
        # job slots per image: one per label plus 2 * s_half bands (see the kernel file's header)
        s_half = 2 * (-(-Z * H * W // MEASURE_BAND_PX)) + 32
        slots = K + 2 * s_half
        # one workspace, 8-byte fields first: band size, partial integers and sums, job list, then
        # the 4-byte ones: partial min / max, boxes, offsets, band counts, job counts
        n8 = B + B * slots * (len(_MEASURE_INT_FIELDS) + 2 * C + 1)
        n4 = B * slots * 2 * C + B * K * 8 + B
        ws = torch.empty(n8 + (n4 + 1) // 2, dtype=torch.int64, device=dev)
        w8 = ws[:n8].split([B, B * slots * len(_MEASURE_INT_FIELDS), B * slots * 2 * C, B * slots])
        bandpx, part_i, part_f, jobs = w8[0], w8[1], w8[2].view(torch.float64), w8[3]
        w4 = ws[n8:].view(torch.int32)[:n4].split([B * slots * 2 * C, B * K * 6, B * K, B * K, B])
        part_m, bbox, off, nb, njobs = w4[0].view(torch.float32), w4[1], w4[2], w4[3], w4[4]
        _native.call("be_cp_measure", _native.ptr(Mc), _native.ptr(imc), B, Z, H, W, C, K, int(bool(volume)), slots, s_half,
                     _native.ptr(bbox), _native.ptr(off), _native.ptr(nb), _native.ptr(jobs), _native.ptr(njobs),
                     _native.ptr(bandpx), _native.ptr(part_i), _native.ptr(part_f), _native.ptr(part_m),
                     _native.ptr(out_i), _native.ptr(out_box), _native.ptr(out_f), _native.ptr(out_m), _native.ptr(edge),
                     _native.stream(dev))
    else:
        for t in (out_i, out_box, out_f, out_m):
            t.zero_()
    res = {}
    for j, name in enumerate(_MEASURE_INT_FIELDS):
        if name in (("sum_yy", "sum_xx", "sum_xy") if volume else ("sum_z",)):
            continue
        res[name] = out_i[..., j].reshape(lead + (K,))
    res["bbox"] = (out_box if volume else out_box[..., [1, 2, 4, 5]]).reshape(lead + (K, 6 if volume else 4))
    if img is not None:
        res["int_sum"], res["int_sumsq"] = (out_f[..., j].reshape(lead + (K, C)) for j in (0, 1))
        res["int_min"], res["int_max"] = (out_m[..., j].reshape(lead + (K, C)) for j in (0, 1))
    if outlines:
        res["outlines"] = edge.bool()
    return res


# ------------------------------------------------------------------ outlines: polygon rings


def _check_rings(B: int, H: int, W: int) -> None:
    """Vertex coordinates and the ``area2`` terms ``x * y`` stay far inside their types up to 2^15
    rows and columns; the corner pass indexes the batch's ``B (H + 1)(W + 1)`` corners in 32 bits."""
    if max(H, W) > 2 ** 15:
        raise ValueError(f"mask_rings_gpu: image {H} x {W} is too large (H and W must not exceed 2^15)")
    if B * (H + 1) * (W + 1) >= 2 ** 31:
        raise ValueError(f"mask_rings_gpu: batch {B} x {H} x {W} is too large (B*(H+1)*(W+1) must be below 2^31)")


def _rings_result(verts, off, lab, area2, img, per_image) -> dict:
    return {"verts": verts, "ring_offsets": off, "ring_label": lab, "ring_area2": area2, "ring_image": img,
            "image_rings": per_image}


def _rings_empty(B: int, dev) -> dict:
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    return _rings_result(z((0, 2), torch.int32), z(1, torch.int64), z(0, torch.int32), z(0, torch.int64),
                         z(0, torch.int32), z(B + 1, torch.int64))


def _rings_oracle(M: torch.Tensor, K: int) -> dict:
    """CPU tensors: :func:`reference.mask_rings` per image, joined into the batch's arrays."""
    parts, nv, counts = [], 0, [0]
    for b, m in enumerate(M.numpy()):
        r = ref.mask_rings(np.where(m > K, 0, m))
        n = r["ring_label"].shape[0]
        parts.append((r["verts"], r["ring_offsets"][:-1] + nv, r["ring_label"], r["ring_area2"], np.full(n, b, np.int32)))
        nv += r["verts"].shape[0]
        counts.append(counts[-1] + n)
    v, off, lab, a2, img = (np.concatenate([p[j] for p in parts]) for j in range(5))
    off = np.concatenate([off, [nv]]).astype(np.int64)
    return _rings_result(*(torch.from_numpy(np.ascontiguousarray(x)) for x in (v, off, lab, a2, img)),
                         torch.tensor(counts, dtype=torch.int64))


def _host_ints(t: torch.Tensor) -> list:
    """One device-to-host read of a small integer tensor (waits for the current stream)."""
    return [int(v) for v in t.tolist()]


def mask_rings_gpu(M: torch.Tensor, nlab: int | None = None, volume: bool = False) -> dict:
    """Outlines of label images as closed rings of pixel-corner coordinates, traced on the device:
    HIP implementation of :func:`reference.mask_rings` (``csrc/kernels/cellpose_rings.hip``), equal
    to it in every array and bit-identical from run to run.

    ``M`` [B, H, W] labels; with ``volume=True`` ``M`` is one [Z, H, W] volume read as Z planes:
    outlines are per plane, with the volume's labels.  Returns device tensors for the whole batch:
    the oracle's ``verts`` int32 [V, 2] (y, x), ``ring_offsets`` int64 [R + 1], ``ring_label`` int32
    [R] and ``ring_area2`` int64 [R], plus ``ring_image`` int32 [R] (the image, or z) and
    ``image_rings`` int64 [B + 1] (image ``b`` owns rings ``image_rings[b]:image_rings[b + 1]``);
    rings are ordered by (image, label, start).  ``nlab``: optional upper bound on the labels + 1, as
    the sibling wrappers take it (saves the ``M.max()`` sync; labels above the bound are not
    traced).  Two values are read back, ``V`` after the count and ``R`` (with the error word) after
    the trace; an empty batch, ``K = 0`` and ``V = 0`` return before the reads they do not need.
    Raises ``RuntimeError`` when a walk ran out of its counted edges, vertices or ring slots (labels
    that changed under the kernel).  Runs on the current stream.  CPU tensors run the oracle."""
    if M.dim() != 3:
        raise ValueError(f"mask_rings_gpu expects [B, H, W] masks (or one [Z, H, W] volume), got {tuple(M.shape)}")
    B, H, W = M.shape
    _check_rings(B, H, W)
    dev = M.device
    if M.numel() == 0:
        return _rings_empty(B, dev)
    if nlab is None:
        nlab = int(M.max().item()) + 1
    K = max(int(nlab) - 1, 0)
    if K == 0:
        return _rings_empty(B, dev)
    if dev.type != "cuda":
        return _rings_oracle(M, K)
    Mc = M.to(torch.int32).contiguous()
    n = B * K
    # per label: corner box, vertices, rings | its segments of verts and of the ring table, its first
    # ring in the result, then the totals (V, ring table size, R, error word)
    w32 = torch.empty(6 * n, dtype=torch.int32, device=dev)
    bbox, nvert, nrings = w32[:4 * n], w32[4 * n:5 * n], w32[5 * n:]
    w64 = torch.empty(3 * n + 4, dtype=torch.int64, device=dev)
    voff, roff, rstart, totals = w64[:n], w64[n:2 * n], w64[2 * n:3 * n], w64[3 * n:]
    sp = _native.stream(dev)
    _native.call("be_cp_rings_count", _native.ptr(Mc), B, H, W, K, _native.ptr(bbox), _native.ptr(nvert), _native.ptr(voff),
                 _native.ptr(roff), _native.ptr(totals), sp)
    V, = _host_ints(totals[:1])
    if V == 0:
        return _rings_empty(B, dev)
    cap = V // 4  # a ring has at least 4 vertices
    verts = torch.empty(V, 2, dtype=torch.int32, device=dev)
    o64 = torch.empty(4 * cap + 1 + B + 1, dtype=torch.int64, device=dev)
    first, tab_a2, off, area2, per_image = o64.split([cap, cap, cap + 1, cap, B + 1])
    o32 = torch.empty(2 * cap, dtype=torch.int32, device=dev)
    nz = (B * H * W + 3) // 4 * 4  # "top edge traced" marks of the boxes beyond 64 x 64, then the error word
    zeroed = torch.zeros(nz + 4, dtype=torch.uint8, device=dev)
    err = zeroed[nz:].view(torch.int32)
    _native.call("be_cp_rings_trace", _native.ptr(Mc), B, H, W, K, _native.ptr(bbox), _native.ptr(nvert), _native.ptr(voff),
                 _native.ptr(roff), _native.ptr(zeroed), _native.ptr(verts), _native.ptr(first), _native.ptr(tab_a2),
                 _native.ptr(nrings), _native.ptr(rstart), _native.ptr(err), _native.ptr(totals), _native.ptr(off),
                 _native.ptr(area2), _native.ptr(o32[:cap]), _native.ptr(o32[cap:]), _native.ptr(per_image), sp)
    R, e = _host_ints(totals[2:])
    if e:
        raise RuntimeError(f"be_cp_rings_trace: a walk left its counted bounds (error word {e}): the labels changed "
                           "while they were traced")
    return _rings_result(verts, off[:R + 1], o32[:R], area2[:R], o32[cap:cap + R], per_image)


# ------------------------------------------------------------------ label surfaces: quad meshes of a volume

SURF_TILE = 256  # corners per workgroup: TILE of label_surface.hip
SURF_SLICES = 8  # workgroups per label of its statistics kernels: SL

_SURF_KEYS = ("corner", "verts", "vert_label", "quads", "quad_label", "label_verts", "label_quads", "faces", "voxels")


def _check_surface(Z: int, H: int, W: int) -> None:
    """Corner coordinates stay inside 16 bits and the corner lattice is indexed in 32 bits."""
    if max(Z, H, W) > 2 ** 15:
        raise ValueError(f"label_surface_gpu: volume {Z} x {H} x {W} is too large (no axis may exceed 2^15)")
    if (Z + 1) * (H + 1) * (W + 1) >= 2 ** 31:
        raise ValueError(f"label_surface_gpu: volume {Z} x {H} x {W} is too large ((Z+1)(H+1)(W+1) must be below 2^31)")


def _surface_empty(K: int, dev) -> dict:
    return {k: torch.from_numpy(v).to(dev) for k, v in ref._empty_surface(K).items()}


def label_surface_gpu(L: torch.Tensor, nlab: int | None = None) -> dict:
    """The surface of every label of a volume as an indexed quad mesh, built on the device: HIP
    implementation of :func:`reference.label_surface` (``csrc/kernels/label_surface.hip``), equal to it
    in every array and bit-identical from run to run.

    ``L`` [Z, H, W] integer labels (any integer dtype, any strides).  Returns the oracle's dict as
    device tensors: ``corner`` int32 [V, 3], ``verts`` float32 [V, 3], ``vert_label`` int32 [V],
    ``quads`` int32 [F, 4], ``quad_label`` int32 [F], ``label_verts`` / ``label_quads`` int64 [K + 1],
    ``faces`` int64 [K, 3], ``voxels`` int64 [K].  ``nlab``: an upper bound on the labels + 1 (saves the
    ``L.max()`` sync; labels above it are not meshed but still bound their neighbours).  The kernels
    read int32: labels of a wider dtype are clamped to [-1, 2^31 - 1] first, which changes no result
    (values outside ``1..K`` only bound their neighbours), and ``K`` must stay below 2^31 - 1
    (``ValueError``).

    A corner pass counts vertices and quads per tile of 256 corners, a prefix sum over the tiles gives
    every tile its offset, a second pass writes the (corner, label) keys at offset + rank, a stable
    sort of the label keys regroups them by label, and gather passes write the mesh, the label
    offsets, the face counts and the voxel counts.  The host reads ``V`` and ``F`` after the count
    (``V`` or ``F`` >= 2^31 raises ``RuntimeError`` before any allocation) and the error word at the
    end: ``RuntimeError`` when the second pass did not find what the first counted (labels that
    changed under the kernel).  An empty volume or ``K = 0`` returns empty arrays with no launch and
    no read.  Runs on the current stream.  CPU tensors run the oracle."""
    if L.dim() != 3:
        raise ValueError(f"label_surface_gpu expects a [Z, H, W] label volume, got {tuple(L.shape)}")
    if L.dtype.is_floating_point or L.dtype.is_complex:
        raise ValueError(f"label_surface_gpu expects integer labels, got {L.dtype}")
    Z, H, W = L.shape
    _check_surface(Z, H, W)
    if nlab is not None and int(nlab) - 1 >= 2 ** 31 - 1:
        raise ValueError(f"label_surface_gpu: nlab {nlab} is too large (labels to mesh must stay below 2^31 - 1)")
    dev = L.device
    if L.numel() == 0 or (nlab is not None and int(nlab) <= 1):
        return _surface_empty(max(int(nlab or 1) - 1, 0), dev)
    if dev.type != "cuda":
        return {k: torch.from_numpy(v) for k, v in ref.label_surface(L.numpy(), nlab).items()}
    if L.dtype in (torch.int64, torch.uint32, torch.uint64):
        # a plain conversion would wrap 2^32 + 1 into label 1; every value outside 1..K is equivalent
        L = L.to(torch.int64).clamp_(-1, 2 ** 31 - 1)
    Lc = L.to(torch.int32).contiguous()
    if nlab is None:
        nlab = int(Lc.max().item()) + 1
        if nlab - 1 >= 2 ** 31 - 1:
            raise ValueError("label_surface_gpu: labels to mesh must stay below 2^31 - 1")
    K = max(int(nlab) - 1, 0)
    if K == 0:
        return _surface_empty(0, dev)
    sp = _native.stream(dev)
    ptr = _native.ptr
    nt = -(-(Z + 1) * (H + 1) * (W + 1) // SURF_TILE)
    tile_cnt = torch.empty(2, nt, dtype=torch.int32, device=dev)
    _native.call("be_surf_count", ptr(Lc), Z, H, W, K, ptr(tile_cnt), sp)
    tile_inc = torch.cumsum(tile_cnt, 1, dtype=torch.int64)  # along the contiguous axis
    V, F = _host_ints(tile_inc[:, -1])
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise RuntimeError(f"label_surface_gpu: {V} vertices and {F} quads do not fit 32-bit indices")
    if V == 0 or F == 0:
        return _surface_empty(K, dev)
    k32 = torch.empty(2 * V + 2 * F, dtype=torch.int32, device=dev)
    vcorner, vlabel, qcorner, qlabel = k32.split([V, V, F, F])
    qside = torch.empty(F, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call("be_surf_emit", ptr(Lc), Z, H, W, K, ptr(tile_inc), V, F, ptr(vcorner), ptr(vlabel), ptr(qcorner),
                 ptr(qside), ptr(qlabel), ptr(err), sp)
    vlab, vperm = torch.sort(vlabel, stable=True)
    qlab, qperm = torch.sort(qlabel, stable=True)
    o64 = torch.empty(2 * (K + 1), dtype=torch.int64, device=dev)
    label_verts, label_quads = o64[:K + 1], o64[K + 1:]
    corner = torch.empty(V, 3, dtype=torch.int32, device=dev)
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    vkey = torch.empty(V, dtype=torch.int32, device=dev)
    quads = torch.empty(F, 4, dtype=torch.int32, device=dev)
    _native.call("be_surf_gather", ptr(Lc), Z, H, W, K, V, F, ptr(vperm), ptr(vcorner), ptr(vlab), ptr(qlab),
                 ptr(label_verts), ptr(label_quads), ptr(corner), ptr(verts), ptr(vkey), ptr(err), sp)
    _native.call("be_surf_remap", Z, H, W, K, V, F, ptr(qperm), ptr(qcorner), ptr(qside), ptr(qlab), ptr(label_verts),
                 ptr(vkey), ptr(quads), ptr(err), sp)
    counts = torch.zeros(4 * K, dtype=torch.int64, device=dev)
    faces, voxels = counts[:3 * K].view(K, 3), counts[3 * K:]
    _native.call("be_surf_faces", Z, H, W, K, F, ptr(qperm), ptr(qcorner), ptr(qside), ptr(label_quads), ptr(faces),
                 ptr(voxels), sp)
    e, = _host_ints(err)
    if e:
        raise RuntimeError(f"label_surface_gpu: the second pass did not find what the first counted (error word {e}): "
                           "the labels changed while they were meshed")
    return {"corner": corner, "verts": verts, "vert_label": vlab, "quads": quads, "quad_label": qlab,
            "label_verts": label_verts, "label_quads": label_quads, "faces": faces, "voxels": voxels}


def surface_stats_gpu(surf: dict, spacing=(1.0, 1.0, 1.0)) -> dict:
    """Per-label surface measurements of a :func:`label_surface_gpu` mesh: the table of
    :func:`reference.surface_stats` (``label``, ``area_voxel``, ``area``, ``mesh_volume``, ``volume``,
    ``sphericity``, ``n_verts``, ``n_quads``; float64 tensors [K]) on the mesh's device.  ``area`` and
    ``mesh_volume`` are summed by ``be_surf_stats`` in fp64 over fixed chunks of every label's quads,
    combined in chunk order (no float atomics: bit-identical from run to run).  Nothing is read back.
    CPU tensors (or arrays) run the oracle."""
    sz, sy, sx = ref._check_spacing(spacing, "surface_stats_gpu")
    faces = surf["faces"]
    if not torch.is_tensor(faces) or faces.device.type != "cuda":
        host = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in surf.items()}
        return {k: torch.from_numpy(v) for k, v in ref.surface_stats(host, (sz, sy, sx)).items()}
    dev = faces.device
    K = faces.shape[0]
    V, F = surf["verts"].shape[0], surf["quads"].shape[0]
    out = torch.zeros(K, 2, dtype=torch.float64, device=dev)
    if K and V and F:
        part = torch.empty(K, SURF_SLICES, 2, dtype=torch.float64, device=dev)
        _native.call("be_surf_stats", K, V, F, _native.ptr(surf["verts"].contiguous()),
                     _native.ptr(surf["quads"].contiguous()), _native.ptr(surf["label_quads"].contiguous()), sz, sy, sx,
                     _native.ptr(part), _native.ptr(out), _native.stream(dev))
    f = faces.double()
    area = out[:, 0]
    volume = surf["voxels"].double() * (sz * sy * sx)
    sph = torch.where(area > 0, math.pi ** (1.0 / 3.0) * (6.0 * volume) ** (2.0 / 3.0) / area,
                      torch.full_like(area, float("nan")))
    return {"label": torch.arange(1, K + 1, dtype=torch.float64, device=dev),
            "area_voxel": f[:, 0] * sy * sx + f[:, 1] * sz * sx + f[:, 2] * sz * sy,
            "area": area, "mesh_volume": out[:, 1], "volume": volume, "sphericity": sph,
            "n_verts": surf["label_verts"].diff().double(), "n_quads": surf["label_quads"].diff().double()}


# ------------------------------------------------------------------ polygons -> labels

RASTER_BAND = 64    # rows of a job of cellpose_raster.hip: one per lane
RASTER_CHUNK = 256  # columns of a job: 64 * CW of cellpose_raster.hip


def _host_array(x) -> np.ndarray:
    """A polygons-dict array on the host.  A device tensor is copied there, which waits for the
    current stream: that serves round trips from :func:`mask_rings_gpu` only."""
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _raster_inputs(polys: dict, B: int, H: int, W: int):
    """Every check of :func:`rasterize_rings_gpu`, on the host: the quantised vertices int64 [V, 2],
    the ring offsets, labels and images (int64 [R])."""
    B, H, W = int(B), int(H), int(W)
    if min(B, H, W) < 0:
        raise ValueError(f"rasterize_rings_gpu: negative size {B} x {H} x {W}")
    if max(H, W) > 2 ** 15:
        raise ValueError(f"rasterize_rings_gpu: image {H} x {W} is too large (H and W must not exceed 2^15)")
    if B * H * W >= 2 ** 31:
        raise ValueError(f"rasterize_rings_gpu: batch {B} x {H} x {W} is too large (B*H*W must be below 2^31)")
    host = {k: _host_array(polys[k]) for k in ("verts", "ring_offsets", "ring_label")}
    q, off, labs = ref.polygon_arrays(host, "rasterize_rings_gpu")
    R = labs.shape[0]
    if q.shape[0] >= 2 ** 31:
        raise ValueError("rasterize_rings_gpu: 2^31 vertices or more are not supported")
    if polys.get("ring_image") is not None:
        img = _host_array(polys["ring_image"]).astype(np.int64).reshape(-1)
        if img.shape[0] != R:
            raise ValueError(f"rasterize_rings_gpu: ring_image has {img.shape[0]} entries for {R} rings")
    elif polys.get("image_rings") is not None:
        per = _host_array(polys["image_rings"]).astype(np.int64).reshape(-1)
        if per.shape[0] != B + 1 or per[0] != 0 or per[-1] != R or (np.diff(per) < 0).any():
            raise ValueError(f"rasterize_rings_gpu: image_rings does not fit {B} images and {R} rings")
        img = np.repeat(np.arange(B, dtype=np.int64), np.diff(per))
    else:
        raise ValueError("rasterize_rings_gpu: a batch of polygons needs ring_image [R] or image_rings [B + 1]")
    if R and (img.min() < 0 or img.max() >= B):
        raise ValueError(f"rasterize_rings_gpu: ring_image must lie in [0, {B}), got {int(img.min())} .. {int(img.max())}")
    return q, off, labs, img


def _raster_plan(q, off, labs, img, H: int, W: int):
    """The edge list and the job table of ``csrc/kernels/cellpose_raster.hip``, in vectorised numpy.

    Rings are sorted by (image, label), so that a *group* -- one label of one image -- is a
    contiguous run of edges int32 [E, 4] (Y0, X0, Y1, X1).  A group's pixel box holds the rows and
    columns whose centre lies inside its vertex range (no pixel outside it can be inside the
    polygon), clipped to the image; a job int32 [8] is (first edge, edges, image, label, first row,
    rows <= 64, first column, columns <= 256).  Returns ``(edges, jobs)``, or None without jobs."""
    n = np.diff(off)
    order = np.lexsort((labs, img))
    order = order[n[order] > 0]
    if order.size == 0:
        return None
    cnt, start = n[order], off[:-1][order]
    eoff = np.concatenate([[0], np.cumsum(cnt)])
    if (np.diff(order) > 0).all():  # already in (image, label) order, the usual case: the vertices stay where they are
        src = q
    else:
        ring = np.repeat(np.arange(order.size), cnt)
        src = q[np.arange(eoff[-1]) + (start - eoff[:-1])[ring]]
    # edge i runs from vertex i to vertex i + 1, the last one of a ring back to the ring's first
    edges = np.empty((int(eoff[-1]), 4), np.int32)
    edges[:, :2] = src
    edges[:-1, 2:] = src[1:]
    edges[eoff[1:] - 1, 2:] = src[eoff[:-1]]
    gi, gl = img[order], labs[order]
    first = np.flatnonzero(np.concatenate([[True], (gi[1:] != gi[:-1]) | (gl[1:] != gl[:-1])]))
    e0 = eoff[first]
    ne = np.diff(np.concatenate([e0, eoff[-1:]]))
    lo = np.stack([np.minimum.reduceat(edges[:, c], e0) for c in (0, 1)], 1).astype(np.int64)
    hi = np.stack([np.maximum.reduceat(edges[:, c], e0) for c in (0, 1)], 1).astype(np.int64)
    half, sub = ref.RASTER_SUBPIX // 2, ref.RASTER_SUBPIX
    p0 = np.maximum(-((half - lo) // sub), 0)                 # first centre at or beyond the minimum
    p1 = np.minimum(-((half - hi) // sub) - 1, (H - 1, W - 1))  # last centre before the maximum
    ok = (p0 <= p1).all(1)
    nb = np.where(ok, (p1[:, 0] - p0[:, 0]) // RASTER_BAND + 1, 0)
    nc = np.where(ok, (p1[:, 1] - p0[:, 1]) // RASTER_CHUNK + 1, 0)
    nj = nb * nc
    J = int(nj.sum())
    if J == 0:
        return None
    if J >= 2 ** 31:
        raise ValueError(f"rasterize_rings_gpu: {J} jobs are too many for one launch")
    g = np.repeat(np.arange(first.size), nj)
    k = np.arange(J) - (np.cumsum(nj) - nj)[g]
    y0 = p0[g, 0] + RASTER_BAND * (k // nc[g])
    x0 = p0[g, 1] + RASTER_CHUNK * (k % nc[g])
    jobs = np.stack([e0[g], ne[g], gi[first][g], gl[first][g], y0, np.minimum(p1[g, 0] - y0 + 1, RASTER_BAND),
                     x0, np.minimum(p1[g, 1] - x0 + 1, RASTER_CHUNK)], 1).astype(np.int32)
    return edges, jobs


def _raster_oracle(q, off, labs, img, B: int, H: int, W: int) -> np.ndarray:
    out = np.zeros((B, H, W), np.int32)
    n = np.diff(off)
    for b in np.unique(img).tolist():
        rs = np.flatnonzero(img == b)
        # the quantised vertices go back as exact multiples of 1 / 256: quantising them again is the identity
        verts = np.concatenate([q[off[r]:off[r + 1]] for r in rs]).astype(np.float64) / ref.RASTER_SUBPIX
        out[b] = ref.rasterize_rings({"verts": verts, "ring_offsets": np.concatenate([[0], np.cumsum(n[rs])]),
                                      "ring_label": labs[rs]}, (H, W))
    return out


def rasterize_rings_gpu(polys: dict, B: int, H: int, W: int, device) -> torch.Tensor:
    """Label images of a batch of polygons, rasterised on the device: HIP implementation of
    :func:`reference.rasterize_rings` (``csrc/kernels/cellpose_raster.hip``), equal to it in every
    pixel, bit-identical from run to run and independent of the launch geometry.

    ``polys``: a polygons dict for the whole batch -- ``verts`` [V, 2] (y, x) of any integer or float
    dtype, ``ring_offsets`` int64 [R + 1], ``ring_label`` int32 [R], and either ``ring_image`` int32
    [R] or ``image_rings`` int64 [B + 1], as :func:`mask_rings_gpu` returns them.  The arrays are
    host arrays; device tensors are copied to the host first, which waits for the current stream
    (that serves the round trip from :func:`mask_rings_gpu` only).  Returns int32 [B, H, W] on
    ``device`` with ``label_bound`` (the largest label + 1, known on the host) set on the tensor, as
    :func:`compute_masks_gpu` sets it.

    Everything is checked on the host before any launch: the oracle's checks (offsets, positive
    labels, finite coordinates inside [-32768, 65536] px), ``H, W <= 2^15``, ``B*H*W < 2^31``,
    ``ring_image`` in ``[0, B)``.  The host also quantises the vertices, sorts the rings by (image,
    label) and builds the job table (:func:`_raster_plan`); the device only ever sees integers.  An
    empty batch, no rings, no vertices and polygons that contain no centre launch nothing and
    return zeros.  Nothing is read back from the device and nothing is waited for; the kernel runs
    on the current stream.  A CPU ``device`` runs the oracle per image."""
    B, H, W = int(B), int(H), int(W)
    q, off, labs, img = _raster_inputs(polys, B, H, W)
    dev = torch.device(device)
    bound = int(labs.max()) + 1 if labs.size else 1
    if dev.type != "cuda":
        out = torch.from_numpy(_raster_oracle(q, off, labs, img, B, H, W))
        out.label_bound = bound
        return out
    out = torch.zeros((B, H, W), dtype=torch.int32, device=dev)
    out.label_bound = bound
    plan = _raster_plan(q, off, labs, img, H, W) if B * H * W and q.shape[0] else None
    if plan is None:
        return out
    edges, jobs = plan
    E, J = edges.shape[0], jobs.shape[0]
    with torch.cuda.device(dev):
        # one upload: the edges (16 bytes each), then the jobs (32 bytes each, 16-byte aligned)
        buf = torch.from_numpy(np.concatenate([edges.reshape(-1), jobs.reshape(-1)])).to(dev, non_blocking=True)
        _native.call("be_cp_raster", _native.ptr(buf[:4 * E]), E, _native.ptr(buf[4 * E:]), J, _native.ptr(out), B, H, W,
                     _native.stream(dev))
    return out


# ------------------------------------------------------------------ evaluation: average precision

AP_MAX_THRESHOLDS = 8  # MAX_THR of cellpose_ap.hip
_ap_thr: dict = {}  # (ascending thresholds, device) -> their fp64 device array


def _ap_capacity(nt: int, np_: int, N: int) -> int:
    """Hash slots per image pair.  The table holds every distinct (true, predicted) pair of an image,
    background sides included: each label meets the background and a handful of labels of the other
    image, so 8 slots per possible label keep the load factor under ~1/2; never below 1024, never
    above the first power of two >= 2 * N (an image has at most N distinct pairs)."""
    cap = 1 << max(10, (8 * max(nt + np_, 1) - 1).bit_length())
    return min(cap, 1 << max(1, (2 * N - 1).bit_length()))


def _ap_thresholds(thresholds) -> list:
    ths = [thresholds] if np.isscalar(thresholds) else list(thresholds)
    if len(ths) > AP_MAX_THRESHOLDS:
        raise ValueError(f"average_precision_gpu takes at most {AP_MAX_THRESHOLDS} thresholds, got {len(ths)}")
    for th in ths:
        if not 0.0 < float(th) <= 1.0:
            raise ValueError(f"average_precision_gpu: thresholds must be in (0, 1], got {th}")
    return ths


def _ap_host_match(t: np.ndarray, p: np.ndarray, nt: int, np_: int) -> int:
    """Maximum-cardinality matching of the edge list (t, p): the oracle's true positives."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching

    if t.size == 0:
        return 0
    g = csr_matrix((np.ones(t.size, np.int8), (t, p)), shape=(nt, np_))
    return int((maximum_bipartite_matching(g, perm_type="column") >= 0).sum())


def average_precision_gpu(T: torch.Tensor, P: torch.Tensor, thresholds=(0.5, 0.75, 0.9), nt: int | None = None,
                          np_: int | None = None, capacity: int | None = None, info: dict | None = None):
    """Average precision of predicted labels ``P`` against true labels ``T`` ([B, ...] integer label
    images or volumes of one shape): HIP implementation of :func:`metrics.average_precision`
    (``csrc/kernels/cellpose_ap.hip``), exactly equal to it.  Returns ``(ap, tp, fp, fn)`` as numpy
    arrays [B, K] (float32, int64, int64, int64).

    The oracle's true positives are the maximum matching of the graph ``{(t, p): iou >= th}``; where
    no label has two edges that is the edge count, which the device returns.  Only a conflicted
    (image, threshold) cell sends that image's compact edge list to the host for
    ``scipy.sparse.csgraph.maximum_bipartite_matching`` (possible at ``th <= 0.5`` only).

    ``nt`` / ``np_``: optional upper bounds on the labels + 1 of ``T`` / ``P`` (save the ``max()`` sync;
    they must be true bounds: a label outside them raises ``ValueError``); ``capacity``: hash slots per
    image, a power of two (default :func:`_ap_capacity`; an overflowing table is retried at twice the
    size).  One host read per call when bounds are given and there is no overflow or conflict.
    ``info`` (a dict) receives ``host_matched``, the number of (image, threshold) cells solved on the
    host, and the final ``capacity``.  Thresholds are sorted for the device and the results put back
    in the caller's order.  CPU tensors run the oracle."""
    from . import metrics

    if not (torch.is_tensor(T) and torch.is_tensor(P)):
        raise TypeError("average_precision_gpu expects tensors")
    if tuple(T.shape) != tuple(P.shape):
        raise ValueError(f"average_precision_gpu: shapes differ, {tuple(T.shape)} and {tuple(P.shape)}")
    if T.dim() < 2:
        raise ValueError(f"average_precision_gpu expects [B, ...] labels, got shape {tuple(T.shape)}")
    ths = _ap_thresholds(thresholds)
    for m in (T, P):
        if m.dtype.is_floating_point or m.dtype.is_complex or m.dtype == torch.bool:
            raise TypeError(f"average_precision_gpu expects integer labels, got {m.dtype}")
    B, K = T.shape[0], len(ths)
    if info is not None:
        info.update(host_matched=0, capacity=0)
    if T.device.type != "cuda" or P.device.type != "cuda":
        ap, tp, fp, fn = metrics.average_precision([m.cpu().numpy() for m in T], [m.cpu().numpy() for m in P], ths)
        return ap, tp, fp, fn
    dev = T.device
    N = T[0].numel() if B else 0
    if N >= 2 ** 31:
        raise ValueError("average_precision_gpu: images of 2^31 pixels or more are not supported")
    if B > 65535:
        raise ValueError("average_precision_gpu: at most 65535 images per call")
    order = np.argsort(np.asarray(ths, np.float64), kind="stable")
    sorted_ths = [float(ths[j]) for j in order]
    tp_s = np.zeros((B, K), np.int64)
    n_true = np.zeros(B, np.int64)
    n_pred = np.zeros(B, np.int64)
    if B > 0 and N > 0 and K > 0:
        Tc = T.reshape(B, N).to(torch.int32).contiguous()
        Pc = P.reshape(B, N).to(torch.int32).contiguous()
        missing = [m for m, bound in ((Tc, nt), (Pc, np_)) if bound is None]
        if missing:
            mx = torch.stack([m.max() for m in missing]).tolist()  # one sync for the bounds not given
            nt = mx.pop(0) + 1 if nt is None else nt
            np_ = mx.pop(0) + 1 if np_ is None else np_
        nt, np_ = max(int(nt), 1), max(int(np_), 1)
        max_cap = 1 << max(1, (2 * N - 1).bit_length())
        cap = _ap_capacity(nt, np_, N) if capacity is None else int(capacity)
        if cap < 1 or cap & (cap - 1):
            raise ValueError("capacity must be a power of two")
        st = _native.stream(dev)
        thr = _ap_thr.get((tuple(sorted_ths), dev))  # the same few threshold sets come again and again
        if thr is None:
            if len(_ap_thr) >= 64:
                _ap_thr.clear()
            thr = _ap_thr[(tuple(sorted_ths), dev)] = torch.tensor(sorted_ths, dtype=torch.float64, device=dev)
        M = AP_MAX_THRESHOLDS
        nwords = 2 + 2 * B * M + 2 * B  # flags, edges, conflict, n_true, n_pred: read back in one copy
        while True:
            # one zero-filled block: keys (64-bit), then the result words, vals, level, areas, degrees
            sizes = [nwords, B * cap, B * cap, B * nt, B * np_, B * K * nt, B * K * np_]
            ws = torch.zeros(B * cap + (sum(sizes) + 1) // 2, dtype=torch.int64, device=dev)
            keys = ws[: B * cap]
            words, vals, level, area_t, area_p, deg_t, deg_p = ws[B * cap:].view(torch.int32)[: sum(sizes)].split(sizes)
            flags, edges, conflict, ntrue, npred = words.split([2, B * M, B * M, B, B])
            _native.call("be_cp_ap_overlap", _native.ptr(Tc), _native.ptr(Pc), B, N, nt, np_, _native.ptr(keys),
                         _native.ptr(vals), cap, _native.ptr(flags), st)
            _native.call("be_cp_ap_match", _native.ptr(keys), _native.ptr(vals), B, cap, nt, np_, _native.ptr(thr), K,
                         _native.ptr(area_t), _native.ptr(area_p), _native.ptr(edges), _native.ptr(conflict),
                         _native.ptr(deg_t), _native.ptr(deg_p), _native.ptr(ntrue), _native.ptr(npred),
                         _native.ptr(level), st)
            host = words.cpu().numpy()  # the host read: every small result word in one copy
            if host[1]:
                raise ValueError(f"average_precision_gpu: a label lies outside its bound (nt={nt}, np_={np_})")
            if host[0] == 0:
                break
            if cap >= max_cap:
                raise RuntimeError("average_precision_gpu: overlap table overflowed at its maximum size")
            cap *= 2  # sizing retry of launches that completed normally; bounded by the pixel count
        h_edges = host[2: 2 + B * M].reshape(B, M)[:, :K]
        h_conf = host[2 + B * M: 2 + 2 * B * M].reshape(B, M)[:, :K]
        n_true[:] = host[2 + 2 * B * M: 2 + 2 * B * M + B]
        n_pred[:] = host[2 + 2 * B * M + B:]
        tp_s[:] = h_edges
        hosted = 0
        for b in np.nonzero(h_conf.any(1))[0]:
            # this image's edge list (t, p, level), compacted on the device
            slot = torch.nonzero(level[b * cap: (b + 1) * cap]).reshape(-1)
            kb = keys[b * cap: (b + 1) * cap][slot]
            el = torch.stack([kb >> 32, kb & 0xFFFFFFFF, level[b * cap: (b + 1) * cap][slot].long()]).cpu().numpy()
            for k in np.nonzero(h_conf[b])[0]:
                sel = el[2] > k
                tp_s[b, k] = _ap_host_match(el[0][sel], el[1][sel], nt, np_)
                hosted += 1
        if info is not None:
            info.update(host_matched=hosted, capacity=cap)
    tp = np.zeros((B, K), np.int64)
    tp[:, order] = tp_s
    return metrics.ap_from_counts(tp, n_true, n_pred)
