"""End-to-end Cellpose inference: normalise -> (rescale) -> tile -> CPnet -> blend -> masks.

``CellposeRunner.eval`` mirrors the call the reference apps make on ``cellpose.models.CellposeModel``
(``model.eval(images, diameter, flow_threshold, cellprob_threshold, niter, min_size, ...)``;
``apps/cellpose-finetuning/main.py:4965-5052`` and ``:3559-3567``) but runs a whole *batch* of images
through one set of kernel launches: the tiles of every image in the batch are one CPnet batch,
blending and mask recovery are batched kernels.  This is what the continuous-batching router feeds.

GPU path: HIP kernels (:mod:`.gpu`, :class:`~bioengine_worker_amd.models.cpnet.CPnetEngine`).
CPU path: the numpy/torch oracle (:mod:`.reference`) — used by CPU tests and CPU-only workers.
"""
from __future__ import annotations

import dataclasses
import math
import os
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from ..models.cpnet import CPnet, CPnetEngine
from ..ops.resize import resize_bilinear
from ..profiling import trace
from . import reference as ref


@dataclass(frozen=True)
class NormParams:
    """The canonical, hashable form of cellpose's ``normalize`` argument (:func:`norm_params`)."""
    normalize: bool = True
    lower: float = 1.0
    upper: float = 99.0
    #: fixed bounds instead of percentiles: ``(lo, hi)`` for every channel, or one pair per channel
    lowhigh: tuple | None = None
    invert: bool = False
    #: local normalisation against percentiles of blocks of about this size (0 = whole image)
    tile_blocksize: int = 0

    @property
    def is_default(self) -> bool:
        return self == NormParams()


#: cellpose ``models.normalize_default``, the dict a ``normalize`` dict is merged over
NORMALIZE_DEFAULT = {"lowhigh": None, "percentile": None, "normalize": True, "norm3D": True, "sharpen_radius": 0,
                     "smooth_radius": 0, "tile_norm_blocksize": 0, "tile_norm_smooth3D": 1, "invert": False}
_UNSUPPORTED_NORM = {"sharpen_radius": 0, "smooth_radius": 0, "tile_norm_smooth3D": 1}


def _num(v, what) -> float:
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError(f"normalize: {what} must be a number, got {v!r}") from None


def _pair(v, what):
    try:
        lo, hi = (float(t) for t in v)
    except (TypeError, ValueError):
        raise ValueError(f"normalize: {what} must be a pair of numbers, got {v!r}") from None
    return lo, hi


def norm_options(value) -> tuple[NormParams, bool | None]:
    """``normalize`` as cellpose takes it (bool, dict with cellpose's keys, or a :class:`NormParams`)
    -> ``(NormParams, norm3D or None)``.  A dict is merged over :data:`NORMALIZE_DEFAULT`; ``norm3D``
    comes back only when the dict names it.  Raises ``ValueError`` for unknown keys, for options
    that are not supported here (``sharpen_radius``, ``smooth_radius``, ``tile_norm_smooth3D`` away
    from their defaults), for bounds out of order, for ``tile_norm_blocksize`` together with
    ``lowhigh`` and for ``invert`` without normalisation (cellpose skips the inversion silently)."""
    if isinstance(value, NormParams):
        return value, None
    if value is None or isinstance(value, (bool, np.bool_)):
        return NormParams(normalize=True if value is None else bool(value)), None
    if not isinstance(value, dict):
        raise ValueError(f"normalize must be a bool, a dict or NormParams, got {type(value).__name__}")
    unknown = sorted(set(value) - set(NORMALIZE_DEFAULT))
    if unknown:
        raise ValueError(f"normalize: unknown key(s) {unknown}; known: {sorted(NORMALIZE_DEFAULT)}")
    d = {**NORMALIZE_DEFAULT, **value}
    for k, dv in _UNSUPPORTED_NORM.items():
        if d[k] is not None and _num(d[k], k) != dv:
            raise ValueError(f"normalize: {k}={d[k]!r} is not supported here (only its default {dv})")
    lower, upper = (1.0, 99.0) if d["percentile"] is None else _pair(d["percentile"], "percentile")
    if not 0.0 <= lower < upper <= 100.0:
        raise ValueError(f"normalize: percentile needs 0 <= lower < upper <= 100, got {[lower, upper]}")
    lowhigh = d["lowhigh"]
    if lowhigh is not None:
        lh = list(lowhigh)
        if len(lh) and isinstance(lh[0], (list, tuple, np.ndarray)):
            lowhigh = tuple(_pair(p, "lowhigh") for p in lh)
            pairs = lowhigh
        else:
            lowhigh = _pair(lh, "lowhigh")
            pairs = (lowhigh,)
        for lo, hi in pairs:
            if not hi - lo > 1e-3:
                raise ValueError(f"normalize: lowhigh needs hi - lo > 1e-3, got {[lo, hi]}")
    bs = d["tile_norm_blocksize"]
    bs = 0.0 if bs is None else _num(bs, "tile_norm_blocksize")
    if isinstance(d["tile_norm_blocksize"], (bool, np.bool_)) or not 0 <= bs < 2 ** 31:
        raise ValueError(f"normalize: tile_norm_blocksize must be a finite number >= 0, got {d['tile_norm_blocksize']!r}")
    bs = int(bs)
    if bs > 0 and lowhigh is not None:
        raise ValueError("normalize: tile_norm_blocksize and lowhigh exclude each other")
    on = bool(d["normalize"])
    if bool(d["invert"]) and not on:
        raise ValueError("normalize: invert needs normalize=True (the inversion is 1 - x of the normalised image)")
    if not on:
        return NormParams(normalize=False), (bool(value["norm3D"]) if "norm3D" in value else None)
    p = NormParams(True, lower, upper, lowhigh, bool(d["invert"]), bs)
    return p, (bool(value["norm3D"]) if "norm3D" in value else None)


def norm_params(value) -> NormParams:
    """:func:`norm_options` without the ``norm3D`` switch."""
    return norm_options(value)[0]


@dataclass
class EvalParams:
    #: cell diameter in pixels the images are rescaled from (to the network's ``diam_mean``): one number
    #: for the whole batch; a sequence or 1-D tensor with one entry per image (``None``, 0 and nan:
    #: that image is not rescaled), which runs the batch through one ragged tile plan
    #: (:class:`gpu.ScaledTilePlan`); or ``"auto"``: a first pass without rescaling, the diameter of
    #: every image from its masks (:func:`reference.derive_measurements`' ``diameter_px``), and one
    #: per-image pass for the images whose estimate asks for a rescale.  :meth:`CellposeRunner.eval_stack`
    #: and :meth:`~CellposeRunner.eval_3d` take a number only.
    diameter: "float | None | str | list | tuple | np.ndarray | torch.Tensor" = None
    niter: int = 200
    flow_threshold: float = 0.4
    cellprob_threshold: float = 0.0
    min_size: int = 15
    max_size_fraction: float = 0.4
    #: cellpose ``normalize``: a bool, a dict with cellpose's keys or a :class:`NormParams`
    #: (:func:`norm_options`); the runner's entry points replace it by its :class:`NormParams`
    normalize: "bool | dict | NormParams" = True
    tile: bool = True
    bsize: int | None = None  # None: the network's native tile (224 CPnet, 256 Cellpose-SAM)
    tile_overlap: float = 0.1
    #: test-time augmentation (cellpose ``augment=True``): tiles overlapping by half, each mirrored by
    #: its position in the tile grid, outputs mirrored back and averaged (reference.make_tiles /
    #: unaugment_tiles).  Needs ``tile=True``; ``tile_overlap`` is ignored.
    augment: bool = False
    compute_masks: bool = True
    #: GPU: split a batch into this many micro-batches and run mask recovery of micro-batch i on a
    #: second HIP stream while the network runs micro-batch i+1 (the mask stage is a chain of
    #: latency-bound kernels and host syncs that leaves most CUs idle on its own).
    pipeline_chunks: int = 1  # measured: 2 -> -9 %, 4 -> -18 % (latency-bound mask stages run once per chunk)
    pipeline_min_chunk: int = 4
    max_tiles: int = 0  # network tiles per launch (0 = sized to free HBM, CellposeRunner.tile_budget)
    # ---- z-stacks (CellposeRunner.eval_stack only; eval() ignores these)
    #: join masks of adjacent planes whose IoU is at least this (0 = return the per-plane masks)
    stitch_threshold: float = 0.0
    #: percentiles over the whole stack instead of per plane.  The library's default for this switch
    #: could not be checked offline; True follows its documented stitching behaviour.
    norm3d: bool = True
    stack_batch: int = 32  # planes per eval() call
    # ---- do_3D (CellposeRunner.eval_3d only; eval() and eval_stack() ignore this)
    #: z spacing / xy spacing: the volume is resampled along z to round(Z * anisotropy) planes before
    #: the three views run (None or 1 = isotropic voxels)
    anisotropy: float | None = None


def resolve_norm(p: EvalParams) -> EvalParams:
    """Canonicalise ``p.normalize`` in place (and take ``norm3D`` of a dict into ``p.norm3d``)."""
    if not isinstance(p.normalize, NormParams):
        p.normalize, n3 = norm_options(p.normalize)
        if n3 is not None:
            p.norm3d = n3
    return p


def _intake(p: "EvalParams | None", kw: dict, copy: bool) -> EvalParams:
    """The ``(p, **kw)`` of an entry point -> its parameters: the keyword overrides set on ``p`` (a
    fresh :class:`EvalParams` for None) and ``normalize`` canonicalised (:func:`resolve_norm`).  With
    ``copy`` both happen on a copy and the caller's object stays as it was (:meth:`~CellposeRunner.
    eval_stack`, :meth:`~CellposeRunner.eval_3d`); without, they are written into the caller's object
    (:meth:`~CellposeRunner.eval`, :meth:`~CellposeRunner.eval_locked`, :meth:`~CellposeRunner.stream`)."""
    if p is None:
        p = EvalParams()
    elif copy:
        p = dataclasses.replace(p)
    for k, v in kw.items():
        setattr(p, k, v)
    return resolve_norm(p)


def norm_on(p: EvalParams) -> bool:
    """Whether ``p`` asks for normalisation, whichever form ``p.normalize`` has."""
    return norm_params(p.normalize).normalize


def _rescale_factor(diameter, diam_mean: float) -> float:
    """``diam_mean / diameter``, the factor an image with cells of this diameter is resized by before
    the network sees it; 1.0 (not rescaled) without a positive diameter (``None``, 0, nan, negative)
    and within the band ``|diam_mean / diameter - 1| <= 1e-3``."""
    if diameter is None or not diameter > 0:
        return 1.0
    r = diam_mean / float(diameter)
    return r if abs(r - 1.0) > 1e-3 else 1.0


def diameter_form(diameter) -> str:
    """``"scalar"`` (a number or None), ``"list"`` (one diameter per image) or ``"auto"``."""
    if isinstance(diameter, str):
        if diameter != "auto":
            raise ValueError(f"diameter must be a number, a sequence with one entry per image or 'auto', got {diameter!r}")
        return "auto"
    if isinstance(diameter, (list, tuple)) or (isinstance(diameter, (np.ndarray, torch.Tensor)) and diameter.ndim > 0):
        return "list"
    return "scalar"


def per_image_diameters(diameter, B: int, diam_mean: float) -> list:
    """The sequence form of ``diameter`` -> a list of ``B`` entries: the diameter as a float, or
    ``None`` where the image is not rescaled (``None``, 0, nan, negative, or within the band
    ``|diam_mean / d - 1| <= 1e-3`` in which the scalar form does not rescale either)."""
    if isinstance(diameter, (np.ndarray, torch.Tensor)):
        if diameter.ndim != 1:
            raise ValueError(f"diameter: expected one entry per image, got shape {tuple(diameter.shape)}")
        diameter = diameter.tolist()
    if len(diameter) != B:
        raise ValueError(f"diameter has {len(diameter)} entries for a batch of {B} images")
    out = []
    for d in diameter:
        try:
            d = None if d is None else float(d)
        except (TypeError, ValueError):
            raise ValueError(f"diameter: every entry must be a number or None, got {d!r}") from None
        out.append(None if _rescale_factor(d, diam_mean) == 1.0 else d)
    return out


class PerImageRescale(list):
    """The rescale factor of every image of a batch (1.0 where it was not rescaled), in place of the
    one ``rescale`` of a scalar ``diameter``; ``diameters`` is what ``masks.diameters`` reports."""

    def __init__(self, factors, diameters):
        super().__init__(factors)
        self.diameters = [0.0 if d is None else float(d) for d in diameters]


def _scalar_diameter_only(p: "EvalParams", what: str) -> None:
    if diameter_form(p.diameter) != "scalar":
        raise ValueError(f"{what} takes one scalar diameter for the whole volume, not a sequence or 'auto': "
                         "per-image diameters belong to eval()")


def as_batch(images, nchan: int, device=None, keep_raw: bool = False):
    """Accept [H,W], [H,W,C], [C,H,W], [B,C,H,W] numpy/torch -> float tensor [B, nchan, H, W] on
    ``device`` (copied in the input's own dtype, e.g. uint16, and converted there).

    ``keep_raw``: return ``(x, raw)`` instead.  An input the fused front end reads as it is
    (:func:`gpu.takes_fused_front`: a contiguous [B, C >= nchan, H, W] uint8 / uint16 / float32
    device tensor) comes back unconverted, in its own dtype and with all its channels, and ``raw``
    is True; :meth:`CellposeRunner._front` decides what becomes of it.  Every other input is
    converted as without the flag and ``raw`` is False."""
    x = torch.as_tensor(np.asarray(images) if not torch.is_tensor(images) else images)
    if device is not None:
        x = x.to(device)
    if x.dim() == 2:
        x = x[None, None]
    elif x.dim() == 3:
        # channel-last if the last dim is small and the first is not
        if x.shape[-1] <= 4 and x.shape[0] > 4:
            x = x.permute(2, 0, 1)
        x = x[None]
    if keep_raw and x.dim() == 4 and x.shape[1] >= nchan:
        from .gpu import takes_fused_front

        if takes_fused_front(x):
            return x, True
    x = x.float()
    B, C, H, W = x.shape
    if C < nchan:
        x = torch.cat([x, torch.zeros(B, nchan - C, H, W, dtype=x.dtype, device=x.device)], 1)
    elif C > nchan:
        x = x[:, :nchan]
    return (x, False) if keep_raw else x


class CellposeRunner:
    """Batched Cellpose inference on one device: cyto3-style CPnet (224 tiles, fused MFMA conv engine)
    or Cellpose-SAM (cellpose 4 ``cpsam``: 256 tiles, 3 channels, ViT-L/8 HIP engine)."""

    def __init__(self, net=None, device: str | torch.device = "cuda", seed: int = 0):
        from ..models.cpsam import CPSAM, CPSAMEngine

        self.device = torch.device(device)
        self.net = (net if net is not None else CPnet().randomize_(seed)).eval()
        self.is_sam = isinstance(self.net, CPSAM)
        if self.is_sam:
            self.nchan = 3
            self.bsize = int(self.net.bsize)
            self.engine = CPSAMEngine(self.net, self.device) if self.device.type == "cuda" else None
        else:
            self.nchan = self.net.nchan
            self.bsize = 224
            if getattr(self.net, "norm_kind", "batch") == "group":
                self.engine = _GroupNormEngine(self.net, self.device)
            else:
                self.engine = CPnetEngine(self.net, self.device)
        self.diam_mean = float(self.net.diam_mean.item())
        self.cin_pad = (self.nchan + 7) // 8 * 8
        self._pinned: torch.Tensor | None = None  # host staging for numpy batches (pinned -> async DMA)
        self._plans: dict = {}
        self._scaled_plans: dict = {}
        self._net_graphs: dict = {}
        self._mask_stream = None  # made on first use (:meth:`_masks_on_side_stream`)

    # ---------------------------------------------------------------- network
    def _plan(self, H, W, p: EvalParams):
        from .gpu import TilePlan

        bs = p.bsize or self.bsize
        key = (H, W, bs, p.tile_overlap, bool(p.augment))
        if key not in self._plans:
            self._plans[key] = TilePlan(H, W, bs, p.tile_overlap, device=self.device, augment=bool(p.augment))
        return self._plans[key]

    #: ragged plans kept (least recently used first): their keys come from requests' diameters
    SCALED_PLANS_MAX = 64

    def _plan_scaled(self, H, W, scales, p: EvalParams):
        from .gpu import ScaledTilePlan

        bs = p.bsize or self.bsize
        sizes = tuple((ref.scaled_size(H, r), ref.scaled_size(W, r)) for r in scales)
        key = (H, W, sizes, bs, p.tile_overlap, bool(p.augment))
        plan = self._scaled_plans.pop(key, None)
        if plan is None:
            plan = ScaledTilePlan(H, W, scales, bs, p.tile_overlap, augment=bool(p.augment), device=self.device)
        self._scaled_plans[key] = plan  # most recently used last
        while len(self._scaled_plans) > self.SCALED_PLANS_MAX:
            self._scaled_plans.pop(next(iter(self._scaled_plans)))
        return plan

    #: HBM bytes one 224^2 CPnet tile keeps live at the forward's peak (measured on MI355X: 23.0-23.4
    #: MB per tile at 16 / 64 tiles, max_memory_allocated over one engine call; rounded up)
    TILE_ACT_BYTES = 32 << 20

    def tile_budget(self, p: EvalParams | None = None) -> int:
        """Tiles per network launch: what the free HBM holds (288 GB MI355X: ~8k tiles of 224^2, a
        ~20k x 20k image) with a quarter kept back; ``EvalParams.max_tiles`` caps it explicitly."""
        cap = getattr(p, "max_tiles", 0) if p is not None else 0
        if self.device.type != "cuda":
            return cap or (1 << 30)
        free, _ = torch.cuda.mem_get_info(self.device)
        n = max(1, int(free * 0.75) // self.TILE_ACT_BYTES)
        return min(n, cap) if cap else n

    def _tile_queue(self, tiles: torch.Tensor, p: EvalParams):
        """Spatial tile queue: the tiles of one batch (or one huge image) go through the network in
        launches of at most :meth:`tile_budget` tiles, written into one output buffer that the blend
        then reads -- an image larger than the HBM-resident activation budget is tiled, not an OOM
        (SURVEY.md §5 "tile queues sized to HBM"; the per-tile outputs are 0.6 MB each)."""
        T = tiles.shape[0]
        budget = self.tile_budget(p)
        if T <= budget:
            return self.engine(tiles)
        yt = st = None
        for i in range(0, T, budget):
            y_i, s_i = self.engine(tiles[i: i + budget])
            if yt is None:
                yt = torch.empty((T,) + tuple(y_i.shape[1:]), dtype=y_i.dtype, device=y_i.device)
                st = torch.empty((T,) + tuple(s_i.shape[1:]), dtype=s_i.dtype, device=s_i.device)
            yt[i: i + y_i.shape[0]] = y_i
            st[i: i + s_i.shape[0]] = s_i
            del y_i, s_i
        return yt, st

    def _sam_tiles(self, tiles: torch.Tensor) -> torch.Tensor:
        """NHWC bf16 tiles [T, by, bx, cpad] -> CPSAM flows [T, 3, by, bx] fp32 (tiles smaller than
        the network's fixed 256 grid are zero-padded, as cellpose 4 pads small images)."""
        T, by, bx, _ = tiles.shape
        bs = self.bsize
        x = torch.zeros(T, 3, bs, bs, dtype=torch.bfloat16, device=tiles.device)
        x[:, :, :by, :bx] = tiles[..., :3].permute(0, 3, 1, 2)
        out = []
        for i in range(0, T, 64):  # bounded activation memory for very large batches
            out.append(self.engine.graphed(x[i: i + 64]))
        y = torch.cat(out) if len(out) > 1 else out[0]
        return y[:, :, :by, :bx].contiguous()

    @torch.no_grad()
    def run_net(self, x: torch.Tensor, p: EvalParams, raw: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
        """x: normalised [B, nchan, H, W] on device -> (y [B, 3, H, W] fp32, style [B, S]).

        ``raw`` (tiled GPU path only): ``x`` is the un-normalised batch in the form :meth:`_front`
        passes on, and the tile gather normalises it (by ``p.normalize``) as it reads."""
        B, C, H, W = x.shape
        norm = norm_params(p.normalize)
        if p.augment and not p.tile:
            raise ValueError("augment=True needs tile=True: the augmentation mirrors tiles")
        if raw and not (self.device.type == "cuda" and p.tile):
            raise ValueError("run_net(raw=True) needs the tiled GPU path")
        if self.device.type == "cuda":
            if p.tile:
                plan = self._plan(H, W, p)
                with trace.span("cellpose.tiles_gather", cuda=True, tiles=B * plan.nt):
                    tiles = (plan.gather_normalized(x, self.cin_pad, self.nchan, params=None if norm.is_default else norm)
                             if raw else plan.gather(x, self.cin_pad))
                with trace.span("cellpose.net", cuda=True, tiles=B * plan.nt):
                    if self.is_sam:
                        yt = self._sam_tiles(tiles)
                        st = torch.zeros(B * plan.nt, 256, device=x.device)
                    else:
                        yt, st = self._tile_queue(tiles, p)
                with trace.span("cellpose.blend", cuda=True):
                    y = plan.blend(yt, B)
                style = st.view(B, plan.nt, -1).sum(1)
            elif self.is_sam:
                raise ValueError("Cellpose-SAM inference needs tile=True (fixed 256x256 network grid)")
            else:
                Hp, Wp = math.ceil(H / 8) * 8, math.ceil(W / 8) * 8
                xin = torch.zeros(B, Hp, Wp, self.cin_pad, dtype=torch.bfloat16, device=x.device)
                xin[:, :H, :W, :C] = x.permute(0, 2, 3, 1)
                y, style = self.engine(xin)
                y = y[:, :, :H, :W].contiguous()
            style = style / torch.sqrt((style * style).sum(1, keepdim=True)).clamp_min(1e-12)
            return y, style
        # CPU oracle path
        ys, styles = [], []
        bs = p.bsize or self.bsize
        for b in range(B):
            img = x[b].numpy()
            if p.tile:
                ya, yb = ref.pad_amounts(H)
                xa, xb = ref.pad_amounts(W)
                imgp = np.pad(img, ((0, 0), (ya, yb), (xa, xb)))
                Lyc, Lxc = imgp.shape[1:]
                if p.augment:
                    tiles, tys, txs, Lyc, Lxc = ref.make_tiles(imgp, bs, augment=True)
                else:
                    tiles, tys, txs = ref.make_tiles(imgp, bs, p.tile_overlap)
                tt = torch.from_numpy(tiles).float()
                if self.is_sam:
                    T, _, by, bx = tt.shape
                    tp = torch.zeros(T, 3, self.bsize, self.bsize)
                    tp[:, :, :by, :bx] = tt[:, :3]
                    yt = self.net(tp)[0][:, :, :by, :bx].detach()
                    st = torch.zeros(T, 256)
                else:
                    yt, st, _ = self.net(tt)
                yt = ref.unaugment_tiles(yt.numpy(), tys, txs) if p.augment else yt.numpy()
                yf = ref.average_tiles(yt, tys, txs, Lyc, Lxc)
                ys.append(torch.from_numpy(yf[:, ya: ya + H, xa: xa + W].copy()))
                styles.append(st.sum(0))
            else:
                yt, st, _ = self.net(x[b: b + 1])
                ys.append(yt[0])
                styles.append(st[0])
        style = torch.stack(styles)
        return torch.stack(ys), style / torch.sqrt((style * style).sum(1, keepdim=True)).clamp_min(1e-12)

    @torch.no_grad()
    def run_net_scaled(self, x: torch.Tensor, p: EvalParams, scales, raw: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
        """:meth:`run_net` on the tiled GPU path with image ``b`` rescaled by ``scales[b]`` (``None``:
        not rescaled): ``x`` [B, C, H, W] at its own size -> (y [B, 3, H, W] fp32, style [B, S]).  The
        rescaling is in the loads of the ragged gather and of the resize that follows the blend
        (:class:`gpu.ScaledTilePlan`); the network runs once per tile shape."""
        if not (self.device.type == "cuda" and p.tile):
            raise ValueError("run_net_scaled needs the tiled GPU path")
        B, C, H, W = x.shape
        norm = norm_params(p.normalize)
        plan = self._plan_scaled(H, W, scales, p)
        with trace.span("cellpose.tiles_gather", cuda=True, tiles=plan.nt_total):
            tiles = (plan.gather_normalized(x, self.cin_pad, self.nchan, params=None if norm.is_default else norm)
                     if raw else plan.gather(x, self.cin_pad))
        with trace.span("cellpose.net", cuda=True, tiles=plan.nt_total):
            yts, sts = [], []
            for t in tiles:
                if self.is_sam:
                    yts.append(self._sam_tiles(t))
                    sts.append(torch.zeros(t.shape[0], 256, device=x.device))
                else:
                    yt, st = self._tile_queue(t, p)
                    yts.append(yt)
                    sts.append(st)
        with trace.span("cellpose.blend", cuda=True):
            y = plan.resize_back(plan.blend(yts), yts[0].shape[1])
        style = plan.sum_styles(sts)
        return y, style / torch.sqrt((style * style).sum(1, keepdim=True)).clamp_min(1e-12)

    # ---------------------------------------------------------------- full eval
    @torch.no_grad()
    def eval(self, images, p: EvalParams | None = None, **kw):
        """Returns (masks [B, H, W] int32 tensor, flows [B, 3, H, W] fp32 tensor, styles [B, S]).
        With a per-image or ``"auto"`` ``diameter`` the masks carry ``masks.diameters``: a float32
        CPU tensor [B] of the diameter used for each image (0: not rescaled; under ``"auto"`` the
        estimate, whether it led to a second pass or not)."""
        p = _intake(p, kw, copy=False)
        form = diameter_form(p.diameter)
        if form == "auto" and not p.compute_masks:
            raise ValueError("diameter='auto' estimates the diameters from the masks: it needs compute_masks=True")
        x, raw = as_batch(self._stage(images), self.nchan, self.device, keep_raw=True)
        if form == "auto":
            return self._eval_auto(x, p, raw)
        if form == "list":
            p = dataclasses.replace(p, diameter=per_image_diameters(p.diameter, x.shape[0], self.diam_mean))
        return self._eval_batch(x, p, raw)

    def _eval_batch(self, x, p: EvalParams, raw: bool):
        B = x.shape[0]
        nch = min(p.pipeline_chunks, B // max(1, p.pipeline_min_chunk))
        if self.device.type == "cuda" and p.compute_masks and nch >= 2:
            return self._eval_pipelined(x, p, nch, raw)
        return self._eval_one(x, p, raw)

    def estimate_diameters(self, masks: torch.Tensor) -> np.ndarray:
        """``diameter_px`` of :func:`reference.derive_measurements` for every image of ``masks``
        [B, H, W]: ``median(sqrt(area)) * 2 / sqrt(pi)`` over its labels (0 without labels), float64
        [B].  On the GPU the areas are :func:`gpu.label_counts`, the medians are taken on the device
        and read back once for the whole batch."""
        B = masks.shape[0]
        if not masks.is_cuda:
            med = np.zeros(B)
            for b in range(B):
                area = np.bincount(masks[b].numpy().ravel().astype(np.int64))[1:]
                if (area > 0).any():
                    med[b] = np.median(np.sqrt(area[area > 0].astype(np.float64)))
            return med * 2.0 / np.sqrt(np.pi)
        from .gpu import label_counts

        nlab = getattr(masks, "label_bound", None) or int(masks.max()) + 1
        if nlab <= 1:
            return np.zeros(B)
        counts = label_counts(masks.to(torch.int32), nlab)
        present = counts > 0
        n = present.sum(1, keepdim=True)
        srt = torch.where(present, counts.double().sqrt(), torch.full((), float("inf"), dtype=torch.float64, device=masks.device))
        srt = srt.sort(1).values
        lo, hi = (n - 1).clamp_(min=0) // 2, (n // 2).clamp_(max=nlab - 1)
        med = torch.where(n > 0, (srt.gather(1, lo) + srt.gather(1, hi)) / 2, torch.zeros((), dtype=torch.float64, device=masks.device))
        return med[:, 0].cpu().numpy() * 2.0 / np.sqrt(np.pi)

    def _eval_auto(self, x, p: EvalParams, raw: bool):
        B = x.shape[0]
        masks, y, style = self._eval_batch(x, dataclasses.replace(p, diameter=None), raw)
        d = self.estimate_diameters(masks)
        redo = [b for b in range(B) if _rescale_factor(d[b], self.diam_mean) != 1.0]
        if redo:
            idx = torch.tensor(redo, device=x.device)
            xs = x if len(redo) == B else x[idx].contiguous()
            m2, y2, s2 = self._eval_batch(xs, dataclasses.replace(p, diameter=[float(d[b]) for b in redo]), raw)
            bounds = [getattr(m, "label_bound", None) for m in (masks, m2)]
            masks[idx], y[idx], style[idx] = m2, y2, s2
            if all(v is not None for v in bounds):
                masks.label_bound = max(bounds)
            elif hasattr(masks, "label_bound"):
                del masks.label_bound
        masks.diameters = torch.tensor(d, dtype=torch.float32)
        return masks, y, style

    @torch.no_grad()
    def eval_stack(self, stack, p: EvalParams | None = None, **kw):
        """Segment a z-stack plane by plane and stitch the masks of adjacent planes into volumetric
        labels (cellpose ``eval(..., stitch_threshold=t)``; semantics in :func:`reference.stitch3d`).

        ``stack``: [Z, H, W], [Z, C, H, W] or [Z, H, W, C], numpy or torch.  Returns
        ``(masks [Z, H, W] int32, flows [Z, 3, H, W] fp32, styles [Z, S])``.  With ``p.normalize and
        p.norm3d`` the percentiles are taken per channel over the whole stack; the planes then run
        through :meth:`eval` in chunks of ``p.stack_batch``.  ``p.stitch_threshold == 0`` returns the
        per-plane masks unstitched."""
        p = _intake(p, kw, copy=True)
        _scalar_diameter_only(p, "eval_stack")
        if norm_on(p) and p.norm3d and p.normalize.tile_blocksize > 0:
            raise ValueError("tile_norm_blocksize over a whole stack (norm3D) is not supported: give norm3D=False "
                             "to normalise every plane against its own block grid")
        x = as_batch(_planes_first(stack, "eval_stack expects"), self.nchan, self.device)
        Z = x.shape[0]
        if Z == 0:
            raise ValueError("eval_stack: empty stack")
        pp = dataclasses.replace(p)
        if norm_on(p) and p.norm3d:
            x = self._normalize_volume(x, p.normalize)
            pp.normalize = False
        masks, flows, styles = [], [], []
        step = max(1, int(p.stack_batch))
        for i in range(0, Z, step):
            m, y, s = self.eval(x[i: i + step], dataclasses.replace(pp))
            masks.append(m)
            flows.append(y)
            styles.append(s)
        flows, styles = torch.cat(flows), torch.cat(styles)
        if not p.compute_masks:
            return None, flows, styles
        M = torch.cat(masks)
        if p.stitch_threshold > 0:
            from .gpu import stitch3d_gpu  # the oracle for CPU tensors

            with trace.span("cellpose.stitch3d", cuda=M.is_cuda, planes=Z):
                M = stitch3d_gpu(M.to(torch.int32), p.stitch_threshold, min_size=p.min_size)
        return M, flows, styles

    #: fewest planes along any axis of an :meth:`eval_3d` volume.  The ZX and ZY views are Z planes
    #: high; the tiled network pads every plane to a multiple of 16 plus an 8-pixel margin, so it
    #: runs from one row up, but trilinear resampling, the 8x downsampling of the untiled path and
    #: the ``diameter`` rescale (never below 8 rows) all need a real third dimension: below 2 planes
    #: a volume is an image and belongs to :meth:`eval`; the untiled path needs 8.
    MIN_DEPTH_3D = 2
    MIN_DEPTH_3D_UNTILED = 8

    @torch.no_grad()
    def eval_3d(self, volume, p: EvalParams | None = None, **kw):
        """Volumetric segmentation (cellpose ``eval(..., do_3D=True)``): the network runs on the YX,
        ZX and ZY planes of the volume, the three outputs are summed into one (dZ, dY, dX, cellprob)
        field (:func:`reference.combine_views3d`) and the flow dynamics, seeding and labelling run in
        three dimensions (:func:`reference.compute_masks3d`; no flow QC, ``flow_threshold`` is unused).

        ``volume``: [Z, H, W], [Z, C, H, W] or [Z, H, W, C], numpy or torch, as :meth:`eval_stack`
        takes.  Returns ``(masks [Z, H, W] int32, flows [4, Z', H, W] fp32 (dZ, dY, dX, cellprob),
        styles [S])``; ``styles`` is the mean style of the YX planes.  The volume is normalised once,
        per channel over all voxels; every view's planes then go through the network stage in chunks
        of ``p.stack_batch`` planes (so ``diameter`` rescales each plane as in :meth:`eval`) and each
        chunk is added to the accumulator as soon as it exists.

        ``p.anisotropy`` (z spacing over xy spacing), when set and not 1: the normalised volume is
        resampled along z to ``Z' = round(Z * anisotropy)`` planes (trilinear, ``align_corners=False``),
        masks are computed there and brought back with the nearest-plane rule ``z_src = min(floor((z +
        0.5) * Z' / Z), Z' - 1)`` and numbered ``1..K`` again.  ``flows`` stay at the resampled depth ``Z'`` (``Z' = Z`` otherwise)."""
        from . import gpu

        p = _intake(p, kw, copy=True)
        _scalar_diameter_only(p, "eval_3d")
        if norm_on(p) and p.normalize.tile_blocksize > 0:
            raise ValueError("tile_norm_blocksize is not supported by eval_3d: the volume is normalised once over all voxels")
        x = as_batch(_planes_first(volume, "eval_3d expects"), self.nchan, self.device)
        Z, C, H, W = x.shape
        aniso = p.anisotropy
        if aniso is not None and not aniso > 0:
            raise ValueError(f"anisotropy must be positive, got {aniso}")
        Zr = Z if aniso is None or aniso == 1 else max(1, int(round(Z * float(aniso))))
        need = self.MIN_DEPTH_3D if p.tile else self.MIN_DEPTH_3D_UNTILED
        if min(Z, Zr, H, W) < need:
            raise ValueError(f"eval_3d needs at least {need} planes along every axis (tile={p.tile}), got a "
                             f"{Z} x {H} x {W} volume" + (f" resampled to {Zr} planes" if Zr != Z else ""))
        on_gpu = self.device.type == "cuda"
        if on_gpu:
            gpu._check_volume(Zr, H, W)
        if norm_on(p):
            x = self._normalize_volume(x, p.normalize)
        if Zr != Z:
            x = F.interpolate(x.permute(1, 0, 2, 3)[None], size=(Zr, H, W), mode="trilinear",
                              align_corners=False)[0].permute(1, 0, 2, 3).contiguous()
        pp = dataclasses.replace(p, normalize=False)
        step = max(1, int(p.stack_batch))
        acc = torch.empty(4, Zr, H, W, dtype=torch.float32, device=self.device) if on_gpu else None
        outs, style, rescale = [], None, 1.0
        with trace.span("cellpose.views3d", cuda=on_gpu, planes=Zr + H + W):
            for view, perm in enumerate(((0, 1, 2, 3), (2, 1, 0, 3), (3, 1, 0, 2))):
                xv = x.permute(*perm)  # [planes, C, rows, columns] of this view
                ys = []
                for i in range(0, xv.shape[0], step):
                    y, s, rescale = self._net_stage(xv[i: i + step].contiguous(), dataclasses.replace(pp))
                    if view == 0:
                        style = s.sum(0) if style is None else style + s.sum(0)
                    if on_gpu:
                        gpu.accum_view3d(acc, y, view, i)
                    else:
                        ys.append(y)
                    del y
                if not on_gpu:
                    outs.append(torch.cat(ys).numpy())
            if not on_gpu:
                dP, cp = ref.combine_views3d(*outs)
                acc = torch.from_numpy(np.concatenate([dP, cp[None]]))
        style = style / Zr
        if not p.compute_masks:
            return None, acc, style
        niter = p.niter if p.niter else int(200 / max(rescale, 1e-3))
        with trace.span("cellpose.masks3d", cuda=on_gpu, planes=Zr):
            M = gpu.compute_masks3d_gpu(acc, None, niter=niter, cellprob_threshold=p.cellprob_threshold,  # CPU: the oracle
                                        min_size=p.min_size, max_size_fraction=p.max_size_fraction)
            if Zr != Z:
                zs = ((torch.arange(Z, device=M.device) * 2 + 1) * Zr // (2 * Z)).clamp_(max=Zr - 1)
                # an instance that lives only on planes the rule skips is gone: number the rest 1..K again
                u, inv = torch.unique(M[zs], return_inverse=True)
                M = (inv if int(u[0]) == 0 else inv + 1).to(torch.int32).contiguous()
        return M, acc, style

    def _stage(self, images):
        """numpy batch -> view of a reusable pinned host buffer, so the H2D copy is one DMA at full
        PCIe rate instead of a pageable staged copy.  The previous eval has finished with the buffer
        (its results were synchronised back) by the time it is reused."""
        if self.device.type != "cuda" or torch.is_tensor(images) or not isinstance(images, np.ndarray):
            return images
        a = np.ascontiguousarray(images)
        if self._pinned is None or self._pinned.numel() < a.nbytes:
            self._pinned = torch.empty(max(a.nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        tdt = torch.from_numpy(np.empty(0, a.dtype)).dtype
        t = self._pinned[: a.nbytes].view(tdt).view(a.shape)  # still a pinned tensor
        np.copyto(t.numpy(), a)
        return t

    #: batches up to this many images run normalize99 + tiling + network + blend from a HIP graph
    #: (captured once per shape / params).  Off by default: measured on MI355X it did not help --
    #: headline 1,813 / 1,813 img/s graphed vs 1,819 / 1,815 eager, batch-1 p50 2.05 / 2.08 vs
    #: 1.99 / 2.03 ms (profiles/r05/headline/graph_ab_s5.jsonl): the eager launches already hide
    #: behind the kernels and the replay adds the static-buffer copies.
    GRAPH_NET_MAX_B = int(os.environ.get("BE_CELLPOSE_GRAPH_MAX_B", "0"))

    def _net_graphed(self, x, p: EvalParams):
        """(y, style) of the network stage (rescale 1) replayed from its HIP graph, or None when this
        call should run eagerly (large batch, CPU, capture failed for this shape)."""
        B = x.shape[0]
        if self.device.type != "cuda" or B > self.GRAPH_NET_MAX_B or not x.is_cuda:
            return None
        key = (tuple(x.shape), x.dtype, norm_params(p.normalize), bool(p.tile), p.bsize, p.tile_overlap, p.max_tiles,
               bool(p.augment))
        ent = self._net_graphs.get(key)
        if ent is False:
            return None
        if ent is None:
            from .gpu import norm_constants

            xs = x.clone()
            # The cached device constants of the options (block starts, lowhigh bounds): the capture
            # bakes their addresses into the graph, and the caches they come from evict, so the
            # entry holds them for as long as the graph lives.
            def consts():
                return norm_constants(norm_params(p.normalize), x.shape[1], x.shape[2], x.shape[3], x.device)

            keep = consts()
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))

            def body():
                xx = self._normalize(xs, p.normalize) if norm_on(p) else xs
                return self.run_net(xx, p)

            try:
                with torch.cuda.stream(side):
                    body()  # lazy state (plans, kernel attributes, workspaces) outside the capture
                torch.cuda.current_stream(self.device).wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    y, style = body()
                if not all(a is b for a, b in zip(keep, consts())):
                    raise RuntimeError("an option constant was evicted and rebuilt while the graph was captured")
            except Exception:  # noqa: BLE001 -- this shape runs eagerly
                self._net_graphs[key] = False
                return None
            ent = self._net_graphs[key] = (g, xs, y, style, keep)
        g, xs, y, style = ent[:4]
        xs.copy_(x)
        g.replay()
        return y.clone(), style.clone()

    def _front(self, x, p: EvalParams, raw: bool):
        """Decide the front end of one network stage for a batch that :func:`as_batch` kept ``raw``
        (own dtype, all channels).  Returns ``(x, raw)``: still raw, ``x`` goes to ``run_net(...,
        raw=True)``, whose gather takes the percentiles on the raw pixels and normalises as it reads
        (:meth:`gpu.TilePlan.gather_normalized`; every :class:`NormParams` with normalisation on
        takes it).  That needs the tiled GPU path with normalisation on, no diameter rescale (the
        resize reads the normalised image) and no HIP-graph replay; otherwise ``x`` comes back as
        float32 [B, nchan, H, W] for the unfused sequence."""
        if not raw:
            return x, False
        from .gpu import takes_fused_front

        rescaled = _rescale_factor(p.diameter, self.diam_mean) != 1.0
        if (self.device.type == "cuda" and norm_on(p) and p.tile and not rescaled and x.shape[0] > self.GRAPH_NET_MAX_B
                and takes_fused_front(x)):
            return x, True
        return x.float()[:, : self.nchan], False

    def _net_stage_list(self, x, p: EvalParams, raw: bool):
        """The network stage for the sequence form of ``p.diameter``: ``(y, style, PerImageRescale)``.
        On the tiled GPU path the whole batch goes through one ragged plan (:meth:`run_net_scaled`),
        from the raw pixels under the conditions the unscaled path takes them (never from a HIP-graph
        replay); tile normalisation normalises first and gathers from float32.  Elsewhere (the CPU
        oracle, ``tile=False``) the images run one by one through the scalar code."""
        B = x.shape[0]
        diams = per_image_diameters(p.diameter, B, self.diam_mean)
        rescale = PerImageRescale([1.0 if d is None else self.diam_mean / d for d in diams], diams)
        if all(d is None for d in diams):
            y, style, _ = self._net_stage(x, dataclasses.replace(p, diameter=None), raw)
            return y, style, rescale
        if not (self.device.type == "cuda" and p.tile):
            outs = [self._net_stage(x[b: b + 1].contiguous(), dataclasses.replace(p, diameter=d), raw)
                    for b, d in enumerate(diams)]
            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), rescale
        from .gpu import takes_fused_front

        norm = norm_params(p.normalize)
        fused = raw and norm.normalize and norm.tile_blocksize == 0 and takes_fused_front(x)
        if not fused:
            if raw:
                x = x.float()[:, : self.nchan]
            if norm.normalize:
                with trace.span("cellpose.normalize99", cuda=True, images=B):
                    x = self._normalize(x, norm)
        y, style = self.run_net_scaled(x, p, [None if d is None else self.diam_mean / d for d in diams], raw=fused)
        return y, style, rescale

    def _eval_one(self, x, p: EvalParams, raw: bool = False):
        y, style, rescale = self._net_stage(x, p, raw)
        if not p.compute_masks:
            return None, y, style
        with trace.span("cellpose.masks", cuda=self.device.type == "cuda", images=x.shape[0]):
            masks = self.compute_masks(y, p, rescale)
        return masks, y, style

    def _net_stage(self, x, p: EvalParams, raw: bool = False):
        """Everything before mask recovery, for a batch as :func:`as_batch` returns it (``raw`` as it
        says): front end, normalisation, the ``diameter`` rescale around the network, blend.
        Returns ``(y [B, 3, H, W], style [B, S], rescale)``, ``rescale`` being what
        :meth:`compute_masks` takes: :func:`_rescale_factor` of a scalar diameter, a
        :class:`PerImageRescale` for the sequence form."""
        if diameter_form(p.diameter) == "list":
            return self._net_stage_list(x, p, raw)
        x, raw = self._front(x, p, raw)
        B, C, H, W = x.shape
        rescale = _rescale_factor(p.diameter, self.diam_mean)
        if rescale == 1.0:
            r = self._net_graphed(x, p)
            if r is not None:
                return r[0], r[1], rescale
        if norm_on(p) and not raw:
            with trace.span("cellpose.normalize99", cuda=True, images=B):
                x = self._normalize(x, p.normalize)
        if rescale != 1.0:
            Hs, Ws = max(8, int(round(H * rescale))), max(8, int(round(W * rescale)))
            xs = resize_bilinear(x, (Hs, Ws))
            y, style = self.run_net(xs, p)
            y = resize_bilinear(y, (H, W))
        else:
            y, style = self.run_net(x, p, raw=True) if raw else self.run_net(x, p)
        return y, style, rescale

    def _masks_on_side_stream(self, y, p: EvalParams, rescale, ev) -> torch.Tensor:
        """:meth:`compute_masks` of ``y`` on the runner's second stream (:func:`mask_stream`, made on
        first use), queued there behind ``ev``, the event recorded after ``y``'s network stage.  The
        masks belong to that stream (``self._mask_stream``); who waits for them, and how, is left
        to the caller: :meth:`_eval_pipelined`, :meth:`eval_locked` and :meth:`stream` each differ."""
        if self._mask_stream is None:
            self._mask_stream = mask_stream(self.device)
        side = self._mask_stream
        with torch.cuda.stream(side):
            side.wait_event(ev)
            y.record_stream(side)
            with trace.span("cellpose.masks", cuda=True, images=y.shape[0]):
                return self.compute_masks(y, p, rescale)

    def _eval_pipelined(self, x, p: EvalParams, nch: int, raw: bool = False):
        """Two-stream software pipeline over micro-batches: net(i+1) on the current stream is queued
        before mask recovery of micro-batch i (which syncs the host on its own stream) starts."""
        main = torch.cuda.current_stream(self.device)
        parts = x.tensor_split(nch)
        ys, styles, masks = [], [], []
        pending = None
        per_image = diameter_form(p.diameter) == "list"
        starts = np.cumsum([0] + [part.shape[0] for part in parts])  # the diameters split with the images
        for i, part in enumerate(parts):
            pp = dataclasses.replace(p, diameter=list(p.diameter[starts[i]: starts[i + 1]])) if per_image else p
            y, style, rescale = self._net_stage(part, pp, raw)
            ys.append(y)
            styles.append(style)
            ev = torch.cuda.Event()
            ev.record(main)
            if pending is not None:
                masks.append(self._masks_on_side_stream(*pending))
            pending = (y, p, rescale, ev)
        masks.append(self._masks_on_side_stream(*pending))
        main.wait_stream(self._mask_stream)
        for m in masks:
            m.record_stream(main)
        out = torch.cat(masks)
        if per_image:
            out.diameters = torch.cat([m.diameters for m in masks])
        return out, torch.cat(ys), torch.cat(styles)

    @torch.no_grad()
    def eval_locked(self, images, net_lock, mask_lock, p: EvalParams | None = None, **kw):
        """:meth:`eval` for concurrent callers (serving threads): the network stage runs under
        ``net_lock`` on the caller's stream, mask recovery under ``mask_lock`` on the runner's second
        stream -- so one batch's mask recovery overlaps the next batch's network (the cross-batch
        overlap of :meth:`stream`, for batches that arrive on different threads).  Returns
        ``(masks, flows, styles, ready)``: ``ready`` is a HIP event recorded after the masks (None
        off the GPU path) -- wait on it on a copy stream rather than on the caller's stream, which may
        already hold the next batch's network."""
        p = _intake(p, kw, copy=False)
        if self.device.type != "cuda" or not p.compute_masks or diameter_form(p.diameter) == "auto":
            with net_lock:  # "auto" is two dependent passes: it runs whole, as eval() runs it
                m, y, st = self.eval(images, p)
                ev = None
                if self.device.type == "cuda":
                    ev = torch.cuda.Event()
                    ev.record()
                return m, y, st, ev
        with net_lock:
            # no shared pinned staging buffer here: the previous batch's H2D may still be reading it
            x, raw = as_batch(images, self.nchan, self.device, keep_raw=True)
            y, style, rescale = self._net_stage(x, p, raw)
            main = torch.cuda.current_stream(self.device)
            ev = torch.cuda.Event()
            ev.record(main)
        with mask_lock:
            m = self._masks_on_side_stream(y, p, rescale, ev)
            done = torch.cuda.Event()
            done.record(self._mask_stream)
        return m, y, style, done

    def stream(self, p: EvalParams | None = None) -> "_EvalStream":
        """Cross-batch pipeline for a stream of batches (continuous serving / offline throughput):
        ``submit(images)`` queues batch i's network on the current stream, then runs mask recovery of
        batch i-1 on a second HIP stream (so its latency-bound kernels and host syncs overlap batch
        i's convs) and returns batch i-1's ``(masks, flows, styles)`` (None for the first batch);
        ``flush()`` returns the last batch's.  Same per-batch results as :meth:`eval`."""
        return _EvalStream(self, _intake(p, {}, copy=False))

    def _normalize_volume(self, x, norm):
        """``x`` [Z, C, H, W] normalised per channel over the whole stack, which :meth:`_normalize`
        sees as one image of ``Z * H`` rows."""
        Z, C, H, W = x.shape
        with trace.span("cellpose.normalize99", cuda=self.device.type == "cuda", images=Z):
            xs = x.permute(1, 0, 2, 3).reshape(1, C, Z * H, W)
            return self._normalize(xs, norm).reshape(C, Z, H, W).permute(1, 0, 2, 3).contiguous()

    def _normalize(self, x, norm=True):
        """``x`` [B, C, H, W] normalised per image by ``norm`` (anything :func:`norm_params` takes)."""
        norm = norm_params(norm)
        if self.device.type == "cuda":
            from .gpu import normalize99, normalize_img_gpu

            return normalize99(x) if norm.is_default else normalize_img_gpu(x, norm)
        if norm.is_default:
            return torch.stack([torch.from_numpy(ref.normalize99(x[b].numpy())) for b in range(x.shape[0])])
        return torch.stack([torch.from_numpy(ref.normalize_img(x[b].numpy(), norm)) for b in range(x.shape[0])])

    def compute_masks(self, y: torch.Tensor, p: EvalParams, rescale: "float | PerImageRescale" = 1.0) -> torch.Tensor:
        """Mask recovery of the flows ``y`` [B, 3, H, W].  ``rescale``: the factor the batch was rescaled
        by, which sets ``niter`` when ``p.niter`` is unset; a :class:`PerImageRescale` recovers the
        masks per group of images that share ``int(200 / r_b)``, so every image gets the result it
        would get alone, and the masks carry ``diameters``."""
        if isinstance(rescale, PerImageRescale):
            niters = [p.niter if p.niter else int(200 / max(r, 1e-3)) for r in rescale]
            if len(set(niters)) == 1:
                out = self._masks_niter(y, p, niters[0])
            else:
                out = torch.zeros(y.shape[0], y.shape[2], y.shape[3], dtype=torch.int32, device=y.device)
                bounds = []
                for n in sorted(set(niters)):
                    idx = torch.tensor([b for b, v in enumerate(niters) if v == n], device=y.device)
                    m = self._masks_niter(y[idx].contiguous(), p, n)
                    out[idx] = m.to(torch.int32)
                    bounds.append(getattr(m, "label_bound", 1))
                if self.device.type == "cuda":
                    out.label_bound = max(bounds)
            out.diameters = torch.tensor(rescale.diameters, dtype=torch.float32)
            return out
        return self._masks_niter(y, p, p.niter if p.niter else int(200 / max(rescale, 1e-3)))

    def _masks_niter(self, y: torch.Tensor, p: EvalParams, niter: int) -> torch.Tensor:
        if self.device.type == "cuda":
            from .gpu import compute_masks_gpu

            return compute_masks_gpu(y, niter=niter, cellprob_threshold=p.cellprob_threshold,
                                     flow_threshold=p.flow_threshold, min_size=p.min_size,
                                     max_size_fraction=p.max_size_fraction)
        out = []
        for b in range(y.shape[0]):
            yb = y[b].numpy()
            m = ref.compute_masks(yb[:2], yb[2], niter=niter, cellprob_threshold=p.cellprob_threshold,
                                  flow_threshold=p.flow_threshold, min_size=p.min_size,
                                  max_size_fraction=p.max_size_fraction)
            out.append(torch.from_numpy(m.astype(np.int32)))
        return torch.stack(out)

    # ---------------------------------------------------------------- measurements
    def measure(self, masks, images=None, volume: bool = False):
        """Per-cell measurement tables (:func:`reference.derive_measurements`) of label images.

        ``masks``: [B, H, W] (or one [H, W] image), as :meth:`eval` returns them; with ``volume=True``
        one [Z, H, W] volume, as :meth:`eval_stack` / :meth:`eval_3d` return it.  ``images``: what was
        segmented (any form :meth:`eval` / :meth:`eval_stack` takes) or None for the geometry alone;
        its channels are padded or cut to the network's, and it is *not* normalised: intensities are in
        the caller's units.  Returns a list with one table (a dict of numpy arrays plus ``n_cells`` and
        ``diameter_px``) per image, or the one table of a volume.  Masks on the GPU are measured by
        the HIP kernel (:func:`gpu.measure_masks_gpu`), everything else by the numpy oracle."""
        m, _ = _label_masks(masks, "measure", volume)
        img = None
        if images is not None:
            img = as_batch(_planes_first(images, "a z-stack is") if volume else images, self.nchan, m.device)
            if img.shape[0] != m.shape[0] or img.shape[2:] != m.shape[1:]:
                raise ValueError(f"measure: images {tuple(img.shape)} do not fit masks {tuple(m.shape)}")
        raws = measure_launch(m, img, volume=volume)
        return measure_tables(raws, volume)

    # ---------------------------------------------------------------- outlines
    def outlines(self, masks, volume: bool = False, nlab: int | None = None):
        """Cell outlines as polygon rings (:func:`reference.mask_rings`): closed rings of pixel-corner
        coordinates whose polygon is exactly the mask.

        ``masks``: [B, H, W] (or one [H, W] image), as :meth:`eval` returns them; with ``volume=True``
        one [Z, H, W] volume, as :meth:`eval_stack` / :meth:`eval_3d` return it, outlined plane by
        plane with the volume's labels.  Returns one rings dict of numpy arrays per image (``verts``
        int32 [V, 2] (y, x), ``ring_offsets`` int64 [R + 1], ``ring_label`` int32 [R], ``ring_area2``
        int64 [R]; :func:`reference.rings_to_geojson` turns one into GeoJSON), or the list of the Z
        planes' dicts for a volume.  ``nlab``: an upper bound on the labels + 1; by default the
        ``label_bound`` the mask stage left on ``masks``, else ``masks.max() + 1``.  Masks on the GPU
        are traced by the HIP kernels (:func:`gpu.mask_rings_gpu`), everything else by the oracle."""
        m, nlab = _label_masks(masks, "outlines", volume, nlab)
        return outline_rings(outline_launch(m, nlab=nlab, volume=volume))

    # ---------------------------------------------------------------- surfaces
    def surfaces(self, masks, spacing=(1.0, 1.0, 1.0), nlab: int | None = None) -> dict:
        """The surface of every label of a volume (:func:`reference.label_surface`): an indexed quad
        mesh with two vertex placements and per-label surface statistics.

        ``masks``: one [Z, H, W] label volume, as :meth:`eval_stack` / :meth:`eval_3d` return it.
        ``spacing``: the voxel size (sz, sy, sx), three positive finite numbers.  Returns ``{"mesh":
        the mesh dict as numpy arrays (``corner``, ``verts``, ``vert_label``, ``quads``, ``quad_label``,
        ``label_verts``, ``label_quads``, ``faces``, ``voxels``), "stats": the table of
        :func:`reference.surface_stats` (``area``, ``area_voxel``, ``mesh_volume``, ``volume``,
        ``sphericity``, ...; one float64 row per label)}``; :func:`reference.surface_to_obj` turns the
        mesh into OBJ text.  Faces on the volume's border count as surface.  ``nlab``: an upper bound
        on the labels + 1; by default the ``label_bound`` the mask stage left on ``masks``, else
        ``masks.max() + 1``.  A volume on the GPU is meshed by the HIP kernels
        (:func:`gpu.label_surface_gpu`, :func:`gpu.surface_stats_gpu`), everything else by the oracle."""
        sp = ref._check_spacing(spacing, "surfaces")
        m, nlab = _label_masks(masks, "surfaces", True, nlab, "one [Z, H, W] label volume")
        return surface_tables(surface_launch(m, sp, nlab=nlab))

    # ---------------------------------------------------------------- polygon annotations
    def labels_from_outlines(self, outlines, shape, device=None) -> torch.Tensor:
        """Label images of polygon annotations (:func:`reference.rasterize_rings`): the way back from
        :meth:`outlines`.

        ``outlines``: a list with one document per image -- anything
        :func:`reference.outlines_to_rings` accepts: a polygons dict, the app's ``"rings"`` list or
        GeoJSON -- or a single document for a single image.  A list of the Z plane documents of a
        stack (the app's ``{z, outlines}`` wrappers are unwrapped) gives the [Z, H, W] volume with the
        volume's labels: it is the same call.  ``shape``: (H, W).  Returns int32 [B, H, W] on the
        runner's device (or ``device``) with ``label_bound`` set, so that :meth:`measure`,
        :meth:`outlines` and :meth:`score` skip their ``max()`` read.  On the GPU the polygons are
        rasterised by the HIP kernel (:func:`gpu.rasterize_rings_gpu`: parsed, quantised and planned
        on the host, nothing read back), everything else by the numpy oracle."""
        from .gpu import rasterize_rings_gpu

        parts = [ref.outlines_to_rings(ref.unwrap_outlines(d)) for d in outline_documents(outlines)]
        H, W = int(shape[0]), int(shape[1])
        return rasterize_rings_gpu(join_polygons(parts), len(parts), H, W, self.device if device is None else device)

    # ---------------------------------------------------------------- evaluation
    def score(self, masks_true, masks_pred, thresholds=(0.5, 0.75, 0.9), volume: bool = False) -> dict:
        """Average precision of predicted labels against ground truth (:func:`metrics.average_precision`).

        ``masks_pred``: [B, H, W] (or one [H, W] image), as :meth:`eval` returns them; with
        ``volume=True`` one [Z, H, W] volume scored as one image.  ``masks_true``: the same shape,
        numpy or torch; it is moved to the prediction's device.  Returns ``ap`` (float32), ``tp``,
        ``fp``, ``fn`` as numpy arrays [B, K], ``n_true`` and ``n_pred`` [B] (the label maxima), and
        under ``summary`` the :func:`metrics.instance_metrics` document.  Predictions on the GPU are
        scored by the HIP kernels (:func:`gpu.average_precision_gpu`; a ``label_bound`` on the
        prediction saves its ``max()`` sync), everything else by the numpy oracle."""
        from . import metrics
        from .gpu import average_precision_gpu

        mp = masks_pred if torch.is_tensor(masks_pred) else torch.as_tensor(np.asarray(masks_pred))
        nt = None
        if is_outline_annotation(masks_true):
            # polygon ground truth: rasterised at the prediction's (H, W) on the prediction's device
            if mp.dim() < 2:
                raise ValueError(f"score expects [B, H, W] masks or one [Z, H, W] volume, got shape {tuple(mp.shape)}")
            mt = self.labels_from_outlines(masks_true, mp.shape[-2:], device=mp.device)
            nt = mt.label_bound
            if mp.dim() == 2 and mt.shape[0] == 1:
                mt = mt[0]
        else:
            mt = masks_true if torch.is_tensor(masks_true) else torch.as_tensor(np.asarray(masks_true))
        if tuple(mt.shape) != tuple(mp.shape):
            raise ValueError(f"score: true masks {tuple(mt.shape)} do not fit predicted masks {tuple(mp.shape)}")
        if volume:
            if mp.dim() != 3:
                raise ValueError(f"score(volume=True) expects one [Z, H, W] volume, got shape {tuple(mp.shape)}")
            mt, mp = mt[None], mp[None]
        elif mp.dim() == 2:
            mt, mp = mt[None], mp[None]
        if mp.dim() < 3:
            raise ValueError(f"score expects [B, H, W] masks or one [Z, H, W] volume, got shape {tuple(mp.shape)}")
        ths = [thresholds] if np.isscalar(thresholds) else list(thresholds)
        bound = getattr(masks_pred, "label_bound", None)
        ap, tp, fp, fn = average_precision_gpu(mt.to(mp.device), mp, ths, nt=nt, np_=bound)
        n_true, n_pred = (tp + fn)[:, 0], (tp + fp)[:, 0]
        return {"ap": ap, "tp": tp, "fp": fp, "fn": fn, "n_true": n_true, "n_pred": n_pred,
                "summary": metrics.metrics_document(ap, ths, n_true.sum(), n_pred.sum())}

    @torch.no_grad()
    def evaluate(self, images, masks_true, p: EvalParams | None = None, thresholds=(0.5, 0.75, 0.9), **kw) -> dict:
        """:meth:`eval` with the given parameters, then :meth:`score` of its masks against
        ``masks_true`` on the device they were computed on.  Returns :meth:`score`'s dict plus
        ``masks`` (the [B, H, W] int32 tensor of :meth:`eval`, not copied to the host)."""
        masks, _, _ = self.eval(images, p, **kw)
        res = self.score(masks_true, masks, thresholds)
        res["masks"] = masks
        return res


def _outline_item(d) -> bool:
    return isinstance(d, dict) and (d.get("type") == "Feature" or "rings" in d)


def outline_documents(outlines) -> list:
    """The per-image documents of a polygon annotation argument.  A dict is one document (a polygons
    dict, a GeoJSON object or a ``{z, outlines}`` wrapper), and so is a non-empty list of GeoJSON
    ``Feature`` s or of the app's ``{label, rings}`` items; any other list holds one document per
    image (an image without cells is ``[]`` or an empty ``FeatureCollection``)."""
    if isinstance(outlines, dict):
        return [outlines]
    if isinstance(outlines, (list, tuple)):
        if outlines and all(_outline_item(d) for d in outlines):
            return [outlines]
        return list(outlines)
    raise ValueError(f"expected a list of outline documents, got {type(outlines).__name__}")


def is_outline_annotation(x) -> bool:
    """Whether a ground-truth argument holds polygon documents and not label arrays."""
    if isinstance(x, dict):
        return True
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(isinstance(d, (dict, list, tuple)) and
                                                              ref.is_outline_document(d) for d in x)


def join_polygons(parts) -> dict:
    """Per-image polygons dicts -> the arrays of the whole batch with ``ring_image``, the input of
    :func:`gpu.rasterize_rings_gpu`.  Vertices become float64, which holds every integer and float
    dtype below 2^53 exactly."""
    vs = [np.asarray(p["verts"], np.float64).reshape(-1, 2) for p in parts]
    offs = [np.asarray(p["ring_offsets"]).astype(np.int64) for p in parts]
    nv = np.cumsum([0] + [v.shape[0] for v in vs])
    return {"verts": np.concatenate(vs) if vs else np.zeros((0, 2)),
            "ring_offsets": np.concatenate([o[:-1] + nv[b] for b, o in enumerate(offs)] + [nv[-1:]]).astype(np.int64),
            "ring_label": np.concatenate([np.asarray(p["ring_label"]).astype(np.int64) for p in parts] + [np.zeros(0, np.int64)]),
            "ring_image": np.concatenate([np.full(o.shape[0] - 1, b, np.int64) for b, o in enumerate(offs)] + [np.zeros(0, np.int64)])}


def _planes_first(stack, what: str) -> torch.Tensor:
    """[Z, H, W], [Z, C, H, W] or [Z, H, W, C] -> [Z, C, H, W]: how every entry point reads a z-stack
    (channel-last as :func:`as_batch` decides it for one image).  ``what`` opens the error text."""
    x = torch.as_tensor(np.asarray(stack) if not torch.is_tensor(stack) else stack)
    if x.dim() == 3:
        return x[:, None]
    if x.dim() == 4:
        return x.permute(0, 3, 1, 2) if x.shape[-1] <= 4 and x.shape[1] > 4 else x
    raise ValueError(f"{what} [Z,H,W], [Z,C,H,W] or [Z,H,W,C], got shape {tuple(x.shape)}")


def _label_masks(masks, method: str, volume: bool, nlab: int | None = None,
                 forms: str = "[B, H, W] masks or one [Z, H, W] volume"):
    """The ``masks`` argument of ``method`` (measure, outlines, surfaces) -> ``(m, nlab)``: a [B or Z,
    H, W] tensor (one [H, W] image is a batch of one, unless a volume is asked for) and the bound on
    the labels + 1, by default the ``label_bound`` the mask stage left on ``masks`` (else None)."""
    m = masks if torch.is_tensor(masks) else torch.as_tensor(np.asarray(masks))
    if m.dim() == 2 and not volume:
        m = m[None]
    if m.dim() != 3:
        raise ValueError(f"{method} expects {forms}, got shape {tuple(m.shape)}")
    return m, (getattr(masks, "label_bound", None) if nlab is None else nlab)


def measure_launch(m: torch.Tensor, img: torch.Tensor | None, volume: bool = False, nlab: int | None = None) -> dict:
    """Raw measurement fields of masks ``m`` [B, H, W] (or one [Z, H, W] volume) with ``img``
    [B or Z, C, H, W] on the same device, as tensors on that device: the HIP kernel on the GPU (queued
    on the current stream, nothing waited for when ``nlab`` is given), the numpy oracle elsewhere."""
    from .gpu import measure_masks_gpu

    return measure_masks_gpu(m, img, nlab=nlab, volume=volume)


def measure_tables(raws: dict, volume: bool = False):
    """Host side of :meth:`CellposeRunner.measure`: raw fields (tensors or arrays, [B, K, ...] or
    [K, ...] for a volume) -> one table per image, each cut to its image's own largest label."""
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in raws.items()}
    if volume:
        host = {k: v[None] for k, v in host.items()}
    tables = []
    for b in range(host["area"].shape[0]):
        present = np.nonzero(host["area"][b] > 0)[0]
        kb = int(present[-1]) + 1 if present.size else 0
        tables.append(ref.derive_measurements({k: (v[b] if k == "outlines" else v[b, :kb]) for k, v in host.items()}))
    return tables[0] if volume else tables


def surface_launch(m: torch.Tensor, spacing=(1.0, 1.0, 1.0), nlab: int | None = None) -> dict:
    """Surface mesh and statistics of one [Z, H, W] label volume on its device, as ``{"mesh",
    "stats"}`` of tensors: the HIP kernels on the GPU (on the current stream, which is waited for
    when the vertex and quad counts and, at the end, the error word are read), the numpy oracle
    elsewhere."""
    from .gpu import label_surface_gpu, surface_stats_gpu

    mesh = label_surface_gpu(m, nlab=nlab)
    return {"mesh": mesh, "stats": surface_stats_gpu(mesh, spacing)}


def surface_tables(raws: dict) -> dict:
    """Host side of :meth:`CellposeRunner.surfaces`: the tensors of :func:`surface_launch` as numpy."""
    return {part: {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in d.items()}
            for part, d in raws.items()}


def outline_launch(m: torch.Tensor, nlab: int | None = None, volume: bool = False) -> dict:
    """Outline rings of masks ``m`` [B, H, W] (or one [Z, H, W] volume, traced per plane) as the
    batch arrays of :func:`gpu.mask_rings_gpu`, on the masks' device: the HIP kernels on the GPU (on
    the current stream, which is waited for twice: for the vertex and for the ring count), the numpy
    oracle elsewhere."""
    from .gpu import mask_rings_gpu

    return mask_rings_gpu(m, nlab=nlab, volume=volume)


def outline_rings(raws: dict) -> list:
    """Host side of :meth:`CellposeRunner.outlines`: the batch arrays of :func:`outline_launch`
    (tensors or arrays) -> one rings dict per image, in the form of :func:`reference.mask_rings`
    (``verts``, ``ring_offsets`` starting at 0, ``ring_label``, ``ring_area2``)."""
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in raws.items()}
    off, per = host["ring_offsets"], host["image_rings"]
    out = []
    for b in range(per.shape[0] - 1):
        r0, r1 = int(per[b]), int(per[b + 1])
        v0, v1 = int(off[r0]), int(off[r1])
        out.append({"verts": host["verts"][v0:v1].copy(), "ring_offsets": off[r0:r1 + 1] - v0,
                    "ring_label": host["ring_label"][r0:r1].copy(), "ring_area2": host["ring_area2"][r0:r1].copy()})
    return out


def mask_stream(device) -> "torch.cuda.Stream":
    """The second stream mask recovery runs on, beside the next batch's network.
    ``BE_MASK_STREAM_PRIO`` (A/B): HIP stream priority, -1 = high (its kernels dispatch ahead of the
    queued conv workgroups), 0 = normal."""
    prio = int(os.environ.get("BE_MASK_STREAM_PRIO", "0"))
    return torch.cuda.Stream(device, priority=prio)


class _GroupNormEngine:
    """Inference for GroupNorm CPnets (e.g. sessions trained data-parallel): GroupNorm statistics are
    per image, so nothing folds into the weights; the HIP training engine's forward -- GN statistics
    kernel + fused conv per layer, no activations saved for a backward -- runs the tiles instead
    (one engine per tile-batch size).  Non-square tile grids fall back to bf16 autocast PyTorch."""

    def __init__(self, net: CPnet, device):
        import copy

        from ..parallel.ddp import FlatParams

        self.device = torch.device(device)
        self.net = copy.deepcopy(net).to(self.device).eval()
        self.fp = FlatParams(self.net, self.device) if self.device.type == "cuda" else None
        self._engs: dict = {}

    @torch.no_grad()
    def __call__(self, tiles: torch.Tensor):
        from ..train.cpnet_engine import CPnetTrainEngine

        T, by, bx, _ = tiles.shape
        x = tiles[..., : self.net.nchan].permute(0, 3, 1, 2).float()
        if by != bx or by % 16 or self.fp is None:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.device.type == "cuda"):
                y, style = self.net(x.contiguous())[:2]
            return y.float().contiguous(), style.float()
        eng = self._engs.get((T, by))
        if eng is None:
            eng = self._engs[(T, by)] = CPnetTrainEngine(self.net, self.fp, T, by, self.device)
        y = eng.forward(x)
        style = eng._act["style"].float()
        eng._act = None
        return y, style


def synthetic_cells(B: int, H: int = 512, W: int = 512, nchan: int = 2, ncells: int = 150, seed: int = 0) -> np.ndarray:
    """Synthetic fluorescence-like images [B, nchan, H, W] uint16: Gaussian blobs (cells) + nuclei + noise."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, nchan, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        cy = rng.uniform(0, H, ncells)
        cx = rng.uniform(0, W, ncells)
        r = rng.uniform(6, 14, ncells)
        img = np.zeros((H, W), np.float32)
        nuc = np.zeros((H, W), np.float32)
        for i in range(ncells):
            y0, y1 = int(max(0, cy[i] - 3 * r[i])), int(min(H, cy[i] + 3 * r[i]))
            x0, x1 = int(max(0, cx[i] - 3 * r[i])), int(min(W, cx[i] + 3 * r[i]))
            d2 = (yy[y0:y1, x0:x1] - cy[i]) ** 2 + (xx[y0:y1, x0:x1] - cx[i]) ** 2
            img[y0:y1, x0:x1] += np.exp(-d2 / (2 * r[i] ** 2))
            nuc[y0:y1, x0:x1] += np.exp(-d2 / (2 * (0.4 * r[i]) ** 2))
        out[b, 0] = img
        if nchan > 1:
            out[b, 1] = nuc
    out += 0.05 * rng.standard_normal(out.shape).astype(np.float32)
    out = np.clip(out, 0, None)
    return (out / out.max() * 4000).astype(np.uint16)


class _EvalStream:
    """See :meth:`CellposeRunner.stream` (GPU only; a CPU runner evaluates each batch directly)."""

    def __init__(self, runner: CellposeRunner, p: EvalParams):
        self.r, self.p = runner, p
        self.pending = None
        # "auto" is two dependent passes per batch: such a stream evaluates every batch directly
        self.cuda = runner.device.type == "cuda" and p.compute_masks and diameter_form(p.diameter) != "auto"

    @torch.no_grad()
    def submit(self, images):
        if not self.cuda:
            return self.r.eval(images, self.p)
        x, raw = as_batch(images, self.r.nchan, self.r.device, keep_raw=True)  # device tensors only: no shared pinned staging
        y, style, rescale = self.r._net_stage(x, self.p, raw)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.r.device))
        prev, self.pending = self.pending, (y, style, rescale, ev)
        return self._finish(prev) if prev is not None else None

    def _finish(self, item):
        y, style, rescale, ev = item
        main = torch.cuda.current_stream(self.r.device)
        m = self.r._masks_on_side_stream(y, self.p, rescale, ev)
        done = torch.cuda.Event()
        done.record(self.r._mask_stream)
        main.wait_event(done)  # consumers on the main stream see finished masks
        m.record_stream(main)
        return m, y, style

    def flush(self):
        if self.pending is None:
            return None
        prev, self.pending = self.pending, None
        return self._finish(prev)
