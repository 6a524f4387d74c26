"""IVF-PQ tier of the cell-image-search vector index (reference FAISS ``IndexIVFPQ``, m=96 x 8-bit
codes, nlist in [4096, 65536], nprobe=64: ``apps/cell-image-search/index_manager.py:67-89``; its README
quotes <100 ms per query at 58 M vectors, ``README.md:130-134``).

MI355X design:

* coarse quantizer: spherical k-means on the GPU (bf16 GEMMs), ``nlist`` lists;
* product quantizer on the residuals ``x - c_list``: ``m`` sub-spaces of ``D/m`` dims, 256 centroids
  each, trained with batched k-means (one ``bmm`` per iteration over all sub-spaces);
* codes ``[N, m]`` uint8 stored list-sorted, so each list is one contiguous slab of HBM -- 58 M
  vectors at m=96 are 5.6 GB, scanned for a query only in its ``nprobe`` lists;
* search: per query one ``[m, 256]`` fp16 lookup table of the query's sub-vectors against the codebooks; inner
  product, so the score is ``<q, c_list> + sum_j LUT[j][code_j]``.  ``search="scan"``: the table by ``bmm``, the
  HIP kernel ``be_ivfpq_scan`` (one workgroup per (query, list), the table in LDS) writes the scores of all
  candidates to HBM, then ``topk`` and a slot -> id lookup in torch.  ``search="fused"``
  (``csrc/kernels/ivfpq_search.hip``): ``be_ivfpq_lut`` makes the table, ``be_ivfpq_scan_topk`` scores equal
  slot ranges of the query's candidate row and keeps the best ``k`` in LDS under (score descending, list-sorted
  row ascending), ``be_ivfpq_merge`` joins the ranges and maps rows to ids: no score row in HBM and no host
  read before the ``[Q, k]`` result.  ``"auto"``: see :meth:`IVFPQIndex.fused_search`.  The coarse probe
  selection (``q @ centroids.T``, ``topk``) is torch on every path.

Build: ``build="torch"`` is the torch code below (batched ``bmm`` distances, ``argmin``); ``"fused"`` runs the PQ
codebook iterations and the residual encoding in ``csrc/kernels/pq_build.hip`` (``be_pq_kmeans_step``,
``be_pq_encode``: fp32 MFMA scores with the argmin inside the kernel, rows read in their stored dtype);
``"auto"`` takes the kernels on a GPU device when the library is loaded and ``D/m`` is 4 or 8.

Coarse quantizer (the nearest centroid of every row in ``add``, in the coarse k-means iterations and for the PQ
sample of ``train``): ``coarse="torch"`` is an fp32 ``x @ centroids.T`` and ``argmax``; ``"fused"``
(``csrc/kernels/coarse_assign.hip``) takes the best two split-bf16 MFMA scores per row inside the kernel, keeps the
rows whose gap proves the argmax (:func:`coarse_certificate_eps`) and gives the others to the torch rule; the
k-means update (``index_add_``) stays torch.  ``"auto"``: see :meth:`IVFPQIndex.fused_coarse`.

Everything has a CPU path (same math in torch) that the GPU kernel is tested against.
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np
import torch

from ..ops import _native
from .list_scan import candidate_offsets, scan_topk_merge, slot_rows


def _kmeans(x: torch.Tensor, k: int, iters: int, g: torch.Generator, spherical: bool, assign=None) -> torch.Tensor:
    """``assign(x, cent) -> [n] int64``: the spherical assignment, :func:`_argmax_ip` by default."""
    cent = x[torch.randperm(x.shape[0], generator=g)[:k].to(x.device)].clone()
    for _ in range(iters):
        if spherical:
            from .index import _argmax_ip

            a = (assign or _argmax_ip)(x, cent)
        else:
            a = torch.cdist(x, cent).argmin(1)
        new = torch.zeros_like(cent).index_add_(0, a, x)
        cnt = torch.bincount(a, minlength=k).to(x.dtype)
        empty = cnt == 0
        new = new / cnt.clamp(min=1)[:, None]
        new[empty] = cent[empty]
        cent = torch.nn.functional.normalize(new, dim=1) if spherical else new
    return cent


def _pq_train(res: torch.Tensor, m: int, iters: int, g: torch.Generator) -> torch.Tensor:
    """Batched k-means (256 centroids) in each of the m sub-spaces: res [S, D] -> codebooks [m, 256, D/m]."""
    S, D = res.shape
    ds = D // m
    x = res.view(S, m, ds).transpose(0, 1).contiguous()  # [m, S, ds]
    init = torch.randperm(S, generator=g)[:256].to(res.device)
    cb = x[:, init].clone()  # [m, 256, ds]
    for _ in range(iters):
        d = (x * x).sum(-1, keepdim=True) - 2 * torch.bmm(x, cb.transpose(1, 2)) + (cb * cb).sum(-1)[:, None, :]
        a = d.argmin(-1)  # [m, S]
        new = torch.zeros_like(cb)
        new.scatter_add_(1, a[..., None].expand(-1, -1, ds), x)
        cnt = torch.zeros(m, 256, device=res.device, dtype=res.dtype).scatter_add_(1, a, torch.ones_like(a, dtype=res.dtype))
        upd = cnt > 0
        cb = torch.where(upd[..., None], new / cnt.clamp(min=1)[..., None], cb)
    return cb


def _pq_encode(res: torch.Tensor, cb: torch.Tensor, chunk: int = 1 << 16) -> torch.Tensor:
    m, _, ds = cb.shape
    out = []
    cbn = (cb * cb).sum(-1)  # [m, 256]
    for i in range(0, res.shape[0], chunk):
        x = res[i:i + chunk].view(-1, m, ds).transpose(0, 1)  # [m, n, ds]
        d = cbn[:, None, :] - 2 * torch.bmm(x, cb.transpose(1, 2))
        out.append(d.argmin(-1).transpose(0, 1).to(torch.uint8))
    return torch.cat(out).contiguous()


# ------------------------------------------------------------------------------- fused build (pq_build.hip)
PQ_BUILDS = ("auto", "torch", "fused")
_PQ_TARGET_BLOCKS = 256  # workgroups of a k-means step: fixes its slab count, and with it its summation order


def pq_fused_supported(dim: int, m: int) -> bool:
    """Shapes ``be_pq_encode`` / ``be_pq_kmeans_step`` serve: sub-spaces of 4 or 8 dims, m a multiple of 16."""
    return m >= 16 and m % 16 == 0 and dim in (4 * m, 8 * m)


def _pq_fused_args(x: torch.Tensor, codebooks: torch.Tensor, what: str):
    if not (x.is_cuda and codebooks.is_cuda and _native.hip_available()):
        raise _native.NativeUnavailable(f"{what} needs GPU tensors and the native kernel library")
    m, k, ds = codebooks.shape
    if k != 256 or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != m * ds or not pq_fused_supported(m * ds, m):
        raise _native.NativeUnavailable(f"{what} serves [n >= 1, m * ds] rows with ds in (4, 8), m % 16 == 0 "
                                        "and 256 codewords")
    return m, ds


def pq_encode_fused(x: torch.Tensor, centroids: torch.Tensor, assign: torch.Tensor,
                    codebooks: torch.Tensor) -> torch.Tensor:
    """``be_pq_encode``: ``x [n, D]`` float32 or bfloat16, ``centroids [nlist, D]``, ``assign [n]``, ``codebooks
    [m, 256, D/m]`` -> codes ``[n, m]`` uint8 of the residuals ``fp32(x) - centroids[assign]``: per sub-space the
    argmin of ``|cb_k|^2 - 2 r.cb_k``, a tie to the smaller ``k``.  No distance reaches HBM, nothing is read back."""
    m, _ = _pq_fused_args(x, codebooks, "be_pq_encode")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    x = x.contiguous()
    cent = centroids.to(x.device, torch.float32).contiguous()
    a = assign.to(x.device, torch.int32).contiguous()
    cb = codebooks.float().contiguous()
    if a.shape != (x.shape[0],) or cent.shape[1] != x.shape[1]:
        raise ValueError("assign [n] and centroids [nlist, D] must match x [n, D]")
    codes = torch.empty(x.shape[0], m, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _native.call("be_pq_encode", _native.ptr(x), int(x.dtype == torch.bfloat16), _native.ptr(cent), _native.ptr(a),
                     _native.ptr(cb), x.shape[0], x.shape[1], m, cent.shape[0], _native.ptr(codes),
                     _native.stream(x.device))
    return codes


def pq_kmeans_step_fused(res: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """``be_pq_kmeans_step``: one Lloyd iteration of the codebooks ``[m, 256, D/m]`` over the residuals ``res [S, D]``
    (float32): assignment as :func:`pq_encode_fused`, sums and counts in a fixed order (no atomics: the same
    input gives the same bits), ``sum / count``; a codeword without rows keeps its value."""
    m, ds = _pq_fused_args(res, codebooks, "be_pq_kmeans_step")
    res = res.float().contiguous()
    cb = codebooks.float().contiguous()
    S = res.shape[0]
    slabs = max(1, min(-(-S // 128), _PQ_TARGET_BLOCKS // (m // 16)))
    part = torch.empty(slabs, m, 256, ds + 1, dtype=torch.float32, device=res.device)
    new = torch.empty_like(cb)
    with torch.cuda.device(res.device):
        _native.call("be_pq_kmeans_step", _native.ptr(res), _native.ptr(cb), S, res.shape[1], m, slabs,
                     _native.ptr(part), _native.ptr(new), _native.stream(res.device))
    return new


def _pq_train_fused(res: torch.Tensor, m: int, iters: int, g: torch.Generator) -> torch.Tensor:
    """:func:`_pq_train` with the iterations in ``be_pq_kmeans_step``: the same initial codewords."""
    S, D = res.shape
    init = torch.randperm(S, generator=g)[:256].to(res.device)
    cb = res[init].view(-1, m, D // m).transpose(0, 1).contiguous()  # [m, 256, ds]
    for _ in range(iters):
        cb = pq_kmeans_step_fused(res, cb)
    return cb


# ------------------------------------------------------------------------------- coarse quantizer (coarse_assign.hip)
PQ_COARSES = ("auto", "torch", "fused")


def coarse_fused_supported(dim: int) -> bool:
    """Row lengths ``be_coarse_top2`` serves: whole 32-element MFMA steps, up to 8192."""
    return 32 <= dim <= 8192 and dim % 32 == 0


def coarse_certificate_eps(d: int, parts: int) -> float:
    """How far the coarse score of ``be_coarse_top2`` can lie from the exact real inner product of a unit row and a
    unit centroid: ``(2 parts - 3) 2^-18 (1 + 2^-8) + (2 parts + 1) d 2^-24 + 128 * 2^-24``.  ``parts = 2``: bf16 rows,
    ``3``: fp32 rows.  With ``u = 2^-24``:

    * The split: ``c = hi + lo + r`` with ``|c - hi| <= 2^-9 |c|`` and ``|r| <= 2^-18 |c|`` per element (bf16 keeps 8
      significand bits, twice; ``c - hi`` is exact in fp32).  A bf16 row is its own ``hi``, so the sum ``x.hi + x.lo``
      drops only ``x.r``: ``<= 2^-18`` by Cauchy-Schwarz.  An fp32 row is split the same way and the sum
      ``x_hi.c_hi + x_hi.c_lo + x_lo.c_hi`` drops ``x_lo.c_lo``, ``(x_hi + x_lo).r_c`` and ``r_x.c``: each
      ``<= 2^-18 (1 + 2^-9)^2``.  That is ``2 parts - 3`` terms of at most ``2^-18 (1 + 2^-8)``.
    * The sum: its ``parts * d`` products of two bf16 values are exact in fp32.  Accumulating them in fp32, in
      whatever order the matrix unit uses, costs at most ``parts * d`` roundings of a partial sum that is bounded by
      the sum of the magnitudes, ``<= (1 + 2^-9)^2 (1 + 2^-8) < 1 + 2^-6`` (Cauchy-Schwarz per part).  The unit's adder
      is not documented to round to nearest, so a rounding is taken as a whole ulp, ``2 u``:
      ``2 parts d u (1 + 2^-6) / (1 - 2 parts d u) < (2 parts + 1) d u`` for ``d <= 8192``.
    * ``128 u`` of slack: the bound in use is ``eps |x| max|c|`` with norms computed in fp32 (each within
      ``(d / 2 + 2) u`` of the real one, relatively, in any summation order: the square root halves the sum's
      ``d u``), fp32 products and an fp32 ``s1 - s2``; against an ``eps`` below ``2^-7`` these are under
      ``(d + 8) 2^-7 u < 128 u``."""
    if parts not in (2, 3):
        raise ValueError("parts is 2 (bf16 rows) or 3 (fp32 rows)")
    return (2 * parts - 3) * 2.0 ** -18 * (1 + 2.0 ** -8) + ((2 * parts + 1) * d + 128) * 2.0 ** -24


def _coarse_top2(x: torch.Tensor, centroids: torch.Tensor):
    """:func:`coarse_top2_fused` and, as a device scalar, the largest centroid norm ``be_coarse_split`` found."""
    if not (x.is_cuda and centroids.is_cuda and _native.hip_available()):
        raise _native.NativeUnavailable("be_coarse_top2 needs GPU tensors and the native kernel library")
    if (x.dim() != 2 or centroids.dim() != 2 or x.shape[1] != centroids.shape[1] or not coarse_fused_supported(x.shape[1])
            or not 1 <= x.shape[0] < 2 ** 31 or not 1 <= centroids.shape[0] < 2 ** 31):
        raise _native.NativeUnavailable("be_coarse_top2 serves x [n >= 1, D] against centroids [nlist >= 1, D] with "
                                        "D % 32 == 0, D <= 8192 and fewer than 2^31 of each")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    x = x.contiguous()
    cent = centroids.to(x.device, torch.float32).contiguous()
    n, D = x.shape
    nlist = cent.shape[0]
    image = torch.empty(nlist, 2 * D, dtype=torch.bfloat16, device=x.device)
    cmax = torch.zeros(1, dtype=torch.float32, device=x.device)
    i1 = torch.empty(n, dtype=torch.int32, device=x.device)
    s1 = torch.empty(n, dtype=torch.float32, device=x.device)
    s2 = torch.empty(n, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _native.call("be_coarse_split", _native.ptr(cent), nlist, D, _native.ptr(image), _native.ptr(cmax),
                     _native.stream(x.device))
        _native.call("be_coarse_top2", _native.ptr(x), int(x.dtype == torch.bfloat16), _native.ptr(image), n, nlist, D,
                     _native.ptr(i1), _native.ptr(s1), _native.ptr(s2), _native.stream(x.device))
    return i1, s1, s2, cmax


def coarse_top2_fused(x: torch.Tensor, centroids: torch.Tensor):
    """``be_coarse_split`` + ``be_coarse_top2``: ``x [n, D]`` bfloat16 or float32, ``centroids [nlist, D]`` -> per row
    ``(i1 int32, s1 fp32, s2 fp32)``: the column of the largest coarse score under (score descending, index
    ascending), that score, and the largest coarse score among the other columns (``-inf`` at ``nlist == 1``).  The
    coarse score is one fp32 MFMA accumulator over ``x.c_hi + x.c_lo`` (bf16 rows) or ``x_hi.c_hi + x_hi.c_lo +
    x_lo.c_hi`` (fp32 rows).  No score reaches HBM, nothing is read back."""
    return _coarse_top2(x, centroids)[:3]


def coarse_assign_fused(x: torch.Tensor, centroids: torch.Tensor):
    """Nearest centroid by inner product -> ``(assign int64 [n], fallback_rows)``.  A row is certified when
    ``s1 - s2 > 2 eps |x| max|c|`` (:func:`coarse_certificate_eps`): every score is within ``eps |x| max|c|`` of the
    exact one, so no other centroid can have a larger exact score and ``i1`` is the true argmax.  The other rows
    (near-ties, exact ties, duplicate centroids) are gathered and get ``_argmax_ip`` of their fp32 values, the torch
    rule: one host read of their count per call."""
    from .index import _argmax_ip

    i1, s1, s2, cmax = _coarse_top2(x, centroids)
    eps = coarse_certificate_eps(x.shape[1], 2 if x.dtype == torch.bfloat16 else 3)
    bound = torch.linalg.vector_norm(x, dim=1, dtype=torch.float32) * cmax * (2.0 * eps)
    rows = torch.nonzero(~(s1 - s2 > bound)).squeeze(1)  # a NaN score is not certified either
    assign = i1.long()
    if rows.numel():
        assign[rows] = _argmax_ip(x[rows].float(), centroids.to(x.device, torch.float32))
    return assign, int(rows.numel())


def _auto_coarse(nlist: int, dim: int) -> bool:
    """The shapes at which ``coarse="auto"`` takes the fused path: those between the measured ones, at all of which it
    was faster than ``"torch"`` by more than both arms' spread (README, "IVF-PQ coarse quantizer": D = 768, 4 096 and
    12 649 lists, bf16 rows in ``add`` and fp32 rows in ``train``)."""
    return dim == 768 and 4096 <= nlist <= 12649


# ------------------------------------------------------------------------------- fused search (ivfpq_search.hip)
PQ_SEARCHES = ("auto", "scan", "fused")
PQ_SEARCH_M = (16, 32, 48, 64, 96, 128, 192)  # table sizes be_ivfpq_scan_topk is instantiated for
PQ_SEARCH_MAX_K = 1024
_PQ_SEARCH_BLOCKS = 256  # workgroups of a scan: one per CU


def ivfpq_splits(Q: int, nprobe: int, kk: int) -> int:
    """Slot ranges per query of ``be_ivfpq_scan_topk``, from the call's shape alone: about ``_PQ_SEARCH_BLOCKS``
    workgroups, at most 16 per query (``be_ivfpq_merge`` takes the ranges one after the other; measured at 10 M rows,
    a single query: 16 ranges 71 us, 64 ranges 110 us) and at most ``16384 / kk``."""
    return max(1, min(16, _PQ_SEARCH_BLOCKS // max(Q, 1), 16384 // kk))


def _auto_fused(m: int, Q: int, k: int) -> bool:
    """The shapes at which ``search="auto"`` takes the fused path: those between the measured ones, at all of which it
    was faster than ``"scan"`` (README, "IVF-PQ search": m = 96 and 192, 1 and 64 queries, k = 20 to 1000)."""
    return m in (96, 192) and Q <= 64


def ivfpq_lut_fused(q: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """``be_ivfpq_lut``: ``q [Q, m * ds]``, ``codebooks [m, 256, ds]`` -> the fp16 table ``[Q, m, 256]``, entry
    ``half_rn`` of one ``fmaf`` chain in ascending ``i`` (the same input gives the same bits)."""
    if not (q.is_cuda and codebooks.is_cuda and _native.hip_available()):
        raise _native.NativeUnavailable("be_ivfpq_lut needs GPU tensors and the native kernel library")
    if codebooks.dim() != 3 or codebooks.shape[1] != 256 or q.dim() != 2 or q.shape[1] != codebooks.shape[0] * codebooks.shape[2]:
        raise _native.NativeUnavailable("be_ivfpq_lut serves q [Q, m * ds] against codebooks [m, 256, ds]")
    m, _, ds = codebooks.shape
    q = q.float().contiguous()
    cb = codebooks.float().contiguous()
    lut = torch.empty(q.shape[0], m, 256, dtype=torch.float16, device=q.device)
    with torch.cuda.device(q.device):
        _native.call("be_ivfpq_lut", _native.ptr(q), _native.ptr(cb), q.shape[0], m, ds, _native.ptr(lut),
                     _native.stream(q.device))
    return lut


def ivfpq_scan_topk_fused(lut_half: torch.Tensor, base: torch.Tensor, probes: torch.Tensor, list_off: torch.Tensor,
                          codes: torch.Tensor, ids: torch.Tensor, kk: int, splits: int | None = None):
    """``be_ivfpq_scan_topk`` + ``be_ivfpq_merge``: the ``kk`` best of ``base[q, p] + sum_j lut[q, j, code_j]`` over the
    rows of the probed lists, ordered by (score descending, list-sorted row ascending) -> ``(scores [Q, kk] fp32,
    ids [Q, kk] int64)`` on the device, ``-inf`` / ``-1`` in empty slots.  ``splits`` forces the slot ranges per
    query (:func:`ivfpq_splits`).  Nothing is read back."""
    t = (lut_half, base, probes, list_off, codes, ids)
    if not (all(x.is_cuda for x in t) and _native.hip_available()):
        raise _native.NativeUnavailable("be_ivfpq_scan_topk needs GPU tensors and the native kernel library")
    Q, nprobe = probes.shape
    m = codes.shape[1]
    if (m not in PQ_SEARCH_M or not 1 <= kk <= PQ_SEARCH_MAX_K or codes.shape[0] >= 2 ** 31 or nprobe < 1
            or lut_half.dtype != torch.float16 or lut_half.shape != (Q, m, 256) or codes.dtype != torch.uint8):
        raise _native.NativeUnavailable(f"be_ivfpq_scan_topk serves m in {PQ_SEARCH_M}, 1 <= kk <= {PQ_SEARCH_MAX_K}, "
                                        "fewer than 2^31 rows and an fp16 table [Q, m, 256]")
    list_off = list_off.long().contiguous()
    P = int(splits) if splits else ivfpq_splits(Q, nprobe, kk)

    def launch(cand_off, part_s, part_r):
        _native.call("be_ivfpq_scan_topk", _native.ptr(lut_half.contiguous()), _native.ptr(base.float().contiguous()),
                     _native.ptr(probes.int().contiguous()), _native.ptr(list_off), _native.ptr(cand_off),
                     _native.ptr(codes.contiguous()), codes.shape[0], Q, nprobe, m, kk, P, _native.ptr(part_s),
                     _native.ptr(part_r), _native.stream(codes.device))

    return scan_topk_merge(launch, list_off, probes, ids, kk, P, merge="be_ivfpq_merge")


class IVFPQIndex:
    """Approximate inner-product index; vectors should be L2-normalised (cosine).  ``build``: how the PQ
    codebooks are trained and the rows encoded, one of ``PQ_BUILDS``; ``search``: how the probed lists are scanned,
    one of ``PQ_SEARCHES``; ``coarse``: how rows find their list in ``train`` / ``add``, one of ``PQ_COARSES`` (module
    docstring).  ``coarse_fallback_rows`` counts the rows the fused coarse quantizer could not certify and
    recomputed by the torch rule."""

    def __init__(self, dim: int = 768, nlist: int = 4096, m: int = 96, nprobe: int = 64, device=None,
                 build: str = "auto", search: str = "auto", coarse: str = "auto"):
        if dim % m or m % 16:
            raise ValueError("dim must be divisible by m, and m a multiple of 16")
        if build not in PQ_BUILDS:
            raise ValueError(f"build must be one of {PQ_BUILDS}")
        if search not in PQ_SEARCHES:
            raise ValueError(f"search must be one of {PQ_SEARCHES}")
        if coarse not in PQ_COARSES:
            raise ValueError(f"coarse must be one of {PQ_COARSES}")
        self.dim, self.nlist, self.m, self.nprobe = dim, nlist, m, nprobe
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        self.centroids: torch.Tensor | None = None  # [nlist, D] fp32
        self.codebooks: torch.Tensor | None = None  # [m, 256, D/m] fp32
        self.codes = torch.empty(0, m, dtype=torch.uint8, device=self.device)  # list-sorted
        self.ids = torch.empty(0, dtype=torch.int64, device=self.device)  # original id per sorted row
        self.list_off = torch.zeros(nlist + 1, dtype=torch.int64, device=self.device)
        self._assign = torch.empty(0, dtype=torch.int32, device=self.device)
        self._raw_codes = torch.empty(0, m, dtype=torch.uint8, device=self.device)
        self.ntotal = 0
        self.build = build
        self.fused_build  # "fused" where the kernels cannot run: raise now, not in the middle of a build
        self.search_mode = search
        self.fused_search(1, 1)  # the same for search="fused"
        self.coarse = coarse
        self.coarse_fallback_rows = 0
        self.fused_coarse(nlist)  # and for coarse="fused"

    @property
    def fused_build(self) -> bool:
        """Whether train / add run on ``pq_build.hip``."""
        if self.build == "torch":
            return False
        ok = self.device.type == "cuda" and pq_fused_supported(self.dim, self.m) and _native.hip_available()
        if self.build == "fused" and not ok:
            raise _native.NativeUnavailable("build='fused' needs a GPU device, the native kernel library and "
                                            "sub-spaces of 4 or 8 dims")
        return ok

    def fused_search(self, Q: int, k: int) -> bool:
        """Whether a search of ``Q`` queries for ``k`` results runs on ``ivfpq_search.hip``.  ``"fused"``: always, or
        it raises; ``"auto"``: where the kernels can run and ``_auto_fused`` holds."""
        if self.search_mode == "scan":
            return False
        ok = self.device.type == "cuda" and self.m in PQ_SEARCH_M and _native.hip_available()
        if self.search_mode == "fused":
            if not ok:
                raise _native.NativeUnavailable(f"search='fused' needs a GPU device, the native kernel library and "
                                                f"m in {PQ_SEARCH_M}")
            if k > PQ_SEARCH_MAX_K:
                raise _native.NativeUnavailable(f"search='fused' keeps at most {PQ_SEARCH_MAX_K} results per query")
            return True
        return ok and k <= PQ_SEARCH_MAX_K and _auto_fused(self.m, Q, k)

    def fused_coarse(self, nlist: int) -> bool:
        """Whether an assignment against ``nlist`` centroids runs on ``coarse_assign.hip``.  ``"fused"``: always, or it
        raises; ``"auto"``: where the kernels can run and ``_auto_coarse`` holds."""
        if self.coarse == "torch":
            return False
        ok = self.device.type == "cuda" and coarse_fused_supported(self.dim) and _native.hip_available()
        if self.coarse == "fused":
            if not ok:
                raise _native.NativeUnavailable("coarse='fused' needs a GPU device, the native kernel library and "
                                                "dim % 32 == 0, dim <= 8192")
            return True
        return ok and _auto_coarse(nlist, self.dim)

    def _coarse_assign(self, x: torch.Tensor, cent: torch.Tensor) -> torch.Tensor:
        """Nearest centroid of the rows ``x`` (fp32, or bf16 as stored) -> int64 ``[n]``."""
        if self.fused_coarse(cent.shape[0]):
            a, fallback = coarse_assign_fused(x, cent)
            self.coarse_fallback_rows += fallback
            return a
        from .index import _argmax_ip

        return _argmax_ip(x.float(), cent)

    @property
    def index_type(self) -> str:
        return f"IVFPQ-GPU(nlist={self.nlist}, m={self.m}, nbits=8)"

    # ------------------------------------------------------------------ build
    def train(self, x, iters: int = 10, pq_iters: int = 12, seed: int = 0, max_sample: int = 262_144,
              pq_sample: int = 65_536) -> None:
        x = torch.as_tensor(x).to(self.device, torch.float32)
        g = torch.Generator().manual_seed(seed)
        n = x.shape[0]
        sample = x[torch.randperm(n, generator=g)[: min(n, max(max_sample, 39 * self.nlist))].to(self.device)]
        self.centroids = _kmeans(sample, min(self.nlist, sample.shape[0]), iters, g, spherical=True,
                                 assign=self._coarse_assign)
        self.nlist = self.centroids.shape[0]
        self.list_off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        ps = sample[:pq_sample]  # PQ codebooks: 256 centroids per sub-space need far fewer points
        a = self._coarse_assign(ps, self.centroids)
        self.codebooks = (_pq_train_fused if self.fused_build else _pq_train)(ps - self.centroids[a], self.m, pq_iters, g)

    def add(self, x, chunk: int = 1 << 18) -> None:
        assert self.centroids is not None, "train() first"
        x = torch.as_tensor(x)
        fused = self.fused_build
        assigns, codes = [], []
        for i in range(0, x.shape[0], chunk):
            if fused and x.dtype == torch.bfloat16:
                # the kernels read the stored bf16 rows; only a torch coarse assignment sees an fp32 copy of the chunk
                xs = x[i:i + chunk].to(self.device)
            else:
                xs = x[i:i + chunk].to(self.device, torch.float32)
            a = self._coarse_assign(xs, self.centroids)
            if fused:
                codes.append(pq_encode_fused(xs, self.centroids, a, self.codebooks))
            else:
                codes.append(_pq_encode(xs - self.centroids[a], self.codebooks))
            assigns.append(a.int())
        self._assign = torch.cat([self._assign] + assigns)
        raw = torch.cat([self._raw()] + codes)
        self.ntotal = int(self._assign.shape[0])
        order = torch.argsort(self._assign, stable=True)
        self.codes = raw[order].contiguous()
        self.ids = order
        # id-order codes are not kept: the list-sorted copy + ids reconstruct them (_raw), so the GPU
        # holds m + 12 bytes per vector (204 B at m = 192: 11.8 GB at 58 M)
        self._raw_codes = None
        del raw
        counts = torch.bincount(self._assign.long(), minlength=self.nlist)
        self.list_off = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])

    def _raw(self) -> torch.Tensor:
        """Codes in id order [N, m]."""
        if self._raw_codes is not None:
            return self._raw_codes
        raw = torch.empty_like(self.codes)
        raw[self.ids] = self.codes
        return raw

    def gpu_bytes(self) -> int:
        t = [self.codes, self.ids, self._assign, self.centroids, self.codebooks, self.list_off]
        return int(sum(x.numel() * x.element_size() for x in t if x is not None))

    # ------------------------------------------------------------------ search
    def _lut(self, q: torch.Tensor) -> torch.Tensor:
        """[Q, m, 256]: <q_j, codebook_j[k]>."""
        Q = q.shape[0]
        ds = self.dim // self.m
        qs = q.view(Q, self.m, ds).transpose(0, 1)  # [m, Q, ds]
        return torch.bmm(qs, self.codebooks.transpose(1, 2)).transpose(0, 1).contiguous()  # [m,Q,256] -> [Q,m,256]

    @torch.no_grad()
    def search(self, q, k: int = 20, nprobe: int | None = None):
        """q [Q, D] -> (scores [Q, k] fp32 numpy, ids [Q, k] int64 numpy; -1 = empty slot)."""
        q = torch.as_tensor(np.asarray(q, np.float32) if not torch.is_tensor(q) else q).to(self.device, torch.float32)
        if q.dim() == 1:
            q = q[None]
        Q = q.shape[0]
        if self.fused_search(Q, k):
            ts, ids = self._search_fused(q, k, nprobe)
            return ts.cpu().numpy(), ids.cpu().numpy()
        nprobe = min(nprobe or self.nprobe, self.nlist)
        cs = q @ self.centroids.T
        base, probes = torch.topk(cs, nprobe, dim=1)
        sizes, cand_off = candidate_offsets(self.list_off, probes)
        tot = sizes.sum(1)
        stride = int(tot.max()) if Q else 0
        S = np.full((Q, k), -np.inf, np.float32)
        I = np.full((Q, k), -1, np.int64)
        if stride == 0:
            return S, I
        lut = self._lut(q)
        out = torch.full((Q, stride), -float("inf"), dtype=torch.float32, device=self.device)
        if self.device.type == "cuda":
            _native.call("be_ivfpq_scan", _native.ptr(lut.half().contiguous()), _native.ptr(base.contiguous()),
                         _native.ptr(probes.int().contiguous()), _native.ptr(self.list_off), _native.ptr(cand_off),
                         _native.ptr(self.codes), Q, nprobe, self.m, stride, _native.ptr(out), _native.stream(self.device))
        else:
            self._scan_reference(lut, base, probes, cand_off, out)
        kk = min(k, stride)
        ts, ti = torch.topk(out, kk, dim=1)
        # candidate slot -> list-sorted row -> original id
        rows = slot_rows(self.list_off, probes, cand_off, ti)
        ids = torch.where(torch.isfinite(ts), self.ids[rows.clamp(min=0)], torch.full_like(rows, -1))
        S[:, :kk] = ts.cpu().numpy()
        I[:, :kk] = ids.cpu().numpy()
        return S, I

    def _search_fused(self, q: torch.Tensor, k: int, nprobe: int | None):
        """q [Q, D] fp32 on the device -> (scores [Q, k], ids [Q, k]) on the device; no host read on the way."""
        Q = q.shape[0]
        nprobe = min(nprobe or self.nprobe, self.nlist)
        if Q == 0 or self.codes.shape[0] == 0:
            return (torch.full((Q, k), -float("inf"), device=self.device),
                    torch.full((Q, k), -1, dtype=torch.int64, device=self.device))
        base, probes = torch.topk(q @ self.centroids.T, nprobe, dim=1)
        return ivfpq_scan_topk_fused(ivfpq_lut_fused(q, self.codebooks), base, probes, self.list_off, self.codes,
                                     self.ids, k)

    @torch.no_grad()
    def search_device(self, q, k: int = 20, nprobe: int | None = None):
        """:meth:`search` with the results left on the index device as tensors (the re-rank shortlist of
        ``VectorIndex.search``)."""
        q = torch.as_tensor(np.asarray(q, np.float32) if not torch.is_tensor(q) else q).to(self.device, torch.float32)
        if q.dim() == 1:
            q = q[None]
        if self.fused_search(q.shape[0], k):
            return self._search_fused(q, k, nprobe)
        S, I = self.search(q, k, nprobe)
        return torch.from_numpy(S).to(self.device), torch.from_numpy(I).to(self.device)

    def _scan_reference(self, lut, base, probes, cand_off, out):
        """torch oracle of be_ivfpq_scan (same fp16 table)."""
        lh = lut.half().float()
        for qi in range(probes.shape[0]):
            for pi in range(probes.shape[1]):
                l = int(probes[qi, pi])
                a, b = int(self.list_off[l]), int(self.list_off[l + 1])
                if a == b:
                    continue
                c = self.codes[a:b].long()  # [n, m]
                s = lh[qi].gather(1, c.T).sum(0) + base[qi, pi]
                o = int(cand_off[qi, pi])
                out[qi, o:o + (b - a)] = s

    # ------------------------------------------------------------------ persistence
    def save(self, out_dir) -> dict:
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        np.save(out / "ivfpq_centroids.npy", self.centroids.cpu().numpy())
        np.save(out / "ivfpq_codebooks.npy", self.codebooks.cpu().numpy())
        np.save(out / "ivfpq_codes.npy", self._raw().cpu().numpy())
        np.save(out / "ivfpq_assign.npy", self._assign.cpu().numpy())
        info = {"n_cells": self.ntotal, "embed_dim": self.dim, "index_type": self.index_type, "nprobe": self.nprobe,
                "index_size_mb": round(self.codes.numel() / 2 ** 20, 3)}
        (out / "ivfpq_info.json").write_text(json.dumps(info, indent=2))
        return info

    @classmethod
    def load(cls, out_dir, device=None, search: str = "auto") -> "IVFPQIndex":
        out = Path(out_dir)
        info = json.loads((out / "ivfpq_info.json").read_text())
        cent = np.load(out / "ivfpq_centroids.npy")
        cb = np.load(out / "ivfpq_codebooks.npy")
        idx = cls(dim=info["embed_dim"], nlist=cent.shape[0], m=cb.shape[0], nprobe=info.get("nprobe", 64), device=device,
                  search=search)
        idx.centroids = torch.from_numpy(cent).to(idx.device)
        idx.codebooks = torch.from_numpy(cb).to(idx.device)
        codes = torch.from_numpy(np.load(out / "ivfpq_codes.npy")).to(idx.device)
        assign = torch.from_numpy(np.load(out / "ivfpq_assign.npy")).to(idx.device)
        idx._assign = assign
        idx.ntotal = int(assign.shape[0])
        order = torch.argsort(assign, stable=True)
        idx.codes, idx.ids = codes[order].contiguous(), order
        idx._raw_codes = None
        counts = torch.bincount(assign.long(), minlength=idx.nlist)
        idx.list_off = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
        return idx


def default_nlist(n: int) -> int:
    """Reference range nlist in [4096, 65536] around 4*sqrt(N) (FAISS guideline)."""
    return int(min(65536, max(4096, 4 * math.sqrt(max(n, 1)))))
