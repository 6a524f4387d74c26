"""GPU vector index for L2-normalised embeddings (inner product = cosine).

Replaces the reference's FAISS indexes (apps/cell-image-search/index_manager.py:36-182,
SURVEY.md K20) with an HBM-resident design: MI355X holds 288 GB, i.e. ~180 M 768-d bf16 vectors,
so exact search is one bf16 GEMM (hipBLASLt) per query batch plus a top-k, streamed over
fixed-size chunks.  Past ``ivf_threshold`` vectors an IVF layer (spherical k-means on the GPU,
``nlist ~ 4 sqrt(N)``, ``nprobe = 64`` as in the reference) restricts each query to its closest
lists, whose list-sorted bf16 slabs are scored EXACTLY by the HIP scan kernel
(``csrc/kernels/ivf_scan.hip``) -- the reference needs 8-bit PQ codes at this size because it is
CPU/DRAM bound; on one 288 GB GPU the full vectors fit, so recall is limited only by probing.  The
compressed IVF-PQ tier (``search/ivfpq.py``) is kept for collections that do not fit:
:meth:`VectorIndex.compress` keeps only the PQ codes on the GPU (m=192: 192 B per vector, 11 GB at
58 M) and moves the full vectors to HOST memory, where the PQ shortlist (``refine * k``
candidates) is gathered and re-scored exactly on the GPU -- FAISS ``IndexRefineFlat`` with the
refine store off the device.  Storage is plain ``.npy`` + JSON (no pickles).

Layout at ``<workspace>/cell_search/``: ``vectors.npy`` (fp16 [N, D]), ``index_info.json``,
``ivf_centroids.npy`` / ``ivf_assign.npy`` (IVF only), ``metadata.parquet``, ``thumbnails.npy``.
"""
from __future__ import annotations

import json
import math
import time
from pathlib import Path

import numpy as np
import torch

from .flat import FLAT_MAX_K, FLAT_SQ8_MAX_K, flat_scan_topk_fused, flat_sq8_scan_topk_fused
from .list_scan import candidate_offsets, scan_topk_merge, slot_rows

CHUNK = 1 << 20  # database rows per GEMM chunk


def _scores(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """q [Q, D] x v [n, D] -> fp32 [Q, n].  bf16 GEMMs keep fp32 outputs (``mm.dtype``): bf16-rounded
    scores (8 mantissa bits, ~0.004 near 1.0) tie near-duplicate neighbours and scramble the top-k."""
    if q.is_cuda and q.dtype == torch.bfloat16:
        return torch.mm(q, v.T, out_dtype=torch.float32)
    return (q @ v.T).float()


def _argmax_ip(x: torch.Tensor, cent: torch.Tensor, budget: int = 1 << 30) -> torch.Tensor:
    """Nearest centroid by inner product, in row chunks sized so the [rows, nlist] score block stays
    under ``budget`` elements (at 58 M x 30 k lists an unchunked product would be ~7 TB)."""
    cent = cent.to(x.dtype)
    rows = max(1, min(x.shape[0], budget // max(1, cent.shape[0])))
    return torch.cat([(x[i:i + rows] @ cent.T).argmax(1) for i in range(0, x.shape[0], rows)])


# ------------------------------------------------------------------------------- fused IVF-Flat search (ivf_scan_topk.hip)
IVF_SEARCHES = ("auto", "scan", "fused")
IVF_SEARCH_CH = (1, 2, 3, 4, 6, 8)  # dim / 128 be_ivf_scan_bf16 and be_ivf_scan_topk are instantiated for
IVF_SEARCH_MAX_K = 1024
_IVF_SEARCH_BLOCKS = 512  # workgroups of a scan: two per CU, the occupancy the kernel is built for


def ivf_splits(Q: int, kk: int) -> int:
    """Slot ranges per query of ``be_ivf_scan_topk``, from the call's shape alone: about ``_IVF_SEARCH_BLOCKS``
    workgroups over all queries, and partial lists of at most 2^20 keys per query.  Measured at D = 768, nprobe 64
    (device time of scan + merge + the wrapper's index arithmetic, us, at 1 M / 10 M rows): one query, kk = 20:
    137 / 195 at P = 16, 99 / 112 at 64, 96 / 105 at 256, 108 / 89 at 512, 94 / 96 at 1024, 113 / 112 at 2048;
    kk = 1000: 182 / 273 at 64, 167 / 238 at 256, 166 / 232 at 512, 184 / 246 at 1024; 64 queries, kk = 20:
    488 / 1520 at P = 2, 315 / 993 at 4, 310 / 945 at 8, 312 / 920 at 16, 315 / 900 at 32, 335 / 881 at 64;
    kk = 1000: 463 / 1154 at 4, 443 / 1080 at 8, 450 / 1105 at 16, 463 / 1178 at 32."""
    return max(1, min(_IVF_SEARCH_BLOCKS // max(Q, 1), (1 << 20) // kk))


def _auto_ivf_fused(dim: int, n: int, Q: int, k: int) -> bool:
    """The shapes at which ``ivf_search="auto"`` takes the fused path: those between the measured ones at which it
    was faster than ``"scan"`` by more than both arms' spread (README, "IVF-Flat search": D = 768, 1 M and 10 M rows,
    1 and 64 queries, k = 20 and 80; at k = 1000 the gap at 10 M rows and one query was inside the scan arm's spread)."""
    return dim == 768 and 1_000_000 <= n <= 10_000_000 and Q <= 64 and k <= 80


def ivf_scan_topk_fused(q: torch.Tensor, probes: torch.Tensor, list_off: torch.Tensor, lvecs: torch.Tensor,
                        sorted_ids: torch.Tensor, kk: int, splits: int | None = None):
    """``be_ivf_scan_topk`` + ``be_topk_merge``: the ``kk`` best exact inner products of ``q [Q, D]`` (fp32) with the
    rows of the probed lists in the list-sorted bf16 ``lvecs [N, D]``, ordered by (score descending, list-sorted row
    ascending) -> ``(scores [Q, kk] fp32, ids [Q, kk] int64)`` on the device, rows mapped through ``sorted_ids``,
    ``-inf`` / ``-1`` in empty slots.  A score is bit-equal to the one ``be_ivf_scan_bf16`` writes for that row.
    ``splits`` forces the slot ranges per query (:func:`ivf_splits`).  Nothing is read back."""
    from ..ops import _native

    t = (q, probes, list_off, lvecs, sorted_ids)
    if not (all(x.is_cuda for x in t) and _native.hip_available()):
        raise _native.NativeUnavailable("be_ivf_scan_topk needs GPU tensors and the native kernel library")
    if (q.dim() != 2 or probes.dim() != 2 or lvecs.dim() != 2 or probes.shape[0] != q.shape[0]
            or lvecs.shape[1] != q.shape[1] or q.shape[1] % 128 or q.shape[1] // 128 not in IVF_SEARCH_CH
            or lvecs.dtype != torch.bfloat16 or not 1 <= kk <= IVF_SEARCH_MAX_K or lvecs.shape[0] >= 2 ** 31
            or probes.shape[1] < 1 or sorted_ids.shape[0] != lvecs.shape[0]):
        raise _native.NativeUnavailable(f"be_ivf_scan_topk serves bf16 rows of dim / 128 in {IVF_SEARCH_CH}, "
                                        f"1 <= kk <= {IVF_SEARCH_MAX_K}, fewer than 2^31 rows and nprobe >= 1")
    Q, nprobe = probes.shape
    list_off = list_off.long().contiguous()
    P = int(splits) if splits else ivf_splits(Q, kk)

    def launch(cand_off, part_s, part_r):
        _native.call("be_ivf_scan_topk", _native.ptr(q.float().contiguous()), _native.ptr(probes.int().contiguous()),
                     _native.ptr(list_off), _native.ptr(cand_off), _native.ptr(lvecs.contiguous()), lvecs.shape[0], Q,
                     nprobe, q.shape[1], kk, P, _native.ptr(part_s), _native.ptr(part_r), _native.stream(lvecs.device))

    return scan_topk_merge(launch, list_off, probes, sorted_ids, kk, P)


# ------------------------------------------------------------------------------- fused flat search (flat_scan_topk.hip)
FLAT_SEARCHES = ("auto", "gemm", "fused")


def _auto_flat_fused(dim: int, n: int, Q: int, k: int) -> bool:
    """The shapes at which ``flat_search="auto"`` takes the fused path: those between the measured ones at which it
    was faster than ``"gemm"`` by more than both arms' spread (README, "Flat search": D = 768, 100 k / 1 M / 5 M rows,
    1 and 64 queries, k = 20 and 100).  One query won at all six shapes; 64 queries won at k = 20 from 1 M rows on, tied
    at 100 k rows and lost or tied at k = 100."""
    if dim != 768 or not 100_000 <= n <= 5_000_000:
        return False
    return k <= 100 if Q == 1 else Q <= 64 and k <= 20 and n >= 1_000_000


class VectorIndex:
    """Tiers (reference FlatIP / IVFFlat / IVFPQ): ``index_type="auto"`` keeps exact bf16 search up
    to ``ivf_threshold`` vectors, IVF-Flat above it and IVF-PQ (``search/ivfpq.py``, m=96 x 8 bit)
    from ``ivfpq_threshold``; ``"flat"`` / ``"ivf"`` / ``"ivfpq"`` force a tier.  ``"ivfsq8"`` (never picked by
    ``"auto"``) is IVF with a list-sorted int8 copy in place of the list-sorted bf16 one (``search/sq8.py``): 3 D bytes
    per vector, the ``refine * k`` best int8 scores re-ranked exactly from the stored rows on the device.
    ``"flatsq8"`` (never picked by ``"auto"`` either) is the flat tier over an id-ordered int8 copy next to the bf16
    rows (``csrc/kernels/flat_sq8_scan_topk.hip``): no lists, every row scored by an int8 MFMA scan, the same re-rank;
    ``3 D + 4`` bytes per vector, so it buys speed and no memory."""

    def __init__(self, dim: int = 768, device=None, ivf_threshold: int = 5_000_000, nprobe: int = 64,
                 index_type: str = "auto", ivfpq_threshold: int = 50_000_000, pq_m: int = 96, refine: int = 4,
                 pq_build: str = "auto", pq_search: str = "auto", pq_coarse: str = "auto", ivf_search: str = "auto",
                 flat_search: str = "auto"):
        if ivf_search not in IVF_SEARCHES:
            raise ValueError(f"ivf_search must be one of {IVF_SEARCHES}")
        if flat_search not in FLAT_SEARCHES:
            raise ValueError(f"flat_search must be one of {FLAT_SEARCHES}")
        self.lvecs: torch.Tensor | None = None
        # int8 codes [N, D] and fp32 scales [N]: list-sorted ("ivfsq8") or in id order ("flatsq8")
        self.sq_codes: torch.Tensor | None = None
        self.sq_scales: torch.Tensor | None = None
        self.dim = dim
        self.refine = refine  # IVF-PQ, IVF-SQ8: re-rank refine*k candidates with the stored vectors (0 = off)
        self.kind = index_type
        self.ivfpq_threshold = ivfpq_threshold
        self.pq_m = pq_m
        self.pq_build = pq_build  # IVFPQIndex(build=...): "auto", "torch" or "fused" (csrc/kernels/pq_build.hip)
        self.pq_search = pq_search  # IVFPQIndex(search=...): "auto", "scan" or "fused" (csrc/kernels/ivfpq_search.hip)
        self.pq_coarse = pq_coarse  # IVFPQIndex(coarse=...): "auto", "torch" or "fused" (csrc/kernels/coarse_assign.hip)
        self.pq = None
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        self.dtype = torch.bfloat16 if self.device.type == "cuda" else torch.float32
        self.vecs = torch.empty(0, dim, dtype=self.dtype, device=self.device)
        self.ivf_threshold = ivf_threshold
        self.nprobe = nprobe
        self.centroids: torch.Tensor | None = None
        self.assign: torch.Tensor | None = None
        self.lists: list[torch.Tensor] | None = None
        self.host_refine = False  # compressed tier: self.vecs lives in host memory (refine store only)
        self.ivf_search = ivf_search  # IVF-Flat: "auto", "scan" or "fused" (csrc/kernels/ivf_scan_topk.hip)
        self.fused_ivf_search(1, 1)  # "fused" where the kernels cannot run: raise now, not at the first query
        self.flat_search = flat_search  # flat tier: "auto", "gemm" or "fused" (csrc/kernels/flat_scan_topk.hip)
        self.fused_flat_search(1, 1)  # the same rule
        if index_type in ("ivfsq8", "flatsq8"):  # the tiers have no other path: the same rule
            from ..ops import _native
            from .sq8 import SQ8_CH, sq8_dim_ok

            if not (self.device.type == "cuda" and _native.hip_available() and sq8_dim_ok(dim)):
                raise _native.NativeUnavailable(f"index_type='{index_type}' needs a GPU device, the native kernel "
                                                f"library and dim / 256 in {SQ8_CH}")

    def fused_ivf_search(self, Q: int, k: int) -> bool:
        """Whether an IVF-Flat search of ``Q`` queries for ``k`` results runs on ``ivf_scan_topk.hip``.  ``"fused"``:
        always, or it raises; ``"auto"``: where the kernels can run and ``_auto_ivf_fused`` holds."""
        if self.ivf_search == "scan":
            return False
        from ..ops import _native

        ok = self.device.type == "cuda" and _native.hip_available()
        have = self.lvecs is not None and self.lvecs.shape[0] == self.ntotal
        if self.ivf_search == "fused":
            if not ok:
                raise _native.NativeUnavailable("ivf_search='fused' needs a GPU device and the native kernel library")
            if self.centroids is not None and not have:
                raise _native.NativeUnavailable(f"ivf_search='fused' needs the list-sorted bf16 rows: dim / 128 in "
                                                f"{IVF_SEARCH_CH}")
            if k > IVF_SEARCH_MAX_K:
                raise _native.NativeUnavailable(f"ivf_search='fused' keeps at most {IVF_SEARCH_MAX_K} results per query")
            return True
        return ok and have and k <= IVF_SEARCH_MAX_K and _auto_ivf_fused(self.dim, self.ntotal, Q, k)

    def fused_flat_search(self, Q: int, k: int) -> bool:
        """Whether a flat search of ``Q`` queries for ``k`` results runs on ``flat_scan_topk.hip``.  ``"fused"``:
        always, or it raises; ``"auto"``: where the kernel can run and ``_auto_flat_fused`` holds."""
        if self.flat_search == "gemm":
            return False
        from ..ops import _native

        ok = self.device.type == "cuda" and _native.hip_available() and self.dim >= 32 and self.dim % 32 == 0
        if self.flat_search == "fused":
            if not ok:
                raise _native.NativeUnavailable("flat_search='fused' needs a GPU device, the native kernel library and "
                                                "dim % 32 == 0")
            if k > FLAT_MAX_K:
                raise _native.NativeUnavailable(f"flat_search='fused' keeps at most {FLAT_MAX_K} results per query")
            return True
        return ok and k <= FLAT_MAX_K and _auto_flat_fused(self.dim, self.ntotal, Q, k)

    # ------------------------------------------------------------------ build
    @property
    def ntotal(self) -> int:
        return int(self.vecs.shape[0])

    @property
    def index_type(self) -> str:
        if self.pq is not None:
            return self.pq.index_type
        if self.centroids is not None and self.kind == "ivfsq8":
            return f"IVFSQ8-GPU(nlist={self.centroids.shape[0]})"
        if self.centroids is not None:
            return f"IVFFlat-GPU(nlist={self.centroids.shape[0]})"
        return "FlatSQ8-GPU" if self.kind == "flatsq8" else "FlatIP-GPU"

    def add(self, x) -> None:
        x = torch.as_tensor(np.asarray(x, np.float32) if not torch.is_tensor(x) else x).to(self.device, self.dtype)
        assert x.dim() == 2 and x.shape[1] == self.dim
        self.vecs = torch.cat([self.vecs, x.to(self.vecs.device)], 0)
        if self.pq is not None:
            self.pq.add(x.float())
        elif self.kind == "flatsq8":  # the new rows' codes alone: a row's code does not depend on the others
            self._encode_flat_sq8(self.ntotal - x.shape[0])
        elif self.kind == "ivfpq" or (self.kind == "auto" and self.ntotal >= self.ivfpq_threshold
                                       and not self._fits_hbm(self.ntotal)):
            self.train_ivfpq()
        elif self.centroids is not None:
            self._assign_new(x, self.ntotal - x.shape[0])
        elif self.kind in ("ivf", "ivfsq8") or (self.kind == "auto" and self.ntotal >= self.ivf_threshold):
            self.train_ivf()

    def _encode_flat_sq8(self, base: int) -> None:
        """``"flatsq8"``: the id-ordered codes of the stored rows from ``base`` on, appended to those before them."""
        from .sq8 import sq8_encode

        codes, scales = sq8_encode(self.vecs[base:], None)
        if base:
            codes, scales = torch.cat([self.sq_codes[:base], codes]), torch.cat([self.sq_scales[:base], scales])
        self.sq_codes, self.sq_scales = codes, scales

    def _fits_hbm(self, n: int) -> bool:
        """The exact-scan IVF tier keeps the vectors twice (id order + list-sorted): use it while
        that fits in a third of this GPU's HBM (58 M x 768 bf16 x 2 = 178 GB of 288 GB: yes)."""
        if self.device.type != "cuda":
            return False
        total = torch.cuda.get_device_properties(self.device).total_memory
        return 2 * n * self.dim * 2 <= 0.66 * total

    def train_ivfpq(self, nlist: int | None = None) -> None:
        from .ivfpq import IVFPQIndex, default_nlist

        n = self.ntotal
        nl = nlist or min(default_nlist(n), max(1, n // 39))
        pq = IVFPQIndex(self.dim, nl, self.pq_m, self.nprobe, self.device, build=self.pq_build, search=self.pq_search,
                        coarse=self.pq_coarse)
        g = torch.Generator(device="cpu").manual_seed(0)
        sample = self.vecs[torch.randperm(n, generator=g)[: min(n, max(262_144, 39 * nl))].to(self.vecs.device)]
        pq.train(sample.float())
        for i in range(0, n, 1 << 22):  # encode in chunks: no fp32 copy of the whole collection
            xc = self.vecs[i:i + (1 << 22)]
            pq.add(xc if pq.fused_build else xc.float())  # be_pq_encode reads the stored bf16 rows
        self.pq = pq
        self.centroids = None

    def compress(self, pq_m: int = 192, refine: int = 50, nlist: int | None = None) -> dict:
        """Switch to the compressed tier: IVF-PQ codes (``pq_m`` bytes per vector) on the GPU, the full
        vectors in host memory as the exact re-rank store.  Search returns the top-k of the
        ``refine * k`` PQ candidates re-scored exactly.  Returns the GPU / host footprint (bytes)."""
        self.pq_m, self.refine = pq_m, refine
        self.lvecs = self.sq_codes = self.sq_scales = None
        self.train_ivfpq(nlist)
        self.vecs = self.vecs.cpu()  # bf16 on the host: ~1.5 KB per vector, gathered per query
        self.host_refine = True
        if self.device.type == "cuda":
            torch.cuda.empty_cache()
        return {"gpu_bytes": self.pq.gpu_bytes(), "host_bytes": int(self.vecs.numel() * self.vecs.element_size())}

    def _refine_rows(self, c: torch.Tensor) -> torch.Tensor:
        """[Q, R] candidate ids (>= 0) -> their stored vectors [Q, R, D] on the index device."""
        if not self.host_refine:
            return self.vecs[c]
        rows = self.vecs.index_select(0, c.reshape(-1).cpu())  # host gather (multi-threaded)
        return rows.to(self.device, non_blocking=False).view(*c.shape, self.dim)

    def _rerank(self, q: torch.Tensor, c: torch.Tensor, k: int):
        """Shortlist ids ``c [Q, R]`` (-1 = empty) re-scored exactly with the stored vectors and cut to the best
        ``min(k, R)`` -> ``(scores, ids)`` on the device, ``-inf`` / ``-1`` in empty slots."""
        ok = c >= 0
        s = torch.einsum("qd,qkd->qk", q.float(), self._refine_rows(c.clamp(min=0)).float())
        s = torch.where(ok, s, torch.full_like(s, -float("inf")))
        ts, ti = torch.topk(s, min(k, s.shape[1]), dim=1)
        return ts, torch.where(torch.isfinite(ts), torch.gather(c, 1, ti), torch.full_like(ti, -1))

    def train_ivf(self, nlist: int | None = None, iters: int = 10, seed: int = 0) -> None:
        n = self.ntotal
        # ~4 sqrt(N) lists (the FAISS guideline the reference's IVF-PQ tier follows): at 58 M that is
        # ~30 k lists of ~1.9 k vectors, so nprobe 64 scans ~120 k exact candidates per query
        nlist = nlist or int(min(65536, max(64, 4 * math.sqrt(n))))
        g = torch.Generator(device="cpu").manual_seed(seed)
        # 64 points per list (FAISS trains IVF on 39-256 per list); scores in the storage dtype
        sample = self.vecs[torch.randperm(n, generator=g)[: min(n, 64 * nlist)].to(self.device)]
        samplef = sample.float()
        cent = samplef[torch.randperm(sample.shape[0], generator=g)[:nlist].to(self.device)].clone()
        for _ in range(iters):  # spherical k-means
            a = _argmax_ip(sample, cent)
            new = torch.zeros_like(cent).index_add_(0, a, samplef)
            cnt = torch.bincount(a, minlength=nlist)
            empty = cnt == 0
            new[empty] = cent[empty]
            cent = torch.nn.functional.normalize(new, dim=1)
        self.centroids = cent.to(self.dtype)
        self.assign = torch.empty(0, dtype=torch.int32, device=self.device)
        self._assign_new(self.vecs, 0)

    def _assign_new(self, x: torch.Tensor, base: int) -> None:
        a = _argmax_ip(x, self.centroids).int()
        self.assign = torch.cat([self.assign, a])
        order = torch.argsort(self.assign, stable=True)
        counts = torch.bincount(self.assign.long(), minlength=self.centroids.shape[0])
        self.sorted_ids = order  # vector ids grouped by list
        self.list_off = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
        self.lists = None
        if self.kind == "ivfsq8":  # the list-sorted int8 copy instead, gathered inside the encoder
            from .sq8 import sq8_encode

            self.lvecs = None
            self.sq_codes, self.sq_scales = sq8_encode(self.vecs, order)
            return
        # list-sorted copy of the vectors: every IVF list is one contiguous HBM slab that the exact
        # scan kernel streams (be_ivf_scan_bf16); built chunk by chunk to bound the temporary
        # (be_ivf_scan_bf16 is instantiated for dim/128 in {1,2,3,4,6,8}; other dims use the bmm path)
        if self.device.type == "cuda" and self.dim % 128 == 0 and self.dim // 128 in (1, 2, 3, 4, 6, 8):
            lv = torch.empty_like(self.vecs)
            for i in range(0, order.numel(), CHUNK):
                lv[i:i + CHUNK] = self.vecs[order[i:i + CHUNK]]
            self.lvecs = lv
        else:
            self.lvecs = None

    # ------------------------------------------------------------------ search
    @torch.no_grad()
    def search(self, q, k: int = 20, nprobe: int | None = None):
        """q [Q, D] -> (scores [Q, k] fp32 numpy, ids [Q, k] int64 numpy; -1 = empty slot).
        ``nprobe`` overrides the IVF probe count for this call."""
        q = torch.as_tensor(np.asarray(q, np.float32) if not torch.is_tensor(q) else q).to(self.device, self.dtype)
        if q.dim() == 1:
            q = q[None]
        Q = q.shape[0]
        k_eff = min(k, self.ntotal)
        if k_eff == 0:
            return np.full((Q, k), -np.inf, np.float32), np.full((Q, k), -1, np.int64)
        if self.pq is not None:
            if not self.refine or self.vecs.shape[0] != self.ntotal:
                return self.pq.search(q.float(), k)
            # IVF-PQ shortlist of refine*k, re-scored exactly with the stored vectors (IVFPQ+R)
            _, c = self.pq.search_device(q.float(), self.refine * k)  # stays on the device
            ts, ids = self._rerank(q, c, k)
            S = np.full((Q, k), -np.inf, np.float32)
            I = np.full((Q, k), -1, np.int64)
            S[:, : ts.shape[1]] = ts.cpu().numpy()
            I[:, : ids.shape[1]] = ids.cpu().numpy()
            return S, I
        if self.kind == "flatsq8":
            best_s, best_i = self._search_flat_sq8(q, k_eff)
        elif self.centroids is None and self.fused_flat_search(Q, k_eff):  # scan and selection in HIP
            best_s, best_i = flat_scan_topk_fused(q, self.vecs, k_eff)
        elif self.centroids is None:
            best_s = torch.full((Q, 0), -float("inf"), device=self.device)
            best_i = torch.empty(Q, 0, dtype=torch.long, device=self.device)
            for i in range(0, self.ntotal, CHUNK):
                s = _scores(q, self.vecs[i:i + CHUNK])
                ts, ti = torch.topk(s, min(k_eff, s.shape[1]), dim=1)
                best_s = torch.cat([best_s, ts], 1)
                best_i = torch.cat([best_i, ti + i], 1)
                best_s, j = torch.topk(best_s, min(k_eff, best_s.shape[1]), dim=1)
                best_i = torch.gather(best_i, 1, j)
        else:
            best_s, best_i = self._search_ivf(q, k_eff, nprobe=nprobe)
        S = np.full((Q, k), -np.inf, np.float32)
        I = np.full((Q, k), -1, np.int64)
        S[:, : best_s.shape[1]] = best_s.cpu().numpy()
        I[:, : best_i.shape[1]] = best_i.cpu().numpy()
        return S, I

    def _search_ivf(self, q: torch.Tensor, k: int, q_chunk: int = 8, nprobe: int | None = None):
        """Batched IVF-Flat: every query's probed lists become one padded candidate row (list-sorted
        vector ids, located through the list offsets).  GPU: the HIP scan kernel scores every
        candidate exactly from the list-sorted bf16 slabs, then one top-k; CPU: one batched GEMM
        per query chunk.  No per-query Python loop either way.  Where :meth:`fused_ivf_search` holds the same
        probes go to :func:`ivf_scan_topk_fused` instead, which keeps the top-k inside the scan."""
        nl = self.centroids.shape[0]
        npb = min(nprobe or self.nprobe, nl)
        if npb == nl:  # every list: no ranking needed (the candidate order does not matter)
            probes = torch.arange(nl, device=q.device).expand(q.shape[0], nl).contiguous()
        else:
            probes = torch.topk((q @ self.centroids.T).float(), npb, dim=1).indices
        if self.kind == "ivfsq8":
            return self._search_sq8(q, probes, k)
        if self.fused_ivf_search(q.shape[0], k):  # scan, selection and row -> id in HIP, no host read
            return ivf_scan_topk_fused(q.float(), probes, self.list_off, self.lvecs, self.sorted_ids, k)
        sizes, cand_off = candidate_offsets(self.list_off, probes)
        stride = int(sizes.sum(1).max())
        Q = q.shape[0]
        best_s = torch.full((Q, k), -float("inf"), device=self.device)
        best_i = torch.full((Q, k), -1, dtype=torch.long, device=self.device)
        if stride == 0:
            return best_s, best_i
        if getattr(self, "lvecs", None) is not None and self.lvecs.shape[0] == self.ntotal:
            from ..ops import _native

            out = torch.full((Q, stride), -float("inf"), dtype=torch.float32, device=self.device)
            _native.call("be_ivf_scan_bf16", _native.ptr(q.float().contiguous()), _native.ptr(probes.int().contiguous()),
                         _native.ptr(self.list_off), _native.ptr(cand_off), _native.ptr(self.lvecs), Q,
                         probes.shape[1], self.dim, stride, _native.ptr(out), _native.stream(self.device))
            ts, ti = torch.topk(out, min(k, stride), dim=1)
            ids = self.sorted_ids[slot_rows(self.list_off, probes, cand_off, ti).clamp(0, self.ntotal - 1)]
            best_s[:, : ts.shape[1]] = ts
            best_i[:, : ts.shape[1]] = torch.where(torch.isfinite(ts), ids, torch.full_like(ids, -1))
            return best_s, best_i
        slots = torch.arange(stride, device=self.device)
        for a in range(0, Q, q_chunk):
            b = min(Q, a + q_chunk)
            sl = slots.expand(b - a, stride).contiguous()
            valid = sl < sizes[a:b].sum(1, keepdim=True)  # the row's end: an empty list holds no slot below it
            rows = slot_rows(self.list_off, probes[a:b], cand_off[a:b], sl)
            ids = self.sorted_ids[rows.clamp(max=self.sorted_ids.numel() - 1)]
            sc = torch.bmm(self.vecs[ids], q[a:b, :, None]).squeeze(-1).float()
            sc = torch.where(valid, sc, torch.full_like(sc, -float("inf")))
            ts, ti = torch.topk(sc, min(k, stride), dim=1)
            best_s[a:b, : ts.shape[1]] = ts
            best_i[a:b, : ts.shape[1]] = torch.where(torch.isfinite(ts), torch.gather(ids, 1, ti), torch.full_like(ti, -1))
        return best_s, best_i

    def _search_sq8(self, q: torch.Tensor, probes: torch.Tensor, k: int):
        """The IVF-SQ8 tier: the best ``min(refine * k, 1024)`` int8 scores of the probed lists
        (``csrc/kernels/ivf_sq8.hip``), re-scored exactly from ``self.vecs`` and cut to ``k``; ``refine == 0``: the
        ``k`` best int8 scores as they are."""
        from ..ops import _native
        from .sq8 import SQ8_MAX_K, ivf_sq8_scan_topk_fused

        if k > SQ8_MAX_K:
            raise _native.NativeUnavailable(f"index_type='ivfsq8' keeps at most {SQ8_MAX_K} results per query")
        kk = min(self.refine * k, SQ8_MAX_K) if self.refine else k
        s, c = ivf_sq8_scan_topk_fused(q.float(), probes, self.list_off, self.sq_codes, self.sq_scales, self.sorted_ids,
                                       kk)
        return self._rerank(q, c, k) if self.refine else (s, c)

    def _search_flat_sq8(self, q: torch.Tensor, k: int):
        """The flat SQ8 tier: the best ``min(refine * k, 256)`` int8 scores of all rows
        (``csrc/kernels/flat_sq8_scan_topk.hip``), re-scored exactly from ``self.vecs`` and cut to ``k``;
        ``refine == 0``: the ``k`` best int8 scores as they are."""
        from ..ops import _native

        if k > FLAT_SQ8_MAX_K:
            raise _native.NativeUnavailable(f"index_type='flatsq8' keeps at most {FLAT_SQ8_MAX_K} results per query")
        kk = min(self.refine * k, FLAT_SQ8_MAX_K) if self.refine else k
        s, c = flat_sq8_scan_topk_fused(q.float(), self.sq_codes, self.sq_scales, kk)
        return self._rerank(q, c, k) if self.refine else (s, c)

    def reconstruct_batch(self, ids) -> np.ndarray:
        return self.vecs[torch.as_tensor(np.asarray(ids), device=self.vecs.device)].float().cpu().numpy()

    # ------------------------------------------------------------------ persistence
    def save(self, out_dir) -> dict:
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        t0 = time.time()
        np.save(out / "vectors.npy", self.vecs.float().cpu().numpy().astype(np.float16))
        if self.pq is not None:
            self.pq.save(out)
        else:
            (out / "ivfpq_info.json").unlink(missing_ok=True)
        if self.centroids is not None:
            np.save(out / "ivf_centroids.npy", self.centroids.float().cpu().numpy())
        else:
            (out / "ivf_centroids.npy").unlink(missing_ok=True)
        info = {"n_cells": self.ntotal, "embed_dim": self.dim, "index_type": self.index_type,
                "host_refine": self.host_refine, "refine": self.refine,
                **({"sq8": True} if self.kind == "ivfsq8" and self.pq is None else {}),
                **({"flat_sq8": True} if self.kind == "flatsq8" and self.pq is None else {}),
                "index_size_mb": round((out / "vectors.npy").stat().st_size / 2 ** 20, 3),
                "build_seconds": round(time.time() - t0, 3),
                "build_time_iso": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())}
        (out / "index_info.json").write_text(json.dumps(info, indent=2))
        return info

    @classmethod
    def load(cls, out_dir, device=None, pq_search: str = "auto", ivf_search: str = "auto",
             flat_search: str = "auto") -> "VectorIndex":
        out = Path(out_dir)
        p = out / "vectors.npy"
        if not p.exists():
            raise FileNotFoundError(f"No index at {p}")
        v = np.load(p)  # allow_pickle=False
        ii = out / "index_info.json"
        info = json.loads(ii.read_text()) if ii.exists() else {}
        # "sq8" / "flat_sq8": the int8 codes are a function of vectors.npy and are rebuilt below
        idx = cls(dim=v.shape[1], device=device, pq_search=pq_search, ivf_search=ivf_search, flat_search=flat_search,
                  index_type="ivfsq8" if info.get("sq8") else "flatsq8" if info.get("flat_sq8") else "auto")
        host = bool(info.get("host_refine")) and (out / "ivfpq_info.json").exists()
        idx.vecs = torch.from_numpy(v.astype(np.float32)).to("cpu" if host else idx.device, idx.dtype)
        if (out / "ivfpq_info.json").exists():
            from .ivfpq import IVFPQIndex

            idx.pq = IVFPQIndex.load(out, device=idx.device, search=pq_search)
            idx.host_refine = host
            idx.refine = int(info.get("refine", idx.refine))
            idx.pq_m = idx.pq.m
            return idx
        c = out / "ivf_centroids.npy"
        if info.get("sq8") or info.get("flat_sq8"):
            idx.refine = int(info.get("refine", idx.refine))
        if idx.kind == "flatsq8" and idx.ntotal:
            idx._encode_flat_sq8(0)
        if c.exists():
            idx.centroids = torch.from_numpy(np.load(c)).to(idx.device, idx.dtype)
            idx.assign = torch.empty(0, dtype=torch.int32, device=idx.device)
            idx._assign_new(idx.vecs, 0)
        return idx
