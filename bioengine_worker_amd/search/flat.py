"""The flat tier's search on ``csrc/kernels/flat_scan_topk.hip``: one MFMA scan of all rows for a few queries with the
top-k kept inside the kernel, then ``be_topk_merge`` (``csrc/kernels/topk_merge.hip``) over the row ranges' partial
lists.  No score matrix is written.  ``csrc/kernels/flat_sq8_scan_topk.hip`` is the same scan over int8 rows (the
``"flatsq8"`` tier): int8 MFMA, the queries split into two int8 vectors inside the kernel."""
from __future__ import annotations

import torch

from ..ops import _native

FLAT_MAX_K = 256
FLAT_SQ8_MAX_K = 256  # csrc/kernels/flat_sq8_scan_topk.hip, on the same selection (flat_select.h)
FLAT_MAX_ROWS = 2 ** 31 - 512  # int32 rows, and the kernel's fetch runs one 256-row tile past a range
_TILE = 256  # rows a workgroup scores per step: 4 waves of 64
_LDS = 160 * 1024 - 256  # one workgroup per CU, less the barrier vote's static bytes


def flat_lds_bytes(group: int, D: int, cap: int) -> int:
    """LDS of a workgroup of ``be_flat_scan_topk`` that holds ``group`` queries: the bf16 query image, and per query
    ``cap`` 8-byte keys, a threshold and a count."""
    return group * D * 2 + group * (cap * 8 + 12)


def flat_group(Q: int, D: int, kk: int) -> int:
    """Queries per workgroup, 16 / 32 / 64: the smallest group that holds all ``Q`` queries where its LDS fits (a
    smaller image leaves the CU to a second workgroup), otherwise the largest that fits; "fits" is the launcher's
    rule, the image and ``kk + 16`` keys per query, rounded up to a multiple of 8.  The kernel reads every row once per group."""
    fits = [g for g in (16, 32, 64) if flat_lds_bytes(g, D, (kk + 23) // 8 * 8) <= _LDS]
    if not fits:
        raise _native.NativeUnavailable(f"be_flat_scan_topk: 16 queries of dim {D} with {kk + 16} keys each exceed the "
                                        f"{_LDS} bytes of LDS")
    return next((g for g in fits if g >= Q), fits[-1])


def flat_splits(n: int, groups: int, kk: int, cus: int = 256) -> int:
    """Row ranges of ``be_flat_scan_topk``: one workgroup per CU over all ``groups`` query groups, and at least one
    256-row tile (four 64-row blocks, one per wave) per range.  ``kk`` does not enter: the merge reads about ``kk + P``
    keys per query whatever ``P`` is.  Measured at D = 768 (device time of scan + merge, us, at 1 M / 5 M rows): one
    query, kk = 20: 1000 / 4723 at P = 64, 565 / 2549 at 128, 361 / 1527 at 256, 351 / 1503 at 512, 367 / 1522 at 1024,
    398 / 1558 at 2048; kk = 100: 1090 / 4826, 638 / 2615, 423 / 1564, 385 / 1489, 423 / 1541, 481 / 1619.  64 queries
    (one group), kk = 20: 1753 / 6787, 1093 / 3780, 745 / 2253, 937 / 2587, 1220 / 3127, 1688 / 3932; kk = 100: 4106 /
    10466, 2984 / 6849, 2265 / 4732, 3284 / 6567, 4754 / 9535, 6509 / 14086.  Spreads 6 to 76 us.  With one query 512
    ranges are 3 to 9 % faster than 256 (two workgroups fit a CU), with 64 queries every workgroup beyond one per CU
    pays its own list warm-up again: P = 256 / groups is kept for both."""
    return max(1, min(cus // max(groups, 1), -(-n // _TILE)))


def flat_sq8_lds_bytes(group: int, D: int, cap: int) -> int:
    """LDS of a workgroup of ``be_flat_sq8_scan_topk`` that holds ``group`` queries: two int8 query images and one
    fp32 ``sq`` per query, and per query ``cap`` 8-byte keys, a threshold and a count."""
    return group * (2 * D + 4) + group * (cap * 8 + 12)


def flat_sq8_group(Q: int, D: int, kk: int) -> int:
    """Queries per workgroup of ``be_flat_sq8_scan_topk``, 16 / 32, by the rule of :func:`flat_group`.  At the dims
    the kernel serves (up to 1024) both fit for every ``kk`` up to ``FLAT_SQ8_MAX_K``."""
    fits = [g for g in (16, 32) if flat_sq8_lds_bytes(g, D, (kk + 23) // 8 * 8) <= _LDS]
    if not fits:
        raise _native.NativeUnavailable(f"be_flat_sq8_scan_topk: 16 queries of dim {D} with {kk + 16} keys each exceed "
                                        f"the {_LDS} bytes of LDS")
    return next((g for g in fits if g >= Q), fits[-1])


def flat_sq8_scan_topk_fused(q: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, kk: int,
                             splits: int | None = None):
    """``be_flat_sq8_scan_topk`` + ``be_topk_merge``: the ``kk`` best SQ8 scores of ``q [Q, D]`` (fp32) with all rows
    of ``codes [N, D]`` int8 / ``scales [N]`` fp32 (``sq8_encode(src, None)``), ordered by (score descending, row
    ascending) -> ``(scores [Q, kk] fp32, ids [Q, kk] int64)`` on the device, ``-inf`` / ``-1`` in empty slots.  The
    query is split into two int8 vectors inside the kernel; the score contract is in
    ``csrc/kernels/flat_sq8_scan_topk.hip``.  ``splits`` forces the row ranges (:func:`flat_splits`, tuned on the bf16
    scan and not on this one).  Nothing is read back."""
    from .sq8 import SQ8_CH, sq8_dim_ok

    if not (q.is_cuda and codes.is_cuda and scales.is_cuda and _native.hip_available()):
        raise _native.NativeUnavailable("be_flat_sq8_scan_topk needs GPU tensors and the native kernel library")
    if (q.dim() != 2 or codes.dim() != 2 or q.shape[1] != codes.shape[1] or not sq8_dim_ok(q.shape[1])
            or q.dtype != torch.float32 or codes.dtype != torch.int8 or scales.dtype != torch.float32
            or scales.shape != codes.shape[:1] or not 1 <= kk <= FLAT_SQ8_MAX_K or codes.shape[0] >= FLAT_MAX_ROWS):
        raise _native.NativeUnavailable(f"be_flat_sq8_scan_topk serves fp32 queries and int8 rows of dim / 256 in "
                                        f"{SQ8_CH} with one fp32 scale each, 1 <= kk <= {FLAT_SQ8_MAX_K} and fewer "
                                        f"than 2^31 - 512 rows")
    (Q, D), N, dev = q.shape, codes.shape[0], codes.device
    out_s = torch.full((Q, kk), -float("inf"), dtype=torch.float32, device=dev)
    out_i = torch.full((Q, kk), -1, dtype=torch.int64, device=dev)
    if Q == 0 or N == 0:
        return out_s, out_i
    group = flat_sq8_group(Q, D, kk)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    P = int(splits) if splits else flat_splits(N, -(-Q // group), kk, cus)
    part_s = torch.empty(Q, P, kk, dtype=torch.float32, device=dev)
    part_r = torch.empty(Q, P, kk, dtype=torch.int32, device=dev)
    q, codes = (t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)
                for t in (q, codes))  # the kernel's 16-byte loads
    with torch.cuda.device(dev):
        st = _native.stream(dev)
        _native.call("be_flat_sq8_scan_topk", _native.ptr(q), _native.ptr(codes), _native.ptr(scales.contiguous()), N,
                     Q, D, kk, P, group, _native.ptr(part_s), _native.ptr(part_r), st)
        _native.call("be_topk_merge", _native.ptr(part_s), _native.ptr(part_r), None, Q, P, kk, _native.ptr(out_s),
                     _native.ptr(out_i), st)
    return out_s, out_i


def flat_scan_topk_fused(q: torch.Tensor, vecs: torch.Tensor, kk: int, splits: int | None = None):
    """``be_flat_scan_topk`` + ``be_topk_merge``: the ``kk`` best inner products of ``q [Q, D]`` with all rows of
    ``vecs [N, D]`` (both bf16, fp32 accumulation in the MFMA), ordered by (score descending, row ascending) ->
    ``(scores [Q, kk] fp32, ids [Q, kk] int64)`` on the device, ``-inf`` / ``-1`` in empty slots.  ``splits`` forces
    the row ranges (:func:`flat_splits`).  Nothing is read back."""
    if not (q.is_cuda and vecs.is_cuda and _native.hip_available()):
        raise _native.NativeUnavailable("be_flat_scan_topk needs GPU tensors and the native kernel library")
    if (q.dim() != 2 or vecs.dim() != 2 or q.shape[1] != vecs.shape[1] or q.shape[1] < 32 or q.shape[1] % 32
            or q.dtype != torch.bfloat16 or vecs.dtype != torch.bfloat16 or not 1 <= kk <= FLAT_MAX_K
            or vecs.shape[0] >= FLAT_MAX_ROWS):
        raise _native.NativeUnavailable(f"be_flat_scan_topk serves bf16 queries and rows of dim % 32 == 0, "
                                        f"1 <= kk <= {FLAT_MAX_K} and fewer than 2^31 - 512 rows")
    (Q, D), N, dev = q.shape, vecs.shape[0], vecs.device
    out_s = torch.full((Q, kk), -float("inf"), dtype=torch.float32, device=dev)
    out_i = torch.full((Q, kk), -1, dtype=torch.int64, device=dev)
    if Q == 0 or N == 0:
        return out_s, out_i
    group = flat_group(Q, D, kk)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    P = int(splits) if splits else flat_splits(N, -(-Q // group), kk, cus)
    part_s = torch.empty(Q, P, kk, dtype=torch.float32, device=dev)
    part_r = torch.empty(Q, P, kk, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream(dev)
        _native.call("be_flat_scan_topk", _native.ptr(q.contiguous()), _native.ptr(vecs.contiguous()), N, Q, D, kk, P,
                     group, _native.ptr(part_s), _native.ptr(part_r), st)
        _native.call("be_topk_merge", _native.ptr(part_s), _native.ptr(part_r), None, Q, P, kk, _native.ptr(out_s),
                     _native.ptr(out_i), st)
    return out_s, out_i
