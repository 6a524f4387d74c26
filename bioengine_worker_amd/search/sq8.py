"""Plain wrappers of ``csrc/kernels/ivf_sq8.hip``: the 8-bit scalar quantiser of the IVF-SQ8 tier and its list scan.

Code format: a row is D signed int8 codes and one fp32 scale.  ``amax = max |x_i|`` over the fp32 values of the stored
row, ``inv = 127 / amax`` and ``scale = amax / 127`` (each one correctly rounded fp32 division), ``c_i =
clamp(rint(x_i * inv), -127, 127)`` with the product rounded to fp32 and ties to even; ``amax == 0`` gives codes 0 and
scale 0.  numpy reproduces the rule bit for bit in float32.  A score is ``scale * sum_i q_i c_i``."""
from __future__ import annotations

import torch

from ..ops import _native
from .list_scan import scan_topk_merge

SQ8_CH = (1, 2, 3, 4)  # dim / 256 the kernels are instantiated for
SQ8_MAX_K = 1024


def sq8_dim_ok(dim: int) -> bool:
    return dim % 256 == 0 and dim // 256 in SQ8_CH


def sq8_encode(src: torch.Tensor, order: torch.Tensor | None = None):
    """``be_sq8_encode``: ``src [N, D]`` bf16, ``order [n]`` int64 rows of ``src`` (``None``: all rows in order) ->
    ``(codes [n, D] int8, scales [n] fp32)``, row ``r`` the code of ``src[order[r]]``.  The gather is inside the
    kernel: no reordered copy of ``src`` is made."""
    if not (src.is_cuda and (order is None or order.is_cuda) and _native.hip_available()):
        raise _native.NativeUnavailable("be_sq8_encode needs GPU tensors and the native kernel library")
    if src.dim() != 2 or src.dtype != torch.bfloat16 or not sq8_dim_ok(src.shape[1]) or (
            order is not None and order.dim() != 1):
        raise _native.NativeUnavailable(f"be_sq8_encode serves bf16 rows of dim / 256 in {SQ8_CH}")
    src = src.contiguous()
    if order is not None:
        order = order.long().contiguous()
    n, D = src.shape[0] if order is None else order.shape[0], src.shape[1]
    codes = torch.empty(n, D, dtype=torch.int8, device=src.device)
    scales = torch.empty(n, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _native.call("be_sq8_encode", _native.ptr(src), _native.ptr(order), n, D, _native.ptr(codes),
                     _native.ptr(scales), _native.stream(src.device))
    return codes, scales


def ivf_sq8_scan_topk_fused(q: torch.Tensor, probes: torch.Tensor, list_off: torch.Tensor, codes: torch.Tensor,
                            scales: torch.Tensor, sorted_ids: torch.Tensor, kk: int, splits: int | None = None):
    """``be_ivf_sq8_scan_topk`` + ``be_topk_merge``: the ``kk`` best SQ8 scores ``scale * sum_i q_i c_i`` of ``q [Q, D]``
    (fp32) with the rows of the probed lists in the list-sorted ``codes [N, D]`` int8 / ``scales [N]`` fp32, ordered by
    (score descending, list-sorted row ascending) -> ``(scores [Q, kk] fp32, ids [Q, kk] int64)`` on the device, rows
    mapped through ``sorted_ids``, ``-inf`` / ``-1`` in empty slots.  ``splits`` forces the slot ranges per query; the
    default is ``index.ivf_splits``, which was tuned on the bf16 scan and not on this one.  Nothing is read back."""
    from .index import ivf_splits

    t = (q, probes, list_off, codes, scales, sorted_ids)
    if not (all(x.is_cuda for x in t) and _native.hip_available()):
        raise _native.NativeUnavailable("be_ivf_sq8_scan_topk needs GPU tensors and the native kernel library")
    if (q.dim() != 2 or probes.dim() != 2 or codes.dim() != 2 or probes.shape[0] != q.shape[0]
            or codes.shape[1] != q.shape[1] or not sq8_dim_ok(q.shape[1]) or codes.dtype != torch.int8
            or scales.dtype != torch.float32 or scales.shape != codes.shape[:1] or not 1 <= kk <= SQ8_MAX_K
            or codes.shape[0] >= 2 ** 31 or probes.shape[1] < 1 or sorted_ids.shape[0] != codes.shape[0]):
        raise _native.NativeUnavailable(f"be_ivf_sq8_scan_topk serves int8 rows of dim / 256 in {SQ8_CH} with one fp32 "
                                        f"scale each, 1 <= kk <= {SQ8_MAX_K}, fewer than 2^31 rows and nprobe >= 1")
    Q, nprobe = probes.shape
    list_off = list_off.long().contiguous()
    P = int(splits) if splits else ivf_splits(Q, kk)

    def launch(cand_off, part_s, part_r):
        _native.call("be_ivf_sq8_scan_topk", _native.ptr(q.float().contiguous()), _native.ptr(probes.int().contiguous()),
                     _native.ptr(list_off), _native.ptr(cand_off), _native.ptr(codes.contiguous()),
                     _native.ptr(scales.contiguous()), codes.shape[0], Q, nprobe, q.shape[1], kk, P,
                     _native.ptr(part_s), _native.ptr(part_r), _native.stream(codes.device))

    return scan_topk_merge(launch, list_off, probes, sorted_ids, kk, P)
