"""What the IVF-Flat and IVF-PQ list scans share on the Python side (``search/index.py``, ``search/ivfpq.py``): the
candidate row of a query, the concatenation of its probed lists, and the fused search around a scan kernel that keeps
its top-k inside (``csrc/kernels/topk_select.h``) and ``be_topk_merge`` (``csrc/kernels/topk_merge.hip``)."""
from __future__ import annotations

import torch

from ..ops import _native


def candidate_offsets(list_off: torch.Tensor, probes: torch.Tensor):
    """``list_off [nlist + 1]``, ``probes [Q, nprobe]`` -> ``(sizes, cand_off)``, both ``[Q, nprobe]``: the probed
    lists' sizes and their exclusive prefix sum, the slot at which each list starts in the query's candidate row."""
    sizes = (list_off[1:] - list_off[:-1])[probes]
    return sizes, (torch.cumsum(sizes, 1) - sizes).contiguous()


def slot_rows(list_off: torch.Tensor, probes: torch.Tensor, cand_off: torch.Tensor, slots: torch.Tensor) -> torch.Tensor:
    """Candidate-row slots ``[Q, n]`` -> list-sorted rows ``[Q, n]``.  A slot lies in the last probed list ``p`` with
    ``cand_off[p] <= slot``: of lists that start at one slot, the one that is not empty."""
    p = (torch.searchsorted(cand_off.contiguous(), slots.contiguous(), right=True) - 1).clamp(min=0)
    return list_off[torch.gather(probes, 1, p)] + (slots - torch.gather(cand_off, 1, p))


def scan_topk_merge(launch, list_off: torch.Tensor, probes: torch.Tensor, ids: torch.Tensor, kk: int, P: int,
                    merge: str = "be_topk_merge"):
    """A fused search over ``list_off`` (int64, contiguous): ``launch(cand_off, part_s, part_r)`` starts the scan
    kernel, which leaves the ``kk`` best (score, list-sorted row) pairs of each of the ``P`` slot ranges of every query
    in ``part_s`` / ``part_r`` ``[Q, P, kk]``; the entry ``merge`` joins them -> ``(scores [Q, kk] fp32, ids [Q, kk]
    int64)`` on the device, rows mapped through ``ids``, ``-inf`` / ``-1`` in empty slots.  Nothing is read back."""
    Q, dev = probes.shape[0], ids.device
    cand_off = candidate_offsets(list_off, probes)[1]
    part_s = torch.empty(Q, P, kk, dtype=torch.float32, device=dev)
    part_r = torch.empty(Q, P, kk, dtype=torch.int32, device=dev)
    out_s = torch.empty(Q, kk, dtype=torch.float32, device=dev)
    out_i = torch.empty(Q, kk, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        launch(cand_off, part_s, part_r)
        _native.call(merge, _native.ptr(part_s), _native.ptr(part_r), _native.ptr(ids.long().contiguous()),
                     Q, P, kk, _native.ptr(out_s), _native.ptr(out_i), _native.stream(dev))
    return out_s, out_i
