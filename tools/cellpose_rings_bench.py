#!/usr/bin/env python3
"""Time of the Cellpose outline stage on one GPU (``gpu.mask_rings_gpu``).

The two workloads of ``cellpose_measure_bench.py``, the stage alone (masks already on the device,
the label bound given):

* a batch: ``B = 32`` images of ``512 x 512``, about 150 cells each (the disks of the cells that
  ``pipeline.synthetic_cells`` draws);
* a volume: ``64 x 256 x 256`` balls on a jittered lattice, traced as 64 planes.

Per workload: the whole call (both launches, the prefix sums and the gather between and after them,
and its two host reads, ``V`` and ``R``), each entry point alone on prepared buffers (``count``:
init + corner pass + prefix sums; ``trace``: walk + prefix sum + gather), what remains of the call
(its allocations, the zeroing of the marks and the two reads), the traffic floor (one read of
the labels plus one write of ``verts`` at the device-copy rate measured in the same run), the
sibling stage on the same masks (``measure_masks_gpu`` without intensities) and the share of labels
whose box is within 64 x 64 (the LDS path).  The result is compared with the numpy oracle in the
same run.  Every time is a HIP-event time, warmed, median of ``--reps`` (>= 10).

Needs a GPU: there is no CPU fallback.  Prints one JSON line per result.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cellpose_measure_bench import lattice_balls, synthetic_masks, timed  # noqa: E402

from bioengine_worker_amd.cellpose import gpu as cg  # noqa: E402
from bioengine_worker_amd.cellpose import reference as ref  # noqa: E402
from bioengine_worker_amd.ops import _native  # noqa: E402


def oracle(M: np.ndarray) -> dict:
    """``reference.mask_rings`` per image, joined into the arrays of the batch."""
    per = [ref.mask_rings(m) for m in M]
    nv = np.cumsum([0] + [r["verts"].shape[0] for r in per])
    return {"verts": np.concatenate([r["verts"] for r in per]).reshape(-1, 2),
            "ring_offsets": np.concatenate([r["ring_offsets"][:-1] + nv[b] for b, r in enumerate(per)] + [nv[-1:]]),
            "ring_label": np.concatenate([r["ring_label"] for r in per]),
            "ring_area2": np.concatenate([r["ring_area2"] for r in per]),
            "ring_image": np.concatenate([np.full(r["ring_label"].shape[0], b, np.int32) for b, r in enumerate(per)]),
            "image_rings": np.cumsum([0] + [r["ring_label"].shape[0] for r in per])}


def bench(name: str, M: torch.Tensor, volume: bool, reps: int, copy_gbs: float) -> dict:
    dev = M.device
    B, H, W = M.shape
    K = int(M.max())
    nlab = K + 1
    res = cg.mask_rings_gpu(M, nlab=nlab, volume=volume)
    want = oracle(M.cpu().numpy())
    same = all(np.array_equal(res[k].cpu().numpy(), want[k]) for k in want)
    V, R = int(res["verts"].shape[0]), int(res["ring_label"].shape[0])
    call_ms = timed(lambda: cg.mask_rings_gpu(M, nlab=nlab, volume=volume), reps)
    # each entry point alone, on the buffers the wrapper would hand it
    n = B * K
    sp = _native.stream(dev)
    w32 = torch.empty(6 * n, dtype=torch.int32, device=dev)
    bbox, nvert, nrings = w32[:4 * n], w32[4 * n:5 * n], w32[5 * n:]
    w64 = torch.empty(3 * n + 4, dtype=torch.int64, device=dev)
    voff, roff, rstart, totals = w64[:n], w64[n:2 * n], w64[2 * n:3 * n], w64[3 * n:]

    def count():
        _native.call("be_cp_rings_count", _native.ptr(M), B, H, W, K, _native.ptr(bbox), _native.ptr(nvert), _native.ptr(voff),
                     _native.ptr(roff), _native.ptr(totals), sp)

    count_ms = timed(count, reps)
    cap = V // 4
    verts = torch.empty(V, 2, dtype=torch.int32, device=dev)
    o64 = torch.empty(4 * cap + 1 + B + 1, dtype=torch.int64, device=dev)
    first, tab_a2, off, area2, per_image = o64.split([cap, cap, cap + 1, cap, B + 1])
    o32 = torch.empty(2 * cap, dtype=torch.int32, device=dev)
    seen = torch.zeros(B * H * W, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def trace():
        _native.call("be_cp_rings_trace", _native.ptr(M), B, H, W, K, _native.ptr(bbox), _native.ptr(nvert), _native.ptr(voff),
                     _native.ptr(roff), _native.ptr(seen), _native.ptr(verts), _native.ptr(first), _native.ptr(tab_a2),
                     _native.ptr(nrings), _native.ptr(rstart), _native.ptr(err), _native.ptr(totals), _native.ptr(off),
                     _native.ptr(area2), _native.ptr(o32[:cap]), _native.ptr(o32[cap:]), _native.ptr(per_image), sp)

    def trace_with_marks():  # the marks of the boxes beyond 64 x 64 must be zero before every trace
        seen.zero_()
        trace()

    trace_ms = timed(trace_with_marks, reps)
    zero_ms = timed(lambda: seen.zero_(), reps)
    assert totals.tolist()[2:] == [R, 0] and torch.equal(verts, res["verts"]) and torch.equal(off[:R + 1], res["ring_offsets"])
    box = bbox.view(n, 4)  # (ymin, ymax, xmin, xmax), inclusive
    present = box[:, 1] >= box[:, 0]
    fast = present & (box[:, 1] - box[:, 0] < 64) & (box[:, 3] - box[:, 2] < 64)
    measure_ms = timed(lambda: cg.measure_masks_gpu(M, None, nlab=nlab, volume=False), reps)
    floor_ms = (M.numel() * 4 + V * 8) / copy_gbs / 1e6
    return {"workload": name, "shape": list(M.shape), "K": K, "labels_traced": int(present.sum()), "V": V, "R": R,
            "equals_oracle": bool(same), "call_ms": round(call_ms, 4), "count_ms": round(count_ms, 4),
            "trace_ms": round(trace_ms - zero_ms, 4), "zero_marks_ms": round(zero_ms, 4),
            "alloc_zero_and_reads_ms": round(call_ms - count_ms - trace_ms, 4), "floor_ms": round(floor_ms, 4),
            "call_over_floor": round(call_ms / floor_ms, 1), "measure_masks_ms": round(measure_ms, 4),
            "call_over_measure": round(call_ms / measure_ms, 2),
            "fast_path_share": round(float(fast.sum()) / max(int(present.sum()), 1), 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ncells", type=int, default=150)
    ap.add_argument("--shape", default="64,256,256")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    reps = max(10, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("cellpose_rings_bench needs a GPU")
    _native.hip()
    dev = torch.device("cuda", 0)

    # device-copy rate of this run: the yardstick of the traffic floor
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), reps)
    copy_gbs = 2 * src.numel() * 4 / copy_ms / 1e6
    print(json.dumps({"device_copy_GBps": round(copy_gbs, 1), "copy_MB": src.numel() * 4 >> 20}), flush=True)
    del src, dst

    B, S = args.batch, args.size
    M = torch.from_numpy(synthetic_masks(B, S, S, args.ncells)).to(dev)
    print(json.dumps(bench("batch", M, False, reps, copy_gbs)), flush=True)
    del M
    Z, H, W = (int(v) for v in args.shape.split(","))
    M = torch.from_numpy(lattice_balls(Z, H, W)).to(dev)
    print(json.dumps(bench("volume_planes", M, True, reps, copy_gbs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
