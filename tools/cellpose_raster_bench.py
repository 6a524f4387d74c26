#!/usr/bin/env python3
"""Time of the Cellpose polygon rasteriser on one GPU (``gpu.rasterize_rings_gpu``).

Two workloads on ``B = 32`` images of ``512 x 512`` with about 150 cells each (the cells that
``pipeline.synthetic_cells`` draws, as ``cellpose_measure_bench.synthetic_masks`` lists them):

* ``rings``: the axis-parallel integer rings ``mask_rings_gpu`` gives for the disks' label images;
* ``gons``:  the same cells as fractional 24-gons (drawn later wins, as in the label images).

Per workload: the whole call from host arrays to the label batch on the device; its host
preparation alone (checks and quantisation, then sort, boxes and job table; wall clock); the device
side alone on prepared buffers (the upload of edges and jobs, the zero fill, the kernel); the
traffic floor (one zero fill and one write of ``B*H*W*4`` bytes plus the upload, at the device-copy
rate measured in the same run); ``mask_rings_gpu`` on the same masks as the sibling yardstick; and
the way without the kernel: the numpy oracle on the host plus the upload of the label batch it
produces.  The result is compared with the oracle in the same run.  Device times are HIP-event
times, warmed, median of ``--reps`` (>= 10).

Needs a GPU: there is no CPU fallback.  Prints one JSON line per result.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cellpose_measure_bench import synthetic_masks, timed  # noqa: E402

from bioengine_worker_amd.cellpose import gpu as cg  # noqa: E402
from bioengine_worker_amd.cellpose import reference as ref  # noqa: E402
from bioengine_worker_amd.ops import _native  # noqa: E402


def cell_gons(B: int, H: int, W: int, ncells: int, sides: int = 24, seed: int = 0) -> dict:
    """The cells of ``synthetic_masks`` (its draws, in its order) as regular ``sides``-gons with
    fractional vertices: a polygons dict of the batch with ``ring_image``."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * (np.arange(sides) + 0.25) / sides
    verts = []
    for _ in range(B):
        cy, cx, r = rng.uniform(0, H, ncells), rng.uniform(0, W, ncells), rng.uniform(6, 14, ncells)
        verts.append(np.stack([cy[:, None] + r[:, None] * np.sin(a), cx[:, None] + r[:, None] * np.cos(a)], -1).reshape(-1, 2))
    n = B * ncells
    return {"verts": np.concatenate(verts), "ring_offsets": np.arange(n + 1, dtype=np.int64) * sides,
            "ring_label": np.tile(np.arange(1, ncells + 1, dtype=np.int32), B),
            "ring_image": np.repeat(np.arange(B, dtype=np.int32), ncells)}


def wall_ms(fn, reps: int) -> float:
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def bench(name: str, polys: dict, shape, masks: torch.Tensor | None, reps: int, copy_gbs: float) -> dict:
    B, H, W = shape
    dev = torch.device("cuda", 0)
    out = cg.rasterize_rings_gpu(polys, B, H, W, dev)
    t = time.perf_counter()
    q, off, labs, img = cg._raster_inputs(polys, B, H, W)
    want = cg._raster_oracle(q, off, labs, img, B, H, W)
    oracle_ms = (time.perf_counter() - t) * 1e3
    same = bool(np.array_equal(out.cpu().numpy(), want))
    if masks is not None:
        same = same and bool(torch.equal(out, masks))
    call_ms = timed(lambda: cg.rasterize_rings_gpu(polys, B, H, W, dev), reps)
    check_ms = wall_ms(lambda: cg._raster_inputs(polys, B, H, W), reps)
    plan_ms = wall_ms(lambda: cg._raster_plan(q, off, labs, img, H, W), reps)
    edges, jobs = cg._raster_plan(q, off, labs, img, H, W)
    E, J = edges.shape[0], jobs.shape[0]
    host = np.concatenate([edges.reshape(-1), jobs.reshape(-1)])
    upload_ms = timed(lambda: torch.from_numpy(host).to(dev, non_blocking=True), reps)
    buf = torch.from_numpy(host).to(dev)
    lab = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    sp = _native.stream(dev)

    def kernel():
        _native.call("be_cp_raster", _native.ptr(buf[:4 * E]), E, _native.ptr(buf[4 * E:]), J, _native.ptr(lab), B, H, W, sp)

    zero_ms = timed(lambda: lab.zero_(), reps)
    both_ms = timed(lambda: (lab.zero_(), kernel()), reps)
    assert torch.equal(lab, out)
    labels_host = torch.from_numpy(want)
    labels_upload_ms = timed(lambda: labels_host.to(dev, non_blocking=True), reps)
    floor_ms = (2 * B * H * W * 4 + host.nbytes) / copy_gbs / 1e6
    res = {"workload": name, "shape": [B, H, W], "rings": int(labs.shape[0]), "edges": int(E), "jobs": int(J),
           "mean_rows_per_job": round(float(jobs[:, 5].mean()), 1), "equals_oracle": same,
           "call_ms": round(call_ms, 3), "host_check_quantise_ms": round(check_ms, 3), "host_plan_ms": round(plan_ms, 3),
           "upload_ms": round(upload_ms, 4), "upload_MB": round(host.nbytes / 1e6, 2), "zero_fill_ms": round(zero_ms, 4),
           "kernel_ms": round(both_ms - zero_ms, 4), "device_ms": round(both_ms + upload_ms, 4),
           "floor_ms": round(floor_ms, 4), "device_over_floor": round((both_ms + upload_ms) / floor_ms, 1),
           "oracle_host_ms": round(oracle_ms, 1), "labels_upload_ms": round(labels_upload_ms, 3),
           "labels_MB": round(want.nbytes / 1e6, 1)}
    if masks is not None:
        nlab = int(labs.max()) + 1
        rings_ms = timed(lambda: cg.mask_rings_gpu(masks, nlab=nlab), reps)
        res.update(mask_rings_ms=round(rings_ms, 4), call_over_mask_rings=round(call_ms / rings_ms, 2))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ncells", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    reps = max(10, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("cellpose_raster_bench needs a GPU")
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
    rings = {k: v.cpu().numpy() for k, v in cg.mask_rings_gpu(M, nlab=args.ncells + 1).items()}
    print(json.dumps(bench("rings", rings, (B, S, S), M, reps, copy_gbs)), flush=True)
    print(json.dumps(bench("gons", cell_gons(B, S, S, args.ncells), (B, S, S), None, reps, copy_gbs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
