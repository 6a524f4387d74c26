#!/usr/bin/env python3
"""Time of the Cellpose per-cell measurement stage on one GPU (``gpu.measure_masks_gpu``).

Two workloads, the stage alone (masks and images already on the device, the label bound given, so
nothing is read back):

* a batch: ``B = 32`` images of ``512 x 512``, 2 channels, about 150 cells each -- the disks of the
  cells that ``pipeline.synthetic_cells`` draws (same centres and radii), with its images;
* a volume: ``64 x 256 x 256``, 2 channels, balls on a jittered lattice.

Per workload three numbers: the HIP stage (all five launches of ``be_cp_measure``), the traffic
floor (one read of the labels plus ``C`` fp32 channels at the device-copy rate measured in the same
run) and the same table built from torch ops (``bincount``, ``scatter_reduce``) on the same device,
checked to give the same integers.  Every time is a HIP-event time, warmed, median of ``--reps``
(>= 10).

Needs a GPU: there is no CPU fallback.  Prints one JSON line per result.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bioengine_worker_amd.cellpose import gpu as cg  # noqa: E402
from bioengine_worker_amd.cellpose.pipeline import synthetic_cells  # noqa: E402
from bioengine_worker_amd.ops import _native  # noqa: E402


def timed(fn, reps: int, warm: int = 3) -> float:
    """Median HIP-event time of ``fn()`` in milliseconds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def synthetic_masks(B: int, H: int, W: int, ncells: int, seed: int = 0) -> np.ndarray:
    """Disks of the cells of ``synthetic_cells(B, H, W, ncells=ncells, seed=seed)`` (its draws, in its
    order); a later cell overwrites an earlier one.  [B, H, W] int32, ids as drawn (some may be hidden)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        cy, cx, r = rng.uniform(0, H, ncells), rng.uniform(0, W, ncells), rng.uniform(6, 14, ncells)
        for i in range(ncells):
            y0, y1 = int(max(0, cy[i] - r[i])), int(min(H, cy[i] + r[i] + 1))
            x0, x1 = int(max(0, cx[i] - r[i])), int(min(W, cx[i] + r[i] + 1))
            d2 = (yy[y0:y1, x0:x1] - cy[i]) ** 2 + (xx[y0:y1, x0:x1] - cx[i]) ** 2
            out[b, y0:y1, x0:x1][d2 <= r[i] ** 2] = i + 1
    return out


def lattice_balls(Z: int, H: int, W: int, pitch: int = 28, seed: int = 0) -> np.ndarray:
    """Balls (radii 6-10) on a jittered lattice: [Z, H, W] int32."""
    rng = np.random.default_rng(seed)
    out = np.zeros((Z, H, W), np.int32)
    n = 0
    for cz in np.arange(16, Z - 10, 32):
        for cy in np.arange(14, H - 10, pitch):
            for cx in np.arange(14, W - 10, pitch):
                r = rng.uniform(6, 10)
                c = np.array([cz, cy, cx]) + rng.uniform(-2, 2, 3)
                lo = np.maximum(np.floor(c - r).astype(int), 0)
                hi = np.minimum(np.ceil(c + r).astype(int) + 1, (Z, H, W))
                g = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij"))
                n += 1
                out[tuple(slice(a, b) for a, b in zip(lo, hi))][((g - c[:, None, None, None]) ** 2).sum(0) <= r * r] = n
    return out


def torch_table(M: torch.Tensor, img: torch.Tensor, K: int, volume: bool) -> dict:
    """The raw fields of ``reference.measure_masks`` from torch ops on the device.  ``M`` [B, H, W]
    (or [Z, H, W] with ``volume``), ``img`` [B or Z, C, H, W].  ``bincount`` weights are float64: the
    integer sums are exact while they stay below 2^53."""
    dev = M.device
    Mv = M[None] if volume else M[:, None]  # [B, Z, H, W]
    B, Z, H, W = Mv.shape
    n = K + 1
    idx = (Mv.long() + n * torch.arange(B, device=dev).view(B, 1, 1, 1)).reshape(-1)

    def count(w=None):
        return torch.bincount(idx, weights=w, minlength=B * n).view(B, n)[:, 1:]

    zz, yy, xx = (t.expand(B, Z, H, W).reshape(-1) for t in torch.meshgrid(
        torch.arange(Z, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij"))
    out = {"area": count().long()}
    for name, c in (("sum_z", zz), ("sum_y", yy), ("sum_x", xx)) if volume else (("sum_y", yy), ("sum_x", xx)):
        out[name] = count(c.double()).long()
    if not volume:
        for name, c in (("sum_yy", yy * yy), ("sum_xx", xx * xx), ("sum_xy", xx * yy)):
            out[name] = count(c.double()).long()
    pad = F.pad(Mv, (1, 1, 1, 1) + ((1, 1) if volume else (0, 0)), value=-1)
    z0 = 1 if volume else 0
    core = pad[:, z0:z0 + Z, 1:1 + H, 1:1 + W]
    edge = torch.zeros_like(Mv, dtype=torch.bool)
    for dz, dy, dx in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0)) + (((-1, 0, 0), (1, 0, 0)) if volume else ()):
        edge |= pad[:, z0 + dz:z0 + dz + Z, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] != core
    out["boundary"] = count(edge.reshape(-1).double()).long()
    coords = (zz, yy, xx) if volume else (yy, xx)
    lo = [torch.full((B * n,), 2 ** 31 - 1, dtype=torch.long, device=dev).scatter_reduce(0, idx, c, "amin") for c in coords]
    hi = [torch.full((B * n,), -1, dtype=torch.long, device=dev).scatter_reduce(0, idx, c, "amax") + 1 for c in coords]
    box = torch.stack(lo + hi, 1).view(B, n, -1)[:, 1:]
    out["bbox"] = torch.where(out["area"][..., None] > 0, box, torch.zeros_like(box)).int()
    # img [B or Z, C, H, W] -> per channel in the order of idx
    iv = img.permute(1, 0, 2, 3).reshape(img.shape[1], -1)
    s1, s2, mn, mx = [], [], [], []
    for c in range(iv.shape[0]):
        v = iv[c]
        d = v.double()
        s1.append(count(d))
        s2.append(count(d * d))
        mn.append(torch.full((B * n,), float("inf"), device=dev).scatter_reduce(0, idx, v, "amin").view(B, n)[:, 1:])
        mx.append(torch.full((B * n,), float("-inf"), device=dev).scatter_reduce(0, idx, v, "amax").view(B, n)[:, 1:])
    has = out["area"][..., None] > 0
    out["int_sum"], out["int_sumsq"] = torch.stack(s1, -1), torch.stack(s2, -1)
    out["int_min"] = torch.where(has, torch.stack(mn, -1), torch.zeros((), device=dev))
    out["int_max"] = torch.where(has, torch.stack(mx, -1), torch.zeros((), device=dev))
    return {k: (v[0] if volume else v) for k, v in out.items()}


def bench(name: str, M: torch.Tensor, img: torch.Tensor, volume: bool, reps: int, copy_gbs: float) -> dict:
    K = int(M.max())
    nlab = K + 1
    res = cg.measure_masks_gpu(M, img, nlab=nlab, volume=volume)
    ref = torch_table(M, img, K, volume)
    exact = ("area", "sum_z", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy", "boundary", "bbox", "int_min", "int_max")
    same = all(torch.equal(res[k], ref[k]) for k in exact if k in res)
    rel = max(float(((res[k] - ref[k]).abs() / ref[k].abs().clamp_min(1e-300)).max()) for k in ("int_sum", "int_sumsq"))
    hip_ms = timed(lambda: cg.measure_masks_gpu(M, img, nlab=nlab, volume=volume), reps)
    geo_ms = timed(lambda: cg.measure_masks_gpu(M, None, nlab=nlab, volume=volume), reps)
    torch_ms = timed(lambda: torch_table(M, img, K, volume), reps, warm=2)
    nbytes = M.numel() * 4 * (1 + img.shape[1])
    floor_ms = nbytes / copy_gbs / 1e6
    present = res["area"] > 0
    return {"workload": name, "shape": list(M.shape), "channels": int(img.shape[1]), "K": K,
            "cells": int(present.sum()), "foreground_fraction": round(float((M > 0).float().mean()), 3),
            "hip_ms": round(hip_ms, 4), "hip_geometry_only_ms": round(geo_ms, 4), "floor_ms": round(floor_ms, 4),
            "hip_over_floor": round(hip_ms / floor_ms, 2), "torch_ops_ms": round(torch_ms, 3),
            "torch_over_hip": round(torch_ms / hip_ms, 1), "integers_equal_torch": bool(same),
            "fp64_sums_max_rel_diff": rel}


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
        raise SystemExit("cellpose_measure_bench needs a GPU")
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
    img = torch.from_numpy(synthetic_cells(B, S, S, ncells=args.ncells).astype(np.float32)).to(dev)
    print(json.dumps(bench("batch", M, img, False, reps, copy_gbs)), flush=True)
    del M, img

    Z, H, W = (int(v) for v in args.shape.split(","))
    M = torch.from_numpy(lattice_balls(Z, H, W)).to(dev)
    img = torch.rand(Z, 2, H, W, device=dev) * 4000
    print(json.dumps(bench("volume", M, img, True, reps, copy_gbs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
