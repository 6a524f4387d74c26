#!/usr/bin/env python3
"""Time of the Cellpose evaluation stage on one GPU (``gpu.average_precision_gpu``).

Two workloads, labels already on the device, the label bounds given (one host read per call):

* a batch: ``B = 32`` pairs of ``512 x 512`` with about 150 cells each -- the disks of
  ``cellpose_measure_bench.synthetic_masks`` as truth, the prediction a jittered copy (moved by a
  pixel or two, a few cells dropped, labels permuted);
* a volume: one ``64 x 256 x 256`` pair, balls on a jittered lattice, the prediction moved likewise.

Per workload: the HIP stage (the whole call: zero-fill, overlap, areas, match, the one read-back),
the overlap launch alone, the passes over the slots alone (each with its zero-fill), a read-back of the
size of the call's one, the traffic floor (one read of ``T`` and ``P`` at the device-copy rate
measured in the same run), and the way of the code before this stage existed on the same data: the
masks copied to the host plus ``metrics.average_precision`` on numpy (dense ``bincount`` overlap and
a Hungarian solve per threshold), and separately the torch-``bincount`` overlap
(``metrics.label_overlap`` on device tensors, image by image).  Device times are HIP-event times,
warmed, median of ``--reps`` (>= 10); the host paths are wall-clock medians of 3.  The result is
checked against the oracle.

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

from cellpose_measure_bench import lattice_balls, synthetic_masks, timed  # noqa: E402

from bioengine_worker_amd.cellpose import gpu as cg  # noqa: E402
from bioengine_worker_amd.cellpose import metrics  # noqa: E402
from bioengine_worker_amd.ops import _native  # noqa: E402

THRESHOLDS = (0.5, 0.75, 0.9)


def jittered(M: np.ndarray, seed: int = 1) -> np.ndarray:
    """A prediction of truth ``M`` [B, ...]: every image moved by one or two pixels along its last two
    axes, a twentieth of the labels dropped, the rest permuted."""
    rng = np.random.default_rng(seed)
    out = np.zeros_like(M)
    for b in range(M.shape[0]):
        dy, dx = rng.integers(1, 3, 2) * rng.choice([-1, 1], 2)
        n = int(M[b].max())
        lut = np.concatenate([[0], rng.permutation(n) + 1]).astype(M.dtype)
        lut[1:][rng.random(n) < 0.05] = 0
        out[b] = lut[np.roll(M[b], (dy, dx), (-2, -1))]
    return out


def wall(fn, reps: int = 3) -> float:
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def bench(name: str, T: torch.Tensor, P: torch.Tensor, reps: int, copy_gbs: float) -> dict:
    """``T`` / ``P`` [B, ...] int32 on the device."""
    B = T.shape[0]
    nt, np_ = int(T.max()) + 1, int(P.max()) + 1
    info = {}
    got = cg.average_precision_gpu(T, P, THRESHOLDS, nt=nt, np_=np_, info=info)
    want = metrics.average_precision(list(T.cpu().numpy()), list(P.cpu().numpy()), list(THRESHOLDS))
    same = all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
    hip_ms = timed(lambda: cg.average_precision_gpu(T, P, THRESHOLDS, nt=nt, np_=np_), reps)
    nobound_ms = timed(lambda: cg.average_precision_gpu(T, P, THRESHOLDS), reps)

    # the overlap launch alone, on a table of the size the call settled on (zero-fill included)
    cap, N = info["capacity"], T[0].numel()
    Tc, Pc = T.reshape(B, N), P.reshape(B, N)
    keys = torch.empty(B, cap, dtype=torch.int64, device=T.device)
    vals = torch.empty(B, cap, dtype=torch.int32, device=T.device)
    flags = torch.empty(2, dtype=torch.int32, device=T.device)
    st = _native.stream(T.device)

    def overlap():
        keys.zero_(), vals.zero_(), flags.zero_()
        _native.call("be_cp_ap_overlap", _native.ptr(Tc), _native.ptr(Pc), B, N, nt, np_, _native.ptr(keys),
                     _native.ptr(vals), cap, _native.ptr(flags), st)

    overlap_ms = timed(overlap, reps)
    assert flags.tolist() == [0, 0]
    pairs = int((keys != 0).sum())

    # the two passes over the slots alone (their outputs zero-filled in one block, as the call does)
    K, MT = len(THRESHOLDS), cg.AP_MAX_THRESHOLDS
    sizes = [B * nt, B * np_, B * MT, B * MT, B * K * nt, B * K * np_, B, B, B * cap]
    out = torch.empty(sum(sizes), dtype=torch.int32, device=T.device)
    parts = out.split(sizes)
    thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device=T.device)

    def match():
        out.zero_()
        _native.call("be_cp_ap_match", _native.ptr(keys), _native.ptr(vals), B, cap, nt, np_, _native.ptr(thr), K,
                     *[_native.ptr(p) for p in parts], st)

    match_ms = timed(match, reps)
    edges_dev = parts[2].view(B, MT)[:, :K].cpu().numpy()
    same = same and np.array_equal(edges_dev, got[1])  # no conflict here: the edge counts are the true positives
    host_ms = timed(lambda: parts[2].cpu(), reps)  # the size of the call's one read-back

    def parent():
        t, p = T.cpu().numpy(), P.cpu().numpy()  # the D2H of the masks
        metrics.average_precision(list(t), list(p), list(THRESHOLDS))

    def torch_overlap():
        for b in range(B):
            metrics.label_overlap(T[b], P[b])

    parent_ms = wall(parent)
    bincount_ms = wall(torch_overlap)
    floor_ms = 2 * T.numel() * 4 / copy_gbs / 1e6
    return {"workload": name, "shape": list(T.shape), "n_true": nt - 1, "n_pred": np_ - 1, "capacity": cap,
            "distinct_pairs": pairs, "host_matched": info["host_matched"], "equals_oracle": bool(same),
            "hip_ms": round(hip_ms, 4), "hip_no_bounds_ms": round(nobound_ms, 4), "overlap_launch_ms": round(overlap_ms, 4),
            "match_launches_ms": round(match_ms, 4), "readback_ms": round(host_ms, 4),
            "floor_ms": round(floor_ms, 4), "hip_over_floor": round(hip_ms / floor_ms, 1),
            "overlap_over_floor": round(overlap_ms / floor_ms, 1),
            "parent_d2h_numpy_ms": round(parent_ms, 2), "parent_over_hip": round(parent_ms / hip_ms, 1),
            "torch_bincount_overlap_ms": round(bincount_ms, 2), "ap_mean": [round(float(v), 4) for v in np.nanmean(got[0], 0)]}


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
        raise SystemExit("cellpose_ap_bench needs a GPU")
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
    M = synthetic_masks(B, S, S, args.ncells)
    print(json.dumps(bench("batch", torch.from_numpy(M).to(dev), torch.from_numpy(jittered(M)).to(dev), reps, copy_gbs)),
          flush=True)

    Z, H, W = (int(v) for v in args.shape.split(","))
    V = lattice_balls(Z, H, W)[None]
    print(json.dumps(bench("volume", torch.from_numpy(V).to(dev), torch.from_numpy(jittered(V)).to(dev), reps, copy_gbs)),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
