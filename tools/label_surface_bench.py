#!/usr/bin/env python3
"""Time of the label-surface stage on one GPU (``gpu.label_surface_gpu`` / ``gpu.surface_stats_gpu``).

Two workloads, the stage alone (labels already on the device as int32, the label bound given):

* the ``64 x 256 x 256`` volume with 162 balls on a jittered lattice that the measurement and AP
  benches use;
* one sparse ``256 x 512 x 512`` volume: the same balls at a pitch of 64.

Per workload: the whole call; its parts from HIP events recorded around the call's launches
(``count``, the prefix sum over the tiles (``scan``), the host's read of ``V`` and ``F``, ``emit``, the
two stable sorts, ``gather`` (label offsets and vertices), ``remap`` (the quads' vertex indices) and
``faces``), ``stats`` on its own; the traffic floor (one read of the labels plus one write of the outputs at the device-copy
rate measured in the same run); and the sibling yardstick ``measure_masks_gpu(volume=True)`` on
the same labels.  Every time is a HIP-event time, warmed, median of ``--reps`` (>= 10).  The result
is compared with the numpy oracle in the same run (``--no-check`` skips it for the large volume).

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

from cellpose_measure_bench import lattice_balls, timed  # noqa: E402

from bioengine_worker_amd.cellpose import gpu as cg  # noqa: E402
from bioengine_worker_amd.cellpose import reference as ref  # noqa: E402
from bioengine_worker_amd.ops import _native  # noqa: E402

PARTS = ("count", "scan", "read", "emit", "sort", "gather", "remap", "faces")


def part_times(L: torch.Tensor, nlab: int, reps: int) -> dict:
    """Median time of every part of one call.  The call itself carries no hook: HIP events are
    recorded around each of its native launches and before its read of ``V`` and ``F`` by wrapping
    ``_native.call`` and ``_host_ints`` here, and the torch steps are the gaps between them (the
    tile scan: end of ``count`` to the read; the sorts: end of ``emit`` to the start of ``gather``)."""
    real_call, real_read = cg._native.call, cg._host_ints
    marks = {}

    def mark(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.setdefault(name, ev)

    def call(name, *a):
        mark(name + ":0")
        real_call(name, *a)
        mark(name + ":1")

    def read(t):
        mark("read:0")  # the first read (V, F); the error word at the end is not timed
        return real_read(t)

    edges = (("count", "be_surf_count:0", "be_surf_count:1"), ("scan", "be_surf_count:1", "read:0"),
             ("read", "read:0", "be_surf_emit:0"), ("emit", "be_surf_emit:0", "be_surf_emit:1"),
             ("sort", "be_surf_emit:1", "be_surf_gather:0"), ("gather", "be_surf_gather:0", "be_surf_gather:1"),
             ("remap", "be_surf_remap:0", "be_surf_remap:1"), ("faces", "be_surf_faces:0", "be_surf_faces:1"))
    rows = []
    cg._native.call, cg._host_ints = call, read
    try:
        for i in range(reps + 3):
            marks.clear()
            cg.label_surface_gpu(L, nlab=nlab)
            torch.cuda.synchronize()
            if i >= 3:
                rows.append([marks[a].elapsed_time(marks[b]) for _, a, b in edges])
    finally:
        cg._native.call, cg._host_ints = real_call, real_read
    med = np.median(np.array(rows), 0)
    return {e[0] + "_ms": round(float(v), 4) for e, v in zip(edges, med)}


def bench(name: str, L: torch.Tensor, reps: int, copy_gbs: float, check: bool) -> dict:
    K = int(L.max())
    nlab = K + 1
    surf = cg.label_surface_gpu(L, nlab=nlab)
    stats = cg.surface_stats_gpu(surf, (2.0, 1.0, 1.0))
    out = {"workload": name, "shape": list(L.shape), "K": K, "V": int(surf["verts"].shape[0]),
           "F": int(surf["quads"].shape[0]), "foreground_fraction": round(float((L > 0).float().mean()), 4)}
    if check:
        want = ref.label_surface(L.cpu().numpy(), nlab)
        out["equals_oracle"] = all(surf[k].cpu().numpy().tobytes() == want[k].tobytes() for k in want)
        wt = ref.surface_stats(want, (2.0, 1.0, 1.0))
        rel = lambda k: float(np.nanmax(np.abs(stats[k].cpu().numpy() - wt[k]) / np.maximum(np.abs(wt[k]), 1e-300)))
        out["area_max_rel_diff"], out["mesh_volume_max_rel_diff"] = rel("area"), rel("mesh_volume")
    out["call_ms"] = round(timed(lambda: cg.label_surface_gpu(L, nlab=nlab), reps), 4)
    out.update(part_times(L, nlab, reps))
    out["stats_ms"] = round(timed(lambda: cg.surface_stats_gpu(surf, (2.0, 1.0, 1.0)), reps), 4)
    nbytes = L.numel() * 4 + sum(int(v.numel()) * v.element_size() for v in surf.values())
    out["floor_ms"] = round(nbytes / copy_gbs / 1e6, 4)
    out["call_over_floor"] = round(out["call_ms"] / out["floor_ms"], 2)
    out["measure_volume_ms"] = round(timed(lambda: cg.measure_masks_gpu(L, None, nlab=nlab, volume=True), reps), 4)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64,256,256")
    ap.add_argument("--sparse-shape", default="256,512,512")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-check", action="store_true", help="skip the oracle comparison of the sparse volume")
    args = ap.parse_args(argv)
    reps = max(10, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("label_surface_bench needs a GPU")
    _native.hip()
    dev = torch.device("cuda", 0)

    # device-copy rate of this run: the yardstick of the traffic floor
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), reps)
    copy_gbs = 2 * src.numel() * 4 / copy_ms / 1e6
    print(json.dumps({"device_copy_GBps": round(copy_gbs, 1), "copy_MB": src.numel() * 4 >> 20}), flush=True)
    del src, dst

    Z, H, W = (int(v) for v in args.shape.split(","))
    L = torch.from_numpy(lattice_balls(Z, H, W)).to(dev)
    print(json.dumps(bench("balls", L, reps, copy_gbs, True)), flush=True)
    del L
    Z, H, W = (int(v) for v in args.sparse_shape.split(","))
    L = torch.from_numpy(lattice_balls(Z, H, W, pitch=64)).to(dev)
    print(json.dumps(bench("sparse", L, reps, copy_gbs, not args.no_check)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
