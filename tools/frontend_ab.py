#!/usr/bin/env python3
"""Time the Cellpose front end alone: raw uint16 batch on the device -> NHWC bf16 network tiles.

Two arms:

* ``seq``   -- convert to fp32, ``normalize99`` into an fp32 image, ``TilePlan.gather`` (the sequence
  every input took before the fused front end, and the one ``BE_CELLPOSE_FUSED_FRONT=0`` restores);
* ``fused`` -- ``TilePlan.gather_normalized`` on the raw pixels (percentile select on the integer
  keys + normalising gather).

``--tree DIR`` imports the package from another checkout (its own native build), so the ``seq`` arm
can be timed on the kernels of an earlier commit.  Each shape runs ``--reps`` timed calls after
``--warmup``; per call the device time between two events.  Prints one JSON line per shape with the
median and the minimum.  ``--check`` also compares the two arms' tiles
bit for bit (current tree only).

Usage: python tools/frontend_ab.py --arm seq|fused [--tree DIR] [--reps 50] [--warmup 10] [--check]"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["seq", "fused"], required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose.pipeline import as_batch, synthetic_cells
    from bioengine_worker_amd.ops import _native

    dev = torch.device("cuda", 0)
    _native.hip()
    plan = cg.TilePlan(512, 512, 224, 0.1, device=dev)
    imgs = torch.from_numpy(synthetic_cells(32, 512, 512, nchan=2, seed=0)).to(dev)

    def seq(x):
        return plan.gather(cg.normalize99(as_batch(x, 2, dev)), 8)

    def fused(x):
        return plan.gather_normalized(x, 8, 2)

    fn = seq if a.arm == "seq" else fused
    for name, x in (("headline_b32", imgs), ("batch1", imgs[:1])):
        for _ in range(a.warmup):
            fn(x)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(x)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        rec = {"arm": a.arm, "tag": a.tag, "shape": name, "reps": a.reps, "median_ms": round(statistics.median(times), 4),
               "min_ms": round(min(times), 4), "lib": str(_native.hip_lib_path())}
        if a.check:
            rec["tiles_equal"] = bool(torch.equal(seq(x).view(torch.int16), fused(x).view(torch.int16)))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
