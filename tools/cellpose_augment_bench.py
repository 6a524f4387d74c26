#!/usr/bin/env python3
"""Cost of Cellpose test-time augmentation: a batch of 32 raw uint16 images of 512 x 512 x 2 on the
device through ``CellposeRunner.eval`` with ``augment`` off and on.

The two arms alternate (off, on, off, on, ...), ``--reps`` timed calls each after ``--warmup`` calls
of both; per call the device time between two events around ``eval`` (the call returns after its last
host read, so the events enclose all its work).  Prints one JSON line per arm with the median and
the minimum time per batch, images per second at the median and the tiles per image of the arm's tile
plan, then one line with the ratio of the medians next to the ratio of the tile counts.

Usage: python tools/cellpose_augment_bench.py [--batch 32] [--size 512] [--reps 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, EvalParams, synthetic_cells
    from bioengine_worker_amd.ops import _native

    dev = torch.device("cuda", 0)
    _native.hip()
    runner = CellposeRunner(device=dev, seed=0)
    imgs = torch.from_numpy(synthetic_cells(a.batch, a.size, a.size, nchan=2, seed=0)).to(dev)
    arms = {"off": False, "on": True}

    def run(aug):
        return runner.eval(imgs, EvalParams(augment=aug))

    for _ in range(a.warmup):
        for aug in arms.values():
            run(aug)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.reps):
        for name, aug in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(aug)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med, tiles = {}, {}
    for name, aug in arms.items():
        med[name] = statistics.median(times[name])
        tiles[name] = runner._plan(a.size, a.size, EvalParams(augment=aug)).nt
        print(json.dumps({"augment": aug, "batch": a.batch, "size": a.size, "reps": a.reps,
                          "median_ms": round(med[name], 3), "min_ms": round(min(times[name]), 3),
                          "img_per_s": round(a.batch / med[name] * 1e3, 1), "tiles_per_image": tiles[name]}), flush=True)
    print(json.dumps({"time_ratio_on_over_off": round(med["on"] / med["off"], 3),
                      "tile_ratio_on_over_off": round(tiles["on"] / tiles["off"], 3)}), flush=True)


if __name__ == "__main__":
    main()
