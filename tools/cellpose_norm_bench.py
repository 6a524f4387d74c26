#!/usr/bin/env python3
"""Cost of the Cellpose normalisation options: a batch of 32 raw uint16 images of 512 x 512 x 2 on the
device through ``CellposeRunner.eval`` under

* ``default``      the 1st / 99th percentile over the whole image,
* ``tile100``      ``normalize={"tile_norm_blocksize": 100}``,
* ``pct_invert``   ``normalize={"percentile": [0.5, 99.5], "invert": True}``,

and the front end alone (what the ``cellpose.tiles_gather`` span encloses: select passes, maps and
the normalising tile gather, :meth:`TilePlan.gather_normalized`) under the same three settings.

All arms alternate within one process (a, b, c, a, b, c, ...), ``--reps`` timed calls each after
``--warmup`` calls of every arm; per call the device time between two HIP events around it.  Prints
one JSON line per arm (median and minimum), then the traffic floor of the tile-norm front end: the
raw batch is read about 1.2^2 times by the overlapping blocks (exactly: the summed block areas over
the image area) and once by the gather, and the bf16 tiles are written once; the bytes are divided
by the rate of a device-to-device copy of a buffer as large as the tiles, measured in the same run.
``net.*`` is ``eval`` without mask recovery: under ``invert`` the masks are recovered from another
image, so the ``eval.*`` arms differ by more than their front ends.

Usage: python tools/cellpose_norm_bench.py [--batch 32] [--size 512] [--reps 10] [--warmup 3]"""
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

    from bioengine_worker_amd.cellpose import reference as ref
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, EvalParams, norm_params, synthetic_cells
    from bioengine_worker_amd.ops import _native

    dev = torch.device("cuda", 0)
    _native.hip()
    runner = CellposeRunner(device=dev, seed=0)
    imgs = torch.from_numpy(synthetic_cells(a.batch, a.size, a.size, nchan=2, seed=0)).to(dev)
    settings = {"default": True, "tile100": {"tile_norm_blocksize": 100},
                "pct_invert": {"percentile": [0.5, 99.5], "invert": True}}
    plan = runner._plan(a.size, a.size, EvalParams())
    # the copy that sets the rate moves as many bytes as the tiles the front end writes (the larger
    # part of its traffic, far more than the last-level cache holds)
    copy_src = torch.empty(a.batch * plan.nt, plan.by, plan.bx, runner.cin_pad, dtype=torch.bfloat16, device=dev).fill_(1)
    copy_dst = torch.empty_like(copy_src)

    def front(norm):
        p = norm_params(norm)
        return plan.gather_normalized(imgs, runner.cin_pad, runner.nchan, params=None if p.is_default else p)

    arms = {}
    for name, norm in settings.items():
        arms["eval." + name] = lambda norm=norm: runner.eval(imgs, EvalParams(normalize=norm))
    for name, norm in settings.items():
        arms["front." + name] = lambda norm=norm: front(norm)
    # the two launches the tile-norm front end adds before its gather, on their own
    from bioengine_worker_amd.cellpose import gpu as cg

    raw_maps = cg.tile_block_percentiles_gpu(imgs, 100, c_use=runner.nchan)
    arms["front.tile100.block_select"] = lambda: cg.tile_block_percentiles_gpu(imgs, 100, c_use=runner.nchan)
    arms["front.tile100.maps"] = lambda: cg.tile_maps_fill_smooth_gpu(raw_maps[0].clone(), raw_maps[1].clone())
    # the network stage without mask recovery: inverting changes the image the masks are recovered
    # from, so eval.* under invert measures other masks, not the front end
    for name, norm in settings.items():
        arms["net." + name] = lambda norm=norm: runner.eval(imgs, EvalParams(normalize=norm, compute_masks=False))
    arms["copy"] = lambda: copy_dst.copy_(copy_src)

    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.reps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in arms:
        row = {"arm": name, "batch": a.batch, "size": a.size, "reps": a.reps, "median_ms": round(med[name], 4),
               "min_ms": round(min(times[name]), 4)}
        if name.startswith("eval."):
            row["img_per_s"] = round(a.batch / med[name] * 1e3, 1)
        print(json.dumps(row), flush=True)
    raw = imgs.numel() * imgs.element_size()
    rate = 2 * copy_src.numel() * 2 / (med["copy"] * 1e-3)  # bytes read + written per second
    ys, bh = ref.tile_norm_blocks(a.size, 100)
    xs, bw = ref.tile_norm_blocks(a.size, 100)
    reread = len(ys) * bh * len(xs) * bw / (a.size * a.size)
    tiles = a.batch * plan.nt * plan.by * plan.bx * runner.cin_pad * 2
    floor_tile = (raw * (reread + 1) + tiles) / rate * 1e3
    floor_default = (raw * 3 + tiles) / rate * 1e3  # two select passes of uint16 + the gather
    print(json.dumps({"copy_GBps": round(rate / 1e9, 1), "raw_MB": round(raw / 1e6, 2), "tiles_MB": round(tiles / 1e6, 2),
                      "block_reread": round(reread, 3), "floor_ms.front.tile100": round(floor_tile, 4),
                      "floor_ms.front.default": round(floor_default, 4),
                      "front.tile100_over_floor": round(med["front.tile100"] / floor_tile, 2),
                      "front.default_over_floor": round(med["front.default"] / floor_default, 2),
                      "front.tile100_over_default": round(med["front.tile100"] / med["front.default"], 3),
                      "net.tile100_over_default": round(med["net.tile100"] / med["net.default"], 4),
                      "net.pct_invert_over_default": round(med["net.pct_invert"] / med["net.default"], 4),
                      "eval.tile100_over_default": round(med["eval.tile100"] / med["eval.default"], 4),
                      "eval.pct_invert_over_default": round(med["eval.pct_invert"] / med["eval.default"], 4)}), flush=True)


if __name__ == "__main__":
    main()
