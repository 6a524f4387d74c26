#!/usr/bin/env python3
"""Per-call timing of CPnet's level-3 entry (profiles/down3): `down[3]` projection + `c0` at the
headline's 288 tiles, the pair in sequence and call by call, on an `xd[2]`-shaped source
([tiles, 56, 56, 128]) with the engine's own packed weights and affines.

--arm parent   the two launches as they were: projection and `c0` on the per-layer kernel, both reading
               the source through the 2x2 max-pool.  Uses only entry points that the commit before the
               change has too, so the same file runs in a tree copy of that commit.
--arm prepool  the source pooled once (`be_pool2_nhwc`), projection and `c0` on the per-layer kernel
               with no input transform.
--arm new      pooled once, projection on the per-layer kernel, `c0` on the ping-pong kernel's
               256-channel build (`be_conv_pp128_c256`).

HIP-event median of --reps launches; one JSON line per call.  Run the arms alternating, 3 rounds each,
every round in a fresh process."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine  # noqa: E402
from bioengine_worker_amd.ops import conv as cv  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["parent", "prepool", "new"], required=True)
    ap.add_argument("--tiles", type=int, default=288)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = CPnetEngine(CPnet().randomize_(0).eval(), dev)
    N = args.tiles
    g = torch.Generator(device="cpu").manual_seed(3)
    src = torch.randn(N, 56, 56, 128, generator=g).bfloat16().to(dev)
    e = eng.down[3]
    c0, c1 = e["c0"], e["c1"]
    post = dict(post_scale=c1.scale, post_shift=c1.shift, post_relu=True)
    if args.arm == "parent":
        def proj():
            return e["proj"](src, inmode="pool2")

        def conv0():
            return cv.fused_conv2d(src, c0.pc, scale=c0.scale, shift=c0.shift, relu=True, inmode="pool2", **post)

        def pair():
            return proj(), conv0()

        calls = [("down/3 proj + c0", pair), ("down/3 proj", proj), ("down/3 c0", conv0)]
    else:
        pooled = cv.pool2_nhwc(src)
        if args.arm == "new":
            assert cv.pp128_takes_c256(c0.pc, pooled), "the native side must take the 256-channel call at this size"

        def pool():
            return cv.pool2_nhwc(src, out=pooled)

        def proj():
            return e["proj"](pooled)

        def conv0():
            if args.arm == "new":
                return cv.fused_conv2d_c256(pooled, c0.pc, scale=c0.scale, shift=c0.shift, relu=True, **post)
            return cv.fused_conv2d(pooled, c0.pc, scale=c0.scale, shift=c0.shift, relu=True, nw=8, **post)

        def pair():
            pool()
            return proj(), conv0()

        calls = [("down/3 proj + c0", pair), ("down/3 pool", pool), ("down/3 proj", proj), ("down/3 c0", conv0)]
    with torch.no_grad():
        for name, fn in calls:
            med, mn = timed(fn, args.reps)
            print(json.dumps({"arm": args.arm, "call": name, "tiles": N, "ms": round(med, 4), "ms_min": round(mn, 4)}),
                  flush=True)


if __name__ == "__main__":
    main()
