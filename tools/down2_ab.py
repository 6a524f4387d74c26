#!/usr/bin/env python3
"""Per-call timing of CPnet's level-2 entry (profiles/down2): `down[2]` projection + `c0` + `c1` at
the headline's 288 tiles, whole sequence and call by call.

--arm parent  the three launches as they were: projection and `c0` on the per-layer kernel (pool2),
              `c1` on the 128-channel ping-pong kernel with the projection as its residual.  Uses only
              entry points that the commit before the change has too, so the same file runs in a tree
              copy of that commit.
--arm c0      `c0` on the ping-pong kernel's pooled build, the projection still a launch of its own
              (BE_CONV_PP128_POOL_PROJ=0 in one process).
--arm new     projection and `c0` in one launch of the pooled build, then `c1`.

HIP-event median of --reps launches; one JSON line per call.  Run the arms alternating, 3 rounds each."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine  # noqa: E402
from bioengine_worker_amd.ops import _native  # noqa: E402
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
    ap.add_argument("--arm", choices=["parent", "c0", "new"], required=True)
    ap.add_argument("--tiles", type=int, default=288)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = CPnetEngine(CPnet().randomize_(0).eval(), dev)
    N = args.tiles
    g = torch.Generator(device="cpu").manual_seed(2)
    src = torch.randn(N, 112, 112, 64, generator=g).bfloat16().to(dev)
    e = eng.down[2]
    if args.arm == "c0":
        _native.call("be_conv_pp128_set_pool", 1, 0)
    if args.arm == "new":
        assert cv.pp128_takes_pool_proj(e["c0"].pc, e["proj"].pc, src), "the native side must take the fused call at this size"
    if args.arm == "c0":
        assert cv.pp128_takes_pool(e["c0"].pc, src) and not cv.pp128_takes_pool_proj(e["c0"].pc, e["proj"].pc, src)

    def proj():
        return e["proj"](src, inmode="pool2")

    def c0():
        return e["c0"](src, inmode="pool2")

    def fused():
        c, p = e["c0"], e["proj"]
        return cv.fused_conv2d_pool_proj(src, c.pc, p.pc, scale=c.scale, shift=c.shift, relu=c.relu, proj_scale=p.scale,
                                         proj_shift=p.shift)

    def entry():
        if args.arm == "new":
            return fused()
        p = proj()
        return c0(), p

    h0, p0 = entry()

    def c1():
        return e["c1"](h0, residual=p0)

    def whole():
        h, p = entry()
        return e["c1"](h, residual=p)

    calls = [("down/2 proj + c0 + c1", whole), ("down/2 c1", c1)]
    if args.arm == "new":
        calls.append(("down/2 proj + c0 (one launch)", fused))
    else:
        calls += [("down/2 proj", proj), ("down/2 c0", c0)]
    with torch.no_grad():
        for name, fn in calls:
            med, mn = timed(fn, args.reps)
            print(json.dumps({"arm": args.arm, "call": name, "tiles": N, "ms": round(med, 4), "ms_min": round(mn, 4)}),
                  flush=True)


if __name__ == "__main__":
    main()
