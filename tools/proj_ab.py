#!/usr/bin/env python3
"""Per-call timing of the two CPnet residual projections that moved into / next to their consumer
(profiles/proj): `down[1]` (1x1 pool2 projection + the pool2 half-block) and `up[2]` (1x1 projection
+ `c1` on the 128-channel ping-pong kernel) at the headline's 288 tiles.

--arm parent  the two launches of each as they were: the projection at the consumer's resolution,
              handed over as a full-resolution residual.  Uses only entry points that the commit
              before the change has too, so the same file runs in a tree copy of that commit.
--arm new     `down[1]`: one launch, the projection inside the pair kernel; `up[2]`: the projection
              at 28^2 and `c1` reading it through an up2 residual.

HIP-event median of --reps launches of each arm's whole sequence; one JSON line per call.  Run parent
and new alternating, 3 rounds per arm."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine  # noqa: E402
from bioengine_worker_amd.ops import conv_pair as cp  # noqa: E402


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
    ap.add_argument("--arm", choices=["parent", "new"], required=True)
    ap.add_argument("--tiles", type=int, default=288)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = CPnetEngine(CPnet().randomize_(0).eval(), dev)
    N = args.tiles
    g = torch.Generator(device="cpu").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)

    # down[1]: x at 224^2 x 32 -> 112^2 x 64
    d1 = eng.down[1]
    sp = eng.pair[("down", 1, 0)]
    fused_spec = sp if getattr(sp, "bias_p", None) is not None else None
    plain = sp.without_proj() if fused_spec is not None else sp
    src = rnd(N, 224, 224, 32).bfloat16()
    out = torch.empty(N, 112, 112, 64, device=dev, dtype=torch.bfloat16)

    def down_parent():
        cp.conv_pair(src, plain, res=d1["proj"](src, inmode="pool2"), res_mode="full", out=out)

    def down_new():
        assert cp.proj_fused(src, fused_spec), "the native side must take the fused call at this size"
        cp.conv_pair(src, fused_spec, out=out)

    # up[2]: x at 28^2 x 256 -> projection 128; c1 at 56^2 x 128
    u2 = eng.up[2]
    xcur = rnd(N, 28, 28, 256).bfloat16()
    h0 = rnd(N, 56, 56, 128).bfloat16()
    shift = (0.1 * rnd(N, 128)).float()

    def up_parent():
        u2["c1"](h0, shift=shift, residual=u2["proj"](xcur, inmode="up2"))

    def up_new():
        u2["c1"](h0, shift=shift, residual=u2["proj"](xcur), residual_mode="up2")

    calls = {"parent": [("down/1 proj + c0c1", down_parent), ("up/2 proj + c1", up_parent)],
             "new": [("down/1 proj + c0c1", down_new), ("up/2 proj + c1", up_new)]}[args.arm]
    with torch.no_grad():
        for name, fn in calls:
            med, mn = timed(fn, args.reps)
            print(json.dumps({"arm": args.arm, "call": name, "tiles": N, "ms": round(med, 4), "ms_min": round(mn, 4)}),
                  flush=True)


if __name__ == "__main__":
    main()
