#!/usr/bin/env python3
"""Phase profile of the 128-channel ping-pong conv (csrc/kernels/conv_pp128.hip), in the manner of
tools/pp_phase_profile.py: wave 0 of each of the two wave groups accumulates s_memtime cycles of every
phase's own work and of its wait at the closing workgroup barrier.

One call at the headline's level-2 shape (288 tiles of 56^2 x 128 channels), with and without a
residual; one JSON line each with cycles per iteration (= 2 tiles of 8 x 28 pixels; mean over
workgroups).  commit1 / mma1 are the chunks 1..3 together.  Usage: python tools/pp128_phase_profile.py"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bioengine_worker_amd.ops import _native  # noqa: E402
from bioengine_worker_amd.ops.conv import PackedConv, fused_conv2d  # noqa: E402

NAMES = ["commit0", "mma0", "commit1", "mma1", "epi"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=288)
    ap.add_argument("--hw", type=int, default=56)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pc = PackedConv.from_weight(torch.randn(128, 128, 3, 3) / 34.0, 0.1 * torch.randn(128)).to(dev)
    pc.frag()
    x = torch.randn(args.tiles, args.hw, args.hw, 128, device=dev).bfloat16()
    res = torch.randn_like(x)
    scale = (1 + 0.1 * torch.randn(128, device=dev)).float()
    shift = (0.1 * torch.randn(args.tiles, 128, device=dev)).float()
    cap = 1024
    buf = torch.zeros(cap * 32, dtype=torch.int64, device=dev)
    for r in (None, res):
        n0 = _native.hip().be_conv_pp128_launches()
        fused_conv2d(x, pc, scale=scale, shift=shift, relu=True, residual=r)  # warm
        buf.zero_()
        _native.call("be_conv_pp128_set_stamps", _native.ptr(buf), cap)
        try:
            fused_conv2d(x, pc, scale=scale, shift=shift, relu=True, residual=r)
            torch.cuda.synchronize()
        finally:
            _native.call("be_conv_pp128_set_stamps", None, 0)
        if _native.hip().be_conv_pp128_launches() - n0 != 2:
            raise SystemExit("the call did not reach conv_pp128_kernel")
        s = buf.view(cap, 2, 16).cpu().double()
        used = s[:, :, 15] > 0
        out = {"residual": r is not None, "workgroups": int(used[:, 0].sum())}
        for g in (0, 1):
            sg = s[:, g][used[:, g]]
            it = sg[:, 15]
            out[f"work_g{g}"] = {NAMES[i]: round(float((sg[:, i] / it).mean())) for i in range(5)}
            out[f"wait_g{g}"] = {NAMES[i]: round(float((sg[:, 8 + i] / it).mean())) for i in range(5)}
        out["cycles_per_2tiles"] = round(sum(out["work_g0"].values()) + sum(out["wait_g0"].values()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
