#!/usr/bin/env python3
"""Phase profile of the 128-channel ping-pong conv (csrc/kernels/conv_pp128.hip), in the manner of
tools/pp_phase_profile.py: wave 0 of each of the two wave groups accumulates s_memtime cycles of every
phase's own work and of its wait at the closing workgroup barrier.

One call at the headline's level-2 shape (288 tiles of 56^2 x 128 channels), with and without a
residual; one JSON line each with cycles per iteration (= 2 tiles of 8 x 28 pixels; mean over
workgroups).  commit1 / mma1 are the chunks 1..3 together.  --pool: the pooled 64 -> 128 builds instead
(the level-2 entry conv from 288 x 112^2 x 64, alone and with the 1x1 projection inside; commit1 / mma1
are chunk 1, epi includes the projection).  --c256: the 128 -> 256 build (the level-3 entry conv on the
pooled tensor, 288 x 28^2 x 128; an iteration is the two halves of one tile).
Usage: python tools/pp128_phase_profile.py [--pool | --c256]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bioengine_worker_amd.ops import _native  # noqa: E402
from bioengine_worker_amd.ops import conv as cv  # noqa: E402
from bioengine_worker_amd.ops.conv import PackedConv, fused_conv2d  # noqa: E402

NAMES = ["commit0", "mma0", "commit1", "mma1", "epi"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=288)
    ap.add_argument("--hw", type=int, default=56)
    ap.add_argument("--pool", action="store_true")
    ap.add_argument("--c256", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.pool:
        return pool(args, dev)
    if args.c256:
        return c256(args, dev)
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
        report({"residual": r is not None}, buf, cap)


def report(out, buf, cap):
    s = buf.view(cap, 2, 16).cpu().double()
    used = s[:, :, 15] > 0
    out["workgroups"] = int(used[:, 0].sum())
    for g in (0, 1):
        sg = s[:, g][used[:, g]]
        it = sg[:, 15]
        out[f"work_g{g}"] = {NAMES[i]: round(float((sg[:, i] / it).mean())) for i in range(5)}
        out[f"wait_g{g}"] = {NAMES[i]: round(float((sg[:, 8 + i] / it).mean())) for i in range(5)}
    out["cycles_per_2tiles"] = round(sum(out["work_g0"].values()) + sum(out["wait_g0"].values()))
    print(json.dumps(out), flush=True)


def pool(args, dev):
    c0 = PackedConv.from_weight(torch.randn(128, 64, 3, 3) / 24.0, 0.1 * torch.randn(128)).to(dev)
    pj = PackedConv.from_weight(torch.randn(128, 64, 1, 1) / 8.0, 0.1 * torch.randn(128)).to(dev)
    c0.frag(), pj.frag()
    x = torch.randn(args.tiles, 2 * args.hw, 2 * args.hw, 64, device=dev).bfloat16()
    aff = [(1 + 0.1 * torch.randn(64, device=dev)).float() for _ in range(4)]
    if not cv.pp128_takes_pool_proj(c0, pj, x):
        raise SystemExit("the native side does not take the pooled call at this size")
    calls = {
        "pool": lambda: fused_conv2d(x, c0, scale=aff[0], shift=aff[1], relu=True, inmode="pool2"),
        "pool_proj": lambda: cv.fused_conv2d_pool_proj(x, c0, pj, scale=aff[0], shift=aff[1], relu=True, proj_scale=aff[2],
                                                       proj_shift=aff[3]),
    }
    cap = 1024
    buf = torch.zeros(cap * 32, dtype=torch.int64, device=dev)
    for name, fn in calls.items():
        n0 = _native.hip().be_conv_pp128_pool_launches()
        fn()  # warm
        buf.zero_()
        _native.call("be_conv_pp128_set_stamps", _native.ptr(buf), cap)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            _native.call("be_conv_pp128_set_stamps", None, 0)
        if _native.hip().be_conv_pp128_pool_launches() - n0 != 2:
            raise SystemExit("the call did not reach the pooled build")
        report({"build": name}, buf, cap)


def c256(args, dev):
    pc = PackedConv.from_weight(torch.randn(256, 128, 3, 3) / 34.0, 0.1 * torch.randn(256)).to(dev)
    pc.frag()
    hw = 28 if args.hw == 56 else args.hw
    x = torch.randn(args.tiles, hw, hw, 128, device=dev).bfloat16()
    aff = [(1 + 0.1 * torch.randn(c, device=dev)).float() for c in (128, 128, 256, 256)]
    if not cv.pp128_takes_c256(pc, x):
        raise SystemExit("the native side does not take the 256-channel call at this size")

    def fn():
        return cv.fused_conv2d_c256(x, pc, scale=aff[0], shift=aff[1], relu=True, post_scale=aff[2], post_shift=aff[3],
                                    post_relu=True)

    cap = 1024
    buf = torch.zeros(cap * 32, dtype=torch.int64, device=dev)
    n0 = _native.hip().be_conv_pp128_c256_launches()
    fn()  # warm
    _native.call("be_conv_pp128_set_stamps", _native.ptr(buf), cap)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _native.call("be_conv_pp128_set_stamps", None, 0)
    if _native.hip().be_conv_pp128_c256_launches() - n0 != 2:
        raise SystemExit("the call did not reach the 256-channel build")
    report({"build": "c256", "hw": hw}, buf, cap)


if __name__ == "__main__":
    main()
