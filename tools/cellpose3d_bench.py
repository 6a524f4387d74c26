#!/usr/bin/env python3
"""Stage times of Cellpose do_3D on one GPU (``CellposeRunner.eval_3d`` and the 3-D mask stage).

Two workloads:

* ``eval_3d`` on a ``Z x H x W`` ``synthetic_cells`` stack with the default random CPnet: end to end,
  and its two halves (the three network views with their accumulation, the mask stage);
* the mask stage alone on a synthetic capped-flow volume of the same size with ~150 ellipsoids, stage
  by stage: accumulate (per view), prep, dynamics, seeds, sort, expand, lookup, fill.

Every time is a HIP-event time, warmed, median of ``--reps`` (>= 10).  Streaming stages are reported
against the bytes they must move and a device-copy rate measured in the same run; the dynamics
against its gather count (foreground voxels x niter x 8 corners x 16 B).  The baseline is the same
algorithm written with torch ops on the same GPU (5-D ``grid_sample`` steps, ``index_put_`` histogram,
``max_pool3d`` seeds and window dilations, ``scatter_reduce`` commit), checked to give the same labels.

Needs a GPU: there is no CPU fallback.  Prints one JSON line per result.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bioengine_worker_amd.cellpose import gpu as cg  # noqa: E402
from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, synthetic_cells  # noqa: E402
from bioengine_worker_amd.ops import _native  # noqa: E402

RPAD = cg.RPAD


def timed(fn, reps: int, warm: int = 3) -> float:
    """Median HIP-event time of ``fn()`` in milliseconds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def capped_volume(Z, H, W, pitch=28, seed=0):
    """Capped radial flows of a lattice of ellipsoids (radii 6-9): [4, Z, H, W] float32, count."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((4, Z, H, W), np.float32)
    acc[3] = -5.0
    n = 0
    for cz in np.arange(16, Z - 10, 32):
        for cy in np.arange(14, H - 10, pitch):
            for cx in np.arange(14, W - 10, pitch):
                r = rng.uniform(6, 9, 3)
                c = np.array([cz, cy, cx]) + rng.uniform(-2, 2, 3)
                lo = np.maximum(np.floor(c - r).astype(int), 0)
                hi = np.minimum(np.ceil(c + r).astype(int) + 1, (Z, H, W))
                g = np.stack(np.meshgrid(*[np.arange(a, b, dtype=np.float64) for a, b in zip(lo, hi)], indexing="ij"))
                v = c[:, None, None, None] - g
                inside = ((v / r[:, None, None, None]) ** 2).sum(0) <= 1.0
                nrm = np.sqrt((v ** 2).sum(0))
                f = 5.0 * v / np.maximum(nrm, 1e-12) * np.minimum(nrm, 1.0)
                sl = tuple(slice(a, b) for a, b in zip(lo, hi))
                for k in range(3):
                    acc[k][sl][inside] = f[k][inside]
                acc[3][sl][inside] = 5.0
                n += 1
    return acc, n


# ------------------------------------------------------------------ torch-op baseline


def torch_follow(flow, niter, thr=0.0):
    """reference.follow_flows3d with torch ops on the device -> (p [3, n], inds [n, 3])."""
    dP, cp = flow[:3], flow[3]
    fg = cp > thr
    Z, H, W = cp.shape
    inds = fg.nonzero()
    p = inds.t().float().contiguous()
    im = (dP * fg / 5.0)[[2, 1, 0]].unsqueeze(0)
    L = torch.tensor([W, H, Z], dtype=torch.float32, device=flow.device)
    hi = (L - 1).flip(0)[:, None]
    for _ in range(niter):
        grid = (2 * p.flip(0).t() / (L - 1) - 1).view(1, 1, 1, -1, 3)
        d = F.grid_sample(im, grid, align_corners=False)[0, :, 0, 0, :]
        p = torch.minimum(torch.clamp_min(p + d.flip(0), 0), hi)
    return p, inds


def torch_masks(p, inds, shape, max_size_fraction=0.4):
    """reference.get_masks3d with torch ops on the device (labels before the hole fill)."""
    Z, H, W = shape
    dev = p.device
    hs = (Z + 2 * RPAD, H + 2 * RPAD, W + 2 * RPAD)
    pt = p.long() + RPAD
    for a in range(3):
        pt[a].clamp_(0, shape[a] + RPAD - 1)
    lin = (pt[0] * hs[1] + pt[1]) * hs[2] + pt[2]
    h1 = torch.zeros(hs[0] * hs[1] * hs[2], dtype=torch.int32, device=dev)
    h1.index_put_((lin,), torch.ones_like(lin, dtype=torch.int32), accumulate=True)
    h3 = h1.view(hs)
    hmax = F.max_pool3d(h3[None, None].float(), 5, 1, 2)[0, 0]
    seeds = ((h3 >= hmax) & (h3 > 10)).nonzero()
    M0 = torch.zeros(shape, dtype=torch.int32, device=dev)
    K = seeds.shape[0]
    if K == 0:
        return M0
    slin = (seeds[:, 0] * hs[1] + seeds[:, 1]) * hs[2] + seeds[:, 2]
    order = torch.argsort((h1[slin].long() << 32) | slin)
    seeds = seeds[order]
    o = torch.arange(-5, 6, device=dev)
    wz = (seeds[:, 0, None] + o)[:, :, None, None]
    wy = (seeds[:, 1, None] + o)[:, None, :, None]
    wx = (seeds[:, 2, None] + o)[:, None, None, :]
    widx = (wz * hs[1] + wy) * hs[2] + wx  # [K, 11, 11, 11]; windows of real end points are inside the padding
    sup = (h1[widx.reshape(-1)].view(K, 1, 11, 11, 11) > 2).float()
    sm = torch.zeros_like(sup)
    sm[:, :, 5, 5, 5] = 1
    for _ in range(5):
        sm = F.max_pool3d(sm, 3, 1, 1) * sup
    rank = torch.arange(1, K + 1, device=dev, dtype=torch.int32).view(K, 1, 1, 1).expand(K, 11, 11, 11)
    on = sm.view(K, 11, 11, 11) > 0
    M1 = torch.zeros(hs[0] * hs[1] * hs[2], dtype=torch.int32, device=dev)
    M1.scatter_reduce_(0, widx[on], rank[on], "amax")
    lab = M1[lin]
    cnt = torch.bincount(lab, minlength=K + 1)
    keep = (cnt > 0) & (cnt <= Z * H * W * max_size_fraction)
    keep[0] = False
    lut = (torch.cumsum(keep.int(), 0) * keep.int()).int()
    M0[inds[:, 0], inds[:, 1], inds[:, 2]] = lut[lab.long()]
    return M0


# ------------------------------------------------------------------ the HIP mask stage, stage by stage


def staged_masks(flow, niter, reps, out):
    _, Z, H, W = flow.shape
    dev = flow.device
    st = _native.stream(dev)
    N = Z * H * W
    Zp, Hp, Wp = Z + 2 * RPAD, H + 2 * RPAD, W + 2 * RPAD
    Np = Zp * Hp * Wp
    flow4 = torch.empty(Z, H, W, 4, dtype=torch.float32, device=dev)
    fg = torch.empty(Z, H, W, dtype=torch.uint8, device=dev)
    hist = torch.zeros(Zp, Hp, Wp, dtype=torch.int32, device=dev)
    pos = torch.empty(Z, H, W, dtype=torch.int32, device=dev)
    p_ = _native.ptr

    def prep():
        _native.call("be_cp_prep_flow3d", p_(flow), Z, H, W, 0.0, p_(flow4), p_(fg), st)

    def follow(variant=0):
        hist.zero_()
        _native.call("be_cp_follow_flows3d", p_(flow4), p_(fg), p_(hist), p_(pos), Z, H, W, niter, variant, st)

    t_zero = timed(hist.zero_, reps)
    out["prep_ms"] = timed(prep, reps)
    out["dynamics_ms"] = timed(follow, reps) - t_zero
    out["dynamics_plain_ms"] = timed(lambda: follow(1), reps) - t_zero
    follow()
    nfg = int(fg.sum())
    cap = N // 11 + 1
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    nseeds = torch.zeros(1, dtype=torch.int32, device=dev)

    def seeds():
        nseeds.zero_()
        _native.call("be_cp_seeds3d", p_(hist), Zp, Hp, Wp, p_(keys), p_(nseeds), cap, st)

    out["seeds_ms"] = timed(seeds, reps)
    k = int(nseeds.item())
    ks = torch.sort(keys[:k])[0]
    out["sort_ms"] = timed(lambda: torch.sort(keys[:k]), reps)
    M1 = torch.zeros(Zp, Hp, Wp, dtype=torch.int32, device=dev)

    def expand():
        _native.call("be_cp_expand3d", p_(hist), p_(ks), k, Zp, Hp, Wp, p_(M1), st)

    out["expand_ms"] = timed(expand, reps)
    M0 = torch.zeros(Z, H, W, dtype=torch.int32, device=dev)
    counts = torch.zeros(1, k + 1, dtype=torch.int32, device=dev)

    def lookup():
        counts.zero_()
        _native.call("be_cp_label_lookup", p_(pos), p_(M1), 1, N, Np, p_(M0), p_(counts), k + 1, st)

    out["lookup_ms"] = timed(lookup, reps)
    keep = (counts > 0) & (counts <= N * 0.4)
    out["renumber_ms"] = timed(lambda: cg._renumber(M0.view(1, N), keep), reps)
    M = cg._renumber(M0.view(1, N), keep).view(Z, H, W)
    out["fill_ms"] = timed(lambda: cg.fill_holes3d_gpu(M, 15, k + 1), reps)
    out.update(voxels=N, foreground=nfg, seeds=k, niter=niter)
    return M, nfg


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64,256,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--niter", type=int, default=200)
    ap.add_argument("--skip-net", action="store_true")
    args = ap.parse_args(argv)
    Z, H, W = (int(v) for v in args.shape.split(","))
    reps = max(10, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("cellpose3d_bench needs a GPU")
    _native.hip()
    dev = torch.device("cuda", 0)
    N = Z * H * W

    # device-copy rate of this run: the yardstick of the streaming stages
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), reps)
    copy_gbs = 2 * src.numel() * 4 / copy_ms / 1e6
    print(json.dumps({"device_copy_GBps": round(copy_gbs, 1), "copy_MB": src.numel() * 4 >> 20}))
    del src, dst

    # ---- mask stage on the capped-flow volume
    acc_np, ncell = capped_volume(Z, H, W)
    flow = torch.from_numpy(acc_np).to(dev)
    out = {"workload": "masks3d_capped", "shape": [Z, H, W], "ellipsoids": ncell}
    raw, nfg = staged_masks(flow, args.niter, reps, out)
    out["compute_masks3d_ms"] = timed(lambda: cg.compute_masks3d_gpu(flow, None, niter=args.niter), reps)
    masks = cg.compute_masks3d_gpu(flow, None, niter=args.niter)
    out["instances"] = int(masks.max())
    gather_bytes = nfg * args.niter * 8 * 16
    out["dynamics_gather_GB"] = round(gather_bytes / 1e9, 2)
    out["dynamics_gather_GBps"] = round(gather_bytes / out["dynamics_ms"] / 1e6, 1)
    prep_bytes = N * (16 + 16 + 1)
    out["prep_floor_ms"] = round(prep_bytes / copy_gbs / 1e6, 4)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))

    # accumulate: whole views in chunks of 32 planes
    ys = [torch.randn(s, device=dev) for s in ((Z, 3, H, W), (H, 3, Z, W), (W, 3, Z, H))]
    acc = torch.empty(4, Z, H, W, dtype=torch.float32, device=dev)
    a = {"workload": "accumulate", "chunk": 32}
    for view, (name, nbytes) in enumerate((("yx", 28 * N), ("zx", 36 * N), ("zy", 36 * N))):
        y = ys[view]

        def run(y=y, view=view):
            for i in range(0, y.shape[0], 32):
                cg.accum_view3d(acc, y[i: i + 32], view, i)

        a[f"{name}_ms"] = round(timed(run, reps), 4)
        a[f"{name}_floor_ms"] = round(nbytes / copy_gbs / 1e6, 4)
    print(json.dumps(a))
    del ys, acc

    # ---- torch-op baseline of the same algorithm (labels before the hole fill)
    b = {"workload": "torch_baseline"}
    p, inds = torch_follow(flow, args.niter)
    b["follow_ms"] = timed(lambda: torch_follow(flow, args.niter), reps, warm=1)
    b["masks_ms"] = timed(lambda: torch_masks(p, inds, (Z, H, W)), reps, warm=1)
    tm = torch_masks(p, inds, (Z, H, W))
    # end points that fall within rounding of a bin edge may bin differently in the two formulations
    b["instances"] = int(tm.max())
    b["voxels_labelled_differently_from_hip"] = int(((tm > 0) != (raw > 0)).sum()) if int(tm.max()) != int(raw.max()) \
        else int((tm != raw).sum())
    hip = out["prep_ms"] + out["dynamics_ms"] + out["seeds_ms"] + out["sort_ms"] + out["expand_ms"] + out["lookup_ms"] \
        + out["renumber_ms"]
    b["hip_same_stages_ms"] = hip
    b["speedup"] = (b["follow_ms"] + b["masks_ms"]) / hip
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in b.items()}))
    del p, inds, tm, flow

    # ---- eval_3d end to end with the random CPnet
    if not args.skip_net:
        runner = CellposeRunner(device=dev)
        stack = torch.from_numpy(synthetic_cells(Z, H, W, ncells=150, seed=0).astype(np.float32)).to(dev)
        e = {"workload": "eval_3d", "shape": [Z, H, W], "planes": Z + H + W}
        e["views_ms"] = timed(lambda: runner.eval_3d(stack, compute_masks=False), reps, warm=2)
        _, f, _ = runner.eval_3d(stack, compute_masks=False)
        e["masks_ms"] = timed(lambda: cg.compute_masks3d_gpu(f, None), reps, warm=2)
        e["eval_3d_ms"] = timed(lambda: runner.eval_3d(stack), reps, warm=2)
        m, _, _ = runner.eval_3d(stack)
        e["foreground"] = int((f[3] > 0).sum())
        e["instances"] = int(m.max())
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in e.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
