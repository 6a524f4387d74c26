#!/usr/bin/env python3
"""Per-image diameters against scalar-diameter calls on the same images (one GPU).

A batch of ``--batch`` uint16 images of ``--size``^2 whose images have ``--groups`` distinct diameters:
(a) one ``eval`` with the list of diameters (one ragged tile plan), (b) one ``eval`` per distinct
diameter with the scalar form on that diameter's images -- the only way to run them before the list
form existed, and the code path of the scalar form today.  Both are timed with device events around
calls that end in a synchronise, warmed, alternating, ``--reps`` repetitions; then one traced pass
of each reports the device time of the ``cellpose.*`` spans.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIAMETERS = (12.0, 17.0, 22.0, 26.0, 34.0, 41.0, 50.0, 60.0)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-masks", action="store_true", help="time the network stage alone")
    args = ap.parse_args(argv)
    import torch

    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, synthetic_cells
    from bioengine_worker_amd.profiling import trace

    if not torch.cuda.is_available():
        raise SystemExit("cellpose_diameter_bench needs a GPU")
    if args.batch % args.groups or not 0 < args.groups <= len(DIAMETERS):
        raise SystemExit("--batch must be a multiple of --groups (at most 8)")
    dev = torch.device("cuda", 0)
    runner = CellposeRunner(device=dev)
    per = args.batch // args.groups
    x = torch.from_numpy(synthetic_cells(args.batch, args.size, args.size, ncells=60)).to(dev)
    ds = DIAMETERS[: args.groups]
    diams = [d for d in ds for _ in range(per)]
    kw = {"compute_masks": not args.no_masks}

    def list_form():
        return runner.eval(x, diameter=diams, **kw)

    def scalar_calls():
        return [runner.eval(x[k * per: (k + 1) * per], diameter=d, **kw) for k, d in enumerate(ds)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        list_form()
        scalar_calls()
    torch.cuda.synchronize()
    t_list, t_scalar = [], []
    for _ in range(args.reps):  # alternating, so drift of a shared machine hits both alike
        t_list.append(timed(list_form))
        t_scalar.append(timed(scalar_calls))

    def spans(fn):
        trace.clear()
        trace.enable(True)
        fn()
        torch.cuda.synchronize()
        s = trace.summary()
        trace.enable(False)
        return {k.split(":", 1)[1]: v["total_ms"] for k, v in s.items() if k.startswith("gpu:cellpose.")}

    # the flows of both forms on the same images: the list form samples inside the gather, the scalar
    # form resizes the normalised image first, so they differ by the bf16 rounding of the input tiles
    y_list = runner.eval(x, diameter=diams, compute_masks=False)[1]
    y_scal = torch.cat([runner.eval(x[k * per: (k + 1) * per], diameter=d, compute_masks=False)[1] for k, d in enumerate(ds)])
    out = {"batch": args.batch, "size": args.size, "diameters": list(ds), "reps": args.reps, "masks": not args.no_masks,
           "list_form_ms": {"median": round(statistics.median(t_list), 3), "min": round(min(t_list), 3), "max": round(max(t_list), 3)},
           "scalar_calls_ms": {"median": round(statistics.median(t_scalar), 3), "min": round(min(t_scalar), 3),
                               "max": round(max(t_scalar), 3)},
           "list_form_spans_ms": spans(list_form), "scalar_calls_spans_ms": spans(scalar_calls),
           "flows_max_abs_diff": float((y_list - y_scal).abs().max()), "flows_max_abs": float(y_scal.abs().max())}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
