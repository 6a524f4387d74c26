#!/usr/bin/env python3
"""Time of the UMAP transform (``search/umap.py``: ``umap_transform_gpu``; ``be_umap_smooth_knn_query`` and
``be_umap_transform`` of ``csrc/kernels/umap.hip``) on one GPU.

Data: L2-normalised 768-d embeddings of 40 Gaussian clusters (seeded), ``--n-train`` of them fitted with
``umap_fit_gpu``, ``m`` more placed on that layout.  Per ``m`` (1, 90 000 and 1 000 000 by default) the arms are
the four stages on prepared inputs (query table, smooth-kNN, start, layout), an empty launch of the transform
kernel (16 queries whose every slot is pruned: all epochs, no work) and the whole ``umap_transform_gpu``; they
alternate inside one process, HIP-event times (wall clock ending in a synchronise for the whole call), warmed,
median of ``--reps`` (>= 10).  ``layout_16_train`` is the layout with the same schedule (it does not depend on
positions) against a 16-point training set, so that every gather hits the same two cache lines: what is left of
the difference to ``layout`` is what the gathers through L2 cost.  Reported beside them: the per-stage spans of
one whole call, the share of the query table (GEMM + top-k) in the sum of the stages, and the layout's time per
query.  ``--compare`` (default
on) also times a whole fit of ``n_train + 90 000`` points, the only other way to a landscape of that size, and
reports the trustworthiness (sklearn, 15 neighbours, cosine, ``--trust`` sampled points) of fit + transform
against that of the whole fit.

Needs a GPU: there is no CPU fallback.  Prints one JSON line per result.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bioengine_worker_amd.ops import _native  # noqa: E402
from bioengine_worker_amd.search import reference as ref  # noqa: E402
from bioengine_worker_amd.search import umap as gu  # noqa: E402
from umap_bench import alternate, trust  # noqa: E402


def embeddings(n: int, d: int = 768, clusters: int = 40, seed: int = 0, dev="cuda") -> torch.Tensor:
    """As ``umap_bench.embeddings`` with the noise drawn on the device (a million rows take seconds on the host)."""
    centres = torch.randn(clusters, d, generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    lab = torch.randint(0, clusters, (n,), generator=g, device=dev)
    x = centres[lab]
    x += 1.5 * torch.randn(n, d, generator=g, device=dev)
    return torch.nn.functional.normalize(x, dim=1)


def bench(m: int, x: torch.Tensor, Yt: torch.Tensor, reps: int) -> dict:
    dev = x.device
    p = gu.UMAPParams()
    E = ref.transform_n_epochs(p)
    a, b = ref.umap_ab(p.spread, p.min_dist)
    q = embeddings(m, seed=1 + m)
    idx, dist = gu.knn_query_table_gpu(q, x, p.n_neighbors)
    _, _, w = gu.smooth_knn_query_gpu(dist)
    Y0 = gu.transform_init_gpu(idx, w, Yt)
    idx16, Yt16 = (idx % 16).contiguous(), Yt[:16].contiguous()  # every gather hits the same two cache lines
    e_idx = torch.zeros(16, 1, dtype=torch.int32, device=dev)
    e_w = torch.zeros(16, 1, device=dev)  # below 1 / E: never fires
    e_Y = torch.zeros(16, 2, device=dev)
    arms = {
        "knn": (lambda: None, lambda _: gu.knn_query_table_gpu(q, x, p.n_neighbors), "event"),
        "smooth_knn": (lambda: None, lambda _: gu.smooth_knn_query_gpu(dist), "event"),
        "init": (lambda: None, lambda _: gu.transform_init_gpu(idx, w, Yt), "event"),
        "layout": (Y0.clone, lambda Y: gu.transform_layout_gpu(Y, Yt, idx, w, E, a, b, p.seed), "event"),
        "layout_16_train": (Y0.clone, lambda Y: gu.transform_layout_gpu(Y, Yt16, idx16, w, E, a, b, p.seed), "event"),
        "empty_launch": (lambda: None, lambda _: gu.transform_layout_gpu(e_Y, Yt, e_idx, e_w, E, a, b, p.seed), "event"),
        "umap_transform_gpu": (lambda: None, lambda _: gu.umap_transform_gpu(q, x, Yt, p), "wall"),
    }
    ms = alternate(arms, reps)
    Y, info = gu.umap_transform_gpu(q, x, Yt, p)
    stages = ms["knn"] + ms["smooth_knn"] + ms["init"] + ms["layout"]
    live = float((w >= 1.0 / E).float().sum(1).mean())
    return {"m": m, "n_train": int(x.shape[0]), "d": int(x.shape[1]), "n_epochs": E,
            **{f"{k}_ms": round(v, 4) for k, v in ms.items()}, "knn_share_of_stages": round(ms["knn"] / stages, 3),
            "layout_ns_per_query": round(1e6 * ms["layout"] / m, 2), "live_slots_per_query": round(live, 2),
            "transform_spans_ms": info["spans_ms"], "finite": bool(torch.isfinite(Y).all())}


def compare(x: torch.Tensor, Yt: torch.Tensor, m: int, reps: int, n_trust: int) -> dict:
    """Fit ``n_train`` + transform ``m`` against one fit of all ``n_train + m`` points."""
    p = gu.UMAPParams()
    q = embeddings(m, seed=1 + m)
    both = torch.cat([x, q])
    ms = alternate({"fit_all": (lambda: None, lambda _: gu.umap_fit_gpu(both, p), "wall"),
                    "fit_train": (lambda: None, lambda _: gu.umap_fit_gpu(x, p), "wall"),
                    "transform": (lambda: None, lambda _: gu.umap_transform_gpu(q, x, Yt, p), "wall")}, reps)
    Yq, _ = gu.umap_transform_gpu(q, x, Yt, p)
    Yall, _ = gu.umap_fit_gpu(both, p)
    sub = np.sort(np.random.default_rng(0).choice(len(both), size=min(len(both), n_trust), replace=False))
    xs = both[sub].cpu().numpy()
    return {"n_train": int(x.shape[0]), "m": m, **{f"{k}_ms": round(v, 3) for k, v in ms.items()},
            "trust_points": int(sub.size), "trust_fit_plus_transform": round(trust(xs, torch.cat([Yt, Yq])[sub].cpu().numpy()), 4),
            "trust_fit_all": round(trust(xs, Yall[sub].cpu().numpy()), 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[1, 90_000, 1_000_000])
    ap.add_argument("--n-train", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trust", type=int, default=2000)
    ap.add_argument("--compare", type=int, default=90_000, help="m of the fit-all comparison; 0 skips it")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("umap_transform_bench needs a GPU")
    _native.hip()
    x = embeddings(args.n_train)
    Yt, _ = gu.umap_fit_gpu(x)
    for m in args.m:
        print(json.dumps(bench(m, x, Yt, max(10, args.reps))), flush=True)
    if args.compare > 0:
        print(json.dumps(compare(x, Yt, args.compare, max(10, args.reps), args.trust)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
