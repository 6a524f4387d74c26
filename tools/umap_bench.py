#!/usr/bin/env python3
"""Time of the in-house UMAP (``search/umap.py``, ``csrc/kernels/umap.hip``) on one GPU.

Data: ``n`` L2-normalised 768-d embeddings of 40 Gaussian clusters (seeded).  Per ``n`` (10 000 and
100 000 by default) the arms are the four stages on prepared inputs (kNN, smooth-kNN, graph, layout), the
PCA initialisation, the whole ``umap_fit_gpu`` and the PCA path of ``projection.project_2d``; they
alternate inside one process, HIP-event times (wall clock ending in a synchronise for the two whole-call
arms, which return host or timed results), warmed, median of ``--reps`` (>= 10).  Reported beside them:
the epoch kernel's time per epoch, the median / maximum degree, the launch-latency share of the layout
(``n_epochs`` x an empty launch of the same kernel, measured in the same run), and the trustworthiness
(sklearn, 15 neighbours, cosine) of the UMAP and the PCA projection on a seeded sub-sample of
``--trust`` points where ``n <= 10 000``.  The numpy oracle is timed once at ``--oracle-n`` points.

Needs a GPU: there is no CPU fallback.  Prints one JSON line per result.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bioengine_worker_amd.ops import _native  # noqa: E402
from bioengine_worker_amd.search import projection  # noqa: E402
from bioengine_worker_amd.search import reference as ref  # noqa: E402
from bioengine_worker_amd.search import umap as gu  # noqa: E402


def embeddings(n: int, d: int = 768, clusters: int = 40, seed: int = 0, dev="cuda") -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn(clusters, d, generator=g)
    lab = torch.randint(0, clusters, (n,), generator=g)
    x = centres[lab] + 1.5 * torch.randn(n, d, generator=g)
    return torch.nn.functional.normalize(x, dim=1).to(dev)


def alternate(arms: dict, reps: int, warm: int = 2) -> dict:
    """``arms``: name -> (setup, run, kind); kind "event" is timed with HIP events around ``run(setup())``,
    kind "wall" with the host clock around a call that ends synchronised.  -> median ms per arm."""
    out = {k: [] for k in arms}
    for r in range(warm + reps):
        for name, (setup, run, kind) in arms.items():
            arg = setup()
            torch.cuda.synchronize()
            if kind == "event":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(arg)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
            else:
                t = time.perf_counter()
                run(arg)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t) * 1e3
            if r >= warm:
                out[name].append(ms)
    return {k: float(np.median(v)) for k, v in out.items()}


def trust(x: np.ndarray, Y: np.ndarray) -> float:
    from sklearn.manifold import trustworthiness

    return float(trustworthiness(x, Y, n_neighbors=15, metric="cosine"))


def bench(n: int, reps: int, n_trust: int) -> dict:
    dev = torch.device("cuda", 0)
    p = gu.UMAPParams()
    x = embeddings(n)
    n_epochs = ref.default_n_epochs(n)
    a, b = ref.umap_ab(p.spread, p.min_dist)
    idx, dist = gu.knn_table_gpu(x, p.n_neighbors)
    _, _, memb = gu.smooth_knn_gpu(idx, dist)
    graph = gu.graph_from_memberships(idx, memb, n_epochs)
    Y0 = gu.pca_init_gpu(x)
    state0 = gu.layout_state_gpu(graph[2])
    dmed, dmax = gu.degree_stats(graph[0])
    # an empty launch of the epoch kernel: 16 vertices without edges
    eg = (torch.zeros(17, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)[:0], None)
    est = {k: torch.zeros(1, device=dev)[:0] for k in ("eps", "epn", "next", "nneg")}
    eY = torch.zeros(16, 2, device=dev)
    xh = x.cpu().numpy()

    def fresh():
        return Y0.clone(), {k: v.clone() for k, v in state0.items()}

    arms = {
        "knn": (lambda: None, lambda _: gu.knn_table_gpu(x, p.n_neighbors), "event"),
        "smooth_knn": (lambda: None, lambda _: gu.smooth_knn_gpu(idx, dist), "event"),
        "graph": (lambda: None, lambda _: gu.graph_from_memberships(idx, memb, n_epochs), "event"),
        "pca_init": (lambda: None, lambda _: gu.pca_init_gpu(x), "event"),
        "layout": (fresh, lambda s: gu.layout_gpu(s[0], graph, s[1], n_epochs, a, b, p.seed), "event"),
        "empty_launches": (lambda: None, lambda _: gu.layout_gpu(eY, eg, est, n_epochs, a, b, p.seed), "event"),
        "umap_fit_gpu": (lambda: None, lambda _: gu.umap_fit_gpu(x, p), "wall"),
        "pca_path": (lambda: None, lambda _: projection.project_2d(xh, 42, "pca"), "wall"),
    }
    ms = alternate(arms, reps)
    Y, info = gu.umap_fit_gpu(x, p)
    res = {"n": n, "d": int(x.shape[1]), "n_epochs": n_epochs, "n_edges": info["n_edges"], "degree_median": dmed,
           "degree_max": dmax, **{f"{k}_ms": round(v, 4) for k, v in ms.items()},
           "epoch_us": round(1e3 * ms["layout"] / n_epochs, 3),
           "empty_launch_us": round(1e3 * ms["empty_launches"] / n_epochs, 3),
           "launch_share_of_layout": round(ms["empty_launches"] / ms["layout"], 3),
           "fit_spans_ms": info["spans_ms"], "finite": bool(torch.isfinite(Y).all()),
           "range": [round(float(Y.min()), 2), round(float(Y.max()), 2)]}
    if n <= 10_000:
        sub = np.sort(np.random.default_rng(0).choice(n, size=min(n, n_trust), replace=False))
        res.update(trust_points=int(sub.size), trust_umap=round(trust(xh[sub], Y.cpu().numpy()[sub]), 4),
                   trust_pca=round(trust(xh[sub], projection.project_2d(xh, 42, "pca")[0][sub]), 4))
    return res


def oracle(n: int) -> dict:
    x = embeddings(n)
    xh = x.cpu().numpy()
    t = time.perf_counter()
    Yo = ref.umap_fit(xh)
    oracle_s = time.perf_counter() - t
    gu.umap_fit_gpu(x)
    torch.cuda.synchronize()
    t = time.perf_counter()
    Yg, _ = gu.umap_fit_gpu(x)
    torch.cuda.synchronize()
    gpu_ms = (time.perf_counter() - t) * 1e3
    return {"oracle_n": n, "numpy_oracle_s": round(oracle_s, 2), "umap_fit_gpu_ms": round(gpu_ms, 2),
            "trust_oracle": round(trust(xh, Yo), 4), "trust_gpu": round(trust(xh, Yg.cpu().numpy()), 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trust", type=int, default=2000)
    ap.add_argument("--oracle-n", type=int, default=2000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("umap_bench needs a GPU")
    _native.hip()
    for n in args.n:
        print(json.dumps(bench(n, max(10, args.reps), args.trust)), flush=True)
    if args.oracle_n > 0:
        print(json.dumps(oracle(args.oracle_n)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
