#!/usr/bin/env python3
"""Cell-image-search latency and recall per index tier (reference README: <5 ms Flat, <100 ms
IVFPQ at 58 M vectors, ~95 % recall@10: ``apps/cell-image-search/README.md:130-137``).

Synthetic clustered, L2-normalised 768-d embeddings (random cluster centres + noise) live on the
GPU; for each N the bench builds

* the exact bf16 Flat tier (ground truth),
* the IVF exact-scan tier (list-sorted bf16 slabs in HBM, HIP scan kernel ``be_ivf_scan_bf16``),
  swept over nprobe,
* the IVF-PQ tier (m=96 x 8 bit, the reference's compressed layout) with and without an exact
  re-rank of the PQ shortlist,

and reports p50 / p95 latency of one query and of a 64-query batch (top-20), build time and two
recall figures against the exact ranking: ``recall@10`` = |approx top-10 ∩ exact top-10| / 10
(strict) and ``R@10`` = fraction of queries whose exact nearest neighbour is in the approx top-10
(the FAISS convention the reference's "~95 % recall@10" uses).  One JSON line per (N, tier, nprobe), and with the
pq96 tier one ``"stage": "pq_build"`` line: ``IVFPQIndex.add`` with ``build="torch"`` against ``build="fused"``, and
the coarse quantizer arms ``coarse="torch"`` against ``"fused"`` (``--pq-build-only`` prints this line alone).
With the pq96 and compressed tiers one ``"stage": "pq_search"`` line per (N, m, Q, k): ``IVFPQIndex.search`` with
``search="scan"`` against ``search="fused"`` (``--pq-search-only`` prints these lines alone).
With the ivf tier one ``"stage": "ivf_search"`` line per (N, Q, k): ``VectorIndex.search`` with ``ivf_search="scan"``
against ``ivf_search="fused"`` (``--ivf-search-only`` prints these lines alone).
``--sq8-only`` prints one ``"stage": "sq8"`` line per (N, Q, k): the IVF-Flat tier with ``ivf_search="fused"`` against
``index_type="ivfsq8"`` on the same centroids (:func:`sq8_times`).
``--flat-search-only`` prints one ``"stage": "flat_search"`` line per (N, Q, k): the flat tier's ``VectorIndex.search``
with ``flat_search="gemm"`` against ``flat_search="fused"`` (:func:`flat_search_times`); the full run prints them too.
``--flat-sq8-only`` prints one ``"stage": "flat_sq8"`` line per (N, Q, k): the flat tier with ``flat_search="fused"``
against ``index_type="flatsq8"`` over the same rows (:func:`flat_sq8_times`).
Usage: ``python tools/search_bench.py --n 10000000,58000000``
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def synth(n, d, dev, seed=0, chunk=1 << 22):
    """Hierarchical clusters like image embeddings: 4096 class centres (norm 1), 64 sub-centres per
    class (offset norm 0.5), per-vector noise (norm 0.2), L2-normalised."""
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(4096, d, device=dev, generator=g), dim=1)
    subs = torch.nn.functional.normalize(torch.randn(4096 * 64, d, device=dev, generator=g), dim=1) * 0.5
    out = torch.empty(n, d, dtype=torch.bfloat16, device=dev)
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        sub = torch.randint(0, 4096 * 64, (m,), device=dev, generator=g)
        v = centres[sub // 64] + subs[sub] + 0.2 * torch.randn(m, d, device=dev, generator=g) / d ** 0.5
        out[i:i + m] = torch.nn.functional.normalize(v, dim=1).bfloat16()
    return out


def ood_queries(nq, d, dev, seed=7):
    """Out-of-distribution queries: the database's class centres (same generator as ``synth``) with
    sub-centre offsets that were NEVER used for indexed vectors, plus noise -- the nearest neighbours
    are spread over the class instead of sitting next to the query, unlike indexed-vector + noise."""
    g = torch.Generator(device=dev).manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(4096, d, device=dev, generator=g), dim=1)
    gq = torch.Generator(device=dev).manual_seed(seed + 1000)
    cls = torch.randint(0, 4096, (nq,), device=dev, generator=gq)
    held_out = torch.nn.functional.normalize(torch.randn(nq, d, device=dev, generator=gq), dim=1) * 0.5
    v = centres[cls] + held_out + 0.2 * torch.randn(nq, d, device=dev, generator=gq) / d ** 0.5
    return torch.nn.functional.normalize(v, dim=1)


def timeit(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[int(0.95 * (len(ts) - 1))]


def recalls(gt, got):
    r10 = float(np.mean([len(set(g[:10]) & set(r[:10])) / 10 for g, r in zip(gt, got)]))
    r1 = float(np.mean([g[0] in set(r[:10]) for g, r in zip(gt, got)]))
    return round(r10, 4), round(r1, 4)


def pq_build_times(pq, x, reps=3):
    """``IVFPQIndex.add(x)`` on the torch path and on ``csrc/kernels/pq_build.hip``, with ``pq``'s trained
    centroids and codebooks: device-event times (ms) of the whole call, both arms warmed up once on all of
    ``x`` and then alternating; medians, the torch arm's spread, and the share of equal code bytes."""
    from bioengine_worker_amd.search.ivfpq import IVFPQIndex

    def arm(build):
        idx = IVFPQIndex(pq.dim, pq.nlist, pq.m, pq.nprobe, pq.device, build=build, coarse="torch")
        idx.centroids, idx.codebooks = pq.centroids, pq.codebooks
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        idx.add(x)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), idx

    ts = {"torch": [], "fused": []}
    raws = {}
    for r in range(reps + 1):
        for build in ts:
            t, idx = arm(build)
            if r:
                ts[build].append(t)
            raws[build] = idx._raw()
            del idx
    med = {b: sorted(v)[len(v) // 2] for b, v in ts.items()}
    # the encoding alone on one chunk of add (2^18 rows, coarse assignment given): be_pq_encode on the stored rows
    # against the residual + _pq_encode of the torch path
    from bioengine_worker_amd.search import ivfpq
    from bioengine_worker_amd.search.index import _argmax_ip

    xc = x[: 1 << 18]
    a = _argmax_ip(xc.float(), pq.centroids)
    enc = {"fused": lambda: ivfpq.pq_encode_fused(xc, pq.centroids, a, pq.codebooks),
           "torch": lambda: ivfpq._pq_encode(xc.float() - pq.centroids[a], pq.codebooks)}
    et = {}
    for b, fn in enc.items():
        fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for e in ev[1:]:
            fn()
            e.record()
        ev[-1].synchronize()
        et[b] = sorted(p.elapsed_time(q) for p, q in zip(ev, ev[1:]))[reps // 2]
    return {"n": int(x.shape[0]), "stage": "pq_build", "m": pq.m, "nlist": pq.nlist, "x_dtype": str(x.dtype),
            "encode_rows": int(xc.shape[0]), "encode_torch_ms": round(et["torch"], 3),
            "encode_fused_ms": round(et["fused"], 3),
            "add_torch_ms": round(med["torch"], 2), "add_fused_ms": round(med["fused"], 2),
            "torch_over_fused": round(med["torch"] / med["fused"], 2),
            "torch_spread_ms": round(max(ts["torch"]) - min(ts["torch"]), 2),
            "fused_spread_ms": round(max(ts["fused"]) - min(ts["fused"]), 2),
            "codes_equal": round(int((raws["torch"] == raws["fused"]).sum()) / raws["torch"].numel(), 6)}


def _alternate(fns, reps, pct=False):
    """Device-event times (ms) of the calls ``fns[name]()``: every arm once as a warm-up, then alternating ``reps``
    times -> per arm (median, max - min, the last call's result); ``pct``: the spread is the 90th minus the 10th
    percentile instead."""
    ts, res = {b: [] for b in fns}, {}
    for r in range(reps + 1):
        for b, fn in fns.items():
            res[b] = None  # the previous result of this arm is freed before the next call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            res[b] = fn()
            e1.record()
            e1.synchronize()
            if r:
                ts[b].append(e0.elapsed_time(e1))
    spread = (lambda v: np.percentile(v, 90) - np.percentile(v, 10)) if pct else (lambda v: max(v) - min(v))
    return {b: (sorted(v)[len(v) // 2], spread(v), res[b]) for b, v in ts.items()}


def pq_coarse_times(pq, x, train_rows, reps=3):
    """The coarse quantizer arms, ``coarse="torch"`` against ``"fused"`` (``csrc/kernels/coarse_assign.hip``), with
    ``build="fused"`` and ``pq``'s trained centroids and codebooks on both: ``IVFPQIndex.add(x)``, the assignment
    alone on one chunk of ``add`` (2^18 stored rows; useful flop ``2 n nlist D`` over the time, the fused arm with its
    fallback recomputation, and the kernels alone), ``IVFPQIndex.train`` on ``train_rows``; the fused arm's share of
    fallback rows and the rows whose list differs between the arms."""
    from bioengine_worker_amd.search import ivfpq
    from bioengine_worker_amd.search.index import _argmax_ip

    def new(coarse):
        return ivfpq.IVFPQIndex(pq.dim, pq.nlist, pq.m, pq.nprobe, pq.device, build="fused", coarse=coarse)

    def add(coarse):
        idx = new(coarse)
        idx.centroids, idx.codebooks = pq.centroids, pq.codebooks
        idx.add(x)
        return idx._assign, idx.coarse_fallback_rows

    def train(coarse):
        idx = new(coarse)
        idx.train(train_rows)
        return idx.coarse_fallback_rows

    arms = ("torch", "fused")
    ad = _alternate({b: (lambda b=b: add(b)) for b in arms}, reps)
    differ = int((ad["torch"][2][0] != ad["fused"][2][0]).sum())
    fallback = ad["fused"][2][1]
    xc = x[: 1 << 18]
    asg = _alternate({"torch": lambda: _argmax_ip(xc.float(), pq.centroids),
                      "fused": lambda: ivfpq.coarse_assign_fused(xc, pq.centroids)[0],
                      "kernels": lambda: ivfpq.coarse_top2_fused(xc, pq.centroids)[0]}, max(reps, 5))
    tr = _alternate({b: (lambda b=b: train(b)) for b in arms}, max(1, reps - 1))
    flop = 2.0 * xc.shape[0] * pq.nlist * pq.dim
    out = {"coarse_assign_rows": int(xc.shape[0]), "coarse_differing_rows": differ,
           "coarse_fallback_share": round(fallback / x.shape[0], 6), "coarse_train_rows": int(train_rows.shape[0]),
           "coarse_train_fallback_rows": int(tr["fused"][2])}
    for b in arms:
        out.update({f"add_coarse_{b}_ms": round(ad[b][0], 2), f"add_coarse_{b}_spread_ms": round(ad[b][1], 2),
                    f"train_coarse_{b}_ms": round(tr[b][0], 1), f"train_coarse_{b}_spread_ms": round(tr[b][1], 1)})
    for b in asg:
        out.update({f"assign_{b}_ms": round(asg[b][0], 3), f"assign_{b}_spread_ms": round(asg[b][1], 3),
                    f"assign_{b}_tflops": round(flop / asg[b][0] * 1e-9, 1)})
    return out


def pq_search_arms(pq):
    """``pq``'s trained, filled index behind ``search="scan"`` and ``search="fused"`` (shared tensors)."""
    from bioengine_worker_amd.search.ivfpq import IVFPQIndex

    arms = {}
    for mode in ("scan", "fused"):
        idx = IVFPQIndex(pq.dim, pq.nlist, pq.m, pq.nprobe, pq.device, search=mode)
        idx.centroids, idx.codebooks, idx.codes, idx.ids, idx.list_off = (pq.centroids, pq.codebooks, pq.codes, pq.ids,
                                                                          pq.list_off)
        idx.ntotal = pq.ntotal
        arms[mode] = idx
    return arms


def search_times(arms, stage, fields, q, gt, qs=(1, 64), ks=(20, 80, 1000), reps=20):
    """``search`` of the ``"scan"`` arm against the ``"fused"`` arm: the host clock around the whole call (it ends in the
    copy of the results, which synchronises), both arms warmed twice on every shape, then alternating; per arm the
    median and the spread (90th minus 10th percentile) of ``reps`` calls, the share of queries whose score lists are
    bit-equal, and both arms' recall against ``gt``.  One dict per (Q, k), opening with the index's ``fields``."""
    out = []
    for Q in qs:
        for k in ks:
            qq = q[:Q]
            ts = {a: [] for a in arms}
            res = {}
            for r in range(reps + 2):
                for a, idx in arms.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    res[a] = idx.search(qq, k)
                    if r >= 2:
                        ts[a].append((time.perf_counter() - t) * 1e3)
            st = {a: (np.median(v), np.percentile(v, 90) - np.percentile(v, 10)) for a, v in ts.items()}
            same = (res["scan"][0].view(np.uint32) == res["fused"][0].view(np.uint32)).all(1)
            rec = {a: recalls(gt[:Q], res[a][1]) for a in arms}
            out.append({**fields, "stage": stage, "Q": Q, "k": k,
                        "scan_ms": round(st["scan"][0], 3), "fused_ms": round(st["fused"][0], 3),
                        "scan_spread_ms": round(st["scan"][1], 3), "fused_spread_ms": round(st["fused"][1], 3),
                        "scan_over_fused": round(st["scan"][0] / st["fused"][0], 2),
                        "score_lists_equal": round(float(same.mean()), 4),
                        "recall@10": {a: rec[a][0] for a in arms}, "R@10": {a: rec[a][1] for a in arms}})
    return out


def pq_search_times(pq, q, gt, **kw):
    """:func:`search_times` of ``IVFPQIndex.search`` with ``search="scan"`` against ``search="fused"`` on ``pq``'s index."""
    fields = {"n": pq.ntotal, "m": pq.m, "nlist": pq.nlist, "nprobe": pq.nprobe}
    return search_times(pq_search_arms(pq), "pq_search", fields, q, gt, **kw)


def ivf_search_arms(ivf):
    """``ivf``'s trained IVF-Flat index behind ``ivf_search="scan"`` and ``ivf_search="fused"`` (shared tensors)."""
    from bioengine_worker_amd.search.index import VectorIndex

    arms = {}
    for mode in ("scan", "fused"):
        idx = VectorIndex(dim=ivf.dim, device=ivf.device, index_type="ivf", nprobe=ivf.nprobe, ivf_search=mode)
        idx.vecs, idx.centroids, idx.assign = ivf.vecs, ivf.centroids, ivf.assign
        idx.sorted_ids, idx.list_off, idx.lvecs = ivf.sorted_ids, ivf.list_off, ivf.lvecs
        arms[mode] = idx
    return arms


def ivf_search_times(ivf, q, gt, **kw):
    """:func:`search_times` of ``VectorIndex.search`` with ``ivf_search="scan"`` against ``"fused"`` on ``ivf``'s index."""
    fields = {"n": ivf.ntotal, "dim": ivf.dim, "nlist": int(ivf.centroids.shape[0]), "nprobe": ivf.nprobe}
    return search_times(ivf_search_arms(ivf), "ivf_search", fields, q, gt, **kw)


def sq8_times(ivf, q, qs=(1, 64), ks=(20, 80), reps=20):
    """``ivf``'s trained IVF-Flat index behind ``ivf_search="fused"`` against the same centroids and lists behind
    ``index_type="ivfsq8"`` (``csrc/kernels/ivf_sq8.hip``), all through :func:`_alternate`: the encode, then per (Q, k)
    the whole ``search`` call of the bf16 arm and of the SQ8 arm with ``refine`` 0 and 4, the fused scan + merge alone
    on the same probes (``kk = k``), the candidate rows and the bytes they stream, and the SQ8 arms' recall@k against
    the bf16 arm's ids.  One ``"stage": "sq8"`` dict per (Q, k), opening with the tiers' device bytes."""
    from bioengine_worker_amd.search.index import VectorIndex, ivf_scan_topk_fused
    from bioengine_worker_amd.search.list_scan import candidate_offsets
    from bioengine_worker_amd.search.sq8 import ivf_sq8_scan_topk_fused, sq8_encode

    arms = {"ivf": VectorIndex(dim=ivf.dim, device=ivf.device, index_type="ivf", nprobe=ivf.nprobe, ivf_search="fused"),
            "sq8_r0": VectorIndex(dim=ivf.dim, device=ivf.device, index_type="ivfsq8", nprobe=ivf.nprobe, refine=0),
            "sq8_r4": VectorIndex(dim=ivf.dim, device=ivf.device, index_type="ivfsq8", nprobe=ivf.nprobe, refine=4)}
    enc = _alternate({"encode": lambda: sq8_encode(ivf.vecs, ivf.sorted_ids)}, 3)["encode"]
    for name, idx in arms.items():
        idx.vecs, idx.centroids, idx.assign = ivf.vecs, ivf.centroids, ivf.assign
        idx.sorted_ids, idx.list_off = ivf.sorted_ids, ivf.list_off
        if name == "ivf":
            idx.lvecs = ivf.lvecs
        else:
            idx.sq_codes, idx.sq_scales = enc[2]
    nbytes = lambda *ts: int(sum(t.numel() * t.element_size() for t in ts))  # noqa: E731
    fields = {"n": ivf.ntotal, "dim": ivf.dim, "nlist": int(ivf.centroids.shape[0]), "nprobe": ivf.nprobe, "stage": "sq8",
              "ivf_bytes": nbytes(ivf.vecs, ivf.lvecs), "sq8_bytes": nbytes(ivf.vecs, *enc[2]),
              "encode_ms": round(enc[0], 2), "encode_spread_ms": round(enc[1], 2)}
    out = []
    for Q in qs:
        qq = q[:Q].to(ivf.dtype)
        probes = torch.topk((qq @ ivf.centroids.T).float(), ivf.nprobe, dim=1).indices
        rows = int(candidate_offsets(ivf.list_off, probes)[0].sum())
        for k in ks:
            ts = _alternate({a: (lambda idx=idx: idx.search(qq, k)) for a, idx in arms.items()}, reps)
            sc = _alternate({"ivf": lambda: ivf_scan_topk_fused(qq.float(), probes, ivf.list_off, ivf.lvecs,
                                                                 ivf.sorted_ids, k),
                             "sq8": lambda: ivf_sq8_scan_topk_fused(qq.float(), probes, ivf.list_off, *enc[2],
                                                                     ivf.sorted_ids, k)}, reps)
            line = {**fields, "Q": Q, "k": k, "candidate_rows": rows, "ivf_scan_bytes": rows * ivf.dim * 2,
                    "sq8_scan_bytes": rows * (ivf.dim + 4)}
            for a in arms:
                line.update({f"{a}_ms": round(ts[a][0], 3), f"{a}_spread_ms": round(ts[a][1], 3)})
            for a in sc:
                line.update({f"scan_{a}_ms": round(sc[a][0], 4), f"scan_{a}_spread_ms": round(sc[a][1], 4)})
            line["scan_ivf_over_sq8"] = round(sc["ivf"][0] / sc["sq8"][0], 2)
            gt = ts["ivf"][2][1]
            for a in ("sq8_r0", "sq8_r4"):
                line[f"recall@{k}_{a}"] = round(float(np.mean([len(set(g) & set(r)) / k for g, r in zip(gt, ts[a][2][1])])), 4)
            out.append(line)
    return out


def flat_search_times(x, q, qs=(1, 64), ks=(20, 100), reps=20, hbm_tbps=8.0):
    """The flat tier over the bf16 rows ``x`` behind ``flat_search="gemm"`` (the chunked GEMM + ``topk`` loop) and
    ``flat_search="fused"`` (``csrc/kernels/flat_scan_topk.hip``), shared tensors, all through :func:`_alternate`: per
    (Q, k) the whole ``search`` call of both arms (median, spread = 90th - 10th percentile), their ratio, the fused scan
    + merge alone, the bytes of rows it streams (once per query group) over that time as a share of ``hbm_tbps``, and
    the share of queries whose id sets agree.  One ``"stage": "flat_search"`` dict per (Q, k)."""
    from bioengine_worker_amd.search.flat import flat_group, flat_scan_topk_fused
    from bioengine_worker_amd.search.index import VectorIndex

    arms = {}
    for mode in ("gemm", "fused"):
        arms[mode] = VectorIndex(dim=x.shape[1], device=x.device, index_type="flat", flat_search=mode)
        arms[mode].vecs = x
    out = []
    for Q in qs:
        qq = q[:Q].to(x.dtype)
        for k in ks:
            ts = _alternate({a: (lambda idx=idx: idx.search(qq, k)) for a, idx in arms.items()}, reps, pct=True)
            sc = _alternate({"scan": lambda: flat_scan_topk_fused(qq, x, k)}, reps, pct=True)["scan"]
            group = flat_group(Q, x.shape[1], k)
            nbytes = -(-Q // group) * x.numel() * 2
            same = [set(a) == set(b) for a, b in zip(ts["gemm"][2][1], ts["fused"][2][1])]
            out.append({"n": int(x.shape[0]), "dim": int(x.shape[1]), "stage": "flat_search", "Q": Q, "k": k,
                        "gemm_ms": round(ts["gemm"][0], 3), "fused_ms": round(ts["fused"][0], 3),
                        "gemm_spread_ms": round(ts["gemm"][1], 3), "fused_spread_ms": round(ts["fused"][1], 3),
                        "gemm_over_fused": round(ts["gemm"][0] / ts["fused"][0], 2), "query_group": group,
                        "fused_scan_ms": round(sc[0], 3), "fused_scan_spread_ms": round(sc[1], 3),
                        "rows_bytes": nbytes, "scan_tbps": round(nbytes / sc[0] * 1e-9, 2),
                        "share_of_hbm_peak": round(nbytes / sc[0] * 1e-9 / hbm_tbps, 3),
                        "id_sets_equal": round(float(np.mean(same)), 4)})
    return out


def flat_sq8_times(x, q, qs=(1, 16, 32, 64), ks=(20, 100), reps=20, hbm_tbps=8.0):
    """The flat tier over the bf16 rows ``x`` behind ``flat_search="fused"`` against ``index_type="flatsq8"`` with
    ``refine`` 0 and 4 over the same rows (``csrc/kernels/flat_sq8_scan_topk.hip``), all through :func:`_alternate`
    (median, spread = 90th - 10th percentile): the encode, then per (Q, k) the whole ``search`` call of the three arms,
    the two scans alone (kernel + merge, ``kk = k``), alternating with each other, the bytes each streams (once per
    query group; ``N (D + 4)`` for SQ8) over that time as a share of ``hbm_tbps``, the ratio of the row rates, and the
    SQ8 arms' recall@k against the bf16 arm's ids.  One ``"stage": "flat_sq8"`` dict per (Q, k)."""
    from bioengine_worker_amd.search.flat import (flat_group, flat_scan_topk_fused, flat_sq8_group,
                                                  flat_sq8_scan_topk_fused)
    from bioengine_worker_amd.search.index import VectorIndex
    from bioengine_worker_amd.search.sq8 import sq8_encode

    n, d = int(x.shape[0]), int(x.shape[1])
    enc = _alternate({"encode": lambda: sq8_encode(x, None)}, 3)["encode"]
    codes, scales = enc[2]
    arms = {"bf16": VectorIndex(dim=d, device=x.device, index_type="flat", flat_search="fused"),
            "sq8_r0": VectorIndex(dim=d, device=x.device, index_type="flatsq8", refine=0),
            "sq8_r4": VectorIndex(dim=d, device=x.device, index_type="flatsq8", refine=4)}
    for name, idx in arms.items():
        idx.vecs = x
        if name != "bf16":
            idx.sq_codes, idx.sq_scales = codes, scales
    out = []
    for Q in qs:
        qq = q[:Q].to(x.dtype)
        qf = qq.float()
        for k in ks:
            ts = _alternate({a: (lambda idx=idx: idx.search(qq, k)) for a, idx in arms.items()}, reps, pct=True)
            sc = _alternate({"bf16": lambda: flat_scan_topk_fused(qq, x, k),
                             "sq8": lambda: flat_sq8_scan_topk_fused(qf, codes, scales, k)}, reps, pct=True)
            groups = {"bf16": -(-Q // flat_group(Q, d, k)), "sq8": -(-Q // flat_sq8_group(Q, d, k))}
            nbytes = {"bf16": groups["bf16"] * n * d * 2, "sq8": groups["sq8"] * n * (d + 4)}
            line = {"n": n, "dim": d, "stage": "flat_sq8", "Q": Q, "k": k, "encode_ms": round(enc[0], 3),
                    "encode_spread_ms": round(enc[1], 3)}
            for a in arms:
                line.update({f"{a}_ms": round(ts[a][0], 3), f"{a}_spread_ms": round(ts[a][1], 3)})
            for a in sc:
                line.update({f"scan_{a}_ms": round(sc[a][0], 3), f"scan_{a}_spread_ms": round(sc[a][1], 3),
                             f"scan_{a}_groups": groups[a], f"scan_{a}_bytes": nbytes[a],
                             f"scan_{a}_tbps": round(nbytes[a] / sc[a][0] * 1e-9, 2),
                             f"scan_{a}_share_of_hbm_peak": round(nbytes[a] / sc[a][0] * 1e-9 / hbm_tbps, 3)})
            line["scan_bf16_over_sq8"] = round(sc["bf16"][0] / sc["sq8"][0], 2)
            gt = ts["bf16"][2][1]
            for a in ("sq8_r0", "sq8_r4"):
                line[f"recall@{k}_{a}"] = round(float(np.mean([len(set(g) & set(r)) / k for g, r in zip(gt, ts[a][2][1])])), 4)
            out.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000000,10000000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nprobes", default="16,32,64,128,256")
    ap.add_argument("--no-pq", action="store_true")
    ap.add_argument("--tiers", default="ivf,pq96,compressed",
                    help="ivf: exact-scan IVF; pq96: IVF-PQ m=96 (+ GPU re-rank); compressed: IVF-PQ m=192 on "
                         "the GPU with the full vectors in host memory as the re-rank store (VectorIndex.compress)")
    ap.add_argument("--refines", default="400,1000,2000", help="compressed tier: re-ranked candidates per query")
    ap.add_argument("--queries", default="near,ood", help="near: indexed vectors + small noise; "
                    "ood: held-out sub-centres of the indexed classes (ood_queries)")
    ap.add_argument("--pq-search-only", action="store_true", help="only the pq_search lines (scan against fused search)")
    ap.add_argument("--pq-ms", default="96,192", help="--pq-search-only: the PQ sizes")
    ap.add_argument("--ivf-search-only", action="store_true", help="only the ivf_search lines (scan against fused search)")
    ap.add_argument("--sq8-only", action="store_true", help="only the sq8 lines (fused IVF-Flat against IVF-SQ8)")
    ap.add_argument("--pq-build-only", action="store_true", help="only the pq_build line (build and coarse arms)")
    ap.add_argument("--flat-search-only", action="store_true", help="only the flat_search lines (gemm against fused)")
    ap.add_argument("--flat-sq8-only", action="store_true", help="only the flat_sq8 lines (fused bf16 flat against flatsq8)")
    ap.add_argument("--flat-ks", default="20,100", help="the flat_search and flat_sq8 lines' k values")
    a = ap.parse_args()
    from bioengine_worker_amd.search.index import VectorIndex
    from bioengine_worker_amd.search.ivfpq import IVFPQIndex, default_nlist

    dev = torch.device("cuda", 0)
    for n in [int(v) for v in a.n.split(",")]:
        x = synth(n, a.dim, dev)
        if a.pq_build_only:
            pq = IVFPQIndex(dim=a.dim, nlist=default_nlist(n), m=96, nprobe=64, device=dev)
            train_rows = x.float() if n <= 2_000_000 else x[torch.randperm(n, device=dev)[:2_000_000]].float()
            pq.train(train_rows)
            print(json.dumps({**pq_build_times(pq, x), **pq_coarse_times(pq, x, train_rows)}), flush=True)
            del x, pq, train_rows
            torch.cuda.empty_cache()
            continue
        gq = torch.Generator(device=dev).manual_seed(7)
        qidx = torch.randint(0, n, (64,), device=dev, generator=gq)
        qsets = {"near": torch.nn.functional.normalize(
            x[qidx].float() + 0.02 * torch.randn(64, a.dim, device=dev, generator=gq), dim=1),
            "ood": ood_queries(64, a.dim, dev)}
        qsets = {k: v for k, v in qsets.items() if k in a.queries.split(",")}
        if a.flat_search_only:  # the flat_search lines alone; the two arms are compared with each other
            for line in flat_search_times(x, next(iter(qsets.values())), ks=[int(v) for v in a.flat_ks.split(",")],
                                          reps=a.reps):
                print(json.dumps(line), flush=True)
            del x
            torch.cuda.empty_cache()
            continue
        if a.flat_sq8_only:  # the flat_sq8 lines alone; the reference is the fused bf16 arm
            for line in flat_sq8_times(x, next(iter(qsets.values())), ks=[int(v) for v in a.flat_ks.split(",")],
                                       reps=a.reps):
                print(json.dumps(line), flush=True)
            del x
            torch.cuda.empty_cache()
            continue
        if a.sq8_only:  # the sq8 lines alone; the reference is the IVF-Flat arm, no exact ground truth is needed
            ivf = VectorIndex(dim=a.dim, device=dev, index_type="ivf", ivf_search="fused")
            ivf.vecs = x
            ivf.train_ivf()
            for line in sq8_times(ivf, next(iter(qsets.values())), reps=a.reps):
                print(json.dumps(line), flush=True)
            del ivf, x
            torch.cuda.empty_cache()
            continue
        flat = VectorIndex(dim=a.dim, device=dev, index_type="flat")
        flat.vecs = x
        # ground truth in fp32 (fp32 query x bf16 vectors upcast per chunk): exact up to fp32 rounding
        gts = {}
        for qn, qv in qsets.items():
            gs, gi = [], []
            for i in range(0, n, 1 << 20):
                sc = qv @ x[i:i + (1 << 20)].float().T
                ts, ti = torch.topk(sc, a.k, dim=1)
                gs.append(ts)
                gi.append(ti + i)
            ts, j = torch.topk(torch.cat(gs, 1), a.k, dim=1)
            gts[qn] = torch.gather(torch.cat(gi, 1), 1, j).cpu().numpy()
        q = next(iter(qsets.values()))
        if a.ivf_search_only:  # the ivf_search lines alone
            ivf = VectorIndex(dim=a.dim, device=dev, index_type="ivf")
            ivf.vecs = x
            ivf.train_ivf()
            for line in ivf_search_times(ivf, q, next(iter(gts.values())), reps=a.reps):
                print(json.dumps(line), flush=True)
            del ivf, x, flat
            torch.cuda.empty_cache()
            continue
        if a.pq_search_only:  # the pq_search lines alone: the m = 96 index and the compressed tier's m = 192
            for m in [int(v) for v in a.pq_ms.split(",")]:
                pq = IVFPQIndex(dim=a.dim, nlist=default_nlist(n), m=m, nprobe=64, device=dev)
                pq.train(x.float() if n <= 2_000_000 else x[torch.randperm(n, device=dev)[:2_000_000]].float())
                for i in range(0, n, 1 << 22):
                    pq.add(x[i:i + (1 << 22)])
                for line in pq_search_times(pq, q, next(iter(gts.values())), reps=a.reps):
                    print(json.dumps(line), flush=True)
                del pq
                torch.cuda.empty_cache()
            continue
        for name, fn in (("flat_q1", lambda: flat.search(q[:1], a.k)), ("flat_q64", lambda: flat.search(q, a.k))):
            fn()
            p50, p95 = timeit(fn, a.reps)
            print(json.dumps({"n": n, "tier": "FlatIP-GPU bf16", "query": name, "p50_ms": round(p50, 3),
                              "p95_ms": round(p95, 3), "recall@10": 1.0, "R@10": 1.0}), flush=True)
        for line in flat_search_times(x, q, ks=[int(v) for v in a.flat_ks.split(",")], reps=a.reps):
            print(json.dumps(line), flush=True)
        tiers = a.tiers.split(",")
        # ---- IVF exact scan over list-sorted HBM slabs
        t0 = time.perf_counter()
        ivf = VectorIndex(dim=a.dim, device=dev, index_type="ivf")
        ivf.vecs = x
        if "ivf" in tiers:
            ivf.train_ivf()
        nprobes = [int(v) for v in a.nprobes.split(",")] if "ivf" in tiers else []
        torch.cuda.synchronize()
        build = time.perf_counter() - t0
        nl = ivf.centroids.shape[0] if ivf.centroids is not None else 0
        for npb in nprobes:
            rec = {qn: recalls(gts[qn], ivf.search(qv, a.k, nprobe=npb)[1]) for qn, qv in qsets.items()}
            r10, r1 = next(iter(rec.values()))
            for name, qq in (("q1", q[:1]), ("q64", q)):
                ivf.search(qq, a.k, nprobe=npb)
                p50, p95 = timeit(lambda: ivf.search(qq, a.k, nprobe=npb), a.reps)
                print(json.dumps({"n": n, "tier": "IVF-exact-scan bf16 (HBM)", "nprobe": npb, "nlist": nl, "query": name,
                                  "p50_ms": round(p50, 3), "p95_ms": round(p95, 3), "recall@10": r10, "R@10": r1,
                                  "recall@10_by_queries": {k: v[0] for k, v in rec.items()},
                                  "R@10_by_queries": {k: v[1] for k, v in rec.items()},
                                  "build_s": round(build, 2), "hbm_gb": round(2 * x.numel() * 2 / 1e9, 2)}), flush=True)
        if "ivf" in tiers:
            for line in ivf_search_times(ivf, q, next(iter(gts.values())), reps=a.reps):
                print(json.dumps(line), flush=True)
        del ivf
        torch.cuda.empty_cache()
        if a.no_pq:
            del x, flat
            torch.cuda.empty_cache()
            continue
        if "compressed" in tiers:
            # ---- compressed tier: m=192 PQ codes on the GPU, full vectors in host memory (re-rank store)
            print(json.dumps({"n": n, "stage": "compressed tier build (IVF-PQ m=192 + host copy)"}), flush=True)
            t0 = time.perf_counter()
            cvi = VectorIndex(dim=a.dim, device=dev, index_type="ivfpq")
            cvi.vecs = x
            fp = cvi.compress(pq_m=192, refine=50)
            torch.cuda.synchronize()
            build = time.perf_counter() - t0
            for line in pq_search_times(cvi.pq, q, next(iter(gts.values())), reps=a.reps):
                print(json.dumps(line), flush=True)
            for R in [int(v) for v in a.refines.split(",")]:
                cvi.refine = max(1, R // a.k)
                rec = {qn: recalls(gts[qn], cvi.search(qv, a.k)[1]) for qn, qv in qsets.items()}
                r10, r1 = next(iter(rec.values()))
                for name, qq in (("q1", q[:1]), ("q64", q)):
                    cvi.search(qq, a.k)
                    p50, p95 = timeit(lambda: cvi.search(qq, a.k), max(3, a.reps // 2))
                    print(json.dumps({"n": n, "tier": f"IVFPQ m=192 GPU + host re-rank {cvi.refine * a.k}",
                                      "query": name, "p50_ms": round(p50, 3), "p95_ms": round(p95, 3),
                                      "recall@10": r10, "R@10": r1,
                                      "recall@10_by_queries": {k: v[0] for k, v in rec.items()},
                                      "R@10_by_queries": {k: v[1] for k, v in rec.items()},
                                      "nlist": cvi.pq.nlist, "nprobe": cvi.pq.nprobe, "build_s": round(build, 2),
                                      "gpu_index_gb": round(fp["gpu_bytes"] / 1e9, 3),
                                      "host_refine_gb": round(fp["host_bytes"] / 1e9, 3)}), flush=True)
            del cvi
            torch.cuda.empty_cache()
        if "pq96" not in tiers:
            del x, flat
            torch.cuda.empty_cache()
            continue
        # ---- IVF-PQ (the reference's compressed layout), PQ-only and with exact re-rank
        t0 = time.perf_counter()
        npl = default_nlist(n)
        pq = IVFPQIndex(dim=a.dim, nlist=npl, m=96, nprobe=64, device=dev)
        train_rows = x.float() if n <= 2_000_000 else x[torch.randperm(n, device=dev)[:2_000_000]].float()
        pq.train(train_rows)
        pq.add(x)
        torch.cuda.synchronize()
        build = time.perf_counter() - t0
        print(json.dumps({**pq_build_times(pq, x), **pq_coarse_times(pq, x, train_rows)}), flush=True)
        del train_rows
        for line in pq_search_times(pq, q, next(iter(gts.values())), reps=a.reps):
            print(json.dumps(line), flush=True)
        for refine, tier in ((0, "IVFPQ-GPU m=96 nprobe=64"), (4, "IVFPQ-GPU + exact rerank 80"),
                             (200, "IVFPQ-GPU + exact rerank 4k")):
            vi = VectorIndex(dim=a.dim, device=dev, index_type="ivfpq", refine=refine)
            vi.vecs, vi.pq = x, pq
            rec = {qn: recalls(gts[qn], vi.search(qv, a.k)[1]) for qn, qv in qsets.items()}
            r10, r1 = next(iter(rec.values()))
            for name, qq in (("q1", q[:1]), ("q64", q)):
                vi.search(qq, a.k)
                p50, p95 = timeit(lambda: vi.search(qq, a.k), a.reps)
                print(json.dumps({"n": n, "tier": tier, "query": name, "p50_ms": round(p50, 3), "p95_ms": round(p95, 3),
                                  "recall@10": r10, "R@10": r1, "recall@10_by_queries": {k: v[0] for k, v in rec.items()},
                                  "R@10_by_queries": {k: v[1] for k, v in rec.items()},
                                  "nlist": pq.nlist, "build_s": round(build, 2),
                                  "codes_gb": round(pq.codes.numel() / 1e9, 3)}), flush=True)
        del x, flat, pq, vi
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
