"""In-house UMAP for the landscape view, on the GPU (``csrc/kernels/umap.hip``).

The rules are ``search/reference.py``'s numpy oracle (written from memory of umap-learn 0.5, never
compared with it; its departures are listed there).  Stages:

* :func:`knn_table_gpu` — plumbing in torch: fp32 row normalisation, chunked ``torch.mm`` score blocks
  (never ``n x n``), ``topk``.
* :func:`smooth_knn_gpu` — ``be_umap_smooth_knn``: rho, sigma and the directed memberships.
* :func:`graph_from_memberships` — reciprocal lookup, fuzzy union, one ``torch.sort`` on an int64
  ``(row, col)`` key, dedupe, pruning, ``row_ptr``.  No atomics decide the order: two runs give identical
  arrays.  One host read (the edge count).
* :func:`layout_gpu` — ``be_umap_layout``: all epochs queued back to back, one launch per epoch, positions
  ping-ponging between two buffers; no host read, no allocation and no synchronisation in between.

New points onto a fitted layout (:func:`umap_transform_gpu`; the rules are ``reference.umap_transform``'s, every
one of them per query):

* :func:`knn_query_table_gpu` — torch: score blocks of query rows against the training set, ``topk``.
* :func:`smooth_knn_query_gpu` — ``be_umap_smooth_knn_query``: rho (the row minimum), sigma and the ``k``
  memberships, which are the edge weights.
* :func:`transform_init_gpu` — torch: the weighted mean of the neighbours' training positions.
* :func:`transform_layout_gpu` — ``be_umap_transform``: all epochs in ONE launch; a query's position and
  schedule stay in the registers of its 16 lanes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from ..ops import _native
from ..profiling import trace
from . import reference as ref


@dataclass(frozen=True)
class UMAPParams:
    n_neighbors: int = 15
    min_dist: float = 0.1
    spread: float = 1.0
    metric: str = "cosine"
    n_epochs: int | None = None
    negative_sample_rate: int = 5
    learning_rate: float = 1.0
    repulsion_strength: float = 1.0
    seed: int = 42
    init: Any = "pca"
    transform_epochs: int | None = None  # of umap_transform_gpu; None: 100, whatever the number of queries


def _seed32(seed: int) -> int:
    s = int(seed) & 0xFFFFFFFF
    return s - (1 << 32) if s >= 1 << 31 else s


def knn_table_gpu(x: torch.Tensor, k: int, metric: str = "cosine", budget: int = 1 << 30):
    """``x [n, d]`` -> ``idx [n, k]`` int32, ``dist [n, k]`` float32 as ``reference.knn_table``: column 0 is
    the point itself at distance 0, then the ``k - 1`` nearest other points, ascending.  Score blocks of
    ``budget // n`` rows keep the temporary bounded (n = 100 000: 10 737 rows per block)."""
    if metric not in ref.UMAP_METRICS:
        raise ValueError(f"metric must be one of {ref.UMAP_METRICS}")
    x = x.float()
    n = x.shape[0]
    if not n > k:
        raise ValueError(f"need more points ({n}) than n_neighbors ({k})")
    if metric == "cosine":
        x = x / x.norm(dim=1, keepdim=True)
    else:
        sq = (x * x).sum(1)
    rows = max(1, min(n, budget // n))
    idx = torch.empty(n, k, dtype=torch.int32, device=x.device)
    dist = torch.empty(n, k, dtype=torch.float32, device=x.device)
    for i in range(0, n, rows):
        s = torch.mm(x[i:i + rows], x.T)
        if metric == "cosine":
            d = (1.0 - s).clamp_(min=0.0)
        else:
            d = (sq[i:i + rows, None] + sq[None, :] - 2.0 * s).clamp_(min=0.0).sqrt_()
        r = torch.arange(d.shape[0], device=x.device)
        d[r, r + i] = -1.0  # the point itself sorts first, whatever duplicates it has
        td, ti = torch.topk(d, k, dim=1, largest=False, sorted=True)
        td[:, 0] = 0.0
        idx[i:i + rows] = ti.int()
        dist[i:i + rows] = td
    return idx, dist


def smooth_knn_gpu(idx: torch.Tensor, dist: torch.Tensor):
    """-> ``rho [n]``, ``sigma [n]``, memberships ``[n, k-1]`` (float32).  The global mean the floor needs is
    computed on the device; nothing is read back."""
    n, k = dist.shape
    if not 2 <= k <= 64:
        raise ValueError("n_neighbors must be in 2..64")
    if not dist.is_cuda:
        raise _native.NativeUnavailable("be_umap_smooth_knn needs a GPU tensor")
    dist = dist.float().contiguous()
    idx = idx.int().contiguous()
    gmean = dist.double().mean().reshape(1)
    rho = torch.empty(n, dtype=torch.float32, device=dist.device)
    sigma = torch.empty_like(rho)
    memb = torch.empty(n, k - 1, dtype=torch.float32, device=dist.device)
    _native.call("be_umap_smooth_knn", _native.ptr(dist), _native.ptr(idx), n, k, _native.ptr(gmean), _native.ptr(rho),
                 _native.ptr(sigma), _native.ptr(memb), _native.stream(dist.device))
    return rho, sigma, memb


def graph_from_memberships(idx: torch.Tensor, memb: torch.Tensor, n_epochs: int, budget: int = 1 << 26):
    """Directed memberships -> the symmetric CSR of ``reference.fuzzy_graph`` ``(row_ptr int64 [n+1], col int32,
    w float32)``.  The reciprocal of ``(i -> j)`` is found by scanning row ``j`` of the table; the union of both
    directions is keyed ``row * n + col``, sorted, deduplicated (both copies of a pair carry the same bits) and
    pruned.  Pure torch: runs on any device."""
    n, k = idx.shape
    km = k - 1
    dev = idx.device
    nb = idx[:, 1:].long()
    rows = torch.arange(n, device=dev).repeat_interleave(km)
    cols = nb.reshape(-1)
    a = memb.float().reshape(-1)
    rec = torch.empty_like(a)
    step = max(1, budget // km)
    for i in range(0, rows.numel(), step):  # [step, k-1] blocks of row j's neighbours
        c = cols[i:i + step]
        hit = nb[c] == rows[i:i + step, None]
        pos = hit.int().argmax(1)
        rec[i:i + step] = torch.where(hit.any(1), memb[c, pos].float(), torch.zeros((), device=dev))
    # fmaf(-a, b, a + b) as the oracle evaluates it: exact product, one rounding to fp64, one to fp32
    w = ((a + rec).double() - a.double() * rec.double()).float()
    ok = rows != cols
    key = torch.cat([(rows * n + cols)[ok], (cols * n + rows)[ok]])
    w2 = torch.cat([w[ok], w[ok]])
    key, order = torch.sort(key)
    w2 = w2[order]
    keep = torch.ones_like(key, dtype=torch.bool)
    keep[1:] = key[1:] != key[:-1]
    keep &= w2 >= w2.max() / torch.tensor(float(n_epochs), dtype=torch.float32, device=dev)
    key, w2 = key[keep], w2[keep]  # the one host read: the edge count
    counts = torch.bincount(torch.div(key, n, rounding_mode="floor"), minlength=n)
    row_ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).long()
    return row_ptr.contiguous(), (key % n).int().contiguous(), w2.contiguous()


def fuzzy_graph_gpu(idx: torch.Tensor, dist: torch.Tensor, n_epochs: int | None = None):
    if n_epochs is None:
        n_epochs = ref.default_n_epochs(idx.shape[0])
    _, _, memb = smooth_knn_gpu(idx, dist)
    return graph_from_memberships(idx, memb, n_epochs)


def layout_state_gpu(w: torch.Tensor, negative_sample_rate: int = 5) -> dict:
    eps = w.max() / w
    epn = eps / float(negative_sample_rate)
    return {"eps": eps.contiguous(), "epn": epn.contiguous(), "next": eps.clone(), "nneg": epn.clone()}


def _check_layout(Y: torch.Tensor, graph, state: dict) -> None:
    row_ptr, col, _ = graph
    n, nnz = Y.shape[0], col.numel()
    if not Y.is_cuda:
        raise _native.NativeUnavailable("the UMAP layout kernel needs GPU tensors")
    assert Y.dtype == torch.float32 and Y.shape == (n, 2) and Y.is_contiguous()
    assert row_ptr.dtype == torch.int64 and row_ptr.numel() == n + 1 and col.dtype == torch.int32
    for s in ("eps", "epn", "next", "nneg"):
        assert state[s].dtype == torch.float32 and state[s].numel() == nnz and state[s].is_contiguous()


def layout_epoch_gpu(Yin: torch.Tensor, Yout: torch.Tensor, graph, state: dict, ep: int, n_epochs: int, a: float,
                     b: float, seed: int, gamma: float = 1.0, lr: float = 1.0) -> None:
    """ONE epoch: reads ``Yin``, writes ``Yout`` (another buffer), updates ``state['next' / 'nneg']`` in place."""
    _check_layout(Yin, graph, state)
    _check_layout(Yout, graph, state)
    row_ptr, col, _ = graph
    _native.call("be_umap_epoch", _native.ptr(Yin), _native.ptr(Yout), Yin.shape[0], _native.ptr(row_ptr), _native.ptr(col),
                 col.numel(), _native.ptr(state["eps"]), _native.ptr(state["epn"]), _native.ptr(state["next"]),
                 _native.ptr(state["nneg"]), ep, float(ref.epoch_alpha(ep, n_epochs, lr)), a, b, gamma, _seed32(seed),
                 _native.stream(Yin.device))


def layout_gpu(Y0: torch.Tensor, graph, state: dict, n_epochs: int, a: float, b: float, seed: int = 42,
               gamma: float = 1.0, lr: float = 1.0, ep0: int = 0, ep1: int | None = None) -> torch.Tensor:
    """Epochs ``ep0 .. ep1 - 1`` queued back to back (no host read between them) -> the final positions.
    ``Y0`` is used as one of the two buffers and is overwritten."""
    _check_layout(Y0, graph, state)
    ep1 = n_epochs if ep1 is None else ep1
    row_ptr, col, _ = graph
    Y1 = torch.empty_like(Y0)
    _native.call("be_umap_layout", _native.ptr(Y0), _native.ptr(Y1), Y0.shape[0], _native.ptr(row_ptr), _native.ptr(col),
                 col.numel(), _native.ptr(state["eps"]), _native.ptr(state["epn"]), _native.ptr(state["next"]),
                 _native.ptr(state["nneg"]), ep0, ep1, n_epochs, lr, a, b, gamma, _seed32(seed),
                 _native.stream(Y0.device))
    return Y0 if (ep1 - ep0) % 2 == 0 else Y1


def pca_init_gpu(x: torch.Tensor) -> torch.Tensor:
    """``reference.pca_init`` on the device: eigenvectors of the fp64 covariance, signed, axes mapped to [0, 10]."""
    xc = x.double()
    xc = xc - xc.mean(0, keepdim=True)
    _, evecs = torch.linalg.eigh(xc.T @ xc)
    V = evecs[:, -2:].flip(1)
    big = torch.gather(V, 0, V.abs().argmax(0, keepdim=True))
    V = V * torch.where(big < 0, -1.0, 1.0)
    p = xc @ V
    lo, hi = p.min(0).values, p.max(0).values
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    return (10.0 * (p - lo) / span).float().contiguous()


def degree_stats(row_ptr: torch.Tensor) -> tuple[int, int]:
    deg = row_ptr[1:] - row_ptr[:-1]
    return int(deg.median()), int(deg.max())


def umap_fit_gpu(x, params: UMAPParams | None = None, device=None):
    """``x [n, d]`` -> ``(coords float32 [n, 2] on the device, info)``.  ``info``: ``n_epochs``, ``n_edges``
    (directed), ``a``, ``b``, ``degree_median``, ``degree_max`` and ``spans_ms`` (device time per stage)."""
    p = params or UMAPParams()
    if not _native.hip_available():
        raise _native.NativeUnavailable("umap_fit_gpu needs a GPU and the native kernel library")
    dev = torch.device(device) if device is not None else (x.device if torch.is_tensor(x) and x.is_cuda else torch.device("cuda"))
    x = (x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, np.float32))).to(dev, torch.float32)
    if x.dim() != 2:
        raise ValueError("x must be [n, d]")
    n = x.shape[0]
    ref.check_umap_limits(n, p.n_neighbors, p.metric)
    ok = torch.isfinite(x).all()
    if p.metric == "cosine":
        ok = ok & (x.norm(dim=1) > 0).all()
    if not bool(ok):
        raise ValueError("non-finite input or, under the cosine metric, a zero-norm row")
    if isinstance(p.init, str) and p.init != "pca":
        raise ValueError('init must be "pca" or an [n, 2] array')
    n_epochs = p.n_epochs or ref.default_n_epochs(n)
    a, b = ref.umap_ab(p.spread, p.min_dist)
    marks = [("start", _mark(dev))]

    with torch.cuda.device(dev):
        with trace.span("umap.knn", cuda=True, n=n):
            idx, dist = knn_table_gpu(x, p.n_neighbors, p.metric)
        marks.append(("knn", _mark(dev)))
        with trace.span("umap.smooth_knn", cuda=True):
            _, _, memb = smooth_knn_gpu(idx, dist)
        marks.append(("smooth_knn", _mark(dev)))
        with trace.span("umap.graph", cuda=True):
            graph = graph_from_memberships(idx, memb, n_epochs)
            state = layout_state_gpu(graph[2], p.negative_sample_rate)
        marks.append(("graph", _mark(dev)))
        with trace.span("umap.init", cuda=True):
            if isinstance(p.init, str):
                Y0 = pca_init_gpu(x)
            else:
                Y0 = torch.as_tensor(np.asarray(p.init, np.float32)).to(dev).contiguous().clone()
                if Y0.shape != (n, 2):
                    raise ValueError("init array must be [n, 2]")
        marks.append(("init", _mark(dev)))
        with trace.span("umap.layout", cuda=True, n_epochs=n_epochs):
            Y = layout_gpu(Y0, graph, state, n_epochs, a, b, p.seed, p.repulsion_strength, p.learning_rate)
        marks.append(("layout", _mark(dev)))
        dmed, dmax = degree_stats(graph[0])
        marks[-1][1].synchronize()
    spans = {name: round(marks[i][1].elapsed_time(ev), 4) for i, (name, ev) in enumerate(marks[1:])}
    info = {"n_epochs": n_epochs, "n_edges": int(graph[1].numel()), "a": a, "b": b, "degree_median": dmed,
            "degree_max": dmax, "spans_ms": spans}
    return Y, info


def _mark(dev):
    ev = torch.cuda.Event(enable_timing=True)
    ev.record(torch.cuda.current_stream(dev))
    return ev


# ------------------------------------------------------------------------------------------- transform
TRANSFORM_CHUNK = 1 << 17  # queries per pass of umap_transform_gpu; no rule looks beyond its own row


def knn_query_table_gpu(q: torch.Tensor, x: torch.Tensor, k: int, metric: str = "cosine", budget: int = 1 << 30):
    """``q [m, d]`` against the training rows ``x [n, d]`` -> ``idx [m, k]`` int32, ``dist [m, k]`` float32 as
    ``reference.knn_query_table``: the ``k`` nearest training rows, ascending, no self column.  Score blocks of
    ``budget // n`` query rows; an ``m x n`` matrix is never materialised."""
    if q.dim() != 2 or x.dim() != 2 or q.shape[1] != x.shape[1]:
        raise ValueError(f"q {tuple(q.shape)} and x {tuple(x.shape)} must be [m, d] and [n, d]")
    m, n = q.shape[0], x.shape[0]
    ref.check_transform_limits(m, n, k, metric)
    q, x = q.float(), x.float()
    if metric == "cosine":
        q = q / q.norm(dim=1, keepdim=True)
        x = x / x.norm(dim=1, keepdim=True)
    else:
        sq, sx = (q * q).sum(1), (x * x).sum(1)
    rows = max(1, min(max(m, 1), budget // n))
    idx = torch.empty(m, k, dtype=torch.int32, device=q.device)
    dist = torch.empty(m, k, dtype=torch.float32, device=q.device)
    xt = x.T
    for i in range(0, m, rows):
        s = torch.mm(q[i:i + rows], xt)
        if metric == "cosine":
            d = (1.0 - s).clamp_(min=0.0)
        else:
            d = (sq[i:i + rows, None] + sx[None, :] - 2.0 * s).clamp_(min=0.0).sqrt_()
        td, ti = torch.topk(d, k, dim=1, largest=False, sorted=True)
        idx[i:i + rows] = ti.int()
        dist[i:i + rows] = td
    return idx, dist


def smooth_knn_query_gpu(dist: torch.Tensor):
    """``dist [m, k]`` (no self column) -> ``rho [m]``, ``sigma [m]``, memberships ``[m, k]`` (float32) as
    ``reference.smooth_knn_query`` / ``memberships_query``: ``be_umap_smooth_knn_query``."""
    m, k = dist.shape
    if not 1 <= k <= 64:
        raise ValueError("n_neighbors must be in 1..64")
    if not dist.is_cuda:
        raise _native.NativeUnavailable("be_umap_smooth_knn_query needs a GPU tensor")
    dist = dist.float().contiguous()
    rho = torch.empty(m, dtype=torch.float32, device=dist.device)
    sigma = torch.empty_like(rho)
    memb = torch.empty(m, k, dtype=torch.float32, device=dist.device)
    _native.call("be_umap_smooth_knn_query", _native.ptr(dist), m, k, _native.ptr(rho), _native.ptr(sigma),
                 _native.ptr(memb), _native.stream(dist.device))
    return rho, sigma, memb


def transform_init_gpu(idx: torch.Tensor, w: torch.Tensor, Y_train: torch.Tensor) -> torch.Tensor:
    """``reference.transform_init``: the ``w``-weighted mean of the neighbours' training positions, in fp64."""
    w64 = w.double()
    Yn = Y_train.double()[idx.long()]
    return ((w64[:, :, None] * Yn).sum(1) / w64.sum(1, keepdim=True)).float().contiguous()


def transform_layout_gpu(Y: torch.Tensor, Y_train: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, n_epochs: int,
                         a: float, b: float, seed: int = 42, gamma: float = 1.0, lr: float = 1.0,
                         negative_sample_rate: int = 5, ep0: int = 0, ep1: int | None = None,
                         state: dict | None = None) -> torch.Tensor:
    """``be_umap_transform``: epochs ``ep0 .. ep1 - 1`` of ``n_epochs`` in ONE launch.  ``Y [m, 2]`` holds the start
    and is updated in place (and returned); ``state`` (``next`` / ``nneg`` ``[m, k]``) is read and written when
    given, else the run starts from the initial schedule, which needs ``ep0 == 0``."""
    m, k = idx.shape
    n = Y_train.shape[0]
    ep1 = n_epochs if ep1 is None else ep1
    if not 1 <= k <= 64:
        raise ValueError("n_neighbors must be in 1..64")
    if state is None and ep0 != 0:
        raise ValueError("a run that does not start at epoch 0 needs its schedule state")
    if not 0 <= ep0 <= ep1 <= n_epochs:
        raise ValueError("need 0 <= ep0 <= ep1 <= n_epochs")
    if negative_sample_rate < 1 or n < 1:
        raise ValueError("negative_sample_rate and the training set must be at least 1")
    if not (Y.is_cuda and Y_train.is_cuda and idx.is_cuda and w.is_cuda):
        raise _native.NativeUnavailable("the UMAP transform kernel needs GPU tensors")
    assert Y.dtype == torch.float32 and Y.shape == (m, 2) and Y.is_contiguous()
    assert Y_train.dtype == torch.float32 and Y_train.shape == (n, 2) and Y_train.is_contiguous()
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    assert w.dtype == torch.float32 and w.shape == (m, k) and w.is_contiguous()
    nxt = nng = None
    if state is not None:
        nxt, nng = state["next"], state["nneg"]
        for t in (nxt, nng):
            assert t.is_cuda and t.dtype == torch.float32 and t.shape == (m, k) and t.is_contiguous()
    _native.call("be_umap_transform", _native.ptr(Y_train), n, _native.ptr(idx), _native.ptr(w), m, k, _native.ptr(Y),
                 _native.ptr(nxt), _native.ptr(nng), ep0, ep1, n_epochs, lr, a, b, gamma, int(negative_sample_rate),
                 _seed32(seed), _native.stream(Y.device))
    return Y


def umap_transform_gpu(q, x_train, Y_train, params: UMAPParams | None = None, device=None):
    """New points ``q [m, d]`` onto the layout ``Y_train [n, 2]`` of ``x_train [n, d]`` (``reference.umap_transform``)
    -> ``(coords float32 [m, 2] on the device, info)``.  ``info``: ``n_epochs`` and ``spans_ms`` (device time of
    ``knn``, ``smooth_knn``, ``init``, ``layout``, summed over the chunks).  Queries go through in chunks of
    ``TRANSFORM_CHUNK`` rows (a host array is uploaded chunk by chunk); every rule is per row, so from the
    neighbour table onward the chunking cannot change a result."""
    p = params or UMAPParams()
    if not _native.hip_available():
        raise _native.NativeUnavailable("umap_transform_gpu needs a GPU and the native kernel library")
    dev = torch.device(device) if device is not None else next(
        (t.device for t in (q, x_train, Y_train) if torch.is_tensor(t) and t.is_cuda), torch.device("cuda"))

    def host_or_dev(t):
        return t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float32)))

    q = host_or_dev(q)
    x = host_or_dev(x_train).to(dev, torch.float32)
    Yt = host_or_dev(Y_train).to(dev, torch.float32).contiguous()
    if q.dim() != 2 or x.dim() != 2 or q.shape[1] != x.shape[1]:
        raise ValueError(f"q {tuple(q.shape)} and x_train {tuple(x.shape)} must be [m, d] and [n, d]")
    m, n = q.shape[0], x.shape[0]
    if Yt.shape != (n, 2):
        raise ValueError("Y_train must be [n, 2]")
    n_epochs = ref.transform_n_epochs(p)
    k = p.n_neighbors
    ref.check_transform_limits(m, n, k, p.metric)

    def bad(t):
        ok = torch.isfinite(t).all()
        if p.metric == "cosine":
            ok = ok & (t.float().norm(dim=1) > 0).all()
        return not bool(ok)

    if bad(x) or not bool(torch.isfinite(Yt).all()) or (m and bad(q)):
        raise ValueError("non-finite input or, under the cosine metric, a zero-norm row")
    a, b = ref.umap_ab(p.spread, p.min_dist)
    out = torch.empty(m, 2, dtype=torch.float32, device=dev)
    spans = {"knn": 0.0, "smooth_knn": 0.0, "init": 0.0, "layout": 0.0}
    marks = []
    with torch.cuda.device(dev):
        for i in range(0, m, TRANSFORM_CHUNK):
            qc = q[i:i + TRANSFORM_CHUNK].to(dev, torch.float32)
            ev = [_mark(dev)]
            with trace.span("umap.transform.knn", cuda=True, m=qc.shape[0], n=n):
                idx, dist = knn_query_table_gpu(qc, x, k, p.metric)
            ev.append(_mark(dev))
            with trace.span("umap.transform.smooth_knn", cuda=True):
                _, _, w = smooth_knn_query_gpu(dist)
            ev.append(_mark(dev))
            with trace.span("umap.transform.init", cuda=True):
                Y = transform_init_gpu(idx, w, Yt)
            ev.append(_mark(dev))
            with trace.span("umap.transform.layout", cuda=True, n_epochs=n_epochs):
                transform_layout_gpu(Y, Yt, idx, w, n_epochs, a, b, p.seed, p.repulsion_strength, p.learning_rate,
                                     p.negative_sample_rate)
                out[i:i + TRANSFORM_CHUNK] = Y
            ev.append(_mark(dev))
            marks.append(ev)
        if marks:
            marks[-1][-1].synchronize()
    for ev in marks:
        for j, name in enumerate(spans):
            spans[name] += ev[j].elapsed_time(ev[j + 1])
    return out, {"n_epochs": n_epochs, "spans_ms": {s: round(v, 4) for s, v in spans.items()}}
