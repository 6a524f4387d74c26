"""Shared case builders of the UMAP tests (``test_umap_reference.py``, ``test_umap_gpu.py``): inputs and the
numpy oracle's results, computed once per process and handed out as copies."""
from __future__ import annotations

import functools

import numpy as np

from bioengine_worker_amd.search import reference as ref

K300, EPOCHS300 = 15, 200
SEED = 42


def _copy(o):
    if isinstance(o, np.ndarray):
        return o.copy()
    if isinstance(o, dict):
        return {k: _copy(v) for k, v in o.items()}
    if isinstance(o, (tuple, list)):
        return type(o)(_copy(v) for v in o)
    return o


def shared(fn):
    cached = functools.lru_cache(maxsize=None)(fn)

    @functools.wraps(fn)
    def get(*a):
        return _copy(cached(*a))

    return get


# ---------------------------------------------------------------------------------------------- data
@shared
def clusters300() -> np.ndarray:
    """300 points of 12 Gaussian clusters in 32-D: centres 3 N(0, 1), unit noise, every coordinate + 5."""
    rng = np.random.default_rng(0)
    centres = 3.0 * rng.standard_normal((12, 32))
    return (centres[np.arange(300) % 12] + rng.standard_normal((300, 32)) + 5.0).astype(np.float32)


KNN_GAP = 1e-4        # k-th against (k+1)-th distance of every row
KNN_INNER_GAP = 2e-5  # any two consecutive distances of a row's table


def knn_gaps(x: np.ndarray, k: int):
    """Per row of the float64 cosine table: the gap between the last listed and the first unlisted distance,
    and the smallest gap between consecutive listed ones."""
    x = x.astype(np.float64)
    xn = x / np.sqrt((x * x).sum(1))[:, None]
    d = np.maximum(0, 1 - xn @ xn.T)
    np.fill_diagonal(d, np.inf)
    s = np.sort(d, 1)[:, :k]  # k - 1 listed + the first unlisted
    g = np.diff(s, axis=1)
    return g[:, -1], (g[:, :-1].min(1) if k > 2 else np.full(len(x), np.inf))


@shared
def tie_free(n: int, d: int, k: int) -> np.ndarray:
    """Gaussian points re-drawn one by one until no row has a near-tie (KNN_GAP at the table's edge,
    KNN_INNER_GAP inside it): the GPU's fp32 GEMM then has to list the same neighbours in the same order."""
    rng = np.random.default_rng(1000 + n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    for _ in range(200):
        edge, inner = knn_gaps(x, k)
        bad = np.nonzero((edge <= 2 * KNN_GAP) | (inner <= 2 * KNN_INNER_GAP))[0]
        if bad.size == 0:
            return x
        x[bad] = rng.standard_normal((bad.size, d)).astype(np.float32)
    raise AssertionError("no tie-free point set found")


@shared
def table(name: str):
    """Oracle neighbour tables ``(idx, dist)``: "n131" / "n300" of the tie-free sets, "c300" of the clusters."""
    if name == "n131":
        return ref.knn_table(tie_free(131, 8, 5), 5)
    if name == "n300":
        return ref.knn_table(tie_free(300, 32, 15), 15)
    if name == "c300":
        return ref.knn_table(clusters300(), K300)
    if name == "hub":
        return hub_table()
    if name == "hand5":
        return hand_table5()
    if name == "hand2":
        return hand_table2()
    raise KeyError(name)


def _ring_idx(n: int, k: int) -> np.ndarray:
    return ((np.arange(n)[:, None] + np.arange(k)[None, :]) % n).astype(np.int32)


def hand_table5():
    """k = 5 rows given directly: duplicates (zero distances), all equal, no positive distance, a spread
    that keeps ``hi == inf`` for several doublings, one exact zero beside generic values, generic rows."""
    rng = np.random.default_rng(5)
    rows = [[0, 0, 0, 0.3, 0.5], [0, 0.4, 0.4, 0.4, 0.4], [0, 0, 0, 0, 0], [0, 1.0, 50.0, 60.0, 70.0],
            [0, 0, 0.2, 0.21, 0.9]]
    rows += [[0.0] + sorted(rng.uniform(0.05, 1.0, 4).tolist()) for _ in range(6)]
    dist = np.asarray(rows, np.float32)
    return _ring_idx(len(rows), 5), dist


def hand_table2():
    rng = np.random.default_rng(2)
    dist = np.zeros((9, 2), np.float32)
    dist[:, 1] = rng.uniform(0.05, 1.0, 9)
    dist[3, 1] = 0.0
    return _ring_idx(9, 2), dist


def hub_table():
    """n = 131 (no multiple of 64), k = 5, every row lists vertex 0: vertex 0 ends with 130 neighbours, more
    than a wave has lanes."""
    n, k = 131, 5
    rng = np.random.default_rng(131)
    idx = np.zeros((n, k), np.int32)
    idx[0] = [0, 1, 2, 3, 4]
    for i in range(1, n):
        idx[i] = [i, 0] + [((i + s) % (n - 1)) + 1 for s in (1, 2, 3)]
    dist = np.sort(rng.uniform(0.1, 1.0, (n, k)).astype(np.float32), 1)
    dist[:, 0] = 0.0
    return idx, dist


GRAPH_EPOCHS = {"n131": 200, "n300": 200, "c300": EPOCHS300, "hub": 200, "hand5": 200, "hand2": 200}


@shared
def graph(name: str):
    idx, dist = table(name)
    return ref.fuzzy_graph(idx, dist, GRAPH_EPOCHS[name])


@shared
def ab():
    return ref.umap_ab()


@shared
def start_positions(name: str) -> np.ndarray:
    if name == "c300":
        return ref.pca_init(clusters300())
    return np.random.default_rng(7).uniform(0.0, 10.0, (table(name)[0].shape[0], 2)).astype(np.float32)


# ------------------------------------------------------------------------------------- layout epochs
@shared
def trajectory(name: str, seed: int = SEED):
    """The float32 oracle run of graph ``name``: per epoch the input ``(Y, next, nneg)`` and the largest
    sample count ``m`` of the epoch."""
    g = graph(name)
    n_epochs = GRAPH_EPOCHS[name]
    a, b = ab()
    Y = start_positions(name)
    st = ref.layout_state(g[2])
    steps = []
    for ep in range(n_epochs):
        Yn, stn, m = ref.layout_epoch(Y, g, st, ep, n_epochs, a, b, seed, return_counts=True)
        steps.append((Y, st["next"], st["nneg"], int(m.max()) if m.size else 0))
        Y, st = Yn, stn
    return steps


def epoch_list(name: str) -> list[int]:
    """0, 1, 7, the last epoch, and the first other epoch in which some edge draws two or more samples."""
    n_epochs = GRAPH_EPOCHS[name]
    eps = [0, 1, 7, n_epochs - 1]
    steps = trajectory(name)
    extra = next(ep for ep in range(n_epochs) if ep not in eps and steps[ep][3] >= 2)
    return eps + [extra]


@shared
def step_case(name: str, ep: int, seed: int = SEED, variant: str = ""):
    """One teacher-forced epoch: the oracle's input before epoch ``ep`` and its float32 / float64 outputs.
    ``variant="coincident"`` moves the tail of an active edge onto its head first."""
    g = graph(name)
    n_epochs = GRAPH_EPOCHS[name]
    a, b = ab()
    Y, nxt, nneg, _ = trajectory(name, seed)[ep]
    base = ref.layout_state(g[2])
    st = {"eps": base["eps"], "epn": base["epn"], "next": nxt, "nneg": nneg}
    if variant == "coincident":
        head = np.repeat(np.arange(Y.shape[0]), np.diff(g[0]))
        e = int(np.nonzero(nxt <= np.float32(ep))[0][0])
        Y[g[1][e]] = Y[head[e]]
    Y32, st32, m = ref.layout_epoch(Y, g, st, ep, n_epochs, a, b, seed, dtype=np.float32, return_counts=True)
    Y64, st64 = ref.layout_epoch(Y, g, st, ep, n_epochs, a, b, seed, dtype=np.float64)
    assert np.array_equal(st32["next"], st64["next"]) and np.array_equal(st32["nneg"], st64["nneg"])
    return {"graph": g, "Y": Y, "state": st, "ep": ep, "n_epochs": n_epochs, "a": a, "b": b, "seed": seed, "Y32": Y32,
            "Y64": Y64, "next": st32["next"], "nneg": st32["nneg"], "m": m}


def self_hits(name: str, ep: int, seed: int) -> int:
    """How many negative samples of epoch ``ep`` land on their own head under ``seed``."""
    g = graph(name)
    n = g[0].size - 1
    _, nxt, nneg, _ = trajectory(name)[ep]
    st = ref.layout_state(g[2])
    head = np.repeat(np.arange(n), np.diff(g[0]))
    act = np.nonzero(nxt <= np.float32(ep))[0]
    m = ((np.float32(ep) - nneg[act]).astype(np.float32) / st["epn"][act]).astype(np.float32).astype(np.int64)
    hits = 0
    for p in range(int(m.max()) if m.size else 0):
        e = act[m > p]
        hits += int((ref.negative_vertex(e, seed, ep, p, n) == head[e]).sum())
    return hits


@shared
def self_hit_seed(name: str, ep: int) -> int:
    """The first seed for which the oracle draws a vertex as its own negative sample in epoch ``ep``.  The
    state before ``ep`` does not depend on the seed for ep <= 1 (nothing moves the schedule but time)."""
    return next(s for s in range(1000) if self_hits(name, ep, s) > 0)


def y_tolerance(case) -> float:
    """4 x the float32 / float64 oracle difference of the step, never less than 8 ulp of the largest
    coordinate magnitude."""
    big = np.float32(np.abs(case["Y64"]).max())
    return max(4.0 * float(np.abs(case["Y32"].astype(np.float64) - case["Y64"]).max()), 8.0 * float(np.spacing(big)))


def trust(x: np.ndarray, Y: np.ndarray) -> float:
    from sklearn.manifold import trustworthiness

    return float(trustworthiness(x, Y, n_neighbors=15, metric="cosine"))
