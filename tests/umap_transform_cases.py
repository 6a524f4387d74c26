"""Shared case builders of the UMAP transform tests (``test_umap_transform_reference.py``,
``test_umap_transform_gpu.py``, ``test_umap_transform_app.py``): training sets, queries and the numpy oracle's
results, computed once per process and handed out as copies."""
from __future__ import annotations

import numpy as np

import umap_cases as uc
from bioengine_worker_amd.search import reference as ref
from bioengine_worker_amd.search.umap import UMAPParams

E = 100  # transform epochs of every case (the default)
SEED = uc.SEED
NSR = 5
NAMES = ("q131", "c300", "k64", "k1")
LABELS300 = np.arange(300) % 12  # cluster of every row of clusters300()


def query_gaps(q: np.ndarray, x: np.ndarray, k: int):
    """Per query row of the float64 cosine table: the gap between the last listed and the first unlisted
    distance, and the smallest gap between consecutive listed ones (``umap_cases.knn_gaps`` for queries)."""
    q, x = q.astype(np.float64), x.astype(np.float64)
    d = np.maximum(0, 1 - (q / np.sqrt((q * q).sum(1))[:, None]) @ (x / np.sqrt((x * x).sum(1))[:, None]).T)
    s = np.sort(d, 1)[:, :k + 1]
    g = np.diff(s, axis=1)
    edge = g[:, -1] if x.shape[0] > k else np.full(len(q), np.inf)
    inner = g[:, :k - 1].min(1) if k > 1 else np.full(len(q), np.inf)
    return edge, inner


def tie_free_queries(m: int, x: np.ndarray, k: int, seed: int) -> np.ndarray:
    """Gaussian query rows, re-drawn one by one until none has a near-tie against ``x`` (as ``tie_free``)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((m, x.shape[1])).astype(np.float32)
    for _ in range(200):
        edge, inner = query_gaps(q, x, k)
        bad = np.nonzero((edge <= 2 * uc.KNN_GAP) | (inner <= 2 * uc.KNN_INNER_GAP))[0]
        if bad.size == 0:
            return q
        q[bad] = rng.standard_normal((bad.size, x.shape[1])).astype(np.float32)
    raise AssertionError("no tie-free query set found")


@uc.shared
def fitted240() -> np.ndarray:
    """The oracle's layout of the first 240 rows of ``clusters300()``."""
    return ref.umap_fit(uc.clusters300()[:240], UMAPParams(n_epochs=uc.EPOCHS300))


@uc.shared
def data(name: str):
    """-> ``(x_train, Y_train, q, k)``."""
    if name == "q131":
        x = uc.tie_free(131, 8, 5)
        return x, uc.start_positions("n131"), tie_free_queries(37, x, 5, 2131), 5
    if name == "c300":
        x = uc.clusters300()
        return x[:240], fitted240(), x[240:], uc.K300
    if name == "k64":
        rng = np.random.default_rng(64)
        x = rng.standard_normal((70, 8)).astype(np.float32)
        return x, rng.uniform(0.0, 10.0, (70, 2)).astype(np.float32), tie_free_queries(3, x, 64, 2064), 64
    if name == "k1":
        x = uc.tie_free(131, 8, 5)
        return x, uc.start_positions("n131"), tie_free_queries(19, x, 1, 2001), 1
    raise KeyError(name)


def hand_table() -> np.ndarray:
    """k = 5 query rows given directly: leading zeros, all equal, all zero, a spread that keeps ``hi == inf`` for
    several doublings, a ``1e-7`` first entry (what a float32 GEMM returns for a duplicate), generic rows."""
    rng = np.random.default_rng(55)
    rows = [[0, 0, 0, 0.3, 0.5], [0.4, 0.4, 0.4, 0.4, 0.4], [0, 0, 0, 0, 0], [1.0, 50.0, 60.0, 70.0, 80.0],
            [1e-7, 0.2, 0.3, 0.4, 0.5]]
    rows += [sorted(rng.uniform(0.05, 1.0, 5).tolist()) for _ in range(6)]
    return np.asarray(rows, np.float32)


@uc.shared
def dist_table(name: str) -> np.ndarray:
    return hand_table() if name == "hand" else case(name)["dist"]


@uc.shared
def case(name: str):
    """The float64-rule oracle stages of a case: table, rho / sigma, memberships ``w``, start ``Y0``."""
    x, Yt, q, k = data(name)
    idx, dist = ref.knn_query_table(q, x, k)
    rho, sigma = ref.smooth_knn_query(dist)
    w = ref.memberships_query(dist, rho, sigma)
    return {"x": x, "Y_train": Yt, "q": q, "k": k, "idx": idx, "dist": dist, "w": w,
            "Y0": ref.transform_init(idx, w, Yt)}


# ------------------------------------------------------------------------------------------- the layout
@uc.shared
def trajectory(name: str, seed: int = SEED):
    """The float32 oracle run: per epoch its input ``(Y, next, nneg)`` and the largest sample count, then the
    final ``(Y, next, nneg, 0)`` as entry ``E``."""
    c = case(name)
    a, b = uc.ab()
    Y = c["Y0"]
    st = ref.transform_state(c["w"], E, NSR)
    steps = []
    for ep in range(E):
        Yn, stn, cnt = ref.transform_epoch(Y, c["Y_train"], c["idx"], st, ep, E, a, b, seed, return_counts=True)
        steps.append((Y, st["next"], st["nneg"], int(cnt.max())))
        Y, st = Yn, stn
    steps.append((Y, st["next"], st["nneg"], 0))
    return steps


def epoch_list(name: str) -> list[int]:
    """0, 1, 7, the last epoch, and the first other epoch in which some slot draws two or more samples."""
    eps = [0, 1, 7, E - 1]
    steps = trajectory(name)
    return eps + [next(ep for ep in range(E) if ep not in eps and steps[ep][3] >= 2)]


@uc.shared
def step_case(name: str, ep: int, variant: str = ""):
    """One teacher-forced epoch: the oracle's input before epoch ``ep`` and its float32 / float64 outputs.
    ``variant="coincident"``: query 0 starts exactly on the training point of one of its active slots (the
    attractive ``d2 == 0``), query 1 exactly on the first negative sample of one of its active slots."""
    c = case(name)
    a, b = uc.ab()
    Y, nxt, nneg, _ = trajectory(name)[ep]
    st = dict(ref.transform_state(c["w"], E, NSR), next=nxt, nneg=nneg)
    if variant == "coincident":
        act = st["live"] & (nxt <= np.float32(ep))
        s0 = int(np.nonzero(act[0])[0][0])
        Y[0] = c["Y_train"][c["idx"][0, s0]]
        cnt = ((np.float32(ep) - nneg[1]) / st["epn"][1]).astype(np.int64)
        s1 = int(np.nonzero(act[1] & (cnt >= 1))[0][0])
        v = int(ref.negative_vertex(ref.transform_key(c["idx"])[1, s1], SEED, ep, 0, c["Y_train"].shape[0]))
        Y[1] = c["Y_train"][v]
    args = (Y, c["Y_train"], c["idx"], st, ep, E, a, b, SEED)
    Y32, st32, cnt = ref.transform_epoch(*args, dtype=np.float32, return_counts=True)
    Y64, st64 = ref.transform_epoch(*args, dtype=np.float64)
    assert np.array_equal(st32["next"], st64["next"]) and np.array_equal(st32["nneg"], st64["nneg"])
    return {"case": c, "Y": Y, "state": st, "ep": ep, "a": a, "b": b, "Y32": Y32, "Y64": Y64, "next": st32["next"],
            "nneg": st32["nneg"], "m": cnt}


@uc.shared
def whole_run(name: str):
    """The float32 and float64 oracle runs from the same start -> ``(Y32, Y64, final state)``."""
    c = case(name)
    a, b = uc.ab()
    Y32, nxt, nneg, _ = trajectory(name)[E]
    Y64 = ref.umap_transform_layout(c["Y0"], c["Y_train"], c["idx"], c["w"], E, a, b, SEED, dtype=np.float64)
    return Y32, Y64, {"next": nxt, "nneg": nneg}


SENSITIVE = 1e-4     # a query on which the two oracles part by more than this is sensitive
SENSITIVE_CAP = 0.1  # at most this share of a case's queries


def sensitivity(name: str):
    """-> ``(per-query |Y32 - Y64|, sensitive mask)``."""
    Y32, Y64, _ = whole_run(name)
    d = np.abs(Y32.astype(np.float64) - Y64).max(1)
    return d, d > SENSITIVE


def same_cluster_hits(Y: np.ndarray) -> int:
    """How many of c300's 60 held-out points have a same-cluster training point as nearest 2-D neighbour."""
    Yt = fitted240().astype(np.float64)
    nn = ((np.asarray(Y, np.float64)[:, None, :] - Yt[None]) ** 2).sum(2).argmin(1)
    return int((LABELS300[nn] == LABELS300[240:]).sum())
