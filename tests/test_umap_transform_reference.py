"""The numpy oracle of the UMAP transform (``search/reference.py``: ``knn_query_table`` .. ``umap_transform``):
hand-computed memberships, the position-independent schedule, per-query independence, quality on held-out
points of ``clusters300()``."""
import numpy as np
import pytest

import umap_cases as uc
import umap_transform_cases as tc
from bioengine_worker_amd.search import reference as ref
from bioengine_worker_amd.search.umap import UMAPParams


def test_query_table_lists_the_nearest_training_rows():
    for name in ("q131", "k64", "k1"):
        c = tc.case(name)
        q, x = c["q"].astype(np.float64), c["x"].astype(np.float64)
        d = 1 - (q / np.linalg.norm(q, axis=1)[:, None]) @ (x / np.linalg.norm(x, axis=1)[:, None]).T
        assert c["idx"].dtype == np.int32 and c["dist"].dtype == np.float32 and c["idx"].shape == (len(q), c["k"])
        assert np.array_equal(c["idx"], np.argsort(d, 1)[:, :c["k"]])
        assert (np.diff(c["dist"], axis=1) >= 0).all()
    x = np.eye(4, dtype=np.float32)[[0, 0, 1, 1]]  # duplicates: ties go by index
    idx, dist = ref.knn_query_table(x[:1], x, 3)
    assert idx.tolist() == [[0, 1, 2]] and dist.tolist() == [[0.0, 0.0, 1.0]]
    idx, dist = ref.knn_query_table(np.array([[3.0, 4.0]]), np.array([[0.0, 0.0], [3.0, 0.0]]), 2, "euclidean")
    assert idx.tolist() == [[1, 0]] and dist.tolist() == [[4.0, 5.0]]


def test_hand_memberships():
    dist = tc.hand_table()
    k = dist.shape[1]
    for dt in (np.float64, np.float32):
        rho, sigma = ref.smooth_knn_query(dist, dt)
        w = ref.memberships_query(dist, rho, sigma)
        assert w.dtype == np.float32 and w.shape == dist.shape
        assert np.array_equal(rho.astype(np.float32), dist.min(1))  # zero included
        assert (w.max(1) == 1.0).all() and (w[:, 0] == 1.0).all()
        assert (w[0, :3] == 1.0).all() and (w[1] == 1.0).all() and (w[2] == 1.0).all()
        assert (sigma > 0).all() and (sigma >= 1e-3 * dist.astype(dt).mean(1) * (1 - 1e-6)).all()
    rho, sigma = ref.smooth_knn_query(dist, np.float64)
    w = ref.memberships_query(dist, rho, sigma)
    # row 0: three ones, exp(-0.3 / s) + exp(-0.5 / s) = log2(5) - 3 has no solution (the left side is < 2 but
    # log2(5) - 3 < 0): the sum stays above the target, sigma collapses to its floor, the tail vanishes
    assert sigma[0] == pytest.approx(1e-3 * dist[0].astype(np.float64).mean()) and (w[0, 3:] < 1e-30).all()
    # row 1, row 2: every gap is 0, the sum is k > log2(k) whatever sigma: floored (row 2: the bisection's 2^-64)
    assert sigma[1] == pytest.approx(1e-3 * 0.4, rel=1e-6) and 0 < sigma[2] < 1e-18
    # rows 3, 4 and the generic ones: 1 + sum exp(-(d - rho) / sigma) = log2(k) to the bisection's tolerance
    for i in range(3, len(dist)):
        gap = dist[i].astype(np.float64) - rho[i]
        assert abs(np.exp(-gap / sigma[i]).sum() - np.log2(k)) < 2e-5
        np.testing.assert_allclose(w[i], np.exp(-gap / sigma[i]).astype(np.float32), rtol=1e-6)
    assert rho[3] == 1.0 and 20 < sigma[3] < 100  # several doublings with hi == inf
    assert rho[4] == np.float32(1e-7) and w[4, 0] == 1.0 and w[4, 1] < 1.0


def test_schedule_and_pruning():
    c = tc.case("c300")
    st = ref.transform_state(c["w"], tc.E, tc.NSR)
    assert np.array_equal(st["live"], c["w"] >= np.float32(1) / np.float32(tc.E)) and not st["live"].all()
    assert np.array_equal(st["eps"], (np.float32(1) / c["w"]).astype(np.float32))
    assert np.array_equal(st["epn"], (st["eps"] / np.float32(5)).astype(np.float32))
    assert np.array_equal(st["next"], st["eps"]) and np.array_equal(st["nneg"], st["epn"])
    steps = tc.trajectory("c300")
    never = ~st["live"]
    assert np.array_equal(steps[tc.E][1][never], st["next"][never])  # a pruned slot never fires
    assert (steps[tc.E][1][st["live"]] > st["next"][st["live"]]).all()  # every live slot does


def test_schedule_does_not_depend_on_positions():
    c = tc.case("c300")
    a, b = uc.ab()
    other = np.random.default_rng(3).uniform(-5, 15, c["Y_train"].shape).astype(np.float32)
    st = [ref.transform_state(c["w"], tc.E, tc.NSR) for _ in range(2)]
    Y = [c["Y0"], ref.transform_init(c["idx"], c["w"], other)]
    for ep in range(tc.E):
        cnt = []
        for r, Yt in enumerate((c["Y_train"], other)):
            Y[r], st[r], m = ref.transform_epoch(Y[r], Yt, c["idx"], st[r], ep, tc.E, a, b, tc.SEED, return_counts=True)
            cnt.append(m)
        assert np.array_equal(cnt[0], cnt[1])
        assert np.array_equal(st[0]["next"], st[1]["next"]) and np.array_equal(st[0]["nneg"], st[1]["nneg"])
    assert not np.array_equal(Y[0], Y[1])


def test_query_alone_equals_query_in_batch():
    x, Yt, q, _ = tc.data("c300")
    whole = ref.umap_transform(q, x, Yt)
    for i in (0, 7, 59):
        assert np.array_equal(ref.umap_transform(q[i:i + 1], x, Yt), whole[i:i + 1])
    assert np.array_equal(ref.umap_transform(q[::-1], x, Yt), whole[::-1])
    assert np.array_equal(whole, tc.whole_run("c300")[0])  # the staged run of the cases is the chained one


@pytest.mark.parametrize("E", [1, 2, 33])
def test_short_runs_stay_finite(E):
    x, Yt, q, _ = tc.data("q131")
    Y = ref.umap_transform(q, x, Yt, UMAPParams(n_neighbors=5, transform_epochs=E))
    assert Y.shape == (37, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()


def test_default_epochs_do_not_depend_on_the_batch():
    assert ref.transform_n_epochs(UMAPParams()) == 100 and ref.transform_n_epochs(None) == 100
    assert ref.transform_n_epochs(UMAPParams(transform_epochs=30)) == 30
    assert UMAPParams().transform_epochs is None


def test_alpha_and_sampler_key():
    assert ref.epoch_alpha(0, 100, np.float32(1.0) / np.float32(4)) == np.float32(0.25)
    idx = np.array([[7, 3, 9], [2 ** 26 + 1, 0, 1]], np.int32)
    assert ref.transform_key(idx).tolist() == [[448, 449, 450], [64, 65, 66]]  # uint32 wrap-around


def test_held_out_points_land_in_their_cluster():
    x, Yt, q, _ = tc.data("c300")
    c = tc.case("c300")
    assert tc.same_cluster_hits(c["Y0"]) == 60
    for seed in range(6):
        Y = ref.umap_transform(q, x, Yt, UMAPParams(seed=seed))
        assert tc.same_cluster_hits(Y) == 60, seed


def test_sensitive_queries_are_few():
    for name in tc.NAMES:
        d, sens = tc.sensitivity(name)
        print(f"{name}: f32/f64 oracle difference median {np.median(d):.3e} max {d.max():.3e}, {sens.sum()} of {d.size} sensitive")
        assert sens.mean() <= tc.SENSITIVE_CAP


def test_value_errors():
    x, Yt, q, _ = tc.data("c300")
    with pytest.raises(ValueError):
        ref.knn_query_table(q, x[:10], 15)  # k > n
    with pytest.raises(ValueError):
        ref.knn_query_table(q[:, :5], x, 15)
    with pytest.raises(ValueError):
        ref.knn_query_table(q, x, 15, "manhattan")
    for k in (0, 65):
        with pytest.raises(ValueError):
            ref.knn_query_table(q, x, k)
    for arr in (q, x):
        for v in (np.inf, np.nan):
            arr[2, 3] = v
            with pytest.raises(ValueError):
                ref.knn_query_table(q, x, 15)
        arr[2] = 0.0
        with pytest.raises(ValueError):
            ref.knn_query_table(q, x, 15)
        ref.knn_query_table(q, x, 15, "euclidean")  # a zero row is a point like any other there
        arr[2] = 1.0
    with pytest.raises(ValueError):
        ref.umap_transform(q, x, Yt[:100])
    with pytest.raises(ValueError):
        ref.umap_transform(q, x, Yt, UMAPParams(transform_epochs=0))
    empty = ref.umap_transform(q[:0], x, Yt)
    assert empty.shape == (0, 2) and empty.dtype == np.float32
