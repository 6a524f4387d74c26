"""The numpy oracle of the in-house UMAP (``search/reference.py``), the projection modes built on it, and
the conditions the GPU comparisons of ``test_umap_gpu.py`` rest on.  CPU only."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import umap_cases as uc
from bioengine_worker_amd.search import projection
from bioengine_worker_amd.search import reference as ref
from bioengine_worker_amd.search.umap import UMAPParams, graph_from_memberships, knn_table_gpu

GRAPH_CASES = ["n131", "c300", "hub"]


def test_curve_fit_defaults():
    a, b = ref.umap_ab()
    assert abs(a - 1.57694346) < 1e-6 and abs(b - 0.89506088) < 1e-6


def test_mix_reproduces_recorded_values():
    """The values were recorded from the definition evaluated in Python integers, not from the function."""
    fixed = {0: 0, 1: 0x688990C0, 42: 0x172733C2, 0xFFFFFFFF: 0x6768824A, 0x12345678: 0xF5E71C96}
    got = ref.mix(np.array(list(fixed), np.uint32))
    assert [int(v) for v in got] == list(fixed.values()) and got.dtype == np.uint32
    assert int(ref.mix(np.uint32(42))) == 0x172733C2
    v = ref.negative_vertex(np.arange(1000), 42, 3, 1, 131)
    assert v.min() >= 0 and v.max() < 131 and np.unique(v).size > 100


def test_knn_table_rules():
    x = uc.tie_free(131, 8, 5)
    idx, dist = ref.knn_table(x, 5)
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and idx.shape == (131, 5)
    assert np.array_equal(idx[:, 0], np.arange(131)) and (dist[:, 0] == 0).all()
    assert (np.diff(dist[:, 1:], axis=1) >= 0).all() and (idx[:, 1:] != np.arange(131)[:, None]).all()
    with pytest.raises(ValueError):
        ref.knn_table(x[:5], 5)
    z = x.copy()
    z[3] = 0
    with pytest.raises(ValueError):
        ref.knn_table(z, 5)
    ref.knn_table(z, 5, "euclidean")


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_torch_knn_table_equals_the_oracle_on_a_cpu(metric):
    x = uc.tie_free(131, 8, 5)
    idx, dist = ref.knn_table(x, 5, metric)
    ti, td = knn_table_gpu(torch.from_numpy(x), 5, metric, budget=131 * 40)  # four score blocks
    if metric == "cosine":  # the set is tie-free under the cosine metric only
        assert np.array_equal(ti.numpy(), idx)
    assert np.abs(np.sort(td.numpy(), 1) - dist).max() < 1e-4


def test_smooth_knn_hand_rows():
    idx, dist = uc.table("hand5")
    rho, sigma = ref.smooth_knn(dist)
    assert rho[0] == np.float32(0.3) and rho[1] == np.float32(0.4) and rho[2] == 0 and rho[3] == 1
    gmean = dist.astype(np.float64).mean()
    assert sigma[2] == 1e-3 * gmean  # no positive distance: the global-mean floor
    assert sigma[1] == 1e-3 * dist[1].astype(np.float64).mean()  # all equal: the sum never moves, the row floor
    assert sigma[3] > 8  # hi stayed inf for several doublings
    a = ref.memberships(idx, dist, rho, sigma)
    assert a.dtype == np.float32 and (a[2] == 1).all() and (a[0, :3] == 1).all() and (a >= 0).all()
    assert a[0, 3] == 0  # three memberships of 1 already exceed log2(5): sigma falls to its floor, the rest vanishes
    target = np.log2(5)
    for i in range(5, len(dist)):  # generic rows: the calibrated sum
        assert abs(a[i].astype(np.float64).sum() - target) < 1e-4


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_fuzzy_graph_is_bitwise_symmetric_and_rows_ascend(name):
    row_ptr, col, w = uc.graph(name)
    n = row_ptr.size - 1
    head = np.repeat(np.arange(n), np.diff(row_ptr))
    key = head * n + col
    assert (np.diff(key) > 0).all()  # rows ascend, no pair twice
    back = np.searchsorted(key, col.astype(np.int64) * n + head)
    assert np.array_equal(key[back], col.astype(np.int64) * n + head)
    assert np.array_equal(w[back].view(np.uint32), w.view(np.uint32))
    assert (head != col).all() and w.dtype == np.float32 and (w <= 1).all() and w.max() > 0.99


def test_hub_vertex_has_more_neighbours_than_a_wave_has_lanes():
    row_ptr, _, _ = uc.graph("hub")
    assert row_ptr[1] - row_ptr[0] > 64 and (row_ptr.size - 1) % 64 != 0


def test_torch_graph_builder_equals_the_oracle_on_a_cpu():
    for name in GRAPH_CASES:
        idx, dist = uc.table(name)
        rho, sigma = ref.smooth_knn(dist)
        a = ref.memberships(idx, dist, rho, sigma)
        rp, col, w = graph_from_memberships(torch.from_numpy(idx), torch.from_numpy(a), uc.GRAPH_EPOCHS[name], budget=64)
        g = uc.graph(name)
        assert np.array_equal(rp.numpy(), g[0]) and np.array_equal(col.numpy(), g[1])
        assert np.array_equal(w.numpy().view(np.uint32), g[2].view(np.uint32))


def test_case_condition_knn_tables_are_tie_free():
    for n, d, k in ((131, 8, 5), (300, 32, 15)):
        edge, inner = uc.knn_gaps(uc.tie_free(n, d, k), k)
        assert edge.min() > uc.KNN_GAP and inner.min() > uc.KNN_INNER_GAP


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_case_condition_no_weight_near_the_pruning_threshold(name):
    """Evaluated on the unpruned union: prune with a threshold no epoch count reaches, then compare."""
    idx, dist = uc.table(name)
    _, _, w = ref.fuzzy_graph(idx, dist, 10 ** 9)
    thr = float(ref.prune_threshold(w, uc.GRAPH_EPOCHS[name]))
    assert (np.abs(w.astype(np.float64) - thr) > 1e-3 * thr).all()


def test_epoch_zero_moves_nothing():
    g = uc.graph("c300")
    st = ref.layout_state(g[2])
    assert (st["eps"] >= 1).all() and np.array_equal(st["next"], st["eps"]) and np.array_equal(st["nneg"], st["epn"])
    Y0 = uc.start_positions("c300")
    a, b = uc.ab()
    Y1, st1 = ref.layout_epoch(Y0, g, st, 0, 200, a, b, 42)
    assert np.array_equal(Y1, Y0) and np.array_equal(st1["next"], st["next"])
    Y2, st2 = ref.layout_epoch(Y1, g, st1, 1, 200, a, b, 42)
    assert not np.array_equal(Y2, Y1) and (st2["next"] >= st1["next"]).all()


def test_epoch_cases_cover_the_paths():
    for name in ("c300", "hub"):
        eps = uc.epoch_list(name)
        assert len(set(eps)) == 5 and uc.step_case(name, eps[-1])["m"].max() >= 2
        assert uc.self_hits(name, 1, uc.self_hit_seed(name, 1)) > 0
    c = uc.step_case("c300", 7, uc.SEED, "coincident")
    head = np.repeat(np.arange(300), np.diff(c["graph"][0]))
    d2 = ((c["Y"][head] - c["Y"][c["graph"][1]]) ** 2).sum(1)
    assert ((d2 == 0) & (c["state"]["next"] <= 7)).any() and np.isfinite(c["Y32"]).all()


def test_quality_beats_the_pca_initialisation():
    x = uc.clusters300()
    Y = ref.umap_fit(x, UMAPParams(n_epochs=uc.EPOCHS300))
    t_umap, t_pca = uc.trust(x, Y), uc.trust(x, ref.pca_init(x))
    print(f"trustworthiness: umap {t_umap:.4f}, pca initialisation {t_pca:.4f}, range [{Y.min():.2f}, {Y.max():.2f}]")
    assert np.isfinite(Y).all() and Y.dtype == np.float32 and t_umap > t_pca


def test_limits():
    x = uc.clusters300()
    for bad in (UMAPParams(n_neighbors=1), UMAPParams(n_neighbors=65), UMAPParams(n_neighbors=300),
                UMAPParams(metric="manhattan"), UMAPParams(init="spectral")):
        with pytest.raises(ValueError):
            ref.umap_fit(x, bad)
    y = x.copy()
    y[0, 0] = np.nan
    with pytest.raises(ValueError):
        ref.umap_fit(y)
    with pytest.raises(ValueError):
        ref.check_umap_limits(2 ** 31 // 15, 15)


# ------------------------------------------------------------------------------------ projection modes
def _todays_pca(vecs, seed=42):
    """``project_2d``'s PCA branch as it stood before ``method`` existed."""
    x = torch.from_numpy(np.asarray(vecs, np.float32))
    x = x - x.mean(0, keepdim=True)
    torch.manual_seed(seed)
    _, _, V = torch.pca_lowrank(x, q=min(6, x.shape[1]), center=False)
    return (x @ V[:, :2]).cpu().numpy()


@pytest.fixture
def cpu_only(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(projection, "_have_umap_learn", lambda: False)


def test_project_2d_modes_on_a_cpu(cpu_only):
    x = uc.clusters300()[:60]
    c, m = projection.project_2d(x, method="pca")
    assert m == "pca" and np.array_equal(c, _todays_pca(x))
    c, m = projection.project_2d(x)
    assert m == "pca" and np.array_equal(c, _todays_pca(x))
    assert projection.resolve_method("umap") == ("umap", "numpy")
    with pytest.raises(ValueError):
        projection.project_2d(x, method="tsne")


def test_pca_cache_is_recomputed_when_umap_is_asked(cpu_only, tmp_path, monkeypatch):
    x = uc.clusters300()[:40]
    index = SimpleNamespace(ntotal=len(x), reconstruct_batch=lambda ids: x[np.asarray(ids)])
    cache = tmp_path / "umap_cache.npz"
    first = projection.compute_projection(index, None, cache, 100, method="auto")
    assert first["method"] == "pca" and first["engine"] == "pca"
    calls = []
    real = projection.project_2d_engine
    monkeypatch.setattr(projection, "project_2d_engine", lambda *a, **k: calls.append(a) or real(*a, **k))
    again = projection.compute_projection(index, None, cache, 100, method="pca")
    assert not calls and again["x"] == first["x"] and again["engine"] == "pca"
    monkeypatch.setattr(ref, "default_n_epochs", lambda n: 30)  # the oracle path, kept short
    forced = projection.compute_projection(index, None, cache, 100, method="umap")
    assert len(calls) == 1 and forced["method"] == "umap" and forced["engine"] == "numpy"
    assert str(np.load(cache)["method"]) == "umap" and str(np.load(cache)["engine"]) == "numpy"
    assert projection.compute_projection(index, None, cache, 100, method="umap")["x"] == forced["x"] and len(calls) == 1
    with pytest.raises(ValueError):
        projection.compute_projection(index, None, cache, 100, method="tsne")
