"""The in-house UMAP on the GPU (``search/umap.py``, ``csrc/kernels/umap.hip``) against the numpy oracle,
stage by stage, each stage fed the ORACLE's input.  The layout is chaotic (the float32 and float64 oracles
part by units within ten epochs), so positions are compared after ONE epoch only; the schedule state is
compared bit for bit."""
import numpy as np
import pytest
import torch

import umap_cases as uc
from bioengine_worker_amd.search import reference as ref
from bioengine_worker_amd.search import umap as gu

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _graph_t(g, dev):
    return _t(g[0], dev), _t(g[1], dev), _t(g[2], dev)


# -------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("n,d,k", [(131, 8, 5), (300, 32, 15)])
def test_knn_table(gpu, n, d, k):
    """Tolerance: an fp32 dot product of unit rows is off by at most d u (u = 2^-24, Cauchy-Schwarz on the
    running error bound), the fp32 normalisation of both rows and the final subtraction by a few u more:
    (d + 8) 2^-23 with the customary factor 2.  The sets are tie-free far beyond that (umap_cases.KNN_GAP)."""
    x = uc.tie_free(n, d, k)
    idx, dist = ref.knn_table(x, k)
    gi, gd = gu.knn_table_gpu(_t(x, gpu), k, budget=n * 50)  # several score blocks, the last one ragged
    assert gi.dtype == torch.int32 and gd.dtype == torch.float32
    err = np.abs(gd.cpu().numpy().astype(np.float64) - dist).max()
    print(f"kNN n={n}: largest distance error {err:.3e}")
    assert np.array_equal(gi.cpu().numpy(), idx)
    assert err <= (d + 8) * 2.0 ** -23


# ------------------------------------------------------------------------------- smooth-kNN, memberships
def _rel(a, b):
    """Largest |a - b| / |b| over the entries where b != 0; where b == 0, a must be 0 as well."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert (a[b == 0] == 0).all()
    nz = b != 0
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0


@pytest.mark.parametrize("name", ["n131", "n300", "hand5", "hand2"])
def test_smooth_knn_and_memberships(gpu, name):
    """rho bit for bit; sigma and the memberships within 4 x the oracle's own float32 / float64 difference on
    the same table, both taken relative to the float64 value rounded to float32 (the kernel's output format).
    The kernel bisects in fp64, so it sits far inside.  Measured on an MI355X, relative, float32 oracle /
    kernel: sigma n131 1.16e-5 / 0, n300 7.1e-6 / 0, hand5 1.3e-7 / 0, hand2 0 / 0; memberships n131 1.12e-5 / 0,
    n300 3.3e-5 / 0, hand5 5.7e-7 / 0, hand2 0 / 0 (k = 2 either stops at once or doubles sigma until the one
    term rounds to 1: both oracles and the kernel take the same steps)."""
    idx, dist = uc.table(name)
    r64, s64 = ref.smooth_knn(dist, np.float64)
    r32, s32 = ref.smooth_knn(dist, np.float32)
    a64, a32 = ref.memberships(idx, dist, r64, s64), ref.memberships(idx, dist, r32, s32)
    rho, sigma, memb = (t.cpu().numpy() for t in gu.smooth_knn_gpu(_t(idx, gpu), _t(dist, gpu)))
    s64f = s64.astype(np.float32)
    ys, ya = _rel(s32, s64f), _rel(a32, a64)
    gs, ga = _rel(sigma, s64f), _rel(memb, a64)
    print(f"{name}: sigma oracle f32/f64 {ys:.3e} kernel {gs:.3e}; memberships oracle {ya:.3e} kernel {ga:.3e}")
    assert np.array_equal(_bits(rho), _bits(r64.astype(np.float32)))
    assert gs <= 4 * ys and ga <= 4 * ya


# ------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize("name", ["n131", "c300", "hub"])
def test_graph(gpu, name):
    idx, dist = uc.table(name)
    want = uc.graph(name)
    w32 = ref.fuzzy_graph(idx, dist, uc.GRAPH_EPOCHS[name], np.float32)
    runs = [gu.fuzzy_graph_gpu(_t(idx, gpu), _t(dist, gpu), uc.GRAPH_EPOCHS[name]) for _ in range(2)]
    rp, col, w = (t.cpu().numpy() for t in runs[0])
    assert rp.dtype == np.int64 and col.dtype == np.int32 and w.dtype == np.float32
    assert np.array_equal(rp, want[0]) and np.array_equal(col, want[1])
    assert np.array_equal(w32[1], want[1])  # the float32 oracle keeps the same pairs: its weights line up
    yard, got = _rel(w32[2], want[2]), _rel(w, want[2])
    print(f"{name}: weights oracle f32/f64 {yard:.3e} kernel {got:.3e}, {col.size} directed edges")
    assert got <= 4 * yard
    n = rp.size - 1
    head = np.repeat(np.arange(n), np.diff(rp))
    key = head * n + col
    back = np.searchsorted(key, col.astype(np.int64) * n + head)
    assert np.array_equal(_bits(w)[back], _bits(w))  # bitwise symmetric
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    if name == "hub":
        assert rp[1] - rp[0] > 64


# ---------------------------------------------------------------------------------- one epoch, teacher-forced
def _run_step(case, dev):
    g = _graph_t(case["graph"], dev)
    st = {k: _t(v, dev) for k, v in case["state"].items()}
    Yin = _t(case["Y"], dev)
    Yout = torch.full_like(Yin, float("nan"))
    gu.layout_epoch_gpu(Yin, Yout, g, st, case["ep"], case["n_epochs"], case["a"], case["b"], case["seed"])
    torch.cuda.synchronize()
    assert torch.equal(Yin, _t(case["Y"], dev))  # the input buffer is read only
    return Yout.cpu().numpy(), st["next"].cpu().numpy(), st["nneg"].cpu().numpy()


def _check_step(case, dev, label):
    Y, nxt, nneg = _run_step(case, dev)
    tol = uc.y_tolerance(case)
    err = float(np.abs(Y.astype(np.float64) - case["Y64"]).max())
    moved = float(np.abs(case["Y64"] - case["Y"]).max())
    print(f"{label}: |Y - f64 oracle| {err:.3e}, tolerance {tol:.3e}, largest move {moved:.3e}, "
          f"active {(case['state']['next'] <= case['ep']).sum()}, max m {case['m'].max()}")
    assert np.array_equal(_bits(nxt), _bits(case["next"])), "activity"
    assert np.array_equal(_bits(nneg), _bits(case["nneg"])), "sample counts"
    assert np.isfinite(Y).all() and err <= tol


@pytest.mark.parametrize("name", ["c300", "hub"])
def test_one_epoch(gpu, name):
    for ep in uc.epoch_list(name):
        _check_step(uc.step_case(name, ep), gpu, f"{name} ep {ep}")


def test_one_epoch_coincident_vertices(gpu):
    _check_step(uc.step_case("c300", 7, uc.SEED, "coincident"), gpu, "coincident")


@pytest.mark.parametrize("name", ["c300", "hub"])
def test_one_epoch_negative_sample_hits_its_own_head(gpu, name):
    seed = uc.self_hit_seed(name, 1)
    _check_step(uc.step_case(name, 1, seed), gpu, f"{name} self-hit seed {seed}")


def test_layout_loop_equals_single_epochs(gpu):
    """``be_umap_layout`` over epochs 0..8 gives the bits of nine ``be_umap_epoch`` calls."""
    g = _graph_t(uc.graph("c300"), gpu)
    a, b = uc.ab()
    Y = _t(uc.start_positions("c300"), gpu)
    st = gu.layout_state_gpu(g[2])
    Yl = gu.layout_gpu(Y.clone(), g, {k: v.clone() for k, v in st.items()}, 200, a, b, uc.SEED, ep1=9)
    cur, nxt = Y.clone(), torch.empty_like(Y)
    for ep in range(9):
        gu.layout_epoch_gpu(cur, nxt, g, st, ep, 200, a, b, uc.SEED)
        cur, nxt = nxt, cur
    assert torch.equal(Yl, cur) and not torch.equal(cur, Y)


# --------------------------------------------------------------------------------- whole fit, application
@pytest.fixture(scope="module")
def fit300(gpu):
    x = uc.clusters300()
    p = gu.UMAPParams(n_epochs=uc.EPOCHS300)
    return x, [gu.umap_fit_gpu(_t(x, gpu), p) for _ in range(2)]


def test_fit_is_deterministic(fit300):
    _, ((Y1, i1), (Y2, i2)) = fit300
    assert torch.equal(Y1, Y2) and i1["n_edges"] == i2["n_edges"]
    assert Y1.dtype == torch.float32 and Y1.shape == (300, 2) and Y1.is_cuda
    assert i1["n_epochs"] == uc.EPOCHS300 and i1["degree_max"] >= i1["degree_median"] > 0
    assert abs(i1["a"] - 1.57694346) < 1e-6 and set(i1["spans_ms"]) == {"knn", "smooth_knn", "graph", "init", "layout"}


def test_fit_quality(fit300):
    """The GPU run is one more sample of the same chaotic process as the float32 oracle under seeds 0..5: its
    trustworthiness may fall below their lowest by one seed-to-seed spread, and must beat the PCA start."""
    x, ((Y, _), _) = fit300
    Y = Y.cpu().numpy()
    assert np.isfinite(Y).all()
    ts = [uc.trust(x, ref.umap_fit(x, gu.UMAPParams(n_epochs=uc.EPOCHS300, seed=s))) for s in range(6)]
    lo, hi = min(ts), max(ts)
    t_gpu, t_pca = uc.trust(x, Y), uc.trust(x, ref.pca_init(x))
    print(f"trustworthiness: gpu {t_gpu:.4f}, oracle seeds 0-5 [{lo:.4f}, {hi:.4f}], pca initialisation {t_pca:.4f}, "
          f"range [{Y.min():.2f}, {Y.max():.2f}]")
    assert t_gpu >= lo - (hi - lo) and t_gpu > t_pca


def test_limits_raise_before_any_launch(gpu):
    x = _t(uc.clusters300(), gpu)
    for bad in (gu.UMAPParams(n_neighbors=1), gu.UMAPParams(n_neighbors=65), gu.UMAPParams(n_neighbors=300)):
        with pytest.raises(ValueError):
            gu.umap_fit_gpu(x, bad)
    y = x.clone()
    y[5, 3] = float("inf")
    with pytest.raises(ValueError):
        gu.umap_fit_gpu(y)


def test_compute_projection_auto_runs_the_hip_umap(gpu, tmp_path, monkeypatch):
    from types import SimpleNamespace

    from bioengine_worker_amd.search import projection

    monkeypatch.setattr(projection, "_have_umap_learn", lambda: False)
    monkeypatch.setattr(ref, "default_n_epochs", lambda n: 100)
    x = uc.clusters300()
    index = SimpleNamespace(ntotal=len(x), reconstruct_batch=lambda ids: x[np.asarray(ids)])
    cache = tmp_path / "umap_cache.npz"
    np.savez(cache, x=np.zeros(300), y=np.zeros(300), labels=np.array(["a"] * 300), colors=np.array(["#000000"] * 300),
             n_total=np.array(300), idx=np.arange(300), method=np.array("pca"))  # the cache of a GPU-less life
    out = projection.compute_projection(index, None, cache, 1000, method="auto")
    assert out["method"] == "umap" and out["engine"] == "hip" and len(out["x"]) == 300
    assert np.isfinite(out["x"]).all() and np.ptp(out["x"]) > 1
    assert str(np.load(cache)["engine"]) == "hip"
    pca = projection.compute_projection(index, None, cache, 1000, method="pca")
    assert pca["method"] == "pca" and pca["engine"] == "pca"
