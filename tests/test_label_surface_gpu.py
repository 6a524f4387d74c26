"""Label surfaces built on the GPU: ``gpu.label_surface_gpu`` / ``gpu.surface_stats_gpu``
(``csrc/kernels/label_surface.hip``) against the oracle ``reference.label_surface`` /
``surface_stats`` on the cases of ``label_surface_cases``: every array exactly (``verts`` as bits),
dtypes included; the fp64 sums to 1e-9 and bit-identical from run to run."""
import numpy as np
import pytest
import torch

import label_surface_cases as sc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu

DTYPES = {"corner": torch.int32, "verts": torch.float32, "vert_label": torch.int32, "quads": torch.int32,
          "quad_label": torch.int32, "label_verts": torch.int64, "label_quads": torch.int64, "faces": torch.int64,
          "voxels": torch.int64}
STATS = ("label", "area_voxel", "area", "mesh_volume", "volume", "sphericity", "n_verts", "n_quads")


def run(gpu, name, **kw):
    from bioengine_worker_amd.cellpose.gpu import label_surface_gpu

    kw.setdefault("nlab", sc.nlab(name))
    return label_surface_gpu(torch.from_numpy(sc.volume(name).copy()).to(gpu), **kw)


def same(got: dict, want: dict, what) -> None:
    assert set(got) == set(DTYPES), what
    for k, dt in DTYPES.items():
        g = got[k]
        assert g.device.type == "cuda" and g.dtype == dt, (what, k)
        assert tuple(g.shape) == want[k].shape, (what, k, tuple(g.shape), want[k].shape)
        assert g.cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k)


def same_stats(got: dict, want: dict, what) -> None:
    """``area`` and ``mesh_volume``: the terms are O(1) (O(spacing^2), O(spacing^3) when scaled) and
    F < 10^5, so summation order moves the sums by about F 2^-53 ~ 1e-11 relative; 1e-9 leaves room
    for FMA contraction in the cross products.  Absolute where the oracle's value is 0."""
    assert tuple(got) == STATS == tuple(want), what
    for k in STATS:
        g = got[k]
        assert g.device.type == "cuda" and g.dtype == torch.float64 and tuple(g.shape) == want[k].shape, (what, k)
        g = g.cpu().numpy()
        if k in ("area", "mesh_volume", "sphericity"):
            w = want[k]
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
            ok = ~np.isnan(w)
            err = np.abs(g[ok] - w[ok])
            bound = np.where(w[ok] == 0, 1e-9, 1e-9 * np.abs(w[ok]))
            assert (err <= bound).all(), (what, k, float(err.max(initial=0)))
        else:
            assert np.array_equal(g, want[k]), (what, k)


@pytest.mark.parametrize("name", sc.CASES)
def test_equals_oracle(gpu, name):
    same(run(gpu, name), sc.oracle(name), name)


@pytest.mark.parametrize("name", sc.CASES)
@pytest.mark.parametrize("spacing", ((1.0, 1.0, 1.0), (2.5, 1.0, 0.5)))
def test_stats_equal_oracle(gpu, name, spacing):
    from bioengine_worker_amd.cellpose.gpu import surface_stats_gpu

    same_stats(surface_stats_gpu(run(gpu, name), spacing), sc.stats(name, spacing), (name, spacing))


def test_literals(gpu):
    from bioengine_worker_amd.cellpose.gpu import surface_stats_gpu

    s = run(gpu, "single")
    assert s["quads"].shape == (6, 4) and s["verts"].shape == (8, 3)
    assert float(surface_stats_gpu(s)["area"][0]) == pytest.approx(6 / 9, rel=1e-6)
    d = run(gpu, "diag")
    assert d["quads"].shape[0] == 18 and d["verts"].shape[0] == 23 and d["voxels"].tolist() == [2, 1]
    b = run(gpu, "ball10")
    assert (b["quads"].shape[0], b["verts"].shape[0]) == sc.BALL_COUNTS["ball10"]
    ratio = float(surface_stats_gpu(b)["area"][0]) / (4 * np.pi * 100)
    assert abs(ratio - sc.BALL_RATIO["ball10"]) < 1e-5


@pytest.mark.parametrize("name", ("cells", "tall"))
def test_reproducible(gpu, name):
    from bioengine_worker_amd.cellpose.gpu import surface_stats_gpu

    runs = []
    for _ in range(2):
        s = run(gpu, name)
        runs.append({**s, **{"stats_" + k: v for k, v in surface_stats_gpu(s, (2.5, 1.0, 0.5)).items()}})
    a, b = runs
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k


def test_nlab_above_and_below_maximum(gpu):
    same(run(gpu, "cells", nlab=None), sc.oracle("cells", None), "the maximum")  # K = 12
    same(run(gpu, "cells", nlab=20), sc.oracle("cells", 20), "above")
    same(run(gpu, "cells", nlab=6), sc.oracle("cells", 6), "below")
    low = sc.oracle("cells", 6)
    assert int(low["quad_label"].max()) == 5 and low["faces"].shape == (5, 3)
    # labels above the bound still bound their neighbours: the kept labels' meshes do not change
    n = low["quads"].shape[0]
    assert np.array_equal(sc.oracle("cells")["quads"][:n], low["quads"])


def test_input_conversion(gpu):
    from bioengine_worker_amd.cellpose.gpu import label_surface_gpu

    L = sc.volume("cells")
    want = sc.oracle("cells")
    same(label_surface_gpu(torch.from_numpy(L.astype(np.int64)).to(gpu), nlab=12), want, "int64")
    same(label_surface_gpu(torch.from_numpy(L.astype(np.uint16)).to(gpu), nlab=12), want, "uint16")
    same(label_surface_gpu(torch.from_numpy(L.astype(np.uint8)).to(gpu), nlab=12), want, "uint8")
    wide = torch.zeros(12, 37, 80, dtype=torch.int64, device=gpu)
    wide[:, :, :70] = torch.from_numpy(L.astype(np.int64)).to(gpu)
    same(label_surface_gpu(wide[:, :, :70], nlab=12), want, "int64, not contiguous")
    zyx = torch.from_numpy(np.ascontiguousarray(L.transpose(2, 1, 0))).to(gpu).permute(2, 1, 0)
    same(label_surface_gpu(zyx, nlab=12), want, "a permuted view")


def test_labels_beyond_int32_do_not_wrap(gpu):
    """int64 labels at or above 2^31 are never meshed (K stays below 2^31 - 1) but bound their
    neighbours, as in the oracle: 2^32 + 1 must not turn into label 1 on the way to the int32 kernels."""
    from bioengine_worker_amd.cellpose.gpu import label_surface_gpu

    L = sc.volume("cells").astype(np.int64)
    L[L == 12] = 2 ** 32 + 1
    L[L == 3] = 2 ** 31
    L[0, 0, 0] = -(2 ** 32) + 2  # would wrap to 2
    want = ref.label_surface(L, 12)
    assert want["voxels"][2] == 0 and want["voxels"][0] == (L == 1).sum()
    same(label_surface_gpu(torch.from_numpy(L).to(gpu), nlab=12), want, "int64 beyond 2^31")
    with pytest.raises(ValueError, match="too large"):
        label_surface_gpu(torch.from_numpy(L).to(gpu), nlab=2 ** 31 + 1)


def test_empty_inputs_launch_nothing(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    def no_read(t):
        raise AssertionError("a value was read back")

    monkeypatch.setattr(cg._native, "call", no_launch)
    monkeypatch.setattr(cg, "_host_ints", no_read)
    for L, nlab, K in ((torch.zeros(0, 9, 11, dtype=torch.int32, device=gpu), None, 0),
                       (torch.zeros(3, 0, 11, dtype=torch.int32, device=gpu), 5, 4),
                       (torch.ones(3, 4, 5, dtype=torch.int32, device=gpu), 1, 0),   # labels present, K = 0
                       (torch.ones(3, 4, 5, dtype=torch.int32, device=gpu), 0, 0)):
        same(cg.label_surface_gpu(L, nlab=nlab), ref._empty_surface(K), (tuple(L.shape), nlab))
    monkeypatch.undo()
    monkeypatch.setattr(cg._native, "call", no_launch)
    same(cg.label_surface_gpu(torch.zeros(3, 4, 5, dtype=torch.int32, device=gpu)), ref._empty_surface(0), "all zero")
    # the statistics of an empty mesh launch nothing either
    st = cg.surface_stats_gpu(cg.label_surface_gpu(torch.zeros(3, 0, 11, dtype=torch.int32, device=gpu), nlab=5))
    assert all(st[k].shape == (4,) for k in STATS) and st["sphericity"].isnan().all() and not st["area"].any()


def test_all_zero_under_a_bound(gpu, monkeypatch):
    """Labels bounded but absent: the count runs, V = F = 0 comes back and nothing else is launched."""
    from bioengine_worker_amd.cellpose import gpu as cg

    calls, reads = [], []
    real_call, real_read = cg._native.call, cg._host_ints
    monkeypatch.setattr(cg._native, "call", lambda name, *a: calls.append(name) or real_call(name, *a))
    monkeypatch.setattr(cg, "_host_ints", lambda t: reads.append(1) or real_read(t))
    same(cg.label_surface_gpu(torch.zeros(3, 4, 5, dtype=torch.int32, device=gpu), nlab=7), ref._empty_surface(6), "zeros")
    assert calls == ["be_surf_count"] and len(reads) == 1
    calls.clear(), reads.clear()
    run(gpu, "diag", nlab=3)
    assert calls == ["be_surf_count", "be_surf_emit", "be_surf_gather", "be_surf_remap", "be_surf_faces"] and len(reads) == 2


def test_bounds_raise_before_any_launch(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(cg._native, "call", no_launch)
    one = torch.zeros(1, dtype=torch.int32, device=gpu)
    for shape in ((2 ** 15 + 1, 2, 2), (2, 2 ** 15 + 1, 2), (2, 2, 2 ** 15 + 1), (2047, 1023, 1023)):
        with pytest.raises(ValueError, match="too large"):
            cg.label_surface_gpu(one.expand(*shape), nlab=2)
    with pytest.raises(ValueError, match="expects"):
        cg.label_surface_gpu(one.expand(8, 8), nlab=2)
    with pytest.raises(ValueError, match="integer"):
        cg.label_surface_gpu(torch.zeros(2, 2, 2, device=gpu), nlab=2)
    with pytest.raises(ValueError, match="spacing"):
        cg.surface_stats_gpu({}, (1.0, 0.0, 1.0))


def test_error_word_and_totals_raise(gpu, monkeypatch):
    """The wrapper's raises, without provoking a mismatch on the device: the values that come back
    are replaced on the host."""
    from bioengine_worker_amd.cellpose import gpu as cg

    real = cg._host_ints
    monkeypatch.setattr(cg, "_host_ints", lambda t: [1] if t.numel() == 1 else real(t))
    with pytest.raises(RuntimeError, match="labels changed"):
        run(gpu, "diag")
    monkeypatch.setattr(cg, "_host_ints", lambda t: [2 ** 31, 5] if t.numel() == 2 else real(t))
    with pytest.raises(RuntimeError, match="32-bit"):
        run(gpu, "diag")


def test_runner_surfaces_uses_label_bound(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    runner = CellposeRunner(device=gpu)
    masks = torch.from_numpy(sc.volume("cells").copy()).to(gpu)
    masks.label_bound = 12  # as compute_masks3d_gpu / stitch3d_gpu leave it: labels + 1 never exceed it
    bounds = []
    real = cg.label_surface_gpu
    monkeypatch.setattr(cg, "label_surface_gpu", lambda L, nlab=None: bounds.append(nlab) or real(L, nlab))
    monkeypatch.setattr(torch.Tensor, "max", lambda *a, **k: (_ for _ in ()).throw(AssertionError("max() was read")))
    out = runner.surfaces(masks, spacing=(2.5, 1.0, 0.5))
    monkeypatch.undo()
    assert bounds == [12]
    want = sc.oracle("cells")
    assert set(out) == {"mesh", "stats"} and set(out["mesh"]) == set(DTYPES)
    for k in DTYPES:
        assert out["mesh"][k].dtype == want[k].dtype and out["mesh"][k].tobytes() == want[k].tobytes(), k
    st = sc.stats("cells", (2.5, 1.0, 0.5))
    assert np.allclose(out["stats"]["area"], st["area"], rtol=1e-9) and np.array_equal(out["stats"]["volume"], st["volume"])
    with pytest.raises(ValueError, match="spacing"):
        runner.surfaces(masks, spacing=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="expects"):
        runner.surfaces(masks[0])
    # host arrays run the oracle
    cpu = runner.surfaces(sc.volume("cells").copy(), nlab=12)
    assert cpu["mesh"]["verts"].tobytes() == want["verts"].tobytes()
