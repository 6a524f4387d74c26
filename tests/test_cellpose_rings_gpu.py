"""Cell outlines traced on the GPU: ``gpu.mask_rings_gpu`` (``csrc/kernels/cellpose_rings.hip``)
against the oracle ``reference.mask_rings`` on the cases of ``cellpose_rings_cases``: every array
exactly, dtypes included."""
import numpy as np
import pytest
import torch

import cellpose_rings_cases as rc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu

DTYPES = {"verts": torch.int32, "ring_offsets": torch.int64, "ring_label": torch.int32, "ring_area2": torch.int64,
          "ring_image": torch.int32, "image_rings": torch.int64}


def run(gpu, name, **kw):
    from bioengine_worker_amd.cellpose.gpu import mask_rings_gpu

    return mask_rings_gpu(torch.from_numpy(rc.masks(name).copy()).to(gpu), volume=name == "vol", **kw)


def same(got: dict, want: dict, what) -> None:
    assert set(got) == set(DTYPES), what
    for k, dt in DTYPES.items():
        g = got[k]
        assert g.device.type == "cuda" and g.dtype == dt, (what, k)
        assert g.shape == want[k].shape and np.array_equal(g.cpu().numpy(), want[k]), (what, k)


@pytest.mark.parametrize("name", rc.CASES)
def test_equals_oracle(gpu, name):
    same(run(gpu, name), rc.batch_oracle(name), name)


def test_hand_literals(gpu):
    res = {k: v.cpu().numpy() for k, v in run(gpu, "hand").items()}
    off = res["ring_offsets"]
    got = [(int(res["ring_label"][i]), [tuple(p) for p in res["verts"][off[i]:off[i + 1]].tolist()], int(res["ring_area2"][i]))
           for i in range(len(off) - 1)]
    assert got == rc.HAND_RINGS and res["image_rings"].tolist() == [0, 6] and not res["ring_image"].any()


def test_batch_with_an_empty_image(gpu):
    res = run(gpu, "ragged")
    per = res["image_rings"].tolist()
    assert len(per) == 4 and per[2] == per[3] == res["ring_label"].shape[0] > per[1] > 0
    assert res["ring_image"].unique().tolist() == [0, 1]
    vol = run(gpu, "vol")
    assert vol["image_rings"].shape == (6,) and vol["ring_image"].unique().tolist() == [0, 1, 2, 3, 4]  # z


@pytest.mark.parametrize("name", ("ragged", "big"))
def test_reproducible(gpu, name):
    a, b = run(gpu, name), run(gpu, name)
    for k in DTYPES:
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k


def test_nlab_above_and_below_maximum(gpu):
    same(run(gpu, "ragged", nlab=40 + 1 + 23), rc.batch_oracle("ragged"), "above")
    same(run(gpu, "vol", nlab=9), rc.batch_oracle("vol"), "vol above")
    # a bound below the true maximum: the labels above it are not traced, the rest are unchanged
    low = rc.join([ref.mask_rings(np.where(m > 10, 0, m)) for m in rc.masks("ragged")])
    same(run(gpu, "ragged", nlab=11), low, "below")
    # image 0 has labels 1..5 only and keeps all its rings; image 1 loses labels 11..40
    assert int(low["ring_label"].max()) == 10 and low["image_rings"][1] == rc.batch_oracle("ragged")["image_rings"][1]
    assert low["image_rings"][2] < rc.batch_oracle("ragged")["image_rings"][2]


def test_input_conversion(gpu):
    from bioengine_worker_amd.cellpose.gpu import mask_rings_gpu

    m = rc.masks("ragged")
    wide = torch.zeros(3, 45, 80, dtype=torch.int64, device=gpu)
    wide[:, :, :67] = torch.from_numpy(m.astype(np.int64)).to(gpu)
    same(mask_rings_gpu(wide[:, :, :67]), rc.batch_oracle("ragged"), "int64, not contiguous")


def test_empty_inputs_launch_nothing(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(cg._native, "call", no_launch)
    empty = {k: np.zeros((0, 2) if k == "verts" else 0, torch.empty(0, dtype=dt).numpy().dtype) for k, dt in DTYPES.items()}
    empty["ring_offsets"] = np.zeros(1, np.int64)
    for M, nlab in ((torch.zeros(2, 9, 11, dtype=torch.int32, device=gpu), None),   # all zero: K = 0
                    (torch.zeros(2, 9, 11, dtype=torch.int32, device=gpu), 1),
                    (torch.zeros(0, 9, 11, dtype=torch.int32, device=gpu), None),   # an empty batch
                    (torch.zeros(3, 0, 11, dtype=torch.int32, device=gpu), 5)):
        same(cg.mask_rings_gpu(M, nlab=nlab), dict(empty, image_rings=np.zeros(M.shape[0] + 1, np.int64)), tuple(M.shape))


def test_all_zero_under_a_bound(gpu, monkeypatch):
    """Labels bounded but absent: the count runs, V = 0 comes back and nothing is traced or read again."""
    from bioengine_worker_amd.cellpose import gpu as cg

    reads = []
    real = cg._host_ints
    monkeypatch.setattr(cg, "_host_ints", lambda t: reads.append(1) or real(t))
    res = cg.mask_rings_gpu(torch.zeros(2, 9, 11, dtype=torch.int32, device=gpu), nlab=7)
    assert res["verts"].shape == (0, 2) and res["image_rings"].tolist() == [0, 0, 0] and len(reads) == 1
    reads.clear()
    cg.mask_rings_gpu(torch.from_numpy(rc.masks("hand").copy()).to(gpu), nlab=7)
    assert len(reads) == 2  # V and R: never more


def test_bounds_raise_before_any_launch(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(cg._native, "call", no_launch)
    one = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="too large"):
        cg.mask_rings_gpu(one.expand(1, 2 ** 15 + 1, 8))
    with pytest.raises(ValueError, match="too large"):
        cg.mask_rings_gpu(one.expand(1, 8, 2 ** 15 + 1))
    with pytest.raises(ValueError, match="too large"):
        cg.mask_rings_gpu(one.expand(2048, 1023, 1023))  # B (H + 1)(W + 1) = 2^31
    with pytest.raises(ValueError, match="expects"):
        cg.mask_rings_gpu(one.expand(8, 8))


def test_error_word_raises(gpu, monkeypatch):
    """The wrapper's raise, without provoking the loop bound on the device: the error word that
    comes back with R is replaced on the host."""
    from bioengine_worker_amd.cellpose import gpu as cg

    real = cg._host_ints

    def flagged(t):
        v = real(t)
        return v if len(v) == 1 else [v[0], 1]

    monkeypatch.setattr(cg, "_host_ints", flagged)
    with pytest.raises(RuntimeError, match="be_cp_rings_trace"):
        cg.mask_rings_gpu(torch.from_numpy(rc.masks("hand").copy()).to(gpu))


# ------------------------------------------------------------------ end to end


def same_rings(got: dict, want: dict) -> None:
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_runner_eval_outlines(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, synthetic_cells

    runner = CellposeRunner(device=gpu)
    masks = runner.eval(synthetic_cells(2, 64, 64, ncells=8, seed=4), flow_threshold=0.0)[0]
    assert masks.is_cuda and masks.label_bound > int(masks.max()) > 0
    bounds = []
    real = cg.mask_rings_gpu
    monkeypatch.setattr(cg, "mask_rings_gpu", lambda M, nlab=None, volume=False: bounds.append(nlab) or real(M, nlab, volume))
    out = runner.outlines(masks)
    assert bounds == [masks.label_bound]  # the bound the mask stage left: no M.max() read
    m = masks.cpu().numpy()
    assert len(out) == 2
    for b in range(2):
        same_rings(out[b], ref.mask_rings(m[b]))
        assert np.array_equal(ref.rings_to_labels(out[b], m[b].shape), m[b])


def test_app_gpu_return_outlines(gpu, tmp_path, monkeypatch):
    """The serving path: traced on the copy stream from the masks on the device; a batch traces if
    any of its requests asks and only those get the field."""
    import asyncio
    import importlib.util
    from pathlib import Path

    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    main_py = Path(__file__).resolve().parents[1] / "apps" / "cellpose-finetuning" / "main.py"
    spec = importlib.util.spec_from_file_location("cellpose_main_rings_gpu_test", main_py)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    app = mod.CellposeFinetune.func_or_class(default_model="cyto3")
    imgs = synthetic_cells(3, 64, 64, ncells=8, seed=4)  # [3, 2, 64, 64] uint16
    kw = {"model": "cyto3", "flow_threshold": 0.0}

    async def main():
        return await asyncio.gather(app.infer(input_arrays=[imgs[0]], **kw),
                                    app.infer(input_arrays=[imgs[1]], return_outlines=True, outline_format="geojson", **kw),
                                    app.infer(input_arrays=[imgs[2]], **kw))

    a, b, c = asyncio.run(asyncio.wait_for(main(), 300))
    assert set(a[0]) - {"weights"} == set(c[0]) - {"weights"} == {"input_path", "output"}
    assert int(b[0]["output"].max()) > 0
    assert b[0]["outlines"] == ref.rings_to_geojson(ref.mask_rings(b[0]["output"]))
