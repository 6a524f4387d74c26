"""Polygon annotations rasterised on the GPU: ``gpu.rasterize_rings_gpu``
(``csrc/kernels/cellpose_raster.hip``) against the oracle ``reference.rasterize_rings`` on the cases
of ``cellpose_raster_cases``: every pixel exactly, dtype, device and ``label_bound`` included."""
import json

import numpy as np
import pytest
import torch

import cellpose_raster_cases as cases
import cellpose_rings_cases as rc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu


def run(gpu, name):
    from bioengine_worker_amd.cellpose.gpu import rasterize_rings_gpu

    p, (B, H, W) = cases.polys(name)
    return rasterize_rings_gpu(p, B, H, W, gpu)


@pytest.mark.parametrize("name", cases.CASES)
def test_equals_oracle(gpu, name):
    out = run(gpu, name)
    want = cases.oracle(name)
    assert out.device == gpu and out.dtype == torch.int32 and tuple(out.shape) == want.shape
    assert np.array_equal(out.cpu().numpy(), want)
    assert out.label_bound == int(np.asarray(cases.polys(name)[0]["ring_label"]).max()) + 1


@pytest.mark.parametrize("name", ("ragged", "gon"))
def test_reproducible(gpu, name):
    a, b = run(gpu, name), run(gpu, name)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("name", rc.CASES)
def test_round_trip_from_traced_rings(gpu, name):
    """``mask_rings_gpu`` -> ``rasterize_rings_gpu`` gives the masks back; the rings stay device
    tensors, which the wrapper copies to the host."""
    from bioengine_worker_amd.cellpose.gpu import mask_rings_gpu, rasterize_rings_gpu

    m = rc.masks(name)
    M = torch.from_numpy(m.copy()).to(gpu)
    rings = mask_rings_gpu(M, volume=name == "vol")
    assert rings["verts"].is_cuda
    out = rasterize_rings_gpu(rings, *m.shape, gpu)
    assert torch.equal(out, M.clamp(min=0)) and out.label_bound == int(m.max()) + 1
    del rings["ring_image"]  # the other form: image_rings alone
    assert torch.equal(rasterize_rings_gpu(rings, *m.shape, gpu), out)


def test_no_host_read(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    def no_read(*a, **k):
        raise AssertionError("a value was read back from the device")

    monkeypatch.setattr(cg, "_host_ints", no_read)
    monkeypatch.setattr(torch.Tensor, "item", no_read)
    monkeypatch.setattr(torch.Tensor, "tolist", no_read)
    monkeypatch.setattr(torch.Tensor, "cpu", no_read)
    p, (B, H, W) = cases.polys("bands")
    out = cg.rasterize_rings_gpu(p, B, H, W, gpu)
    monkeypatch.undo()
    assert np.array_equal(out.cpu().numpy(), cases.oracle("bands"))


def test_runs_on_the_current_stream(gpu):
    from bioengine_worker_amd.cellpose.gpu import rasterize_rings_gpu

    p, (B, H, W) = cases.polys("many")
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        out = rasterize_rings_gpu(p, B, H, W, gpu)
        total = (out > 0).sum()  # ordered after the kernel on the same stream
    side.synchronize()
    assert int(total) == int((cases.oracle("many") > 0).sum())


def test_empty_inputs_launch_nothing(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(cg._native, "call", no_launch)
    none = {"verts": np.zeros((0, 2)), "ring_offsets": np.zeros(1, np.int64), "ring_label": np.zeros(0, np.int32),
            "ring_image": np.zeros(0, np.int32)}
    p, (B, H, W) = cases.polys("overlap")
    hollow = {"verts": np.zeros((0, 2)), "ring_offsets": np.zeros(3, np.int64), "ring_label": np.asarray([4, 2], np.int32),
              "ring_image": np.zeros(2, np.int32)}  # R = 2, V = 0
    sliver, _ = cases.polys("sliver")
    thin = {k: (v[1:] if k in ("ring_label", "ring_image") else v) for k, v in sliver.items()}
    thin["verts"], thin["ring_offsets"] = sliver["verts"][6:], sliver["ring_offsets"][1:] - 6  # no centre inside
    for polys, shape, bound in ((none, (2, 9, 11), 1), (none, (0, 9, 11), 1), (hollow, (1, 9, 11), 5),
                                (dict(p, ring_image=np.zeros(0, np.int32), ring_label=p["ring_label"][:0],
                                      ring_offsets=np.zeros(1, np.int64), verts=p["verts"][:0]), (3, 0, 11), 1),
                                (thin, (1, 16, 16), 3)):
        out = cg.rasterize_rings_gpu(polys, *shape, gpu)
        assert out.device == gpu and out.dtype == torch.int32 and tuple(out.shape) == shape and out.label_bound == bound
        assert not out.any()


def test_invalid_inputs_raise_before_any_launch(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    calls = []
    monkeypatch.setattr(cg._native, "call", lambda *a, **k: calls.append(a[0]))
    for p, (B, H, W), match in cases.invalid_inputs():
        with pytest.raises(ValueError, match=match):
            cg.rasterize_rings_gpu(p, B, H, W, gpu)
    assert calls == []


# ------------------------------------------------------------------ end to end


def test_runner_score_with_outline_documents(gpu):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    runner = CellposeRunner(device=gpu)
    masks = rc.masks("ragged")
    docs = [json.loads(json.dumps(ref.rings_to_geojson(r))) for r in rc.oracle("ragged")]
    lab = runner.labels_from_outlines(docs, masks.shape[1:])
    assert lab.device == gpu and lab.label_bound == int(masks.max()) + 1 and np.array_equal(lab.cpu().numpy(), masks)
    pred = torch.from_numpy(np.roll(masks, 1, 2).copy()).to(gpu)
    a, b = runner.score(docs, pred), runner.score(masks.copy(), pred)
    assert set(a) == set(b)
    for k in ("ap", "tp", "fp", "fn", "n_true", "n_pred"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["summary"] == b["summary"] and int(a["tp"].sum()) > 0
    # the rasterised truth feeds the sibling stages with its bound: no max() read
    assert len(runner.outlines(lab)) == 3


def test_load_pairs_on_the_device(gpu, tmp_path):
    from bioengine_worker_amd.train.session import load_pairs

    p = cases.image_polys("edges", 0)
    off = p["ring_offsets"]
    doc = [{"label": int(l), "rings": [p["verts"][a:b, ::-1].tolist()]} for l, a, b in zip(p["ring_label"], off[:-1], off[1:])]
    (tmp_path / "a_mask.json").write_text(json.dumps(doc))
    np.save(tmp_path / "a.npy", np.zeros((60, 90), np.float32))
    imgs, labs = load_pairs([{"image": str(tmp_path / "a.npy"), "annotation": str(tmp_path / "a_mask.json")}], nchan=2, device=gpu)
    assert labs[0].dtype == np.int32 and np.array_equal(labs[0], cases.oracle("edges")[0])
