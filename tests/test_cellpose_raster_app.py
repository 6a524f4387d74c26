"""The Cellpose app with polygon annotations: ``evaluate`` takes ``label_outlines`` as a keyword and
in the dict form and scores as with the rasterised label images; the outlines ``infer`` returns can
be handed straight back; ``start_training`` stores polygon labels as ``*_masks.geojson``.  Runs on
whatever device the app picks (the CPU without a GPU) with the random cyto3-architecture CPnet."""
import asyncio
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import cellpose_raster_cases as cases
from bioengine_worker_amd.cellpose import reference as ref

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"
KW = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_raster_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


def images():
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    return synthetic_cells(2, 48, 56, ncells=6, seed=2)  # [2, 2, H, W] uint16


def polygon_documents():
    """Fractional polygons on 48 x 56, one GeoJSON document and one 'rings' document."""
    gons = [cases.ngon(9, 12.3, 14.8, 8.2), cases.ngon(5, 30.4, 40.1, 9.7), cases.ngon(12, 33.6, 15.2, 7.9)]
    geo = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [g[:, ::-1].tolist() + [g[0, ::-1].tolist()]]}}
        for g in gons]}
    items = [{"label": k + 1, "rings": [g[:, ::-1].tolist()]} for k, g in enumerate(gons[:2])]
    return [geo, items]


def test_evaluate_with_label_outlines(app):
    imgs = images()
    docs = polygon_documents()
    labs = [ref.rasterize_rings(ref.outlines_to_rings(d), (48, 56)) for d in docs]
    assert [int(l.max()) for l in labs] == [3, 2]

    async def main():
        want = await app.evaluate(input_arrays=[imgs[0], imgs[1]], label_arrays=labs, **KW)
        kw = await app.evaluate(input_arrays=[imgs[0], imgs[1]], label_outlines=json.loads(json.dumps(docs)), **KW)
        dict_form = await app.evaluate({"input_arrays": [imgs[0], imgs[1]], "label_outlines": docs, **KW})
        return want, kw, dict_form

    want, kw, dict_form = asyncio.run(asyncio.wait_for(main(), 600))
    assert [it["n_true"] for it in want["per_image"]] == [3, 2]
    assert kw == want and dict_form == want


def test_infer_outlines_fed_back_to_evaluate(app):
    imgs = images()

    async def main():
        res = await app.infer(input_arrays=[imgs[0], imgs[1]], return_outlines=True, outline_format="geojson", **KW)
        rings = await app.infer(input_arrays=[imgs[0]], return_outlines=True, **KW)
        e = await app.evaluate(input_arrays=[imgs[0], imgs[1]], label_outlines=[it["outlines"] for it in res], **KW)
        e_rings = await app.evaluate(input_arrays=[imgs[0]], label_outlines=[rings[0]["outlines"]], **KW)
        return res, e, e_rings

    res, e, e_rings = asyncio.run(asyncio.wait_for(main(), 600))
    assert any(int(np.asarray(it["output"]).max()) > 0 for it in res)
    for it, score in zip(res, e["per_image"]):
        n = int(np.asarray(it["output"]).max())
        assert score["n_true"] == score["n_pred"] == n
        assert score["ap"] == ([1.0, 1.0, 1.0] if n else [None, None, None])
        assert score["fp"] == [0, 0, 0] and score["fn"] == [0, 0, 0]
    assert e_rings["per_image"][0] == e["per_image"][0]


def test_label_arrays_and_label_outlines_exclude_each_other(app):
    imgs = images()
    docs = polygon_documents()

    async def main():
        await app.evaluate(input_arrays=[imgs[0]], label_arrays=[np.zeros((48, 56), np.int32)], label_outlines=docs[:1], **KW)

    with pytest.raises(ValueError, match="not both"):
        asyncio.run(asyncio.wait_for(main(), 600))

    async def count():
        await app.evaluate(input_arrays=[imgs[0], imgs[1]], label_outlines=docs[:1], **KW)

    with pytest.raises(ValueError, match="2 images but 1"):
        asyncio.run(asyncio.wait_for(count(), 600))


def test_training_data_with_polygon_labels(app, tmp_path):
    """``_prepare_data`` stores polygon labels as ``*_masks.geojson`` and the session's loader
    rasterises them at the image's size; label arrays stay ``.npy``."""
    from bioengine_worker_amd.train.session import load_pairs

    sdir = tmp_path / "sessions" / "s1"  # the app keeps its sessions under $HOME, which the fixture set
    sdir.mkdir(parents=True)
    imgs = images()
    docs = polygon_documents()
    lab1 = ref.rasterize_rings(ref.outlines_to_rings(docs[1]), (48, 56))
    arrays = {"train_images": [imgs[0], imgs[1]], "train_labels": [docs[0], lab1], "test_images": [imgs[1]], "test_labels": [docs[1]]}
    asyncio.run(app._prepare_data("s1", {}, arrays))
    pairs = json.loads((sdir / "pairs.json").read_text())
    names = [Path(p["annotation"]).name for p in pairs["train"] + pairs["test"]]
    assert names == ["train_0000_masks.geojson", "train_0001_masks.npy", "test_0000_masks.geojson"]
    _, labs = load_pairs(pairs["train"] + pairs["test"], nchan=2)
    assert np.array_equal(labs[0], ref.rasterize_rings(ref.outlines_to_rings(docs[0]), (48, 56)))
    assert np.array_equal(labs[1], lab1) and np.array_equal(labs[2], lab1)
