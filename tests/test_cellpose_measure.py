"""Per-cell measurements on the CPU: the oracle ``reference.measure_masks`` against hand literals,
``derive_measurements`` against closed forms, ``CellposeRunner.measure`` and the app's
``infer(return_measurements=True)``."""
import asyncio
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import cellpose_measure_cases as mc
from bioengine_worker_amd.cellpose import reference as ref

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"

pytestmark = pytest.mark.unit


def same_table(a: dict, b: dict) -> None:
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ------------------------------------------------------------------ oracle


def test_oracle_hand_literals():
    raw = ref.measure_masks(mc.HAND, mc.HAND_IMAGE, outlines=True)
    for k, want in mc.HAND_RAW.items():
        assert np.array_equal(raw[k], np.asarray(want)), k
    assert raw["area"].dtype == np.int64 and raw["bbox"].dtype == np.int32 and raw["boundary"].dtype == np.int64
    assert raw["int_sum"].dtype == np.float64 and raw["int_min"].dtype == np.float32
    assert raw["outlines"].dtype == bool and np.array_equal(raw["outlines"], mc.HAND_OUTLINES)
    assert "int_sum" not in ref.measure_masks(mc.HAND) and "outlines" not in ref.measure_masks(mc.HAND)


def test_oracle_edge_cases():
    empty = ref.measure_masks(np.zeros((4, 5), np.int32), np.ones((2, 4, 5), np.float32))
    assert empty["area"].shape == (0,) and empty["bbox"].shape == (0, 4) and empty["int_sum"].shape == (0, 2)
    t = ref.derive_measurements(empty)
    assert t["n_cells"] == 0 and t["diameter_px"] == 0.0 and t["centroid"].shape == (0, 2)
    # 3-D: one voxel in a Z = 1 volume has both z neighbours outside the array
    v = np.zeros((1, 3, 3), np.int32)
    v[0] = 1
    raw = ref.measure_masks(v)
    assert raw["boundary"].tolist() == [9] and raw["bbox"].tolist() == [[0, 0, 0, 1, 3, 3]] and "sum_yy" not in raw
    assert ref.measure_masks(v[0])["boundary"].tolist() == [8]  # the same plane as an image: its centre is interior
    with pytest.raises(ValueError):
        ref.measure_masks(np.zeros(5, np.int32))
    with pytest.raises(ValueError):
        ref.measure_masks(mc.HAND, np.zeros((1, 7, 8), np.float32))


def test_oracle_volume_fields():
    raw = mc.oracle("vol", "int")
    m = mc.masks("vol")
    assert raw["area"].tolist() == [int((m == l).sum()) for l in range(1, 6)] and raw["area"][3] == 0
    assert raw["bbox"][1, 0] == 0 and raw["bbox"][1, 3] == 5  # label 2 spans all planes
    zz = np.nonzero(m == 3)[0]
    assert raw["sum_z"][2] == zz.sum() and raw["bbox"][2, 0] == 3
    img = mc.image("vol", "int")
    assert raw["int_sum"][0, 1] == img[:, 1][m == 1].astype(np.float64).sum()
    assert raw["int_max"][4, 0] == img[:, 0][m == 5].max()


# ------------------------------------------------------------------ derived values


@pytest.mark.parametrize("a,b", [(4, 7), (7, 4), (5, 5), (1, 6)])
def test_derive_rectangle(a, b):
    m = np.zeros((12, 13), np.int32)
    m[3:3 + a, 2:2 + b] = 1
    t = ref.derive_measurements(ref.measure_masks(m))
    assert t["centroid"][0].tolist() == [3 + (a - 1) / 2, 2 + (b - 1) / 2]  # exact
    myy, mxx = (a * a - 1) / 12, (b * b - 1) / 12
    l1, l2 = max(myy, mxx), min(myy, mxx)
    assert t["axis_major"][0] == pytest.approx(4 * np.sqrt(l1), rel=1e-12)
    assert t["axis_minor"][0] == pytest.approx(4 * np.sqrt(l2), rel=1e-12, abs=1e-12)
    assert t["eccentricity"][0] == pytest.approx(np.sqrt(1 - l2 / l1), abs=1e-6)  # sqrt of a 1e-14 cancellation error
    if a != b:
        assert t["orientation"][0] == pytest.approx(0.0 if b > a else np.pi / 2, abs=1e-12)
    assert t["equivalent_diameter"][0] == pytest.approx(np.sqrt(4 * a * b / np.pi), rel=1e-15)
    assert t["area"][0] == a * b and t["boundary"][0] == (a * b - max(a - 2, 0) * max(b - 2, 0))
    assert t["n_cells"] == 1 and t["label"].tolist() == [1]


def test_derive_hand():
    t = ref.derive_measurements(ref.measure_masks(mc.HAND, mc.HAND_IMAGE))
    assert t["n_cells"] == 5 and t["label"].tolist() == [1, 2, 3, 4, 5, 6]
    # one pixel: no extent
    assert t["eccentricity"][0] == 0 and t["axis_major"][0] == 0 and t["axis_minor"][0] == 0
    assert t["centroid"][0].tolist() == [5.0, 4.0] and t["int_mean"][0, 0] == 54.0 and t["int_std"][0, 0] == 0.0
    # the absent label: zeros everywhere
    for k in ("area", "boundary", "axis_major", "axis_minor", "eccentricity", "orientation", "equivalent_diameter"):
        assert t[k][3] == 0, k
    assert not t["centroid"][3].any() and not t["bbox"][3].any() and t["int_mean"][3, 0] == 0
    # the ring has the moments of a 3 x 3 square minus its centre: isotropic
    assert t["axis_major"][2] == pytest.approx(t["axis_minor"][2]) and t["eccentricity"][2] == pytest.approx(0, abs=1e-6)
    assert t["int_mean"][4, 0] == 36.0
    assert t["int_std"][4, 0] == pytest.approx(np.std([10 * y + x for y in (2, 3, 4) for x in (5, 6, 7)]), rel=1e-12)
    areas = np.array([1, 3, 8, 9, 3.0])
    assert t["diameter_px"] == pytest.approx(np.median(np.sqrt(areas)) * 2 / np.sqrt(np.pi), rel=1e-15)


def test_diameter_equal_squares():
    m = np.zeros((40, 40), np.int32)
    for i in range(9):
        y, x = 2 + 12 * (i // 3), 2 + 12 * (i % 3)
        m[y:y + 10, x:x + 10] = i + 1
    t = ref.derive_measurements(ref.measure_masks(m))
    assert t["n_cells"] == 9 and t["diameter_px"] == pytest.approx(10 * 2 / np.sqrt(np.pi), rel=1e-15)
    assert np.allclose(t["equivalent_diameter"], t["diameter_px"], rtol=1e-15)


def test_derive_volume():
    t = ref.derive_measurements(mc.oracle("vol", "float"))
    m = mc.masks("vol")
    assert t["n_cells"] == 4 and "axis_major" not in t and t["centroid"].shape == (5, 3)
    assert np.allclose(t["centroid"][1], np.argwhere(m == 2).mean(0), rtol=1e-14)
    assert t["equivalent_diameter"][1] == pytest.approx(np.cbrt(6 * (m == 2).sum() / np.pi), rel=1e-15)
    v = mc.image("vol", "float")[:, 1][m == 2].astype(np.float64)
    assert t["int_mean"][1, 1] == pytest.approx(v.mean(), rel=1e-13) and t["int_std"][1, 1] == pytest.approx(v.std(), rel=1e-9)
    assert (t["int_max"][t["area"] > 0, 1] < 0).all() and (t["int_min"][t["area"] > 0, 0] > 0).all()


# ------------------------------------------------------------------ runner


@pytest.fixture(scope="module")
def cpu_runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpnet import CPnet

    return CellposeRunner(CPnet().randomize_(0), device="cpu")


def test_runner_measure_cpu(cpu_runner):
    m, img = mc.masks("ragged"), mc.image("ragged", "float")
    tabs = cpu_runner.measure(torch.from_numpy(m.copy()), img)
    assert isinstance(tabs, list) and len(tabs) == 3
    for b in range(3):
        same_table(tabs[b], ref.derive_measurements(ref.measure_masks(m[b], img[b])))
    assert [t["n_cells"] for t in tabs] == [5, 40, 0]
    # numpy masks, one image, one channel padded to the network's two (not normalised)
    one = cpu_runner.measure(m[0], img[0, 0])
    pad = np.stack([img[0, 0], np.zeros_like(img[0, 0])])
    same_table(one[0], ref.derive_measurements(ref.measure_masks(m[0], pad)))
    # geometry alone
    geo = cpu_runner.measure(m[1])[0]
    assert "int_mean" not in geo and np.array_equal(geo["area"], tabs[1]["area"])
    # a volume, planes first; channel-last stacks are read as eval_stack reads them
    vm, vi = mc.masks("vol"), mc.image("vol", "int")
    want = ref.derive_measurements(ref.measure_masks(vm, vi.transpose(1, 0, 2, 3)))
    same_table(cpu_runner.measure(vm, vi, volume=True), want)
    same_table(cpu_runner.measure(vm, np.ascontiguousarray(vi.transpose(0, 2, 3, 1)), volume=True), want)
    with pytest.raises(ValueError):
        cpu_runner.measure(m, img[:2])


def test_measure_wrapper_cpu_matches_oracle():
    """``gpu.measure_masks_gpu`` on CPU tensors runs the oracle; rows are padded to the batch maximum."""
    from bioengine_worker_amd.cellpose import gpu

    m, img = mc.masks("ragged"), mc.image("ragged", "int")
    res = gpu.measure_masks_gpu(torch.from_numpy(m.copy()), torch.from_numpy(img.copy()), outlines=True)
    assert res["area"].shape == (3, 40) and res["bbox"].shape == (3, 40, 4) and res["int_sum"].shape == (3, 40, 2)
    for b, o in enumerate(mc.oracle("ragged", "int")):
        k = o["area"].shape[0]
        for name, v in o.items():
            got = res[name][b].numpy()
            assert np.array_equal(got if name == "outlines" else got[:k], v), name
            assert name == "outlines" or not got[k:].any()
    with pytest.raises(ValueError, match="too large"):
        gpu.measure_masks_gpu(torch.zeros(1, dtype=torch.int32).expand(2048, 1024, 1024), volume=True)
    with pytest.raises(ValueError, match="too large"):
        gpu.measure_masks_gpu(torch.zeros(1, dtype=torch.int32).expand(1, 2 ** 15 + 1, 4))


# ------------------------------------------------------------------ app


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_measure_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


def test_app_return_measurements(app):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    imgs = synthetic_cells(2, 48, 56, ncells=6, seed=2)  # [2, 2, H, W] uint16
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}

    async def main():
        a = await app.infer(input_arrays=[imgs[0], imgs[1]], return_measurements=True, **kw)
        d = await app.infer({"input_arrays": [imgs[0]], "return_measurements": True, **kw})
        plain = await app.infer(input_arrays=[imgs[0]], **kw)
        j = await app.infer(input_arrays=[imgs[0]], return_measurements=True, json_safe=True, **kw)
        # one batch, only one request asks: the other gets nothing extra
        mixed = await asyncio.gather(app.infer(input_arrays=[imgs[0]], return_measurements=True, **kw),
                                     app.infer(input_arrays=[imgs[1]], **kw))
        return a, d, plain, j, mixed

    a, d, plain, j, mixed = asyncio.run(asyncio.wait_for(main(), 600))
    assert set(plain[0]) - {"weights"} == {"input_path", "output"}
    assert set(mixed[1][0]) - {"weights"} == {"input_path", "output"}
    for b, item in enumerate(a):
        t = item["measurements"]
        assert np.array_equal(item["output"], plain[0]["output"]) or b == 1
        assert t["n_cells"] == int(item["output"].max()) == t["area"].shape[0]
        assert item["diameter_px"] == t["diameter_px"]
        same_table(t, ref.derive_measurements(ref.measure_masks(item["output"], imgs[b].astype(np.float32))))
    assert a[0]["measurements"]["n_cells"] > 0  # the comparison above is not about empty tables
    same_table(d[0]["measurements"], a[0]["measurements"])
    same_table(mixed[0][0]["measurements"], a[0]["measurements"])
    tj = j[0]["measurements"]
    assert isinstance(tj["area"], list) and isinstance(tj["centroid"], list) and isinstance(tj["n_cells"], int)
    assert tj["area"] == a[0]["measurements"]["area"].tolist() and isinstance(j[0]["diameter_px"], float)
    assert not any(isinstance(v, np.ndarray) for v in tj.values())


def test_app_return_measurements_stacks(app):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    vol = np.ascontiguousarray(synthetic_cells(6, 20, 24, ncells=3, seed=1)[:, 0])  # [Z, H, W] uint16
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0, "return_measurements": True}

    async def main():
        s = await app.infer(input_arrays=[vol], stitch_threshold=0.25, **kw)
        v = await app.infer(input_arrays=[vol], do_3D=True, **kw)
        p = await app.infer(input_arrays=[vol], do_3D=True, model="cyto3", niter=20)
        return s, v, p

    s, v, p = asyncio.run(asyncio.wait_for(main(), 600))
    assert set(p[0]) - {"weights"} == {"input_path", "output"}
    pad = np.stack([vol.astype(np.float32), np.zeros(vol.shape, np.float32)])  # [C, Z, H, W], not normalised
    for item in (s[0], v[0]):
        t = item["measurements"]
        assert item["output"].shape == vol.shape and t["centroid"].shape[1] == 3
        assert t["n_cells"] == int(item["output"].max()) and item["diameter_px"] == t["diameter_px"]
        same_table(t, ref.derive_measurements(ref.measure_masks(item["output"], pad)))
