"""Per-cell measurements on the GPU: ``gpu.measure_masks_gpu`` (``csrc/kernels/cellpose_measure.hip``)
against the oracle ``reference.measure_masks`` on the cases of ``cellpose_measure_cases``."""
import numpy as np
import pytest
import torch

import cellpose_measure_cases as mc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu

INT_FIELDS_2D = ("area", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy", "boundary")
INT_FIELDS_3D = ("area", "sum_z", "sum_y", "sum_x", "boundary")


def run(gpu, name, kind, **kw):
    from bioengine_worker_amd.cellpose.gpu import measure_masks_gpu

    M = torch.from_numpy(mc.masks(name).copy()).to(gpu)
    img = None if kind is None else torch.from_numpy(mc.image(name, kind).copy()).to(gpu)
    return measure_masks_gpu(M, img, volume=name in mc.CASES_3D, **kw)


def check_image(got: dict, want: dict, name: str, kind, b=None) -> None:
    """``got``: the rows of image ``b`` of a batch, or of the volume (``b`` None), as tensors with at
    least the oracle's K rows; exact in everything but the float field's fp64 sums, which must meet
    the summation bound."""
    volume = b is None
    k = want["area"].shape[0]
    fields = INT_FIELDS_3D if volume else INT_FIELDS_2D
    assert set(got) == set(want), (name, kind)
    for f in fields + ("bbox",) + (("int_min", "int_max") if kind else ()):
        g, w = got[f].cpu(), torch.from_numpy(want[f])
        assert g.dtype == w.dtype and g.shape[1:] == w.shape[1:], (name, kind, f)
        assert torch.equal(g[:k], w), (name, kind, f)
        assert not g[k:].any(), (name, kind, f, "rows above the image's own maximum must be zero")
    assert torch.equal(got["outlines"].cpu(), torch.from_numpy(want["outlines"])), (name, kind, "outlines")
    if not kind:
        return
    for f in ("int_sum", "int_sumsq"):
        g, w = got[f].cpu(), torch.from_numpy(want[f])
        assert g.dtype == torch.float64 and not g[k:].any()
        if kind == "int":  # integer-valued intensities: every partial sum is exact in float64
            assert torch.equal(g[:k], w), (name, kind, f)
    if kind == "float":
        # any summation order of n float64 terms is within (n - 1) u sum|x| of the true sum, u = 2^-53;
        # the kernel's and the oracle's orders differ, so they are within 2 (n - 1) u sum|x| < n 2^-52 sum|x|
        m = mc.masks(name) if volume else mc.masks(name)[b]
        img = mc.image(name, kind).astype(np.float64)
        for lab in range(1, k + 1):
            for c in range(img.shape[1]):
                x = (img[:, c] if volume else img[b, c])[m == lab]
                n = x.size
                for f, v in (("int_sum", x), ("int_sumsq", x * x)):
                    bound = n * 2.0 ** -52 * np.abs(v).sum()
                    d = abs(float(got[f][lab - 1, c]) - float(want[f][lab - 1, c]))
                    assert d <= bound, (name, f, lab, c, d, bound)


def check(res: dict, name: str, kind) -> None:
    want = mc.oracle(name, kind)
    if name in mc.CASES_3D:
        check_image(res, want, name, kind)
        return
    for b, w in enumerate(want):
        check_image({k: v[b] for k, v in res.items()}, w, name, kind, b)


@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("name", mc.CASES_2D + mc.CASES_3D)
def test_equals_oracle(gpu, name, kind):
    res = run(gpu, name, kind, outlines=True)
    k = max(int(mc.masks(name).max()), 0)
    lead = () if name in mc.CASES_3D else (mc.masks(name).shape[0],)
    assert res["area"].shape == lead + (k,) and res["int_sum"].shape == lead + (k, 2)
    assert res["bbox"].shape == lead + (k, 6 if name in mc.CASES_3D else 4)
    assert all(v.device.type == "cuda" for v in res.values())
    check(res, name, kind)


def test_hand_literals(gpu):
    from bioengine_worker_amd.cellpose.gpu import measure_masks_gpu

    res = measure_masks_gpu(torch.from_numpy(mc.HAND[None].copy()).to(gpu), torch.from_numpy(mc.HAND_IMAGE[None].copy()).to(gpu),
                            outlines=True)
    for f, want in mc.HAND_RAW.items():
        assert res[f][0].cpu().tolist() == want, f
    assert np.array_equal(res["outlines"][0].cpu().numpy(), mc.HAND_OUTLINES)


def test_big_sums_need_64_bits(gpu):
    res = run(gpu, "big", None)
    assert int(res["sum_yy"][0, 0]) == 300 * sum(y * y for y in range(300)) > 2 ** 31
    assert int(res["area"][0, 0]) == 90000 and int(res["boundary"][0, 0]) == 4 * 299
    assert res["bbox"][1, 0].tolist() == [0, 0, 300, 300]  # the spiral's box is the whole image


@pytest.mark.parametrize("name", ("big", "ragged"))
def test_reproducible(gpu, name):
    a = run(gpu, name, "float", outlines=True)
    b = run(gpu, name, "float", outlines=True)
    assert set(a) == set(b)
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k  # bit for bit, the fp64 sums included


@pytest.mark.parametrize("name", ("hand", "ragged", "vol"))
def test_null_image(gpu, name):
    res = run(gpu, name, None, outlines=True)
    assert not any(k.startswith("int_") for k in res)
    check(res, name, None)
    assert "outlines" not in run(gpu, name, None)


def test_volume_differs_from_planes(gpu):
    vol = run(gpu, "vol", "int", outlines=True)
    from bioengine_worker_amd.cellpose.gpu import measure_masks_gpu

    M = torch.from_numpy(mc.masks("vol").copy()).to(gpu)
    img = torch.from_numpy(mc.image("vol", "int").copy()).to(gpu)
    planes = measure_masks_gpu(M, img, outlines=True)  # the same array read as a batch of 5 images
    assert "sum_z" in vol and "sum_yy" not in vol and "sum_z" not in planes and "sum_yy" in planes
    assert torch.equal(planes["area"].sum(0), vol["area"]) and torch.equal(planes["int_sum"].sum(0), vol["int_sum"])
    # label 2 spans all planes: per plane only its rim is boundary, in the volume the two end planes are too
    assert int(planes["boundary"][:, 1].sum()) < int(vol["boundary"][1])
    assert int(vol["boundary"][1]) == int(planes["boundary"][1:4, 1].sum() + planes["area"][0, 1] + planes["area"][4, 1])
    assert not torch.equal(planes["outlines"], vol["outlines"])


def test_nlab_above_maximum(gpu):
    base = run(gpu, "ragged", "float", outlines=True)
    res = run(gpu, "ragged", "float", outlines=True, nlab=40 + 1 + 23)
    assert res["area"].shape == (3, 63) and res["int_min"].shape == (3, 63, 2)
    for k, v in res.items():
        if k == "outlines":
            assert torch.equal(v, base[k])
        else:
            assert torch.equal(v[:, :40], base[k]) and not v[:, 40:].any(), k
    vol = run(gpu, "vol", None, nlab=9)
    assert vol["area"].shape == (8,) and not vol["area"][5:].any() and not vol["bbox"][5:].any()
    # a bound below the true maximum: the labels above it are not measured, the rest are unchanged
    low = run(gpu, "ragged", "float", nlab=11)
    assert torch.equal(low["area"], base["area"][:, :10]) and torch.equal(low["int_sum"], base["int_sum"][:, :10])


def test_input_conversion_and_empty(gpu):
    from bioengine_worker_amd.cellpose.gpu import measure_masks_gpu

    m = mc.masks("ragged")
    want = run(gpu, "ragged", "int")
    M64 = torch.from_numpy(m.astype(np.int64)).to(gpu)
    wide = torch.zeros(3, 45, 80, dtype=torch.int64, device=gpu)
    wide[:, :, :67] = M64
    img = torch.from_numpy(mc.image("ragged", "int").copy()).to(gpu)
    res = measure_masks_gpu(wide[:, :, :67], img.double())  # int64 and not contiguous; float64 image
    for k in want:
        assert torch.equal(res[k], want[k]), k
    none = measure_masks_gpu(torch.zeros(2, 9, 11, dtype=torch.int32, device=gpu), torch.ones(2, 2, 9, 11, device=gpu),
                             outlines=True)
    assert none["area"].shape == (2, 0) and none["int_sum"].shape == (2, 0, 2) and not none["outlines"].any()


def test_bounds_raise_before_any_launch(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(cg._native, "call", no_launch)
    one = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="too large"):
        cg.measure_masks_gpu(one.expand(2048, 1024, 1024), volume=True)  # Z * H * W = 2^31
    with pytest.raises(ValueError, match="too large"):
        cg.measure_masks_gpu(one.expand(1, 2 ** 15 + 1, 8))  # the second moments need H, W <= 2^15
    with pytest.raises(ValueError, match="too large"):
        cg.measure_masks_gpu(one.expand(1, 8, 2 ** 15 + 1))


def test_many_channels(gpu):
    """More channels than one walk of the box takes (4): the second walk adds intensities only."""
    from bioengine_worker_amd.cellpose.gpu import measure_masks_gpu

    m = mc.masks("ragged")[1]
    rng = np.random.default_rng(3)
    img = rng.integers(0, 4096, (6,) + m.shape).astype(np.float32)
    want = ref.measure_masks(m, img)
    res = measure_masks_gpu(torch.from_numpy(m.copy()).to(gpu)[None], torch.from_numpy(img).to(gpu)[None])
    for k, v in want.items():
        assert torch.equal(res[k][0].cpu(), torch.from_numpy(v)), k


# ------------------------------------------------------------------ end to end


@pytest.fixture(scope="module")
def runner(gpu):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    return CellposeRunner(device=gpu)


def same_table(a: dict, b: dict) -> None:
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_runner_eval_measure(runner):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    x = synthetic_cells(2, 64, 64, ncells=8, seed=4)  # [2, 2, 64, 64] uint16: fp64 sums are exact
    masks = runner.eval(x, flow_threshold=0.0)[0]
    assert masks.is_cuda
    tabs = runner.measure(masks, x)
    m = masks.cpu().numpy()
    assert len(tabs) == 2
    for b in range(2):
        same_table(tabs[b], ref.derive_measurements(ref.measure_masks(m[b], x[b].astype(np.float32))))
        assert tabs[b]["n_cells"] == int(m[b].max())
    # the bound the mask stage leaves on its result plans the launch without reading M.max()
    from bioengine_worker_amd.cellpose.pipeline import EvalParams, measure_launch, measure_tables

    mm = runner.compute_masks(runner.eval(x, compute_masks=False)[1], EvalParams(flow_threshold=0.0))
    assert torch.equal(mm, masks) and mm.label_bound > int(mm.max()) > 0
    img = torch.from_numpy(x.astype(np.float32)).to(mm.device)
    for b, t in enumerate(measure_tables(measure_launch(mm, img, nlab=mm.label_bound))):
        same_table(t, tabs[b])


def test_runner_eval_3d_measure(runner):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    vol = np.ascontiguousarray(synthetic_cells(8, 32, 32, ncells=4, seed=5)[:, 0])  # [8, 32, 32] uint16
    masks = runner.eval_3d(vol)[0]
    tab = runner.measure(masks, vol, volume=True)
    pad = np.stack([vol.astype(np.float32), np.zeros(vol.shape, np.float32)])
    same_table(tab, ref.derive_measurements(ref.measure_masks(masks.cpu().numpy(), pad)))
    assert tab["n_cells"] == int(masks.max()) and tab["centroid"].shape[1] == 3


def test_app_gpu_return_measurements(gpu, tmp_path, monkeypatch):
    """The serving path: tables computed on the copy stream from the staged batch and the masks on the
    device, copied back with the masks; a batch measures if any of its requests asks."""
    import asyncio
    import importlib.util
    from pathlib import Path

    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    main_py = Path(__file__).resolve().parents[1] / "apps" / "cellpose-finetuning" / "main.py"
    spec = importlib.util.spec_from_file_location("cellpose_main_measure_gpu_test", main_py)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    app = mod.CellposeFinetune.func_or_class(default_model="cyto3")
    imgs = synthetic_cells(3, 64, 64, ncells=8, seed=4)  # [3, 2, 64, 64] uint16
    hwc = np.ascontiguousarray(imgs[2].transpose(1, 2, 0))  # staged channel-last, permuted on the device
    kw = {"model": "cyto3", "flow_threshold": 0.0}

    async def main():
        both = await asyncio.gather(app.infer(input_arrays=[imgs[0]], return_measurements=True, **kw),
                                    app.infer(input_arrays=[imgs[1]], **kw))
        many = await app.infer(input_arrays=[imgs[0], imgs[1], hwc], return_measurements=True, json_safe=False, **kw)
        vol = await app.infer(input_arrays=[np.ascontiguousarray(imgs[:, 0])], stitch_threshold=0.25,
                              return_measurements=True, **kw)
        return both, many, vol

    both, many, vol = asyncio.run(asyncio.wait_for(main(), 300))
    assert set(both[1][0]) - {"weights"} == {"input_path", "output"}
    for item, x in [(both[0][0], imgs[0])] + list(zip(many, imgs)):
        t = item["measurements"]
        assert t["n_cells"] == int(item["output"].max()) > 0 and item["diameter_px"] == t["diameter_px"]
        same_table(t, ref.derive_measurements(ref.measure_masks(item["output"], x.astype(np.float32))))
    pad = np.stack([imgs[:, 0].astype(np.float32), np.zeros(imgs[:, 0].shape, np.float32)])
    same_table(vol[0]["measurements"], ref.derive_measurements(ref.measure_masks(vol[0]["output"], pad)))
