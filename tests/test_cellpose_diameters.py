"""Per-image and automatic ``diameter`` of ``CellposeRunner.eval`` on the CPU oracle path, the oracle
additions they are checked with (``resize_bilinear_ref``, ``scaled_tiles``), and the app's batching of
requests that differ in their diameter."""
import asyncio
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bioengine_worker_amd.cellpose import reference as ref

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"

RESIZE_SIZES = [(65, 94), (74, 106), (111, 200), (37, 60), (64, 40), (20, 100), (9, 13), (38, 54), (37, 53)]


@pytest.mark.unit
@pytest.mark.parametrize("size", RESIZE_SIZES)
def test_resize_bilinear_ref_is_interpolate(size):
    """float32: the taps and weights are those of ``F.interpolate(align_corners=False)`` on the CPU and
    the values equal it up to the association of the sums, which torch's CPU kernel leaves to its
    compiler (at most four units in the last place of the largest pixel; bit for bit at sizes where
    its kernel fuses as the oracle does).  float64 stays within float32 rounding of both."""
    x = torch.rand(2, 3, 37, 53, generator=torch.Generator().manual_seed(sum(size))) * 100
    want = F.interpolate(x, size=size, mode="bilinear", align_corners=False).numpy()
    got = ref.resize_bilinear_ref(x.numpy(), size)
    assert got.dtype == np.float32 and got.shape == want.shape
    ulp = float(np.spacing(np.float32(100.0)))
    diff = float(np.abs(got - want).max())
    print(f"resize_bilinear_ref {size}: largest difference to F.interpolate {diff:.3e} (bound {4 * ulp:.3e})")
    assert diff <= 4 * ulp
    if size in ((65, 94), (74, 106), (111, 200), (37, 60), (37, 53)):
        assert np.array_equal(got, want)
    g64 = ref.resize_bilinear_ref(x.numpy(), size, np.float64)
    assert g64.dtype == np.float64 and float(np.abs(g64 - want).max()) < 1e-3


@pytest.mark.unit
@pytest.mark.parametrize("augment", [False, True])
def test_scaled_tiles_is_resize_pad_tile(augment):
    img = np.random.default_rng(0).uniform(0, 1, (2, 40, 52)).astype(np.float32)
    for r in (None, 2.0, 0.5, 30 / 17):
        Hs, Ws = ref.scaled_size(40, r), ref.scaled_size(52, r)
        assert (Hs, Ws) == ((40, 52) if r is None else (max(8, int(round(40 * r))), max(8, int(round(52 * r)))))
        xs = img if r is None else ref.resize_bilinear_ref(img, (Hs, Ws))
        ya, yb = ref.pad_amounts(Hs)
        xa, xb = ref.pad_amounts(Ws)
        want = ref.make_tiles(np.pad(xs, ((0, 0), (ya, yb), (xa, xb))), 32, 0.1, augment=augment)
        got = ref.scaled_tiles(img, r, 32, 0.1, augment)
        assert len(got) == len(want) and np.array_equal(got[0], want[0]) and list(got[1:]) == list(want[1:])
    assert ref.scaled_size(20, 0.1) == 8
    assert ref.scaled_tiles(img, 0.5, 32, dtype=np.float64)[0].dtype == np.float64


@pytest.fixture(scope="module")
def cpu_runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpnet import CPnet

    return CellposeRunner(CPnet().randomize_(0), device="cpu")


@pytest.mark.unit
def test_sequence_diameter_equals_scalar_calls(cpu_runner):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    x = synthetic_cells(4, 48, 64, ncells=6, seed=3)
    diams = [15, None, 60.0, 0]
    m, y, s = cpu_runner.eval(x, diameter=diams, niter=0)
    assert m.shape == (4, 48, 64) and y.shape == (4, 3, 48, 64)
    assert m.diameters.dtype == torch.float32 and m.diameters.tolist() == [15.0, 0.0, 60.0, 0.0]
    for b, d in enumerate(diams):
        mb, yb, sb = cpu_runner.eval(x[b: b + 1], diameter=d, niter=0)
        assert torch.equal(m[b: b + 1], mb) and torch.equal(y[b: b + 1], yb) and torch.equal(s[b: b + 1], sb)
        assert not hasattr(mb, "diameters")  # the scalar form is today's code path
    # tensors and arrays are sequences too; nan and entries inside the 1e-3 band are "no rescale"
    m2, y2, _ = cpu_runner.eval(x, diameter=torch.tensor([15.0, float("nan"), 60.0, 30 / 1.0005]), niter=0)
    assert torch.equal(m2, m) and torch.equal(y2, y) and m2.diameters.tolist() == [15.0, 0.0, 60.0, 0.0]
    # with niter unset the images run in groups that share int(200 / r_b): here 100, 200 and 400
    assert [int(200 / r) for r in (2.0, 1.0, 0.5)] == [100, 200, 400]
    for bad in ([15, 30], [15] * 5, np.array([[15.0] * 4])):
        with pytest.raises(ValueError, match="diameter"):
            cpu_runner.eval(x, diameter=bad)
    with pytest.raises(ValueError, match="diameter"):
        cpu_runner.eval(x, diameter="largest")


@pytest.mark.unit
@pytest.mark.parametrize("diameter", [[15.0, 30.0, 15.0], "auto", np.array([15.0, 30.0, 15.0])])
def test_stacks_and_volumes_take_a_scalar_only(cpu_runner, diameter):
    vol = np.zeros((3, 32, 32), np.float32)
    for fn in (cpu_runner.eval_stack, cpu_runner.eval_3d):
        with pytest.raises(ValueError, match="scalar diameter"):
            fn(vol, diameter=diameter)


def _disks(H, W, centres, r2):
    yy, xx = np.mgrid[0:H, 0:W]
    M = np.zeros((H, W), np.int32)
    for k, (cy, cx) in enumerate(centres):
        M[(yy - cy) ** 2 + (xx - cx) ** 2 <= r2] = k + 1
    return M


@pytest.mark.unit
def test_auto_diameter_with_a_standin_network(cpu_runner, monkeypatch):
    """Three 96 x 96 images: disks of diameter ~15, disks of diameter ~30 and nothing.  The stand-in
    network serves the oracle's flows of the disks of the image it is shown (channel 1 of the image
    carries the image's number), resized to the size it is asked for."""
    from bioengine_worker_amd.cellpose.pipeline import measure_tables

    H = W = 96
    truth = [_disks(H, W, [(y, x) for y in (12, 36, 60, 84) for x in (12, 36, 60, 84)], 56),
             _disks(H, W, [(y + 0.25, x + 0.25) for y in (24, 72) for x in (24, 72)], 224.5),
             np.zeros((H, W), np.int32)]
    served = []
    for M in truth:
        dP = ref.masks_to_flows(M)
        dP = dP[0] if isinstance(dP, tuple) else dP
        served.append(torch.from_numpy(np.concatenate([5 * dP, np.where(M > 0, 5.0, -5.0)[None]]).astype(np.float32)))
    # the oracle recovers the disks from their flows, and the 30 px disks (707 pixels each) fall within the band
    for M, y in zip(truth, served):
        assert np.array_equal(ref.compute_masks(y[:2].numpy(), y[2].numpy()), M)
    want_d = [measure_tables({k: np.asarray(v)[None] for k, v in ref.measure_masks(M).items()})[0]["diameter_px"] for M in truth]
    assert abs(want_d[0] - 15) < 0.5 and abs(30 / want_d[1] - 1) <= 1e-3 and want_d[2] == 0.0
    x = np.zeros((3, 2, H, W), np.float32)
    for b, M in enumerate(truth):
        x[b, 0], x[b, 1] = M > 0, b
    asked = []

    def run_net(xx, p):
        ys = []
        for img in xx:
            b = int(round(float(img[1].mean())))
            asked.append((b, tuple(img.shape[1:])))
            ys.append(F.interpolate(served[b][None], size=tuple(img.shape[1:]), mode="bilinear", align_corners=False)[0])
        return torch.stack(ys), torch.ones(xx.shape[0], 4)

    monkeypatch.setattr(cpu_runner, "run_net", run_net)
    first = cpu_runner.eval(x, normalize=False)
    m1, y1 = first[0].clone(), first[1].clone()
    assert asked == [(0, (H, W)), (1, (H, W)), (2, (H, W))] and not hasattr(first[0], "diameters")
    del asked[:]
    m, y, s = cpu_runner.eval(x, normalize=False, diameter="auto")
    hs = int(round(96 * 30 / want_d[0]))
    assert asked == [(0, (H, W)), (1, (H, W)), (2, (H, W)), (0, (hs, hs))]  # pass 2: image 0 only, at its scale
    assert m.diameters.dtype == torch.float32 and m.diameters.shape == (3,)
    assert torch.equal(m.diameters, torch.tensor(want_d, dtype=torch.float32))
    assert torch.equal(m[1:], m1[1:]) and torch.equal(y[1:], y1[1:])  # images 1 and 2 keep their pass-1 result
    assert not torch.equal(y[0], y1[0]) and int(m[0].max()) == 16
    with pytest.raises(ValueError, match="compute_masks"):
        cpu_runner.eval(x, normalize=False, diameter="auto", compute_masks=False)


class _FakeRunner:
    """What the app needs of a runner, recording the ``diameter`` of every ``eval`` call."""
    nchan, device = 2, "cpu"

    def __init__(self):
        self.calls = []

    def eval(self, batch, **prm):
        B, _, H, W = np.asarray(batch).shape
        self.calls.append((B, prm.get("diameter")))
        m = torch.zeros(B, H, W, dtype=torch.int32)
        if prm.get("diameter") == "auto":
            m.diameters = torch.arange(1, B + 1, dtype=torch.float32) * 10
        return m, torch.zeros(B, 3, H, W), torch.zeros(B, 4)


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.setenv("BE_CELLPOSE_PREWARM", "0")
    spec = importlib.util.spec_from_file_location("cellpose_main_diameters_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cls = mod.CellposeFinetune.func_or_class
    fake = _FakeRunner()

    async def _runner(self, model_id):
        return fake

    monkeypatch.setattr(cls, "_runner", _runner)
    return cls(default_model="cyto3"), fake


@pytest.mark.unit
def test_app_batches_requests_of_different_diameters(app):
    app, fake = app
    img = np.zeros((40, 48), np.uint16)

    async def two(d0, d1, **kw):
        return await asyncio.gather(app.infer(input_arrays=[img], model="cyto3", diameter=d0, **kw),
                                    app.infer(input_arrays=[img], model="cyto3", diameter=d1, **kw))

    a, b = asyncio.run(asyncio.wait_for(two(17.0, 41.0), 120))
    assert fake.calls == [(2, [17.0, 41.0])]  # one batch, the list of its requests' diameters
    assert a[0]["output"].shape == (40, 48) and "diameter_px" not in a[0]
    del fake.calls[:]
    asyncio.run(asyncio.wait_for(two(17.0, 17.0), 120))
    assert fake.calls == [(2, 17.0)]  # equal diameters: the scalar form
    del fake.calls[:]
    asyncio.run(asyncio.wait_for(two(17.0, None), 120))
    assert fake.calls == [(2, [17.0, None])]
    del fake.calls[:]
    a, b = asyncio.run(asyncio.wait_for(two("auto", 17.0), 120))
    assert sorted(fake.calls, key=str) == sorted([(1, "auto"), (1, 17.0)], key=str)  # "auto" is its own group
    assert a[0]["diameter_px"] == 10.0 and "diameter_px" not in b[0]
    del fake.calls[:]
    a, b = asyncio.run(asyncio.wait_for(two("auto", "auto"), 120))
    assert fake.calls == [(2, "auto")] and [a[0]["diameter_px"], b[0]["diameter_px"]] == [10.0, 20.0]
    with pytest.raises(ValueError, match="auto"):
        asyncio.run(app.infer(input_arrays=[np.zeros((3, 40, 48), np.uint16)], model="cyto3", diameter="auto", z_axis=0))
    with pytest.raises(ValueError, match="diameter"):
        asyncio.run(app.infer(input_arrays=[img], model="cyto3", diameter="big"))
