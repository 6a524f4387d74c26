"""z-stack stitching, CPU: the numpy oracle ``reference.stitch3d`` (the yardstick of the HIP kernels
in ``test_cellpose_stitch_gpu.py``), ``CellposeRunner.eval_stack`` on a CPU runner and the stack mode
of the Cellpose app's ``infer``."""
import asyncio
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import stitch_cases as sc
from bioengine_worker_amd.cellpose import reference as ref

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"


def _bijection(out, truth):
    """Every truth id maps to exactly one output id and back (background to background)."""
    pairs = np.unique(np.stack([truth.ravel(), out.ravel()], 1), axis=0)
    return len(set(pairs[:, 0])) == len(pairs) == len(set(pairs[:, 1])) and (pairs[pairs[:, 0] == 0][:, 1] == 0).all()


def _first_appearance_ids(out, masks):
    """Output ids in order of first appearance: plane, then ascending local label."""
    seen = []
    for z in range(out.shape[0]):
        for lab in np.unique(masks[z][masks[z] > 0]):
            g = int(out[z][masks[z] == lab][0])
            if g and g not in seen:
                seen.append(g)
    return seen


@pytest.mark.unit
def test_prisms_bijection_and_order():
    truth, masks = sc.prisms()
    out = ref.stitch3d(masks, 0.25)
    assert out.dtype == np.int32 and out.shape == masks.shape
    assert _bijection(out, truth)
    K = int(truth.max())
    assert K == 20 and int(out.max()) == K
    assert _first_appearance_ids(out, masks) == list(range(1, K + 1))


@pytest.mark.unit
def test_spheres_counts():
    truth, masks = sc.spheres()
    n = int(truth.max())
    assert n == 10
    out = ref.stitch3d(masks, 0.25)
    assert int(out.max()) == 15  # small polar caps split off at t = 0.25
    big = ref.stitch3d(masks, 0.25, min_size=60)
    assert int(big.max()) == 10
    # min_size leaves one label per sphere: every kept label lies in one sphere and no sphere has two
    pairs = np.unique(np.stack([truth[big > 0], big[big > 0]], 1), axis=0)
    assert len(pairs) == n and len(set(pairs[:, 0])) == n and len(set(pairs[:, 1])) == n
    loose = ref.stitch3d(masks, 0.1)
    assert int(loose.max()) == 10 and _bijection(loose, truth)  # no sphere is split at t = 0.1


@pytest.mark.unit
def test_threshold_equality_links():
    m = sc.threshold_pair()
    assert (m[0] > 0).sum() == 20 and ((m[0] > 0) & (m[1] > 0)).sum() == 8  # ov 8, u 32
    assert int(ref.stitch3d(m, 0.25).max()) == 1
    assert int(ref.stitch3d(m, 0.26).max()) == 2


@pytest.mark.unit
def test_ties():
    m = sc.tie_two_next()
    out = ref.stitch3d(m, 0.25)
    assert set(out[1][m[1] == 2]) == {1} and set(out[1][m[1] == 5]) == {2}  # smaller id links, other is new
    m = sc.owns_two_unequal()
    out = ref.stitch3d(m, 0.25)
    g3, g4 = int(out[0][m[0] == 3][0]), int(out[0][m[0] == 4][0])
    assert (g3, g4) == (1, 2) and set(out[1][m[1] == 1]) == {g4}
    m = sc.equal_ratios()  # 2/6 and 4/12 are one ratio: the smaller previous label is the link
    out = ref.stitch3d(m, 0.25)
    assert set(out[1][m[1] == 1]) == {int(out[0][m[0] == 2][0])}
    m = sc.EDGE_CASES["equal_ratios_owner"]()  # the same tie on the owner side: the smaller next label
    out = ref.stitch3d(m, 0.25)
    assert set(out[1][m[1] == 2]) == {1} and set(out[1][m[1] == 3]) == {2}


@pytest.mark.unit
def test_edge_cases():
    out = ref.stitch3d(sc.empty_leading(), 0.25)
    assert not out[0].any() and int(out.max()) == 1 and (out[1] == out[2]).all()
    m = sc.empty_middle()
    out = ref.stitch3d(m, 0.25)
    assert not out[1].any() and int(out.max()) == 4
    assert set(np.unique(out[0])) == {0, 1, 2} and set(np.unique(out[2])) == {0, 3, 4}  # no id reused
    assert (out[2] == out[3]).all()
    z = ref.stitch3d(np.zeros((3, 8, 12), np.int32), 0.25)
    assert z.shape == (3, 8, 12) and z.dtype == np.int32 and not z.any()
    one = ref.stitch3d(sc.gaps()[:1], 0.25)
    assert one.shape == (1, 8, 12) and set(np.unique(one)) == {0, 1, 2}
    m = sc.gaps()
    out = ref.stitch3d(m, 0.25)
    assert int(out.max()) == 2 and (out[0] == out[1]).all() and (out[0] == out[2]).all()
    assert set(out[0][m[0] == 3]) == {1} and set(out[0][m[0] == 7]) == {2}
    # volume filter: the 3 x 3 object has 27 voxels over the stack, the 4 x 4 one 48
    out = ref.stitch3d(m, 0.25, min_size=30)
    assert int(out.max()) == 1 and (out > 0).sum() == 48


@pytest.mark.unit
def test_cpu_tensor_wrapper_runs_oracle():
    from bioengine_worker_amd.cellpose.gpu import stitch3d_gpu

    m = sc.gaps()
    out = stitch3d_gpu(torch.from_numpy(m), 0.25)
    assert out.dtype == torch.int32 and np.array_equal(out.numpy(), ref.stitch3d(m, 0.25))


# ------------------------------------------------------------------ runner

#: a random network's flows fail the flow-error QC, which would leave nothing to stitch
QC_OFF = {"flow_threshold": 0.0}


@pytest.fixture(scope="module")
def cpu_runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpnet import CPnet

    return CellposeRunner(CPnet().randomize_(0), device="cpu")


@pytest.fixture(scope="module")
def stack():
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    return synthetic_cells(3, 64, 64, ncells=6, seed=1)  # [3, 2, 64, 64] uint16


@pytest.fixture(scope="module")
def plane_results(cpu_runner, stack):
    """eval(normalize=False) on the stack-normalised planes: the per-plane reference of eval_stack."""
    x = stack.astype(np.float32)
    Z, C, H, W = x.shape
    xn = ref.normalize99(x.transpose(1, 0, 2, 3).reshape(C, Z * H, W)).reshape(C, Z, H, W).transpose(1, 0, 2, 3)
    m, y, s = cpu_runner.eval(np.ascontiguousarray(xn), normalize=False, **QC_OFF)
    assert all(int(pl.max()) >= 4 for pl in m)  # the random network gives masks in every plane
    return m.clone(), y.clone(), s.clone()


@pytest.mark.unit
def test_eval_stack_cpu(cpu_runner, stack, plane_results):
    pm, py, ps = plane_results
    m, y, s = cpu_runner.eval_stack(stack, stitch_threshold=0.25, **QC_OFF)
    assert m.shape == (3, 64, 64) and m.dtype == torch.int32
    assert y.shape == (3, 3, 64, 64) and y.dtype == torch.float32 and s.shape[0] == 3
    assert torch.equal(y, py)
    want = ref.stitch3d(pm.numpy(), 0.25, min_size=15)
    assert np.array_equal(m.numpy(), want) and 0 < int(want.max()) < int(sum(pl.max() for pl in pm))  # some link
    m0, _, _ = cpu_runner.eval_stack(stack, stitch_threshold=0.0, **QC_OFF)
    assert torch.equal(m0, pm)  # unstitched: the per-plane masks unchanged
    # channel-last and single-channel layouts
    ml, _, _ = cpu_runner.eval_stack(np.ascontiguousarray(stack.transpose(0, 2, 3, 1)), stitch_threshold=0.25,
                                      **QC_OFF)
    assert torch.equal(ml, m)
    assert cpu_runner.eval_stack(stack[:, 0], stitch_threshold=0.25, **QC_OFF)[0].shape == (3, 64, 64)


@pytest.mark.unit
def test_eval_stack_norm3d_off_is_per_plane_eval(cpu_runner, stack):
    m, y, _ = cpu_runner.eval_stack(stack, stitch_threshold=0.0, norm3d=False, **QC_OFF)
    pm, py, _ = cpu_runner.eval(stack, **QC_OFF)
    assert torch.equal(m, pm) and torch.equal(y, py) and int(pm.max()) > 0


@pytest.mark.unit
def test_eval_ignores_stack_fields(cpu_runner, stack):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams

    p = EvalParams()
    assert (p.stitch_threshold, p.norm3d, p.stack_batch) == (0.0, True, 32)
    a, _, _ = cpu_runner.eval(stack)
    b, _, _ = cpu_runner.eval(stack, EvalParams(stitch_threshold=0.5, norm3d=False, stack_batch=1))
    assert torch.equal(a, b)


# ------------------------------------------------------------------ app


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_stitch_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


@pytest.mark.unit
def test_app_stack_mode(app, stack):
    vol = np.ascontiguousarray(stack[:, 0])  # [Z, H, W]

    async def main():
        a = await app.infer(input_arrays=[vol], model="cyto3", stitch_threshold=0.25, flow_threshold=0.0)
        b = await app.infer(input_arrays=[np.ascontiguousarray(vol.transpose(1, 2, 0))], model="cyto3",
                            stitch_threshold=0.25, z_axis=2, flow_threshold=0.0)
        c = await app.infer({"input_arrays": [vol], "model": "cyto3", "stitch_threshold": 0.25, "z_axis": 0,
                             "return_flows": True, "flow_threshold": 0.0})
        j = await app.infer(input_arrays=[vol], model="cyto3", z_axis=0, json_safe=True)
        with pytest.raises(ValueError, match="z-stack"):
            await app.infer(input_arrays=[vol[0]], model="cyto3", stitch_threshold=0.25)
        # default call: what the runner's eval gives for the same image, as before
        d = await app.infer(input_arrays=[vol[0]], model="cyto3", flow_threshold=0.0)
        runner = await app._runner("cyto3")
        return a, b, c, j, d, runner

    a, b, c, j, d, runner = asyncio.run(asyncio.wait_for(main(), 600))
    out = a[0]["output"]
    assert out.shape == vol.shape and out.dtype == np.uint16 and a[0]["input_path"] == "input_arrays[0]"
    want, _, _ = runner.eval_stack(vol, stitch_threshold=0.25, flow_threshold=0.0)
    assert np.array_equal(out, want.cpu().numpy()) and int(out.max()) > 0
    assert np.array_equal(b[0]["output"], out) and np.array_equal(c[0]["output"], out)
    rgb, dp, cp = c[0]["flows"]
    assert rgb.shape == vol.shape + (3,) and dp.shape == (3, 2, 64, 64) and cp.shape == vol.shape
    assert isinstance(j[0]["output"], list) and len(j[0]["output"]) == 3
    assert j[0]["output"][0]["encoding"] == "mask_png_base64"
    pm, _, _ = runner.eval(vol[0], flow_threshold=0.0)
    assert d[0]["output"].shape == (64, 64) and np.array_equal(d[0]["output"], pm[0].cpu().numpy())
    assert int(pm.max()) > 0
