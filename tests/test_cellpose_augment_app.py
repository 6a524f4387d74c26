"""The Cellpose app with ``augment`` (test-time augmentation): ``infer`` and ``evaluate`` take it as a
keyword and in the dict form, forward it to the runner, and keep requests that differ in it out of
each other's batch.  Runs on whatever device the app picks (the CPU without a GPU) with the random cyto3-architecture CPnet."""
import asyncio
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_augment_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


@pytest.fixture()
def evals(monkeypatch):
    """Every network stage (``CellposeRunner.run_net``, which all the eval paths on the CPU and on
    the GPU end in) as (images in the batch, its ``augment``)."""
    from bioengine_worker_amd.cellpose import pipeline

    seen = []
    real = pipeline.CellposeRunner.run_net

    def spy(self, x, p, *args, **kw):
        seen.append((int(x.shape[0]), bool(p.augment)))
        return real(self, x, p, *args, **kw)

    monkeypatch.setattr(pipeline.CellposeRunner, "run_net", spy)
    return seen


def test_app_infer_with_augment(app, evals):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    imgs = synthetic_cells(2, 48, 56, ncells=6, seed=2)  # [2, 2, H, W] uint16
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}

    async def main():
        on = await app.infer(input_arrays=[imgs[0]], augment=True, return_flows=True, **kw)
        n_solo = len(evals)
        d = await app.infer({"input_arrays": [imgs[0]], "augment": True, "return_flows": True, **kw})
        off = await app.infer(input_arrays=[imgs[0]], return_flows=True, **kw)
        del evals[:]
        # one batching window: the two requests that differ only in augment run apart ...
        mixed = await asyncio.gather(app.infer(input_arrays=[imgs[0]], augment=True, return_flows=True, **kw),
                                     app.infer(input_arrays=[imgs[0]], return_flows=True, **kw))
        apart = list(evals)
        del evals[:]
        # ... and two that agree share a batch
        await asyncio.gather(app.infer(input_arrays=[imgs[0]], augment=True, **kw),
                             app.infer(input_arrays=[imgs[1]], augment=True, **kw))
        return on, n_solo, d, off, mixed, apart, list(evals)

    on, n_solo, d, off, mixed, apart, together = asyncio.run(asyncio.wait_for(main(), 600))
    assert n_solo == 1
    assert on[0]["output"].shape == (48, 56) and np.isfinite(on[0]["flows"][1]).all()
    assert np.array_equal(d[0]["output"], on[0]["output"]) and np.array_equal(d[0]["flows"][1], on[0]["flows"][1])
    assert not np.array_equal(on[0]["flows"][1], off[0]["flows"][1])  # the option reaches the network stage
    assert sorted(apart) == [(1, False), (1, True)]
    assert np.array_equal(mixed[0][0]["flows"][1], on[0]["flows"][1])
    assert np.array_equal(mixed[1][0]["flows"][1], off[0]["flows"][1])
    assert together == [(2, True)]


def test_app_stacks_and_evaluate_with_augment(app, evals):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    imgs = synthetic_cells(2, 48, 56, ncells=6, seed=2)
    vol = np.ascontiguousarray(synthetic_cells(3, 20, 24, ncells=3, seed=1)[:, 0])  # [Z, H, W] uint16
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}

    async def main():
        s = await app.infer({"input_arrays": [vol], "stitch_threshold": 0.25, "augment": True, **kw})
        stack_calls = list(evals)
        plain = await app.infer(input_arrays=[imgs[0], imgs[1]], augment=True, **kw)
        labs = [np.asarray(it["output"]).astype(np.int32) for it in plain]
        del evals[:]
        e = await app.evaluate(input_arrays=[imgs[0], imgs[1]], label_arrays=labs, augment=True, **kw)
        n_eval = list(evals)
        return s, stack_calls, labs, e, n_eval

    s, stack_calls, labs, e, n_eval = asyncio.run(asyncio.wait_for(main(), 600))
    assert s[0]["output"].shape == vol.shape
    assert stack_calls and all(aug for _, aug in stack_calls)  # eval_stack passed it on to every eval
    assert n_eval == [(2, True)]
    # scored against its own augmented masks: a perfect score wherever there are cells
    for it, lab in zip(e["per_image"], labs):
        assert it["n_pred"] == it["n_true"] == int(lab.max())
        assert it["fp"] == [0, 0, 0] and it["fn"] == [0, 0, 0]


@pytest.mark.gpu
def test_app_do_3d_with_augment(gpu, app, evals):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    vol = np.ascontiguousarray(synthetic_cells(8, 32, 40, ncells=4, seed=1)[:, 0])  # [Z, H, W] uint16

    async def main():
        return await app.infer({"input_arrays": [vol], "do_3D": True, "augment": True, "return_flows": True,
                                "model": "cyto3", "niter": 20})

    v = asyncio.run(asyncio.wait_for(main(), 600))
    assert v[0]["output"].shape == vol.shape and np.isfinite(v[0]["flows"][1]).all()
    assert len(evals) >= 3 and all(aug for _, aug in evals)  # every view's planes
