"""Average precision on the CPU: the fact the GPU scorer rests on (the oracle's true positives are
the maximum matching of the threshold graph, and the edge count where no label has two edges), the
properties of the case set the GPU tests rely on, and the public routes on CPU tensors
(``gpu.average_precision_gpu``, ``CellposeRunner.score`` / ``evaluate``, the app's ``evaluate``,
``train.session.instance_metrics``)."""
import asyncio
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import ap_cases as ac
from bioengine_worker_amd.cellpose import metrics

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"

pytestmark = pytest.mark.unit


# ------------------------------------------------------------------ the rule


@pytest.mark.parametrize("name", ac.CASES)
def test_tp_is_maximum_matching(name):
    t, p = ac.pair(name)
    _, tp, fp, fn = ac.oracle(name, ac.ALL_THRESHOLDS)
    for b in range(t.shape[0]):
        for k, th in enumerate(ac.ALL_THRESHOLDS):
            assert tp[b, k] == ac.max_matching(t[b], p[b], th), (name, b, th)
            if not ac.has_two_edge_label(t[b], p[b], th):
                assert tp[b, k] == int(ac.edges(t[b], p[b], th).sum()), (name, b, th)
        assert (tp[b] + fn[b] == int(t[b].max())).all() and (tp[b] + fp[b] == int(p[b].max())).all()


def test_case_set_properties():
    for name in ac.NO_TWO_EDGE:
        t, p = ac.pair(name)
        for b in range(t.shape[0]):
            for th in ac.HIGH_THRESHOLDS:
                assert not ac.has_two_edge_label(t[b], p[b], th), (name, b, th)
    for name, ths in ac.TWO_EDGE.items():
        t, p = ac.pair(name)
        for th in ths:
            assert any(ac.has_two_edge_label(t[b], p[b], th) for b in range(t.shape[0])), (name, th)
    # every noise image needs the host at 0.1; the exact-half split has tp 1, not its 2 edges
    t, p = ac.pair("noise")
    assert all(ac.has_two_edge_label(t[b], p[b], 0.1) for b in range(t.shape[0]))
    assert ac.oracle("exact_half", (0.5,))[1].tolist() == [[1]]
    t, p = ac.pair("disks")
    assert [int(x.max()) for x in t] == list(ac.DISK_COUNTS) and len({int(x.max()) for x in p}) == 3
    assert (ac.oracle("disks")[1][:, 0] > 15).all()  # real matches, not empty graphs
    t, p = ac.pair("exact_iou")
    iou = metrics.intersection_over_union(t[0], p[0])[1:, 1:]
    assert np.diag(iou).tolist() == [1 / 2, 3 / 4, 9 / 10, 27 / 30] and 27 / 30 == 0.9


# ------------------------------------------------------------------ wrapper on CPU tensors


@pytest.mark.parametrize("name", ["boxes", "disks_noise", "empty", "volume"])
def test_wrapper_cpu_matches_oracle(name):
    from bioengine_worker_amd.cellpose import gpu

    t, p = ac.pair(name)
    info = {}
    got = gpu.average_precision_gpu(torch.from_numpy(t.copy()), torch.from_numpy(p.copy()), ac.ALL_THRESHOLDS, info=info)
    ac.same(got, ac.oracle(name, ac.ALL_THRESHOLDS))
    assert set(info) == {"host_matched", "capacity"}


def test_wrapper_errors_and_order():
    from bioengine_worker_amd.cellpose import gpu

    t, p = (torch.from_numpy(x.copy()) for x in ac.pair("boxes"))
    with pytest.raises(ValueError):
        gpu.average_precision_gpu(t, p[:, :40])
    with pytest.raises(ValueError):
        gpu.average_precision_gpu(t, p, [0.1 * i for i in range(1, 10)])
    for bad in ([0.0], [1.5], [-0.5, 0.5]):
        with pytest.raises(ValueError):
            gpu.average_precision_gpu(t, p, bad)
    # unsorted thresholds come back in the caller's order; other integer dtypes are converted
    got = gpu.average_precision_gpu(t.long(), p.to(torch.int16), [0.9, 0.5, 0.75])
    ac.same(got, ac.oracle("boxes", (0.9, 0.5, 0.75)))
    assert np.array_equal(got[1][:, [1, 2, 0]], ac.oracle("boxes")[1])


def test_metrics_helpers_keep_the_oracle():
    """``ap_from_counts`` and ``metrics_document`` are the oracle's own expressions."""
    t, p = ac.pair("disks_noise")
    ap, tp, fp, fn = ac.oracle("disks_noise", ac.ALL_THRESHOLDS)
    ac.same(metrics.ap_from_counts(tp, t.reshape(5, -1).max(1), p.reshape(5, -1).max(1)), (ap, tp, fp, fn))
    doc = metrics.instance_metrics(list(t), list(p))
    assert doc == metrics.metrics_document(ac.oracle("disks_noise")[0], metrics.DEFAULT_THRESHOLDS,
                                           sum(int(x.max()) for x in t), sum(int(x.max()) for x in p))
    assert set(doc) == {"ap_0_5", "ap_0_75", "ap_0_9", "n_true", "n_pred"}


# ------------------------------------------------------------------ runner


@pytest.fixture(scope="module")
def cpu_runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpnet import CPnet

    return CellposeRunner(CPnet().randomize_(0), device="cpu")


def test_runner_score_and_evaluate_cpu(cpu_runner):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    imgs = synthetic_cells(2, 48, 56, ncells=6, seed=2)
    kw = {"niter": 20, "flow_threshold": 0.0}
    masks, _, _ = cpu_runner.eval(imgs, **kw)
    truth = masks.numpy().copy()
    truth[truth == 1] = 0  # one cell painted out
    assert int(masks.max()) > 1
    want = metrics.average_precision(list(truth), list(masks.numpy()), [0.5, 0.75, 0.9])
    res = cpu_runner.evaluate(imgs, truth, **kw)
    assert torch.equal(res["masks"], masks)
    ac.same([res[k] for k in ("ap", "tp", "fp", "fn")], want)
    assert res["n_true"].tolist() == [int(x.max()) for x in truth]
    assert res["n_pred"].tolist() == [int(x.max()) for x in masks.numpy()]
    assert res["summary"] == metrics.instance_metrics(list(truth), list(masks.numpy()))
    sc = cpu_runner.score(truth, masks, thresholds=[0.25, 0.5])
    ac.same([sc[k] for k in ("ap", "tp", "fp", "fn")],
            metrics.average_precision(list(truth), list(masks.numpy()), [0.25, 0.5]))
    assert set(sc) == {"ap", "tp", "fp", "fn", "n_true", "n_pred", "summary"}
    # one [H, W] image; a volume is one image
    one = cpu_runner.score(truth[0], masks[0])
    assert one["tp"].shape == (1, 3) and np.array_equal(one["tp"][0], want[1][0])
    vt, vp = ac.pair("volume")
    vol = cpu_runner.score(vt[0], vp[0], volume=True)
    ac.same([vol[k] for k in ("ap", "tp", "fp", "fn")], ac.oracle("volume"))
    with pytest.raises(ValueError):
        cpu_runner.score(truth[:1], masks)


# ------------------------------------------------------------------ app


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_ap_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


def test_app_evaluate(app):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    imgs = synthetic_cells(3, 48, 56, ncells=6, seed=2)  # [3, 2, H, W] uint16
    small = np.ascontiguousarray(imgs[2][:, :40, :44])  # another shape: its own group
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}

    async def main():
        plain = await app.infer(input_arrays=[imgs[0], imgs[1], small], **kw)
        labs = [np.asarray(it["output"]).astype(np.int32) for it in plain]
        labs[0] = np.where(labs[0] == 1, 0, labs[0])
        a = await app.evaluate(input_arrays=[imgs[0], imgs[1], small], label_arrays=labs, **kw)
        d = await app.evaluate({"input_arrays": [imgs[0], imgs[1], small], "label_arrays": labs,
                                "thresholds": [0.5, 0.75, 0.9], **kw})
        errs = []
        for bad in ({"input_arrays": [imgs[0], imgs[1]], "label_arrays": labs[:1]},
                    {"input_arrays": [imgs[0]], "label_arrays": [labs[0][:40]]}):
            try:
                await app.evaluate(**bad, **kw)
                errs.append(None)
            except ValueError as e:
                errs.append(e)
        return plain, labs, a, d, errs

    plain, labs, a, d, errs = asyncio.run(asyncio.wait_for(main(), 600))
    assert all(isinstance(e, ValueError) for e in errs)
    assert a == d and json.loads(json.dumps(a)) == a  # JSON-safe, NaN-free
    assert a.get("weights") == "random"
    preds = [np.asarray(it["output"]).astype(np.int32) for it in plain]
    assert int(preds[0].max()) > 1
    ap, tp, fp, fn = metrics.average_precision(labs, preds, [0.5, 0.75, 0.9])
    assert [it["input_path"] for it in a["per_image"]] == [f"input_arrays[{i}]" for i in range(3)]
    for i, it in enumerate(a["per_image"]):
        assert set(it) == {"input_path", "ap", "tp", "fp", "fn", "n_true", "n_pred"}
        assert it["tp"] == tp[i].tolist() and it["fp"] == fp[i].tolist() and it["fn"] == fn[i].tolist()
        assert it["ap"] == [float(x) if np.isfinite(x) else None for x in ap[i]]
        assert it["n_true"] == int(labs[i].max()) and it["n_pred"] == int(preds[i].max())
    assert a["instance_metrics"] == metrics.instance_metrics(labs, preds, [0.5, 0.75, 0.9])


# ------------------------------------------------------------------ training session


def test_session_instance_metrics_cpu(monkeypatch):
    from bioengine_worker_amd.cellpose import pipeline
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells
    from bioengine_worker_amd.models.cpnet import CPnet
    from bioengine_worker_amd.train import session

    imgs = synthetic_cells(2, 48, 56, ncells=6, seed=2)
    labs = [np.asarray(x, np.int32) for x in ac.pair("ragged37")[0]]
    labs = [np.pad(l, ((0, 11), (0, 3))) for l in labs]  # 48 x 56
    net = CPnet().randomize_(0)
    seen = []
    real_eval = pipeline.CellposeRunner.eval

    def spy(self, images, p=None, **kw):
        out = real_eval(self, images, p, **kw)
        seen.append(out[0][0].cpu().numpy().copy())
        return out

    monkeypatch.setattr(pipeline.CellposeRunner, "eval", spy)
    doc = session.instance_metrics(net, list(imgs), labs, torch.device("cpu"))
    assert set(doc) == {"ap_0_5", "ap_0_75", "ap_0_9", "n_true", "n_pred"} and len(seen) == 2
    assert doc == metrics.instance_metrics(labs, seen)
