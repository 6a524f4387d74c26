"""Average precision on the GPU (csrc/kernels/cellpose_ap.hip) against ``metrics.average_precision``:
every result equals the oracle exactly (integer tp / fp / fn, bit-equal float32 ap, NaN positions
included).  Cases and their shared oracle results: tests/ap_cases.py."""
import numpy as np
import pytest
import torch

import ap_cases as ac
from bioengine_worker_amd.cellpose import metrics

pytestmark = pytest.mark.gpu


def dev_pair(name, gpu):
    t, p = ac.pair(name)
    return torch.from_numpy(t).to(gpu), torch.from_numpy(p).to(gpu)


def score(name, gpu, ths, **kw):
    from bioengine_worker_amd.cellpose.gpu import average_precision_gpu

    t, p = dev_pair(name, gpu)
    return average_precision_gpu(t, p, ths, **kw)


@pytest.mark.parametrize("name", ["boxes", "split", "ragged37", "ragged7", "large", "empty", "volume"])
def test_cases_all_thresholds(gpu, name):
    """Hand-built boxes, the split box, ragged sizes 37 x 53 and 1 x 7, one large label against one
    large label (all atomics on one key), empty truth / prediction / both, a volume as one image."""
    ac.same(score(name, gpu, ac.ALL_THRESHOLDS), ac.oracle(name, ac.ALL_THRESHOLDS))
    ac.same(score(name, gpu, ac.HIGH_THRESHOLDS), ac.oracle(name))


def test_exact_iou_equality_counts(gpu):
    """IoU exactly 1/2, 3/4, 9/10 and 27/30 at 0.5 / 0.75 / 0.9 and at the next double above each:
    the comparison is fp64 and equality counts."""
    ths = tuple(x for th in ac.HIGH_THRESHOLDS for x in (th, float(np.nextafter(th, 2.0))))
    want = ac.oracle("exact_iou", ths)
    assert want[1].tolist() == [[4, 3, 3, 2, 2, 0]]
    info = {}
    ac.same(score("exact_iou", gpu, ths, info=info), want)
    assert info["host_matched"] == 0


def test_exact_half_split_takes_the_host(gpu):
    info = {}
    got = score("exact_half", gpu, ac.HIGH_THRESHOLDS, info=info)
    ac.same(got, ac.oracle("exact_half"))
    assert got[1].tolist() == [[1, 0, 0]] and info["host_matched"] == 1


def test_disks_stay_on_the_device(gpu):
    """B = 3 with a different label count per image: no conflict at 0.5 / 0.75 / 0.9, so nothing is
    matched on the host (an implementation that always falls back fails here)."""
    info = {}
    ac.same(score("disks", gpu, ac.HIGH_THRESHOLDS, info=info), ac.oracle("disks"))
    assert info["host_matched"] == 0 and info["capacity"] >= 1024
    # bounds given (larger than needed): same result
    ac.same(score("disks", gpu, ac.HIGH_THRESHOLDS, nt=41, np_=77), ac.oracle("disks"))
    ac.same(score("disks", gpu, ac.HIGH_THRESHOLDS, nt=4096, np_=41), ac.oracle("disks"))


def test_disks_and_noise_fall_back_at_low_thresholds(gpu):
    info = {}
    ths = (0.1, 0.5, 0.25, 0.9)  # unsorted: results come back in this order
    ac.same(score("disks_noise", gpu, ths, info=info), ac.oracle("disks_noise", ths))
    assert info["host_matched"] >= 2  # at least the two noise images at 0.1
    ac.same(score("disks_noise", gpu, ac.ALL_THRESHOLDS), ac.oracle("disks_noise", ac.ALL_THRESHOLDS))
    ac.same(score("noise", gpu, ac.ALL_THRESHOLDS), ac.oracle("noise", ac.ALL_THRESHOLDS))


def test_many_labels_and_overflow_retry(gpu):
    """1,600 labels per image on 200 x 200: more distinct pairs per workgroup than its LDS table
    holds.  ``capacity=64`` overflows (the launch returns with the overflow word set); the retries at
    twice the size give the identical result."""
    want = ac.oracle("grid1600")
    info = {}
    ac.same(score("grid1600", gpu, ac.HIGH_THRESHOLDS, info=info), want)
    assert info["host_matched"] == 0
    small = {}
    ac.same(score("grid1600", gpu, ac.HIGH_THRESHOLDS, capacity=64, info=small), want)
    assert small["capacity"] > 64 and small["host_matched"] == 0
    ac.same(score("grid1600", gpu, ac.ALL_THRESHOLDS, capacity=64), ac.oracle("grid1600", ac.ALL_THRESHOLDS))


def test_tables_smaller_than_a_wave(gpu):
    """Below 64 slots a wave's slots span several images: the match pass counts edges per lane there."""
    info = {}
    ac.same(score("boxes", gpu, ac.ALL_THRESHOLDS, capacity=16, info=info), ac.oracle("boxes", ac.ALL_THRESHOLDS))
    assert info["capacity"] == 16
    ac.same(score("exact_half", gpu, ac.HIGH_THRESHOLDS, capacity=2, info=info), ac.oracle("exact_half"))
    assert info["capacity"] == 2 and info["host_matched"] == 1
    ac.same(score("disks_noise", gpu, ac.ALL_THRESHOLDS, capacity=32), ac.oracle("disks_noise", ac.ALL_THRESHOLDS))


def test_unaligned_view_and_dtypes(gpu):
    """A view whose ``data_ptr() % 16 == 4`` takes the scalar loads; int64 / int16 labels are converted."""
    from bioengine_worker_amd.cellpose.gpu import average_precision_gpu

    t, p = ac.pair("disks")
    n = t.size
    bt = torch.zeros(n + 8, dtype=torch.int32, device=gpu)
    bp = torch.zeros(n + 8, dtype=torch.int32, device=gpu)
    vt, vp = bt[1: n + 1].view(t.shape), bp[1: n + 1].view(p.shape)
    vt.copy_(torch.from_numpy(t))
    vp.copy_(torch.from_numpy(p))
    assert vt.data_ptr() % 16 == 4 and vp.data_ptr() % 16 == 4 and vt.is_contiguous()
    ac.same(average_precision_gpu(vt, vp), ac.oracle("disks"))
    ac.same(average_precision_gpu(vt.long(), vp.to(torch.int16)), ac.oracle("disks"))


def test_errors(gpu):
    from bioengine_worker_amd.cellpose.gpu import average_precision_gpu

    t, p = dev_pair("disks", gpu)
    with pytest.raises(ValueError):
        average_precision_gpu(t, p[:, :90])
    with pytest.raises(ValueError):
        average_precision_gpu(t, p, [0.1 * i for i in range(1, 10)])
    with pytest.raises(ValueError):
        average_precision_gpu(t, p, [0.0, 0.5])
    with pytest.raises(ValueError, match="bound"):  # a label outside its bound sets the error word, nothing is indexed by it
        average_precision_gpu(t, p, nt=20, np_=41)
    neg = p.clone()
    neg[0, 0, 0] = -3
    with pytest.raises(ValueError, match="bound"):
        average_precision_gpu(t, neg, nt=41, np_=41)


def test_two_runs_identical(gpu):
    a = score("disks_noise", gpu, ac.ALL_THRESHOLDS)
    b = score("disks_noise", gpu, ac.ALL_THRESHOLDS)
    ac.same(a, b)


def test_metrics_route_device_tensors(gpu):
    """``metrics.average_precision`` / ``instance_metrics`` send CUDA label tensors to the GPU scorer:
    one batch per shape, ragged lists grouped, single tensors one image."""
    td, pd = dev_pair("disks", gpu)
    tr, pr = dev_pair("ragged37", gpu)
    lt, lp = list(td) + list(tr), list(pd) + list(pr)
    nt, npd = [x.cpu().numpy() for x in lt], [x.cpu().numpy() for x in lp]
    ac.same(metrics.average_precision(lt, lp, ac.ALL_THRESHOLDS), metrics.average_precision(nt, npd, ac.ALL_THRESHOLDS))
    ac.same(metrics.average_precision(td[0], pd[0]), metrics.average_precision(nt[0], npd[0]))
    assert metrics.instance_metrics(lt, lp) == metrics.instance_metrics(nt, npd)


@pytest.fixture(scope="module")
def runner(gpu):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    return CellposeRunner(device=gpu)


def test_runner_score_volume(gpu, runner):
    t, p = dev_pair("volume", gpu)  # [1, 5, 40, 40]
    res = runner.score(t[0], p[0], volume=True)
    ac.same([res[k] for k in ("ap", "tp", "fp", "fn")], ac.oracle("volume"))
    assert res["n_true"].tolist() == [9] and res["n_pred"].tolist() == [9]
    assert res["summary"] == metrics.instance_metrics([ac.pair("volume")[0][0]], [ac.pair("volume")[1][0]])
    # numpy truth against a device prediction
    res2 = runner.score(ac.pair("volume")[0][0], p[0], volume=True, thresholds=ac.ALL_THRESHOLDS)
    ac.same([res2[k] for k in ("ap", "tp", "fp", "fn")], ac.oracle("volume", ac.ALL_THRESHOLDS))


def test_runner_evaluate_end_to_end(runner):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    x = synthetic_cells(4, 128, 128, ncells=12)
    own = runner.eval(x, flow_threshold=0.0)[0].cpu().numpy()
    truth = own.copy()
    truth[truth == 1] = 0  # one cell painted out of every image
    res = runner.evaluate(x, truth, flow_threshold=0.0)
    masks = res["masks"]
    assert masks.is_cuda and int(masks.max()) > 0
    m = masks.cpu().numpy()
    want = metrics.average_precision(list(truth), list(m), [0.5, 0.75, 0.9])
    ac.same([res[k] for k in ("ap", "tp", "fp", "fn")], want)
    assert res["n_true"].tolist() == [int(v.max()) for v in truth] and res["n_pred"].tolist() == [int(v.max()) for v in m]
    assert res["summary"] == metrics.instance_metrics(list(truth), list(m))


def test_session_instance_metrics_on_device(gpu, monkeypatch):
    """The training session keeps its per-image eval and scores the device masks: the document
    equals the oracle's on the masks it predicted."""
    from bioengine_worker_amd.cellpose import pipeline
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells
    from bioengine_worker_amd.models.cpnet import CPnet
    from bioengine_worker_amd.train import session

    imgs = synthetic_cells(2, 64, 64, ncells=8, seed=4)
    seen = []
    real_eval = pipeline.CellposeRunner.eval

    def spy(self, images, p=None, **kw):
        out = real_eval(self, images, p, **kw)
        seen.append(out[0][0].cpu().numpy().copy())
        return out

    monkeypatch.setattr(pipeline.CellposeRunner, "eval", spy)
    labs = [np.asarray(v, np.int32) for v in ac.pair("disks")[0][:2, :64, :64]]
    doc = session.instance_metrics(CPnet().randomize_(0), list(imgs), labs, gpu)
    assert len(seen) == 2 and doc == metrics.instance_metrics(labs, seen)
    assert set(doc) == {"ap_0_5", "ap_0_75", "ap_0_9", "n_true", "n_pred"}
