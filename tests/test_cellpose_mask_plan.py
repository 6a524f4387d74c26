"""The mask-recovery job plan on the host: which row of ``be_cp_plan_masks``'s job array is which
named bucket of ``MaskPlan``, for every plan kind (no GPU: the launch result is hand-built)."""
import pytest
import torch

from bioengine_worker_amd.cellpose import gpu as cg

K = cg.PlanKind
NCAP = len(cg.DIFFUSE_BUCKETS)
SINGLE = ("big", "sparse_big", "queue_wave", "queue_group", "wave_small", "wave_big")
# (kind, counts given) -> (rows of the lds buckets, {other bucket: row}), as the comments at
# plan_masks_kernel and be_cp_plan_masks state them
LAYOUTS = {
    (K.DIFFUSE, False): (range(NCAP), {"big": NCAP}),
    (K.DIFFUSE, True): (range(NCAP), {"sparse_big": NCAP, "big": NCAP + 1}),
    (K.DIFFUSE_QUEUE, True): (range(2, NCAP + 2), {"queue_wave": 0, "queue_group": 1, "sparse_big": NCAP + 2,
                                                   "big": NCAP + 3}),
    (K.FILL, False): (range(1), {"big": 1}),
    (K.FILL_WAVE, False): (range(2, 3), {"wave_small": 0, "wave_big": 1, "big": 3}),
}


def test_kind_numbers_are_the_kernels():
    assert [int(k) for k in (K.DIFFUSE, K.FILL, K.DIFFUSE_QUEUE, K.FILL_WAVE)] == [0, 1, 2, 3]
    assert set(cg.PLAN_LAYOUT) == set(LAYOUTS)


@pytest.mark.parametrize("kind,split", list(LAYOUTS), ids=lambda v: v.name if isinstance(v, K) else f"counts{int(v)}")
def test_plan_finish_names_the_kernels_bucket_rows(kind, split):
    lds_rows, single = LAYOUTS[kind, split]
    nb = len(lds_rows) + len(single)
    n = nb + 1
    jobs = torch.zeros(nb, n, 4, dtype=torch.int64)
    jobs[:, :, 0] = torch.arange(nb)[:, None]
    bucket_n = torch.arange(1, nb + 1, dtype=torch.int32)
    niter_img = torch.tensor([11, 13], dtype=torch.int32)
    launched = (jobs, bucket_n, torch.tensor([7]), niter_img, (kind, split))
    (plan,) = cg._plan_finish([launched])

    def check(t, row):
        assert t.dtype == torch.int64 and tuple(t.shape) == (row + 1, 4)
        assert (t[:, 0] == row).all()

    assert plan.kind is kind and plan.scratch_total == 7 and plan.niter_img is niter_img
    assert len(plan.lds) == len(lds_rows)
    for t, row in zip(plan.lds, lds_rows):
        check(t, row)
    for name in SINGLE:
        if name in single:
            check(getattr(plan, name), single[name])
        else:
            t = getattr(plan, name)
            assert t.dtype == torch.int64 and tuple(t.shape) == (0, 4)


def test_two_plans_share_one_readback():
    """Both plans of compute_masks_gpu come out of one concatenated host read, each with its own sizes."""
    def launched(kind, split, nb, tot):
        jobs = torch.zeros(nb, nb + 1, 4, dtype=torch.int64)
        return jobs, torch.arange(1, nb + 1, dtype=torch.int32), torch.tensor([tot]), torch.zeros(1, dtype=torch.int32), (kind, split)

    a, b = cg._plan_finish([launched(K.DIFFUSE_QUEUE, True, NCAP + 4, 5), launched(K.FILL_WAVE, False, 4, 9)])
    assert (a.scratch_total, b.scratch_total) == (5, 9)
    assert a.big.shape[0] == NCAP + 4 and [t.shape[0] for t in (b.wave_small, b.wave_big, b.lds[0], b.big)] == [1, 2, 3, 4]


def test_bucket_without_jobs_is_empty():
    jobs = torch.ones(4, 5, 4, dtype=torch.int64)
    launched = (jobs, torch.tensor([0, 2, 0, 0], dtype=torch.int32), torch.tensor([0]), torch.zeros(1, dtype=torch.int32),
                (K.FILL_WAVE, False))
    (plan,) = cg._plan_finish([launched])
    assert [tuple(t.shape) for t in (plan.wave_small, plan.wave_big, plan.lds[0], plan.big)] == [(0, 4), (2, 4), (0, 4), (0, 4)]
    assert plan.scratch_total == 0 and len(plan.lds) == 1


@pytest.mark.parametrize("kind,counts", [(K.DIFFUSE_QUEUE, False), (K.FILL, True), (K.FILL_WAVE, True)],
                         ids=["queue_without_counts", "fill_with_counts", "fill_wave_with_counts"])
def test_plan_launch_refuses_a_layout_the_kernel_does_not_have(kind, counts):
    """The queue kind without pixel counts made the kernel write two buckets past the job array."""
    bbox = torch.zeros(2, 3, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        cg._plan_launch(bbox, None, kind, torch.ones(2, 3, dtype=torch.int32) if counts else None)
