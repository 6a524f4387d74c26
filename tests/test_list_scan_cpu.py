"""The candidate row of ``search/list_scan.py`` against numpy: every slot of every query maps to the row that the
concatenation of its probed lists gives, on the fixture of the fused-search GPU tests plus a probe row that starts
with an empty list and has two empty lists side by side."""
import numpy as np
import torch

from bioengine_worker_amd.search.list_scan import candidate_offsets, slot_rows

SIZES = [300, 0, 1, 513, 7, 64, 1200, 2, 0, 900]
PROBES = np.array([[1, 2, 4, 7, 8], [0, 1, 2, 3, 6], [3, 5, 6, 7, 9], [1, 8, 0, 2, 4]])
OFF = np.concatenate([[0], np.cumsum(SIZES)])


def test_candidate_offsets_and_slot_rows():
    list_off, probes = torch.from_numpy(OFF), torch.from_numpy(PROBES)
    sizes, cand_off = candidate_offsets(list_off, probes)
    want_sizes = np.asarray(SIZES)[PROBES]
    assert cand_off.is_contiguous() and np.array_equal(sizes.numpy(), want_sizes)
    assert np.array_equal(cand_off.numpy(), np.cumsum(want_sizes, 1) - want_sizes)
    for qi in range(len(PROBES)):
        rows = np.concatenate([np.arange(OFF[l], OFF[l + 1]) for l in PROBES[qi]])
        slots = torch.arange(len(rows))[None]
        got = slot_rows(list_off, probes[qi:qi + 1], cand_off[qi:qi + 1], slots)
        assert np.array_equal(got.numpy()[0], rows)
    # all queries at once, each row's slots padded to the longest: the slots a query has are as above
    tot = want_sizes.sum(1)
    slots = torch.arange(int(tot.max())).expand(len(PROBES), -1)
    got = slot_rows(list_off, probes, cand_off, slots).numpy()
    for qi in range(len(PROBES)):
        rows = np.concatenate([np.arange(OFF[l], OFF[l + 1]) for l in PROBES[qi]])
        assert np.array_equal(got[qi, :tot[qi]], rows)
