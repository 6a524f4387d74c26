"""Cellpose test-time augmentation (``augment=True``), CPU: the oracle's tile starts, the mirrored
tiles, ``unaugment_tiles`` (parity rule and both signs, pinned exactly by an equivariant stand-in
network) and the CPU path of ``CellposeRunner.eval``."""
import numpy as np
import pytest
import torch

import cellpose_augment_cases as ac
from bioengine_worker_amd.cellpose import reference as ref


def _image(H, W, C=2, seed=0):
    return np.random.default_rng(seed).standard_normal((C, H, W)).astype(np.float32)


@pytest.mark.parametrize("geo", list(ac.GEOMETRIES))
def test_starts_and_canvas(geo):
    H, W, bs = geo
    (Hp, Wp), ys, xs = ac.GEOMETRIES[geo]
    imgp = ac.padded(_image(H, W))
    assert imgp.shape[1:] == (Hp, Wp)
    assert ref.tile_starts_augment(Hp, bs) == ys and ref.tile_starts_augment(Wp, bs) == xs
    tiles, tys, txs, Ly, Lx = ref.make_tiles(imgp, bs, augment=True)
    assert (tys, txs) == (ys, xs) and (Ly, Lx) == (max(Hp, bs), max(Wp, bs))
    assert tiles.shape == (len(ys) * len(xs), 2, bs, bs)
    # tile_overlap is ignored
    assert ref.make_tiles(imgp, bs, 0.3, augment=True)[1:3] == (ys, xs)


def test_tile_counts_of_the_70x90_case():
    imgp = ac.padded(_image(70, 90))
    assert ref.make_tiles(imgp, 32, augment=True)[0].shape[0] == 42
    assert ref.make_tiles(imgp, 32)[0].shape[0] == 20


@pytest.mark.parametrize("geo", list(ac.GEOMETRIES))
def test_make_tiles_is_slicing_and_mirroring(geo):
    H, W, bs = geo
    imgp = ac.padded(_image(H, W, seed=1))
    tiles, ys, xs, Ly, Lx = ref.make_tiles(imgp, bs, augment=True)
    canvas = np.zeros((2, Ly, Lx), np.float32)
    canvas[:, : imgp.shape[1], : imgp.shape[2]] = imgp
    t = np.arange(bs)
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            rows = y + (bs - 1 - t if i % 2 else t)
            cols = x + (bs - 1 - t if j % 2 else t)
            assert np.array_equal(tiles[j * len(xs) + i], canvas[:, rows[:, None], cols[None, :]]), (j, i)
    if geo == (20, 100, 64):  # the bottom 16 rows of every un-mirrored tile are the extra end padding
        plain = ac.plain_tiles(imgp, ys, xs, bs)
        assert not plain[:, :, 48:].any() and plain[:, :, :48].any()


@pytest.mark.parametrize("geo", list(ac.GEOMETRIES))
def test_unaugment_is_exact_on_an_equivariant_network(geo):
    H, W, bs = geo
    imgp = ac.padded(_image(H, W, seed=2))
    tiles, ys, xs, _, _ = ref.make_tiles(imgp, bs, augment=True)
    got = ref.unaugment_tiles(ac.standin_net(tiles), ys, xs)
    want = ac.standin_net(ac.plain_tiles(imgp, ys, xs, bs))
    assert want[:, 0].any() and want[:, 1].any()
    assert np.array_equal(got, want)
    # the signs matter: without un-mirroring the outputs differ
    assert not np.array_equal(ac.standin_net(tiles), want)


def test_unaugment_leaves_further_channels_and_input_alone():
    y = np.random.default_rng(3).standard_normal((4, 4, 6, 6)).astype(np.float32)
    keep = y.copy()
    out = ref.unaugment_tiles(y, [0, 0], [0, 0])
    assert np.array_equal(y, keep)
    assert np.array_equal(out[0], y[0])  # tile (0, 0): not mirrored
    assert np.array_equal(out[1], y[1][:, ::-1] * np.array([-1, 1, 1, 1], np.float32)[:, None, None])  # i odd: y
    assert np.array_equal(out[2], y[2][:, :, ::-1] * np.array([1, -1, 1, 1], np.float32)[:, None, None])  # j odd: x
    assert np.array_equal(out[3], y[3][:, ::-1, ::-1] * np.array([-1, -1, 1, 1], np.float32)[:, None, None])
    with pytest.raises(ValueError):
        ref.unaugment_tiles(y[:3], [0, 0], [0, 0])


@pytest.fixture(scope="module")
def runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    return CellposeRunner(device="cpu", seed=0)


@pytest.fixture(scope="module")
def cells():
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    return synthetic_cells(1, 64, 80, ncells=8, seed=4)  # [1, 2, 64, 80] uint16


def test_cpu_eval_with_augment(runner, cells):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams

    masks, flows, styles = runner.eval(cells, augment=True, niter=20)
    assert masks.shape == (1, 64, 80) and flows.shape == (1, 3, 64, 80) and styles.shape[0] == 1
    assert torch.isfinite(flows).all() and torch.isfinite(styles).all()
    plain = runner.eval(cells, niter=20)
    assert not torch.equal(flows, plain[1])  # other tiles, other average
    # augment=False is what not passing it is
    off = runner.eval(cells, EvalParams(augment=False), niter=20)
    for a, b in zip(off, plain):
        assert torch.equal(a, b)


def test_augment_needs_tiles(runner, cells):
    with pytest.raises(ValueError, match="tile"):
        runner.eval(cells, tile=False, augment=True)


def test_cpu_cellpose_sam_with_augment():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpsam import CPSAM

    r = CellposeRunner(CPSAM(dim=128, depth=1, heads=2, ps=8, bsize=64).randomize_(0), device="cpu")
    img = np.random.default_rng(5).integers(0, 4000, (1, 3, 40, 50)).astype(np.uint16)  # padded 64 x 80: 2 x 3 tiles of 64
    _, flows, _ = r.eval(img, augment=True, compute_masks=False)
    assert flows.shape == (1, 3, 40, 50) and torch.isfinite(flows).all()
    assert not torch.equal(flows, r.eval(img, compute_masks=False)[1])
