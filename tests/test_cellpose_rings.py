"""Cell outlines as polygon rings: the numpy oracle ``reference.mask_rings`` with its inverse and its
GeoJSON form, ``CellposeRunner.outlines`` and the app's ``infer(return_outlines=...)`` on the CPU.
Nothing here is compared with cellpose, OpenCV or scikit-image (none is installed): the checks are
the rules' own invariants, independent constructions with ``scipy.ndimage`` and literals."""
import asyncio
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

import cellpose_rings_cases as rc
from bioengine_worker_amd.cellpose import reference as ref

APP_MAIN = Path(__file__).resolve().parents[1] / "apps" / "cellpose-finetuning" / "main.py"


def ring_list(r: dict) -> list:
    off = r["ring_offsets"]
    return [(int(r["ring_label"][i]), r["verts"][off[i]:off[i + 1]], int(r["ring_area2"][i]))
            for i in range(r["ring_label"].shape[0])]


def images():
    return [(name, b, rc.masks(name)[b], rc.oracle(name)[b]) for name in rc.CASES for b in range(rc.masks(name).shape[0])]


def test_hand_literals():
    r = ref.mask_rings(rc.masks("hand")[0])
    assert r["verts"].dtype == np.int32 and r["ring_offsets"].dtype == np.int64
    assert r["ring_label"].dtype == np.int32 and r["ring_area2"].dtype == np.int64
    got = [(lab, [tuple(p) for p in v.tolist()], a2) for lab, v, a2 in ring_list(r)]
    assert got == rc.HAND_RINGS
    assert r["ring_offsets"].tolist() == [0, 4, 10, 14, 18, 22, 26]


def test_empty_and_bad_shape():
    r = ref.mask_rings(np.zeros((4, 5), np.int32))
    assert r["verts"].shape == (0, 2) and r["ring_offsets"].tolist() == [0] and r["ring_label"].shape == (0,)
    assert {k: v.dtype for k, v in r.items()} == {k: v.dtype for k, v in rc.oracle("hand")[0].items()}
    assert not ref.rings_to_labels(r, (4, 5)).any()
    with pytest.raises(ValueError):
        ref.mask_rings(np.zeros((2, 3, 4), np.int32))


def test_round_trip_and_area():
    for name, b, m, r in images():
        assert np.array_equal(ref.rings_to_labels(r, m.shape), m), (name, b)
        area = ref.measure_masks(m)["area"]
        got = np.zeros(area.shape[0] + 1, np.int64)
        np.add.at(got, r["ring_label"], r["ring_area2"])
        assert np.array_equal(got[1:], 2 * area), (name, b)
        # the shoelace sum over the emitted vertices is what is stored
        for lab, v, a2 in ring_list(r):
            y, x = v[:, 0].astype(np.int64), v[:, 1].astype(np.int64)
            assert int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum()) == a2 != 0, (name, b, lab)


def test_ring_counts_match_connected_components():
    for name, b, m, r in images():
        labs, a2 = r["ring_label"], r["ring_area2"]
        for lab in np.unique(m[m > 0]):
            member = m == lab
            outer = ndimage.label(member)[1]  # 4-connected components
            pad = np.pad(~member, 1, constant_values=True)
            holes = ndimage.label(pad, structure=np.ones((3, 3)))[1] - 1  # 8-connected complement, minus the outside
            assert int(((labs == lab) & (a2 > 0)).sum()) == outer, (name, b, lab)
            assert int(((labs == lab) & (a2 < 0)).sum()) == holes, (name, b, lab)


def test_vertex_count_is_local():
    for name, b, m, r in images():
        k = max(int(m.max()), 0)
        want = np.bincount(r["ring_label"], weights=np.diff(r["ring_offsets"]), minlength=k + 1)[1:].astype(np.int64)
        assert np.array_equal(ref.ring_vertex_counts(m), want), (name, b)
    assert rc.oracle("big")[1]["verts"].shape[0] == 602  # the spiral
    assert rc.oracle("nested")[0]["ring_label"].shape[0] == 4096 and rc.oracle("many")[0]["ring_label"].shape[0] == 1024


def test_start_order_and_evenness():
    for name, b, m, r in images():
        H, W = m.shape
        keys = []
        for lab, v, a2 in ring_list(r):
            n = v.shape[0]
            assert n >= 4 and n % 2 == 0, (name, b, lab)
            nxt = np.roll(v, -1, 0)
            d = nxt - v
            assert ((d[:, 0] == 0) != (d[:, 1] == 0)).all(), "edges between turn vertices are axis-parallel"
            horiz = d[:, 0] == 0
            assert (horiz != np.roll(horiz, 1)).all(), "every vertex is a turn"
            y0, x0 = v[0]
            # the first vertex is the tail of a top edge going +x: the pixel is the label's, the one above is not
            assert m[y0, x0] == lab and (y0 == 0 or m[y0 - 1, x0] != lab) and d[0, 0] == 0 and d[0, 1] > 0
            # ... and the raster-first top edge of the ring: no +x run of the ring starts earlier
            runs = v[horiz & (d[:, 1] > 0)]
            assert (y0 * (W + 1) + x0) == (runs[:, 0].astype(np.int64) * (W + 1) + runs[:, 1]).min()
            if a2 > 0:
                assert y0 * (W + 1) + x0 == (v[:, 0].astype(np.int64) * (W + 1) + v[:, 1]).min()
            keys.append((lab, int(y0) * W + int(x0)))
        assert keys == sorted(keys) and len(set(keys)) == len(keys), (name, b)


def test_saddle_and_diagonal():
    rings = ring_list(rc.oracle("saddle")[0])
    assert [lab for lab, _, _ in rings] == [1, 2, 2]
    v = [tuple(p) for p in rings[0][1].tolist()]
    assert v.count((2, 2)) == 2 and len(v) == 10 and rings[0][2] == 2 * 7  # one ring through the corner twice
    assert [a2 for _, _, a2 in rings[1:]] == [2, 2]  # diagonal neighbours stay apart
    assert [tuple(rings[i][1][0]) for i in (1, 2)] == [(4, 4), (5, 5)]


def test_geojson():
    r = rc.oracle("holes")[0]
    g = ref.rings_to_geojson(r)
    assert g["type"] == "FeatureCollection" and [f["properties"]["label"] for f in g["features"]] == [1, 2]
    json.loads(json.dumps(g))
    f1, f2 = g["features"]
    m = rc.masks("holes")[0]
    assert f1["properties"] == {"label": 1, "area": int((m == 1).sum()), "n_rings": 5}
    assert f2["properties"] == {"label": 2, "area": 1, "n_rings": 1}
    assert f2["geometry"] == {"type": "Polygon", "coordinates": [[[5, 5], [6, 5], [6, 6], [5, 6], [5, 5]]]}  # [x, y]
    assert f1["geometry"]["type"] == "MultiPolygon"
    big, island = f1["geometry"]["coordinates"]
    assert big[0][0] == [1, 1] and len(big) == 3 and len(island) == 2
    # the island's own hole goes to the island (the smaller of the two outer rings that contain it)
    assert island[0][0] == [5, 10] and island[1][0] == [6, 12]
    assert sorted(h[0] for h in big[1:]) == [[3, 8], [3, 14]]
    for poly in (big, island):
        for k, ring in enumerate(poly):
            assert ring[0] == ring[-1] and len(ring) >= 5
            x, y = np.array(ring[:-1]).T
            a2 = int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
            assert (a2 > 0) == (k == 0), "exterior counter-clockwise in (x, y), holes clockwise"
    # a non-square label: x and y are not swapped
    gb = ref.rings_to_geojson(rc.oracle("border")[0], z=3)
    assert gb["features"][0]["geometry"] == {"type": "Polygon", "coordinates": [[[0, 0], [70, 0], [70, 1], [0, 1], [0, 0]]]}
    assert all(f["properties"]["z"] == 3 for f in gb["features"])
    assert ref.rings_to_geojson(ref.mask_rings(np.zeros((3, 3), np.int32))) == {"type": "FeatureCollection", "features": []}
    for name, b, m, r in images():
        if name not in ("big", "nested", "many"):
            g = ref.rings_to_geojson(r)
            assert [f["properties"]["area"] for f in g["features"]] == [int((m == f["properties"]["label"]).sum())
                                                                        for f in g["features"]]


def test_rings_to_labels_raises():
    a, b = ref.mask_rings(np.array([[1, 1, 0]])), ref.mask_rings(np.array([[0, 2, 2]]))
    both = rc.join([a, b])
    both = {k: both[k] for k in a}
    both["ring_offsets"] = np.array([0, 4, 8])
    with pytest.raises(ValueError, match="another label"):
        ref.rings_to_labels(both, (1, 3))
    twice = dict(both, ring_label=np.array([1, 1], np.int32))
    with pytest.raises(ValueError, match="winding"):
        ref.rings_to_labels(twice, (1, 3))
    flipped = dict(a, verts=a["verts"][::-1].copy())
    with pytest.raises(ValueError, match="winding"):
        ref.rings_to_labels(flipped, (1, 3))
    with pytest.raises(ValueError, match="outside"):
        ref.rings_to_labels(a, (1, 1))


# ------------------------------------------------------------------ wrapper and runner on the CPU


def same_rings(got: dict, want: dict) -> None:
    assert set(got) == set(want)
    for k in want:
        g = got[k].numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), k


def test_wrapper_cpu_matches_oracle():
    from bioengine_worker_amd.cellpose import gpu

    for name in ("ragged", "vol", "holes"):
        same_rings(gpu.mask_rings_gpu(torch.from_numpy(rc.masks(name).copy()), volume=name == "vol"), rc.batch_oracle(name))
    m = rc.masks("ragged")
    low = gpu.mask_rings_gpu(torch.from_numpy(m.copy()), nlab=11)
    same_rings(low, rc.join([ref.mask_rings(np.where(x > 10, 0, x)) for x in m]))
    none = gpu.mask_rings_gpu(torch.zeros(2, 3, 4, dtype=torch.int32))
    assert none["verts"].shape == (0, 2) and none["image_rings"].tolist() == [0, 0, 0] and none["ring_offsets"].tolist() == [0]
    with pytest.raises(ValueError, match="too large"):
        gpu.mask_rings_gpu(torch.zeros(1, dtype=torch.int32).expand(1, 2 ** 15 + 1, 4))
    with pytest.raises(ValueError, match="too large"):
        gpu.mask_rings_gpu(torch.zeros(1, dtype=torch.int32).expand(2048, 1023, 1023))
    with pytest.raises(ValueError):
        gpu.mask_rings_gpu(torch.zeros(4, 4, dtype=torch.int32))


@pytest.fixture(scope="module")
def cpu_runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpnet import CPnet

    return CellposeRunner(CPnet().randomize_(0), device="cpu")


def test_runner_outlines_cpu(cpu_runner):
    m = rc.masks("ragged")
    out = cpu_runner.outlines(torch.from_numpy(m.copy()))
    assert isinstance(out, list) and len(out) == 3
    for b in range(3):
        same_rings(out[b], rc.oracle("ragged")[b])
    same_rings(cpu_runner.outlines(m[1])[0], rc.oracle("ragged")[1])  # numpy, one image
    planes = cpu_runner.outlines(rc.masks("vol"), volume=True)
    assert len(planes) == 5
    for z in range(5):
        same_rings(planes[z], rc.oracle("vol")[z])
    low = cpu_runner.outlines(m[1], nlab=11)[0]
    assert int(low["ring_label"].max()) == 10
    with pytest.raises(ValueError):
        cpu_runner.outlines(np.zeros((2, 2, 3, 3), np.int32))


# ------------------------------------------------------------------ app


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_rings_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


def check_ring_items(items: list, mask: np.ndarray) -> None:
    """The ``"rings"`` form of one image against the oracle on the returned mask."""
    want = ref.mask_rings(mask)
    rings = ring_list(want)
    assert [it["label"] for it in items] == sorted({lab for lab, _, _ in rings})
    flat = [(it["label"], ring, a2) for it in items for ring, a2 in zip(it["rings"], it["area2"])]
    assert len(flat) == len(rings)
    for (lab, ring, a2), (wl, wv, wa) in zip(flat, rings):
        assert (lab, a2) == (wl, wa) and ring == wv[:, ::-1].tolist()  # [x, y]
        assert all(type(c) is int for p in ring for c in p) and type(a2) is int and type(lab) is int


def test_app_return_outlines(app):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    imgs = synthetic_cells(2, 48, 56, ncells=6, seed=2)  # [2, 2, H, W] uint16
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}

    async def main():
        a = await app.infer(input_arrays=[imgs[0], imgs[1]], return_outlines=True, **kw)
        d = await app.infer({"input_arrays": [imgs[0]], "return_outlines": True, "outline_format": "geojson", **kw})
        j = await app.infer(input_arrays=[imgs[0]], return_outlines=True, json_safe=True, **kw)
        # one batch, only one request asks: the other gets nothing extra
        mixed = await asyncio.gather(app.infer(input_arrays=[imgs[0]], return_outlines=True, **kw),
                                     app.infer(input_arrays=[imgs[1]], **kw))
        with pytest.raises(ValueError, match="outline_format"):
            await app.infer(input_arrays=[imgs[0]], return_outlines=True, outline_format="roi", **kw)
        with pytest.raises(ValueError, match="outline_format"):
            await app.infer(input_arrays=[imgs[0]], outline_format="wkt", **kw)
        return a, d, j, mixed

    a, d, j, mixed = asyncio.run(asyncio.wait_for(main(), 600))
    assert set(mixed[1][0]) - {"weights"} == {"input_path", "output"}
    assert set(a[0]) - {"weights"} == {"input_path", "output", "outlines"}
    assert int(a[0]["output"].max()) > 0  # the comparison is not about empty lists
    for item in a:
        check_ring_items(item["outlines"], item["output"])
    assert mixed[0][0]["outlines"] == a[0]["outlines"] == j[0]["outlines"]  # the same under json_safe
    json.loads(json.dumps(j[0]["outlines"]))
    assert d[0]["outlines"] == ref.rings_to_geojson(ref.mask_rings(a[0]["output"]))
    json.loads(json.dumps(d[0]["outlines"]))


def test_app_return_outlines_stack(app):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    vol = np.ascontiguousarray(synthetic_cells(6, 20, 24, ncells=3, seed=1)[:, 0])  # [Z, H, W] uint16
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0, "stitch_threshold": 0.25}

    async def main():
        s = await app.infer(input_arrays=[vol], return_outlines=True, **kw)
        g = await app.infer(input_arrays=[vol], return_outlines=True, outline_format="geojson", **kw)
        p = await app.infer(input_arrays=[vol], **kw)
        return s, g, p

    s, g, p = asyncio.run(asyncio.wait_for(main(), 600))
    assert set(p[0]) - {"weights"} == {"input_path", "output"}
    m = s[0]["output"]
    assert m.shape == vol.shape and len(s[0]["outlines"]) == len(g[0]["outlines"]) == 6
    for z in range(6):
        plane = s[0]["outlines"][z]
        assert plane["z"] == z
        check_ring_items(plane["outlines"], m[z])
        assert g[0]["outlines"][z] == ref.rings_to_geojson(ref.mask_rings(m[z]), z=z)
