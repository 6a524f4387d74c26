"""Polygon annotations -> label images on the CPU: the oracle ``reference.rasterize_rings``, the
parser ``reference.outlines_to_rings``, the host side of ``gpu.rasterize_rings_gpu`` (its checks and
its job plan, replayed in numpy) and the readers that accept GeoJSON annotations."""
import importlib.util
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import cellpose_raster_cases as cases
import cellpose_rings_cases as rc
from bioengine_worker_amd.cellpose import gpu as cg
from bioengine_worker_amd.cellpose import reference as ref

ROOT = Path(__file__).resolve().parents[1]


def one(verts, shape, label=1, dtype=np.float64) -> np.ndarray:
    v = np.asarray(verts, dtype).reshape(-1, 2)
    return ref.rasterize_rings({"verts": v, "ring_offsets": [0, v.shape[0]], "ring_label": [label]}, shape)


@pytest.fixture(scope="module")
def outline_items():
    from bioengine_worker_amd.compat import install

    install()
    spec = importlib.util.spec_from_file_location("cellpose_main_raster_items", ROOT / "apps" / "cellpose-finetuning" / "main.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.outline_items


# ------------------------------------------------------------------ the rule


@pytest.mark.parametrize("name", rc.CASES)
def test_round_trip(name, outline_items):
    for m, r in zip(rc.masks(name), rc.oracle(name)):
        want = np.maximum(m, 0).astype(np.int32)
        got = ref.rasterize_rings(r, m.shape)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        via_geojson = ref.outlines_to_rings(json.loads(json.dumps(ref.rings_to_geojson(r))))
        assert via_geojson["verts"].dtype == np.float64
        assert np.array_equal(ref.rasterize_rings(via_geojson, m.shape), want)
        via_items = ref.outlines_to_rings(json.loads(json.dumps(outline_items(r, "rings"))))
        assert np.array_equal(ref.rasterize_rings(via_items, m.shape), want)
        wrapped = ref.unwrap_outlines(outline_items(r, "rings", z=3))
        assert np.array_equal(ref.rasterize_rings(ref.outlines_to_rings(wrapped), m.shape), want)


def test_literals():
    sq = one(cases.SQUARE, (4, 4))
    want = np.zeros((4, 4), np.int32)
    want[:2, :2] = 1
    assert np.array_equal(sq, want)
    assert one(cases.TRIANGLE, (5, 5)).sum(1).tolist() == [4, 3, 2, 1, 0]
    assert one(cases.BOW_TIE, (8, 8)).sum(1).tolist() == [7, 5, 3, 1, 1, 3, 5, 7]
    assert np.array_equal(one(cases.SQUARE[::-1], (4, 4)), want)  # the orientation does not matter
    assert np.array_equal(one(cases.SQUARE, (4, 4), dtype=np.float32), want)
    assert np.array_equal(one([(0, 0), (0, 2), (2, 2), (2, 0)], (4, 4), dtype=np.int16), want)
    ties = cases.oracle("ties")
    assert np.array_equal(ties[0, :4, :4], want) and ties[1].sum(1).tolist() == [4, 3, 2, 1, 0, 0, 0, 0]


def test_partition_covers_every_pixel_once():
    tris = cases.partition_triangles()
    assert len(tris) == 72
    count = sum((one(t, (40, 40)) > 0).astype(np.int64) for t in tris)
    assert (count == 1).all()
    assert (cases.oracle("partition") > 0).all()


def test_overlap_takes_the_largest_label():
    p, (_, H, W) = cases.polys("overlap")
    off = p["ring_offsets"]
    singles = [one(p["verts"][off[r]:off[r + 1]], (H, W), int(p["ring_label"][r])) for r in range(3)]
    assert ((singles[0] > 0) & (singles[1] > 0) & (singles[2] > 0)).any()  # all three overlap somewhere
    assert np.array_equal(cases.oracle("overlap")[0], np.maximum.reduce(singles))
    # two parts of ONE label cancel where they overlap (even-odd over all the rings of a label)
    both = ref.rasterize_rings(dict(p, ring_label=np.asarray([4, 4, 9], np.int32)), (H, W))
    a, b = singles[0] > 0, singles[1] > 0
    assert np.array_equal(both == 4, (a ^ b) & ~(singles[2] > 0))


def fraction_inside(v: np.ndarray, y: int, x: int) -> bool:
    """The rule on the unquantised lattice: crossings at or left of the centre, in exact fractions
    of the quantised vertices (the quantisation itself is the specification's, not under test)."""
    q = ref.quantize_verts(v)
    pts = [(Fraction(int(a), 256), Fraction(int(b), 256)) for a, b in q]
    cy, cx = Fraction(2 * y + 1, 2), Fraction(2 * x + 1, 2)
    n = 0
    for (y0, x0), (y1, x1) in zip(pts, pts[1:] + pts[:1]):
        if (y0 <= cy) != (y1 <= cy):
            n += x0 + (cy - y0) * (x1 - x0) / (y1 - y0) <= cx
    return bool(n & 1)


def test_equals_fraction_evaluation():
    want = cases.oracle("stars")
    for b, v in enumerate(cases.star_polygons()):
        got = np.asarray([[fraction_inside(v, y, x) for x in range(24)] for y in range(24)])
        assert np.array_equal(got, want[b] > 0), b
    assert len({int(w.sum()) for w in want}) > 10  # really different polygons


def test_gon_area():
    p, _ = cases.polys("gon")
    v = p["verts"]
    nxt = np.roll(v, -1, 0)
    area = abs(float((v[:, 1] * nxt[:, 0] - nxt[:, 1] * v[:, 0]).sum())) / 2
    perimeter = float(np.hypot(*(nxt - v).T).sum())
    n = int((cases.oracle("gon") > 0).sum())
    assert 60000 < area < 70000 and abs(n - area) <= perimeter


def test_case_properties():
    assert set(np.unique(cases.oracle("sliver")).tolist()) == {0, 1}  # label 2 holds no centre
    assert set(np.unique(cases.oracle("outside")).tolist()) == {0, 1, 4}
    m = cases.oracle("multi")[0]
    assert np.array_equal(m[:, 16:] > 0, m[:, :16] > 0) and set(np.unique(m[:, 16:]).tolist()) == {0, 2}
    assert m[2, 2] == 1 and m[5, 5] == 0 and m[7, 7] == 1  # shell, hole, island
    d = cases.oracle("degenerate")[0]
    assert set(np.unique(d).tolist()) == {0, 1, 2, 3, 6}  # the two-vertex ring and the empty ring leave nothing
    assert (d[3, 12:19] == 3).all() and (d[2, 12:19] == 0).all()  # top edge on the centre line y = 3.5: inside
    assert (d[8, 12:19] == 3).all() and (d[9, 12:19] == 0).all()  # bottom edge on y = 9.5: outside
    b = cases.oracle("bands")
    for i, (rows, cols) in enumerate(((63, 255), (64, 256), (65, 257))):
        ys, xs = np.nonzero(b[i])
        assert (ys.max() + 1, xs.max() + 1) == (rows, cols) and ys.min() == xs.min() == 0
    assert np.unique(cases.oracle("many")).size == 1025
    r = cases.oracle("ragged")
    assert r[0].any() and not r[1].any() and r[2].any()


def test_quantisation():
    assert ref.RASTER_SUBPIX == 256
    assert ref.quantize_verts([[0.498046875, -0.498046875]]).tolist() == [[128, -127]]  # x.5 rounds up
    q = ref.quantize_verts(np.asarray([[1, 2]], np.uint8))
    assert q.dtype == np.int64 and q.tolist() == [[256, 512]]
    assert ref.quantize_verts(np.zeros((0, 2))).shape == (0, 2)
    assert ref.quantize_verts([[-32768.0, 65536.0]]).tolist() == [[-2 ** 23, 2 ** 24]]
    for bad in ([[np.nan, 0.0]], [[0.0, np.inf]], [[65536.01, 0.0]], [[0.0, -32768.01]]):
        with pytest.raises(ValueError):
            ref.quantize_verts(bad)
    # a centre exactly on a vertical edge after rounding: 0.498046875 quantises to the centre of column 0
    assert one([(0, 0.498046875), (0, 2), (2, 2), (2, 0.498046875)], (2, 3)).tolist() == [[1, 1, 0], [1, 1, 0]]
    assert one([(0, 0.5 + 1 / 256), (0, 2), (2, 2), (2, 0.5 + 1 / 256)], (2, 3)).tolist() == [[0, 1, 0], [0, 1, 0]]


def test_rasterize_errors():
    sq = np.asarray(cases.SQUARE)
    ok = {"verts": sq, "ring_offsets": [0, 4], "ring_label": [1]}
    for bad in (dict(ok, ring_offsets=[0, 3]), dict(ok, ring_offsets=[1, 4]), dict(ok, ring_offsets=[0, 2, 4]),
                dict(ok, ring_offsets=[0, 5, 4], ring_label=[1, 1]), dict(ok, ring_label=[0]), dict(ok, ring_label=[-2]),
                dict(ok, verts=sq * np.nan), dict(ok, verts=sq * 1e6)):
        with pytest.raises(ValueError):
            ref.rasterize_rings(bad, (4, 4))
    assert not ref.rasterize_rings({"verts": np.zeros((0, 2)), "ring_offsets": [0], "ring_label": []}, (3, 3)).any()


# ------------------------------------------------------------------ the parser


def feature(coords, label=None, kind="Polygon"):
    f = {"type": "Feature", "properties": {} if label is None else {"label": label}, "geometry": {"type": kind, "coordinates": coords}}
    return f


RING = [[1, 1], [5, 1], [5, 4], [1, 4], [1, 1]]


def test_parser_forms():
    want = {"verts": [[1, 1], [1, 5], [4, 5], [4, 1]], "ring_offsets": [0, 4], "ring_label": [1]}

    def same(doc, labels=(1,)):
        got = ref.outlines_to_rings(doc)
        assert got["verts"].dtype == np.float64 and got["ring_offsets"].dtype == np.int64 and got["ring_label"].dtype == np.int32
        n = len(labels)
        assert got["verts"].tolist() == want["verts"] * n and got["ring_label"].tolist() == list(labels)
        assert got["ring_offsets"].tolist() == [4 * i for i in range(n + 1)]

    same({"type": "Polygon", "coordinates": [RING]})
    same(feature([RING]))
    same([feature([RING]), feature([RING])], (1, 2))  # labels by position
    same({"type": "FeatureCollection", "features": [feature([RING], 7), feature([[RING]], 7, "MultiPolygon")]}, (7, 7))
    same(feature([[[x, y, 9.5] for x, y in RING[:-1]]]))  # z ignored, ring not closed
    same([{"label": 3, "rings": [RING[:-1], RING[:-1]]}], (3, 3))
    same({"type": "FeatureCollection", "features": [feature([RING], 2.0)]}, (2,))
    empty = ref.outlines_to_rings({"type": "FeatureCollection", "features": []})
    assert empty["verts"].shape == (0, 2) and empty["ring_offsets"].tolist() == [0] and ref.outlines_to_rings([])["ring_label"].size == 0
    polys = {"verts": np.asarray(want["verts"], np.float32), "ring_offsets": np.asarray([0, 4]), "ring_label": np.asarray([5])}
    assert ref.outlines_to_rings(polys) is polys


@pytest.mark.parametrize("doc, match", [
    ([feature([RING]), {"type": "Feature", "properties": {}, "geometry": {"type": "Point", "coordinates": [1, 2]}}], "feature 1"),
    ([feature([RING]), {"type": "Feature", "properties": {}, "geometry": None}], "feature 1"),
    ({"type": "Feature", "properties": {}, "geometry": {"type": "GeometryCollection", "geometries": []}}, "feature 0"),
    ({"type": "LineString", "coordinates": RING}, "feature 0"),
    ({"type": "FeatureCollection", "features": [feature([RING]), {"type": "Polygon", "coordinates": [RING]}]}, "feature 1"),
    (feature([[[1, 1], [5, 1], [1, 1]]]), "three vertices"),
    (feature([[[1, 1], [5, 1]]]), "three vertices"),
    (feature([[[1, 1], [5], [5, 4]]]), "positions"),
    (feature([[[1, 1], [5, "a"], [5, 4]]]), "positions"),
    ([feature([RING], 1), feature([RING])], "some features"),
    (feature([RING], 0), "label"),
    (feature([RING], -3), "label"),
    (feature([RING], 1.5), "label"),
    (feature([RING], "a"), "label"),
    (feature([RING], 2 ** 31 - 1), "label"),
    (feature([[[1, 1], [5, float("nan")], [5, 4]]]), "finite"),
    ([{"rings": [RING]}], "no label"),
    ({"verts": np.zeros((3, 2)), "ring_offsets": [0, 3]}, "needs"),
    ({"verts": np.zeros((3, 2)), "ring_offsets": [0, 2], "ring_label": [1]}, "ring_offsets"),
    ({"verts": np.zeros((3, 2)), "ring_offsets": [0, 3], "ring_label": [0]}, "labels"),
    (7, "expects"),
    ("Polygon", "expects"),
    ({"features": []}, "expects"),
])
def test_parser_errors(doc, match):
    with pytest.raises(ValueError, match=match):
        ref.outlines_to_rings(doc)


# ------------------------------------------------------------------ the host side of the GPU path


def replay(p: dict, B: int, H: int, W: int) -> np.ndarray:
    """The job table of ``gpu._raster_plan`` executed in numpy with the kernel's arithmetic: the
    first column of every crossing from one exact floor division, parity over a job's chunk, the
    maximum committed.  Every job must lie inside its image and its group's edges."""
    q, off, labs, img = cg._raster_inputs(p, B, H, W)
    out = np.zeros((B, H, W), np.int32)
    plan = cg._raster_plan(q, off, labs, img, H, W)
    if plan is None:
        return out
    edges, jobs = plan
    assert edges.dtype == np.int32 and jobs.dtype == np.int32 and edges.shape[1] == 4 and jobs.shape[1] == 8
    E = edges.astype(np.int64)
    for e0, ne, b, lab, y0, nr, x0, nc in jobs.tolist():
        assert 0 <= b < B and 0 <= y0 and y0 + nr <= H and 0 <= x0 and x0 + nc <= W
        assert 0 < nr <= cg.RASTER_BAND and 0 < nc <= cg.RASTER_CHUNK and 0 <= e0 and ne > 0 and e0 + ne <= E.shape[0]
        Y0, X0, Y1, X1 = (E[e0:e0 + ne, k][None] for k in range(4))
        cy = (np.arange(y0, y0 + nr) * 256 + 128)[:, None]
        cross = (Y0 <= cy) != (Y1 <= cy)
        up = Y1 > Y0
        D = np.where(Y1 == Y0, 1, np.abs(Y1 - Y0))
        N = (cy - Y0) * np.where(up, X1 - X0, X0 - X1)
        rel = ((X0 - ((-N) // D) + 127) >> 8) - x0
        par = ((rel[:, :, None] <= np.arange(nc)[None, None]) & cross[:, :, None]).sum(1) & 1
        sub = out[b, y0:y0 + nr, x0:x0 + nc]
        sub[par == 1] = np.maximum(sub[par == 1], lab)
    return out


@pytest.mark.parametrize("name", cases.CASES)
def test_job_plan_replayed_equals_oracle(name):
    p, (B, H, W) = cases.polys(name)
    assert np.array_equal(replay(p, B, H, W), cases.oracle(name))


def test_job_plan_shapes():
    p, (B, H, W) = cases.polys("bands")
    edges, jobs = cg._raster_plan(*cg._raster_inputs(p, B, H, W), H, W)
    per_image = np.bincount(jobs[:, 2], minlength=B).tolist()
    assert per_image == [1, 1, 4, 9]  # 63 x 255 and 64 x 256: one job; 65 x 257: 2 x 2; 131 x 599: 3 x 3
    big = jobs[jobs[:, 2] == 3]
    assert sorted(set(big[:, 4].tolist())) == [0, 64, 128] and sorted(set(big[:, 6].tolist())) == [0, 256, 512]
    p, (B, H, W) = cases.polys("edges")
    edges, jobs = cg._raster_plan(*cg._raster_inputs(p, B, H, W), H, W)
    assert jobs[:, 1].tolist() == [63, 64, 65, 129, 80] and jobs[:, 0].tolist() == [0, 63, 127, 192, 321]
    p, (B, H, W) = cases.polys("sliver")
    assert cg._raster_plan(*cg._raster_inputs(p, B, H, W), H, W)[1][:, 3].tolist() == [1]  # no job for the sliver


def test_cpu_device_runs_the_oracle():
    for name in ("ragged", "ties", "rings:vol"):
        p, (B, H, W) = cases.polys(name)
        out = cg.rasterize_rings_gpu(p, B, H, W, "cpu")
        assert out.dtype == torch.int32 and tuple(out.shape) == (B, H, W) and np.array_equal(out.numpy(), cases.oracle(name))
        assert out.label_bound == int(np.asarray(p["ring_label"]).max()) + 1
    z = cg.rasterize_rings_gpu({"verts": np.zeros((0, 2)), "ring_offsets": [0], "ring_label": [], "ring_image": []}, 2, 5, 6, "cpu")
    assert tuple(z.shape) == (2, 5, 6) and not z.any() and z.label_bound == 1


@pytest.mark.parametrize("k", range(13))
def test_invalid_inputs_raise_on_the_host(k):
    p, (B, H, W), match = cases.invalid_inputs()[k]
    with pytest.raises(ValueError, match=match):
        cg.rasterize_rings_gpu(p, B, H, W, "cpu")


# ------------------------------------------------------------------ the public interface on the CPU


def test_runner_labels_from_outlines_and_score():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    runner = CellposeRunner(device="cpu")
    masks = rc.masks("ragged")
    docs = [ref.rings_to_geojson(r) for r in rc.oracle("ragged")]
    lab = runner.labels_from_outlines(docs, masks.shape[1:])
    assert lab.dtype == torch.int32 and np.array_equal(lab.numpy(), masks) and lab.label_bound == int(masks.max()) + 1
    single = runner.labels_from_outlines(docs[0], masks.shape[1:])  # one document, one image
    assert np.array_equal(single.numpy(), masks[:1])
    feats = runner.labels_from_outlines(docs[0]["features"], masks.shape[1:])  # a list of features is one document
    assert np.array_equal(feats.numpy(), masks[:1])
    # a stack: one entry per plane, {z, outlines} wrappers unwrapped, the volume's labels kept
    vol = rc.masks("vol")
    planes = [{"z": z, "outlines": [{"label": int(l), "rings": [r["verts"][a:b, ::-1].tolist()]} for l, a, b in
                                    zip(r["ring_label"], r["ring_offsets"][:-1], r["ring_offsets"][1:])]}
              for z, r in enumerate(rc.oracle("vol"))]
    assert np.array_equal(runner.labels_from_outlines(planes, vol.shape[1:]).numpy(), vol)
    pred = torch.from_numpy(np.roll(masks, 1, 2).copy())
    a, b = runner.score(docs, pred), runner.score(masks.copy(), pred)
    assert set(a) == set(b)
    for k in ("ap", "tp", "fp", "fn", "n_true", "n_pred"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["summary"] == b["summary"]
    one_img = runner.score(docs[0], pred[0])
    assert np.array_equal(one_img["tp"], b["tp"][:1])
    with pytest.raises(ValueError, match="do not fit"):
        runner.score(docs[:2], pred)


def write_pair(tmp_path, name="a"):
    masks = rc.masks("holes")[0]
    img = tmp_path / f"{name}.npy"
    np.save(img, (masks > 0).astype(np.float32) * 100)
    ann = tmp_path / f"{name}_mask.geojson"
    ann.write_text(json.dumps(ref.rings_to_geojson(rc.oracle("holes")[0])))
    return img, ann, masks


def test_read_labels_geojson(tmp_path, outline_items):
    from bioengine_worker_amd.cellpose import datasets as ds

    img, ann, masks = write_pair(tmp_path)
    got = ds.read_labels(ann, shape=masks.shape)
    assert got.dtype == np.int32 and np.array_equal(got, masks)
    assert np.array_equal(ds.read_labels(ann, shape=(8, 20)), np.pad(masks[:8], ((0, 0), (0, 4))))
    with pytest.raises(ValueError, match="shape"):
        ds.read_labels(ann)
    items = tmp_path / "b_mask.json"
    items.write_text(json.dumps(outline_items(rc.oracle("holes")[0], "rings")))
    assert np.array_equal(ds.read_labels(items, shape=masks.shape), masks)
    assert ds.has_foreground(ann) and ds.has_foreground(items)
    empty = tmp_path / "c_mask.geojson"
    empty.write_text(json.dumps({"type": "FeatureCollection", "features": []}))
    broken = tmp_path / "d_mask.geojson"
    broken.write_text("{")
    assert not ds.has_foreground(empty) and not ds.has_foreground(broken)
    with pytest.raises(ValueError, match="JSON"):
        ds.read_labels(broken, shape=(4, 4))
    np.save(tmp_path / "e_mask.npy", masks)
    assert np.array_equal(ds.read_labels(tmp_path / "e_mask.npy"), masks)  # label images as ever


def test_pairing_with_geojson_annotations():
    from bioengine_worker_amd.cellpose.datasets import match_image_annotation_pairs

    ims, ans = ["images/a.tif", "images/b.tif"], ["annotations/b_mask.geojson", "annotations/a_mask.geojson"]
    want = [("images/a.tif", "annotations/a_mask.geojson"), ("images/b.tif", "annotations/b_mask.geojson")]
    assert match_image_annotation_pairs(ims, ans, "images/*.tif", "annotations/*_mask.geojson") == want
    assert match_image_annotation_pairs(ims, ans, "images/", "annotations/") == want  # by base name


def test_listing_keeps_geojson_annotations():
    import asyncio

    from bioengine_worker_amd.cellpose.datasets import list_matching_artifact_paths

    class Artifact:
        async def ls(self, folder):
            return [{"name": "a_mask.geojson", "type": "file"}, {"name": "b_mask.tif", "type": "file"}] if folder == "annotations/" else []

    got = asyncio.run(list_matching_artifact_paths(Artifact(), "annotations/"))
    assert got == ["annotations/a_mask.geojson", "annotations/b_mask.tif"]
    assert asyncio.run(list_matching_artifact_paths(Artifact(), "annotations/*_mask.geojson")) == ["annotations/a_mask.geojson"]


def test_load_pairs_with_geojson_annotation(tmp_path):
    from bioengine_worker_amd.cellpose.datasets import create_dataset_split
    from bioengine_worker_amd.train.session import load_pairs

    img, ann, masks = write_pair(tmp_path)
    split = create_dataset_split([{"image": str(img), "annotation": str(ann)}], [])
    assert split["train_labels_files"] == [str(ann)]
    imgs, labs = load_pairs([{"image": str(img), "annotation": str(ann)}], nchan=2)
    assert imgs[0].shape == (2, 16, 16) and labs[0].dtype == np.int32 and np.array_equal(labs[0], masks)
