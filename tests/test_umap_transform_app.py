"""Placing new points on a cached landscape: ``projection.place_points``, ``compute_projection(extend_to=...)``
and the cell-search app's ``project_query_onto_umap`` / ``project_embeddings_onto_umap``.  Everything here runs
the numpy oracle of the transform (the HIP library is reported absent), on 300 points."""
import asyncio
import base64
import importlib.util
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import umap_cases as uc
from bioengine_worker_amd.search import projection
from bioengine_worker_amd.search import reference as ref

ROOT = Path(__file__).resolve().parents[1]
CACHE_KEYS = {"x", "y", "labels", "colors", "n_total", "idx", "method", "engine"}
DICT_KEYS = {"x", "y", "labels", "colors", "n_total", "sample_idx", "method", "engine"}


def _nearest(x):
    def search(q, k):
        q = np.asarray(q, np.float64)
        s = (q / np.linalg.norm(q, axis=1)[:, None]) @ (x / np.linalg.norm(x, axis=1)[:, None]).T
        i = s.argmax(1)
        return s[np.arange(len(q)), i][:, None].astype(np.float32), i[:, None]

    return search


@pytest.fixture()
def index(monkeypatch):
    from bioengine_worker_amd.ops import _native

    monkeypatch.setattr(projection, "_have_umap_learn", lambda: False)
    monkeypatch.setattr(ref, "default_n_epochs", lambda n: 100)
    monkeypatch.setattr(_native, "hip_available", lambda: False)
    x = uc.clusters300()
    return SimpleNamespace(ntotal=len(x), dim=x.shape[1], reconstruct_batch=lambda ids: x[np.asarray(ids)],
                           search=_nearest(x.astype(np.float64)), vecs=x)


def test_place_points_on_a_umap_cache_runs_the_transform(index, tmp_path):
    cache = tmp_path / "umap_cache.npz"
    out = projection.compute_projection(index, None, cache, 240, method="umap")
    assert out["engine"] == "numpy" and len(out["x"]) == 240 and set(out) == DICT_KEYS
    assert set(np.load(cache).files) == CACHE_KEYS
    rest = np.setdiff1d(np.arange(300), out["sample_idx"])
    coords, how = projection.place_points(index, cache, index.vecs[rest])
    assert how == "transform:numpy" and coords.shape == (60, 2) and coords.dtype == np.float32
    fitted = np.stack([out["x"], out["y"]], 1)
    nn = ((coords[:, None, :] - fitted[None]) ** 2).sum(2).argmin(1)
    lab = np.arange(300) % 12
    assert (lab[np.asarray(out["sample_idx"])[nn]] == lab[rest]).mean() >= 0.95  # lands among its own cluster
    want = ref.umap_transform(index.vecs[rest], index.vecs[out["sample_idx"]], fitted.astype(np.float32))
    assert np.array_equal(coords, want)
    again, how = projection.place_points(index, cache, index.vecs[rest], "transform")
    assert how == "transform:numpy" and np.array_equal(again, coords)
    near, how = projection.place_points(index, cache, index.vecs[rest[:3]], "nearest")
    assert how == "nearest" and (near[:, None, :] == fitted[None].astype(np.float32)).all(2).any(1).all()
    with pytest.raises(ValueError):
        projection.place_points(index, cache, index.vecs[:1], "closest")


def test_place_points_on_pca_caches(index, tmp_path):
    cache = tmp_path / "umap_cache.npz"
    out = projection.compute_projection(index, None, cache, 240, method="pca")
    d = dict(np.load(cache))
    assert set(d) == CACHE_KEYS | {"pca_mean", "pca_V"} and d["pca_V"].shape == (32, 2) and set(out) == DICT_KEYS
    assert np.array_equal(out["x"], projection._pca_2d(index.vecs[out["sample_idx"]], 42)[:, 0])  # coordinates unchanged
    coords, how = projection.place_points(index, cache, index.vecs[out["sample_idx"]])
    assert how == "pca"
    fitted = np.stack([out["x"], out["y"]], 1)
    # float32 rounding of a 32-term product sum at |coordinate| <= ~40
    assert np.abs(coords - fitted).max() <= 32 * 2.0 ** -23 * np.abs(fitted).max()
    assert projection.place_points(index, cache, index.vecs[:4], "transform")[1] == "pca"
    # a cache of before the axes were stored
    old = tmp_path / "old.npz"
    np.savez(old, **{k: v for k, v in d.items() if not k.startswith("pca_")})
    coords, how = projection.place_points(index, old, index.vecs[:4])
    assert how == "nearest" and coords.shape == (4, 2)
    sidx = np.asarray(out["sample_idx"])
    for i in range(4):  # today's rule: the sampled cell whose index number is closest to the nearest neighbour's
        j = int(np.argmin(np.abs(sidx - i)))
        assert coords[i].tolist() == [np.float32(out["x"][j]), np.float32(out["y"][j])]
    with pytest.raises(ValueError):
        projection.place_points(index, old, index.vecs[:4], "transform")


def test_extend_to(index, tmp_path):
    labels = [f"c{i % 12}" for i in range(300)]
    a, b = tmp_path / "a" / "umap_cache.npz", tmp_path / "b" / "umap_cache.npz"
    plain = projection.compute_projection(index, labels, a, 240, method="umap")
    zero = projection.compute_projection(index, labels, b, 240, method="umap", extend_to=0)
    assert zero == plain and set(zero) == DICT_KEYS
    assert a.read_bytes() == b.read_bytes() and [p.name for p in b.parent.iterdir()] == ["umap_cache.npz"]
    assert projection.compute_projection(index, labels, b, 240, method="umap", extend_to=240) == plain  # nothing to add

    ext = projection.compute_projection(index, labels, b, 240, method="umap", extend_to=300)
    assert set(ext) == DICT_KEYS | {"n_fitted", "placement"}
    assert ext["n_fitted"] == 240 and ext["placement"] == "transform:numpy" and ext["n_total"] == 300
    assert all(len(ext[s]) == 300 for s in ("x", "y", "labels", "colors", "sample_idx"))
    assert all(ext[s][:240] == plain[s] for s in ("x", "y", "labels", "colors", "sample_idx"))
    assert sorted(ext["sample_idx"]) == list(range(300)) and ext["sample_idx"][240:] == sorted(ext["sample_idx"][240:])
    assert ext["labels"][240:] == [labels[i] for i in ext["sample_idx"][240:]]
    cmap = dict(zip(plain["labels"], plain["colors"]))
    assert ext["colors"][240:] == [cmap[s] for s in ext["labels"][240:]]  # the same palette mapping
    assert a.read_bytes() == b.read_bytes()  # the base cache is untouched
    sib = b.with_name("umap_cache.ext.npz")
    e = np.load(sib)
    assert {"n_total", "method", "engine", "n_fitted", "seed", "extend_to"} <= set(e.files) and int(e["extend_to"]) == 300

    stamp = sib.read_bytes()
    placer = projection._placer
    try:
        projection._placer = None  # a second call must not place anything
        assert projection.compute_projection(index, labels, b, 240, method="umap", extend_to=300) == ext
    finally:
        projection._placer = placer
    assert sib.read_bytes() == stamp
    less = projection.compute_projection(index, labels, b, 240, method="umap", extend_to=270)  # another request
    assert len(less["x"]) == 270 and int(np.load(sib)["extend_to"]) == 270
    assert projection.compute_projection(index, labels, b, 240, method="umap") == plain


@pytest.fixture()
def app(index, tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cell_search_main_transform_test", ROOT / "apps" / "cell-image-search" / "main.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cls = mod.CellImageSearch.func_or_class
    a = cls.__new__(cls)
    a._index, a._metadata_df, a._workspace_dir = index, None, str(tmp_path)

    async def embed(image, plow, phigh):
        return index.vecs[int(np.asarray(image).ravel()[0])] * np.float32(1.01), None

    monkeypatch.setattr(a, "_embed_query", embed, raising=False)
    monkeypatch.setattr(mod, "_decode_image_b64", lambda s: np.frombuffer(base64.b64decode(s), np.uint8))
    real = projection.compute_projection
    # a 240-point sample of the 300, as a real index would have; "auto" would be the PCA on a host without a GPU
    monkeypatch.setattr(projection, "compute_projection",
                        lambda index, labels, cache, n, seed, force, tag, method, extend_to=0: real(
                            index, labels, cache, min(n, 240), seed, force, tag, "umap", extend_to))
    return a


def test_app_query_placement(app, index):
    b64 = base64.b64encode(bytes([250])).decode()  # "image" of cell 250

    async def main():
        proj = await app.get_umap_preview()
        assert len(proj["x"]) == 240 and set(proj) == DICT_KEYS and proj["engine"] == "numpy"
        old = await app.project_query_onto_umap(image_b64=b64)
        j = int(np.argmin(np.abs(np.asarray(proj["sample_idx"]) - 250)))
        assert set(old) == {"umap_x", "umap_y", "nearest_score", "nearest_compound", "nearest_moa"}
        assert (old["umap_x"], old["umap_y"]) == (proj["x"][j], proj["y"][j])  # today's rule, today's keys
        new = await app.project_query_onto_umap(image_b64=b64, placement="auto")
        assert new["placement"] == "transform:numpy" and set(new) == set(old) | {"placement"}
        assert new["nearest_score"] == old["nearest_score"]
        cache = Path(app._umap_cache())
        want, _ = projection.place_points(index, cache, (index.vecs[250] * np.float32(1.01))[None])
        assert (new["umap_x"], new["umap_y"]) == (float(want[0, 0]), float(want[0, 1]))
        both = await app.project_embeddings_onto_umap(embeddings=index.vecs[[250, 7]].tolist())
        assert both["placement"] == "transform:numpy" and len(both["x"]) == len(both["y"]) == 2
        assert abs(both["x"][0] - new["umap_x"]) < 1e-3  # the same cell but for the 1.01 (cosine: the same direction)
        assert "error" in await app.project_embeddings_onto_umap(embeddings=[[1.0] * 5])
        ext = await app.get_umap_preview(extend_to=300)
        assert len(ext["x"]) == 300 and ext["n_fitted"] == 240

    asyncio.run(main())
