"""2-D projection of embeddings for the landscape view (reference index_manager.py:185-271, K23).

``method="auto"`` uses umap-learn when importable, else the in-house UMAP on the GPU
(``search/umap.py``, ``csrc/kernels/umap.hip``) when a GPU and the native library are there, else a PCA
(``torch.pca_lowrank``), the reference's own fallback.  ``"umap"`` forces the in-house UMAP (on a host
without a GPU: its numpy oracle, slow, for small samples); ``"pca"`` forces the PCA.  Results are cached
in ``umap_cache.npz`` (plain arrays; no pickles) with the method and the engine that made them."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch


def palette(n: int) -> list[str]:
    import colorsys

    out = []
    for i in range(max(n, 1)):
        r, g, b = colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 0.65, 0.9)
        out.append("#%02x%02x%02x" % (int(r * 255), int(g * 255), int(b * 255)))
    return out


METHODS = ("auto", "umap", "pca")
N_NEIGHBORS = 15  # of every engine's UMAP here


def _pca_2d_model(vecs: np.ndarray, seed: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> ``(coords [n, 2], mean [d], V [d, 2])``: ``coords = (vecs - mean) @ V``."""
    dev = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    x = torch.from_numpy(np.asarray(vecs, np.float32)).to(dev)
    mean = x.mean(0, keepdim=True)
    x = x - mean
    torch.manual_seed(seed)
    _, _, V = torch.pca_lowrank(x, q=min(6, x.shape[1]), center=False)
    return (x @ V[:, :2]).cpu().numpy(), mean[0].cpu().numpy(), V[:, :2].cpu().numpy()


def _pca_2d(vecs: np.ndarray, seed: int) -> np.ndarray:
    return _pca_2d_model(vecs, seed)[0]


def _have_umap_learn() -> bool:
    try:
        from umap import UMAP  # noqa: F401

        return True
    except ImportError:
        return False


def resolve_method(method: str = "auto", n: int | None = None) -> tuple[str, str]:
    """-> ``(method, engine)`` the request runs as: ``("umap", "umap-learn" | "hip" | "numpy")`` or
    ``("pca", "pca")``.  ``n``: the sample size; ``"auto"`` never picks the in-house UMAP for a sample too
    small for its neighbour graph (``n <= n_neighbors``), ``"umap"`` raises there."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if method == "pca":
        return "pca", "pca"
    from ..ops import _native

    if method == "auto" and _have_umap_learn():
        return "umap", "umap-learn"
    if method == "auto" and n is not None and n <= N_NEIGHBORS:
        return "pca", "pca"
    if _native.hip_available():
        return "umap", "hip"
    return ("umap", "numpy") if method == "umap" else ("pca", "pca")


def project_2d_engine(vecs: np.ndarray, seed: int = 42, method: str = "auto", model: dict | None = None
                      ) -> tuple[np.ndarray, str, str]:
    """-> ``(coords [n, 2], method, engine)``.  ``model``: a dict that receives what places further points on
    the result without its training data (the PCA's ``pca_mean`` / ``pca_V``)."""
    method, engine = resolve_method(method, len(vecs))
    if engine == "umap-learn":
        from umap import UMAP

        coords = UMAP(n_neighbors=15, min_dist=0.1, metric="cosine", random_state=seed).fit_transform(vecs)
    elif engine == "hip":
        from .umap import UMAPParams, umap_fit_gpu

        Y, _ = umap_fit_gpu(np.asarray(vecs, np.float32), UMAPParams(seed=seed))
        coords = Y.cpu().numpy()
    elif engine == "numpy":
        from .reference import umap_fit
        from .umap import UMAPParams

        coords = umap_fit(np.asarray(vecs, np.float32), UMAPParams(seed=seed))
    else:
        coords, mean, V = _pca_2d_model(vecs, seed)
        if model is not None:
            model.update(pca_mean=mean, pca_V=V)
    return coords, method, engine


def project_2d(vecs: np.ndarray, seed: int = 42, method: str = "auto") -> tuple[np.ndarray, str]:
    coords, method, _ = project_2d_engine(vecs, seed, method)
    return coords, method


PLACEMENTS = ("auto", "transform", "nearest")
PLACE_CHUNK = 65536  # points per place_points call of an extension


def _placer(index, cache_path: Path, placement: str = "auto"):
    """-> ``(place(vecs [m, d]) -> coords [m, 2], how)`` for the landscape cached at ``cache_path``.  Needs only the
    cache's ``idx``, ``x``, ``y`` and the training vectors (``index.reconstruct_batch(idx)``), so it also places
    points on a landscape umap-learn made."""
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be one of {PLACEMENTS}, not {placement!r}")
    d = np.load(cache_path)
    idx = np.asarray(d["idx"])
    Yt = np.stack([d["x"], d["y"]], 1).astype(np.float32)
    stored = str(d["method"])
    if placement != "nearest" and stored == "umap" and len(idx) >= N_NEIGHBORS:
        from ..ops import _native
        from .umap import UMAPParams

        xt = np.asarray(index.reconstruct_batch(idx), np.float32)
        if _native.hip_available():
            from .umap import umap_transform_gpu

            xt_d, Yt_d = torch.from_numpy(xt).cuda(), torch.from_numpy(Yt).cuda()
            return (lambda v: umap_transform_gpu(np.asarray(v, np.float32), xt_d, Yt_d, UMAPParams())[0].cpu().numpy(),
                    "transform:hip")
        from .reference import umap_transform

        return lambda v: umap_transform(np.asarray(v, np.float32), xt, Yt, UMAPParams()), "transform:numpy"
    if placement != "nearest" and stored == "pca" and "pca_mean" in d.files and "pca_V" in d.files:
        mean, V = np.asarray(d["pca_mean"], np.float32), np.asarray(d["pca_V"], np.float32)
        return lambda v: (np.asarray(v, np.float32) - mean[None, :]) @ V, "pca"
    if placement == "transform":
        raise ValueError(f"the cached landscape ({stored!r}, {len(idx)} points) has no transform: it predates the "
                         "stored PCA axes or is too small for a neighbour table")

    def nearest(v):
        """The sampled cell whose index number is closest to the nearest indexed neighbour's."""
        _, nn = index.search(np.asarray(v, np.float32), 1)
        nn = np.asarray(nn).reshape(-1)
        j = np.abs(idx[None, :] - nn[:, None]).argmin(1)
        return np.where((nn >= 0)[:, None], Yt[j], np.float32(0))

    return nearest, "nearest"


def place_points(index, cache_path: Path, vecs: np.ndarray, placement: str = "auto") -> tuple[np.ndarray, str]:
    """New vectors ``[m, d]`` onto the cached landscape -> ``(coords [m, 2], how)``.  ``how``: ``"transform:hip"``
    (cached method ``"umap"``, the UMAP transform kernel), ``"transform:numpy"`` (the same rules by the numpy
    oracle where there is no HIP library), ``"pca"`` (a PCA cache that carries its mean and axes) or ``"nearest"``
    (the position of a sampled cell near the nearest indexed neighbour; what ``"auto"`` falls back to).
    ``placement="transform"`` raises where ``"auto"`` would fall back; ``"nearest"`` forces the old rule."""
    place, how = _placer(index, Path(cache_path), placement)
    vecs = np.asarray(vecs, np.float32).reshape(-1, np.shape(vecs)[-1])
    return np.asarray(place(vecs), np.float32).reshape(len(vecs), 2), how


def _extend(index, labels, cache_path: Path, base: dict, seed: int, extend_to: int, force: bool) -> dict:
    """``base`` plus a further seeded sample of indexed cells, disjoint from the fitted one, placed on the cached
    landscape and appended after the fitted points.  Cached in ``<cache stem>.ext.npz`` beside the base cache,
    reused only for the same base and request."""
    n_total, n_fit = base["n_total"], len(base["x"])
    want = min(int(extend_to), n_total)
    if want <= n_fit:
        return base
    ext_path = cache_path.with_name(cache_path.stem + ".ext.npz")
    meta = {"n_total": n_total, "method": base["method"], "engine": base["engine"], "n_fitted": n_fit, "seed": int(seed),
            "extend_to": int(extend_to)}
    e = None
    if ext_path.exists() and not force:
        e = np.load(ext_path)
        if any(k not in e.files or str(e[k]) != str(meta[k]) for k in meta):
            e = None
    if e is not None:
        xy, idx, how = np.stack([e["x"], e["y"]], 1), e["idx"], str(e["placement"])
        lab, col = [str(s) for s in e["labels"]], [str(s) for s in e["colors"]]
    else:
        rest = np.ones(n_total, bool)
        rest[np.asarray(base["sample_idx"], np.int64)] = False
        rest = np.nonzero(rest)[0]
        idx = np.sort(np.random.default_rng([int(seed), 1]).choice(rest, size=want - n_fit, replace=False))
        place, how = _placer(index, cache_path, "auto")
        xy = np.concatenate([np.asarray(place(np.asarray(index.reconstruct_batch(idx[i:i + PLACE_CHUNK]), np.float32)),
                                        np.float32).reshape(-1, 2) for i in range(0, len(idx), PLACE_CHUNK)])
        lab = [str(labels[i]) if labels is not None and i < len(labels) else "unknown" for i in idx]
        cmap = dict(zip(base["labels"], base["colors"]))  # the fitted sample's mapping; unseen labels take the next colours
        new = sorted(set(lab) - set(cmap))
        cmap.update(zip(new, palette(len(set(cmap)) + len(new))[len(set(cmap)):]))
        col = [cmap[s] for s in lab]
        np.savez(ext_path, x=xy[:, 0], y=xy[:, 1], labels=np.array(lab, dtype=str), colors=np.array(col, dtype=str),
                 idx=idx, placement=np.array(how), **{k: np.array(v) for k, v in meta.items()})
    out = dict(base)
    out.update(x=base["x"] + xy[:, 0].tolist(), y=base["y"] + xy[:, 1].tolist(), labels=base["labels"] + lab,
               colors=base["colors"] + col, sample_idx=base["sample_idx"] + np.asarray(idx).tolist(), n_fitted=n_fit,
               placement=how)
    return out


def compute_projection(index, labels: list[str] | None, cache_path: Path, n_samples: int = 10_000, seed: int = 42,
                       force: bool = False, tag: str = "", method: str = "auto", extend_to: int = 0) -> dict:
    """A cache is served only when its stored method is what ``method`` resolves to here and now: a worker
    that gained a GPU does not keep returning the PCA of its earlier life.  ``extend_to`` above the fitted
    sample size places further cells on the fitted landscape (``place_points``) up to that many points; the
    dict then gains ``n_fitted`` and ``placement``.  With 0 the dict and the cache file are the fit's alone."""
    cache_path = Path(cache_path)
    base = _fit_projection(index, labels, cache_path, n_samples, seed, force, method)
    if extend_to and base["method"] != "none":
        return _extend(index, labels, cache_path, base, seed, extend_to, force)
    return base


def _fit_projection(index, labels, cache_path: Path, n_samples: int, seed: int, force: bool, method: str) -> dict:
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    n_total = index.ntotal if index is not None else 0
    if cache_path.exists() and not force:
        d = np.load(cache_path)
        stored = str(d["method"])
        n_req = min(n_samples, n_total) if n_total else len(d["x"])
        if stored == resolve_method(method, n_req)[0]:
            engine = str(d["engine"]) if "engine" in d.files else ("pca" if stored == "pca" else "umap-learn")
            return {"x": d["x"].tolist(), "y": d["y"].tolist(), "labels": [str(s) for s in d["labels"]],
                    "colors": [str(s) for s in d["colors"]], "n_total": int(d["n_total"]),
                    "sample_idx": d["idx"].tolist(), "method": stored, "engine": engine}
    if n_total == 0:
        return {"x": [], "y": [], "labels": [], "colors": [], "n_total": 0, "sample_idx": [], "method": "none",
                "engine": "none"}
    n = min(n_samples, n_total)
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(n_total, size=n, replace=False))
    model: dict = {}
    coords, method, engine = project_2d_engine(index.reconstruct_batch(idx), seed, method, model)
    lab = [str(labels[i]) if labels is not None and i < len(labels) else "unknown" for i in idx]
    uniq = sorted(set(lab))
    cmap = dict(zip(uniq, palette(len(uniq))))
    col = [cmap[s] for s in lab]
    cache_path.parent.mkdir(parents=True, exist_ok=True)
    np.savez(cache_path, x=coords[:, 0], y=coords[:, 1], labels=np.array(lab, dtype=str), colors=np.array(col, dtype=str),
             n_total=np.array(n_total), idx=idx, method=np.array(method), engine=np.array(engine), **model)
    return {"x": coords[:, 0].tolist(), "y": coords[:, 1].tolist(), "labels": lab, "colors": col, "n_total": n_total,
            "sample_idx": idx.tolist(), "method": method, "engine": engine}
