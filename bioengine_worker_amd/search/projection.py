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


def _pca_2d(vecs: np.ndarray, seed: int) -> np.ndarray:
    dev = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    x = torch.from_numpy(np.asarray(vecs, np.float32)).to(dev)
    x = x - x.mean(0, keepdim=True)
    torch.manual_seed(seed)
    _, _, V = torch.pca_lowrank(x, q=min(6, x.shape[1]), center=False)
    return (x @ V[:, :2]).cpu().numpy()


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


def project_2d_engine(vecs: np.ndarray, seed: int = 42, method: str = "auto") -> tuple[np.ndarray, str, str]:
    """-> ``(coords [n, 2], method, engine)``."""
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
        coords = _pca_2d(vecs, seed)
    return coords, method, engine


def project_2d(vecs: np.ndarray, seed: int = 42, method: str = "auto") -> tuple[np.ndarray, str]:
    coords, method, _ = project_2d_engine(vecs, seed, method)
    return coords, method


def compute_projection(index, labels: list[str] | None, cache_path: Path, n_samples: int = 10_000, seed: int = 42,
                       force: bool = False, tag: str = "", method: str = "auto") -> dict:
    """A cache is served only when its stored method is what ``method`` resolves to here and now: a worker
    that gained a GPU does not keep returning the PCA of its earlier life."""
    cache_path = Path(cache_path)
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
    coords, method, engine = project_2d_engine(index.reconstruct_batch(idx), seed, method)
    lab = [str(labels[i]) if labels is not None and i < len(labels) else "unknown" for i in idx]
    uniq = sorted(set(lab))
    cmap = dict(zip(uniq, palette(len(uniq))))
    col = [cmap[s] for s in lab]
    cache_path.parent.mkdir(parents=True, exist_ok=True)
    np.savez(cache_path, x=coords[:, 0], y=coords[:, 1], labels=np.array(lab, dtype=str), colors=np.array(col, dtype=str),
             n_total=np.array(n_total), idx=idx, method=np.array(method), engine=np.array(engine))
    return {"x": coords[:, 0].tolist(), "y": coords[:, 1].tolist(), "labels": lab, "colors": col, "n_total": n_total,
            "sample_idx": idx.tolist(), "method": method, "engine": engine}
