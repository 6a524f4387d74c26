"""CPU oracle of the cell-image-search pre-processing (numpy + PIL), mirroring the reference's
normalizer.py:32-153 and ingestion.py:317-387 semantics.  Used by tests and as the CPU path.

UMAP for the landscape view (second half of the file; the oracle of ``search/umap.py`` and
``csrc/kernels/umap.hip``).  The rules are written from memory of umap-learn 0.5 (``UMAP(n_neighbors=15, min_dist=0.1,
metric="cosine")``, two components).  umap-learn is not installed where this project is built and
tested, so NOTHING here has been compared with it; the oracle is the definition the GPU path is
tested against, stage by stage.

Deliberate departures from umap-learn:

1. The layout step is SYNCHRONOUS (every position read in an epoch is of the epoch's input) and its
   negative samples come from a stateless counter hash of (edge, seed, epoch, sample).  umap-learn
   updates positions in place, edge by edge, with a per-vertex ``tau_rand`` state.  The synchronous
   form is what makes a GPU run bitwise reproducible and comparable with an oracle at all.
2. The initialisation is PCA (umap-learn's ``init="pca"``), not the spectral layout.
3. No noise is added to the initial coordinates.

Precision: the neighbour table, the bisection and the memberships take a ``dtype`` (float64 is the
rule, float32 the yardstick the GPU tests measure rounding with); the symmetric weights and the whole
schedule state are float32 with every operation rounded on its own.

UMAP ``transform`` of new points onto a fitted layout (third part of the file; ``umap_transform``), again
from memory of umap-learn 0.5 and never compared with it.  Every rule is PER QUERY, so a query's result
depends on nothing else in its batch.  Deliberate departures, beside the synchronous epoch above:

4. ``rho`` is the row's minimum distance, zero included (umap-learn: ``rho = 0``), all ``k`` columns are
   summed in the bisection (umap-learn skips column 0), and the floor of ``sigma`` is 1e-3 of the row's
   own mean (umap-learn: of the mean over the whole query batch, which ties a result to its batch).
   ``rho = min`` instead of "smallest positive" keeps the rule continuous when a query duplicates an
   indexed point and a float32 GEMM returns ``1e-8`` instead of ``0``.  The nearest training point always
   has membership exactly 1.
5. A slot is pruned when ``w < 1 / E``: umap-learn's ``max / n_epochs`` with the row maximum (always 1)
   in place of the batch-wide maximum.
6. ``E`` is 100 whatever the number of queries (umap-learn: 100 or 30 by batch size).
7. The negative samples of a query are keyed by its nearest training point and the slot, not by the
   query's place in the batch.
"""
from __future__ import annotations

import numpy as np

IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], np.float32)
JUMP_CH_DNA, JUMP_CH_ER, JUMP_CH_RNA, JUMP_CH_AGP, JUMP_CH_MITO = 0, 1, 2, 3, 4


def percentile_stretch(img: np.ndarray, plow: float = 1.0, phigh: float = 99.0) -> np.ndarray:
    lo, hi = np.percentile(img, plow), np.percentile(img, phigh)
    if hi <= lo:
        hi = lo + 1.0
    t = (img.astype(np.float32) - lo) / (hi - lo)
    return (np.clip(t, 0.0, 1.0) * 255.0).astype(np.uint8)


def channel_map(n_ch: int, rgb_channels=None) -> list[int]:
    """Source channel per RGB output; -1 means (ch0 + ch1) / 2 (two-channel images)."""
    if rgb_channels is not None:
        return list(rgb_channels)
    if n_ch == 1:
        return [0, 0, 0]
    if n_ch == 2:
        return [0, 1, -1]
    if n_ch == 3 or n_ch == 4:
        return [0, 1, 2]
    return [JUMP_CH_AGP, JUMP_CH_ER, JUMP_CH_DNA]


def to_hwc(img: np.ndarray) -> np.ndarray:
    if img.ndim == 3 and img.shape[0] <= 7 and img.shape[0] < img.shape[2]:
        img = np.moveaxis(img, 0, -1)
    if img.ndim == 2:
        img = img[..., None]
    return img


def to_rgb_uint8(img: np.ndarray, rgb_channels=None, plow: float = 1.0, phigh: float = 99.0) -> np.ndarray:
    img = to_hwc(img)
    cm = channel_map(img.shape[-1], rgb_channels)
    out = np.zeros(img.shape[:2] + (3,), np.uint8)
    for c, sc in enumerate(cm):
        src = img[..., sc] if sc >= 0 else (img[..., 0].astype(np.float32) + img[..., 1]) / 2
        out[..., c] = percentile_stretch(src, plow, phigh)
    return out


def to_dinov2_array(img_rgb_uint8: np.ndarray, size: int = 224) -> np.ndarray:
    from PIL import Image

    pil = Image.fromarray(img_rgb_uint8, mode="RGB").resize((size, size), Image.BICUBIC)
    arr = np.asarray(pil, dtype=np.float32) / 255.0
    return ((arr - IMAGENET_MEAN) / IMAGENET_STD).transpose(2, 0, 1)


def otsu_threshold_u8(img: np.ndarray) -> int:
    """skimage.filters.threshold_otsu on an integer image (histogram over [min, max])."""
    v = img.ravel().astype(np.int64)
    mn = int(v.min())
    hist = np.bincount(v - mn).astype(np.float64)
    centers = np.arange(mn, mn + hist.size, dtype=np.float64)
    if hist.size == 1:
        return mn
    w1 = np.cumsum(hist)
    w2 = np.cumsum(hist[::-1])[::-1]
    m1 = np.cumsum(hist * centers) / np.maximum(w1, 1e-300)
    m2 = (np.cumsum((hist * centers)[::-1]) / np.maximum(w2[::-1], 1e-300))[::-1]
    var = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return int(centers[int(np.argmax(var))])


def label8(mask: np.ndarray) -> np.ndarray:
    """8-connected components, labels 1..n in raster order of each component's first pixel."""
    from scipy import ndimage

    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    # ndimage numbers components in raster order of first pixel as well
    return lab


def nucleus_centroids(image: np.ndarray, n_crops: int = 100, dna_channel: int = 0, min_area: int = 200):
    img = to_hwc(image)
    dna = img[..., dna_channel].astype(np.float32)
    dn = percentile_stretch(dna)
    mask = dn > otsu_threshold_u8(dn)
    lab = label8(mask)
    n = int(lab.max())
    if n == 0:
        return []
    idx = np.arange(1, n + 1)
    from scipy import ndimage

    area = ndimage.sum(np.ones_like(lab), lab, idx)
    cy, cx = np.array(ndimage.center_of_mass(np.ones_like(lab), lab, idx)).T
    keep = [i for i in range(n) if area[i] > min_area]
    keep.sort(key=lambda i: -area[i])
    return [(int(cy[i]), int(cx[i])) for i in keep[:n_crops]]


def grid_centroids(H: int, W: int, crop_size: int, n_crops: int):
    half = crop_size // 2
    stride = max(crop_size, min(H, W) // max(1, int(np.sqrt(n_crops))))
    return [(y + half, x + half) for y in range(half, H - half, stride) for x in range(half, W - half, stride)][:n_crops]


def crops_at(image: np.ndarray, centroids, crop_size: int = 224):
    img = to_hwc(image)
    H, W = img.shape[:2]
    half = crop_size // 2
    out = []
    for cy, cx in centroids:
        y0, x0 = cy - half, cx - half
        if y0 < 0 or x0 < 0 or y0 + crop_size > H or x0 + crop_size > W:
            continue
        out.append(img[y0:y0 + crop_size, x0:x0 + crop_size])
    return out


def extract_cell_crops(image: np.ndarray, crop_size: int = 224, n_crops: int = 100, dna_channel: int = 0):
    img = to_hwc(image)
    H, W = img.shape[:2]
    try:
        cents = nucleus_centroids(img, n_crops, dna_channel)
    except Exception:  # noqa: BLE001
        cents = []
    if len(cents) < 10:
        cents = grid_centroids(H, W, crop_size, n_crops)
    return crops_at(img, cents[:n_crops], crop_size)


# ---------------------------------------------------------------------------------------------------
# UMAP for the landscape view: the numpy oracle of search/umap.py and csrc/kernels/umap.hip
# ---------------------------------------------------------------------------------------------------
UMAP_METRICS = ("cosine", "euclidean")
SMOOTH_K_TOLERANCE = 1e-5
MIN_K_DIST_SCALE = 1e-3
_F32 = np.float32


def umap_ab(spread: float = 1.0, min_dist: float = 0.1) -> tuple[float, float]:
    """Least-squares fit of ``1 / (1 + a x^(2b))`` to ``1 if x < min_dist else exp(-(x - min_dist) / spread)``
    sampled on ``linspace(0, 3 spread, 300)`` (umap's ``find_ab_params``)."""
    from scipy.optimize import curve_fit

    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(a), float(b)


def knn_table(x: np.ndarray, k: int, metric: str = "cosine", dtype=np.float64):
    """-> ``idx [n, k]`` int32, ``dist [n, k]`` float32.  ``k`` counts the point itself: column 0 is
    forced to ``(i, 0.0)``, the others are the ``k - 1`` nearest OTHER points, ascending (ties by index)."""
    if metric not in UMAP_METRICS:
        raise ValueError(f"metric must be one of {UMAP_METRICS}")
    x = np.asarray(x, dtype)
    n = x.shape[0]
    if not n > k:
        raise ValueError(f"need more points ({n}) than n_neighbors ({k})")
    if metric == "cosine":
        nrm = np.sqrt((x * x).sum(1))
        if (nrm == 0).any():
            raise ValueError("cosine metric: zero-norm row")
        xn = x / nrm[:, None]
        d = np.maximum(0, 1 - xn @ xn.T)
    else:
        sq = (x * x).sum(1)
        d = np.sqrt(np.maximum(0, sq[:, None] + sq[None, :] - 2 * (x @ x.T)))
    np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind="stable")[:, : k - 1]
    idx = np.concatenate([np.arange(n)[:, None], order], 1).astype(np.int32)
    dist = np.concatenate([np.zeros((n, 1), d.dtype), np.take_along_axis(d, order, 1)], 1).astype(_F32)
    return idx, dist


def smooth_knn(dist: np.ndarray, dtype=np.float64, n_iter: int = 64):
    """umap's ``smooth_knn_dist`` with ``local_connectivity = 1``, ``bandwidth = 1`` -> ``rho [n]``,
    ``sigma [n]`` in ``dtype``.  ``rho_i`` is the smallest strictly positive entry of row i (0 without
    one); ``sigma_i`` the bisection of ``sum_{j>=1} (exp(-(d_ij - rho_i) / sigma) if d_ij > rho_i else 1)``
    to ``log2(k)``, floored at 1e-3 of the row's mean (of the global mean when ``rho_i == 0``)."""
    d = np.asarray(dist, _F32).astype(dtype)
    n, k = d.shape
    one = dtype(1)
    target = dtype(np.log2(dtype(k)))
    gmean = d.mean(dtype=dtype)
    rho = np.zeros(n, dtype)
    sigma = np.zeros(n, dtype)
    for i in range(n):
        row = d[i]
        pos = row[row > 0]
        r = pos.min() if pos.size else dtype(0)
        gap = row[1:] - r
        lo, hi, mid = dtype(0), dtype(np.inf), one
        for _ in range(n_iter):
            psum = np.where(gap > 0, np.exp(-(np.maximum(gap, 0) / mid)), one).sum(dtype=dtype)
            if abs(psum - target) < SMOOTH_K_TOLERANCE:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / dtype(2)
            else:
                lo = mid
                mid = mid * dtype(2) if np.isinf(hi) else (lo + hi) / dtype(2)
        floor = dtype(MIN_K_DIST_SCALE) * (row.mean(dtype=dtype) if r > 0 else gmean)
        rho[i] = r
        sigma[i] = max(mid, floor)
    return rho, sigma


def memberships(idx: np.ndarray, dist: np.ndarray, rho: np.ndarray, sigma: np.ndarray) -> np.ndarray:
    """Directed memberships ``a [n, k-1]`` (float32) of columns 1..k-1, computed in ``rho.dtype``:
    1 when ``d - rho <= 0`` or ``sigma == 0``, else ``exp(-(d - rho) / sigma)``; 0 for a listed self."""
    dt = rho.dtype.type
    gap = np.asarray(dist, _F32).astype(dt)[:, 1:] - rho[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where((gap <= 0) | (sigma[:, None] == 0), dt(1), np.exp(-(np.maximum(gap, 0) / sigma[:, None])))
    a = np.where(idx[:, 1:] == np.arange(idx.shape[0])[:, None], dt(0), a)
    return a.astype(_F32)


def default_n_epochs(n: int) -> int:
    return 500 if n <= 10000 else 200


def fuzzy_union(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """``fmaf(-a, b, a + b)`` in float32: the sum is rounded to float32, the product of two float32 is
    exact in float64, the difference is rounded once to float64 and once to float32.  Symmetric in its
    arguments bit for bit, so ``w_ij == w_ji`` exactly; the layout schedule relies on that."""
    a = np.asarray(a, _F32)
    b = np.asarray(b, _F32)
    return ((a + b).astype(np.float64) - a.astype(np.float64) * b.astype(np.float64)).astype(_F32)


def fuzzy_graph(idx: np.ndarray, dist: np.ndarray, n_epochs: int | None = None, dtype=np.float64):
    """Neighbour table -> symmetric CSR ``(row_ptr int64 [n+1], col int32, w float32)``: the fuzzy union of
    the directed memberships over every pair present in either direction, pairs with
    ``w < max(w) / n_epochs`` dropped, columns ascending within a row.  A row of ``idx`` must not list
    a vertex twice (a neighbour table never does)."""
    idx = np.asarray(idx)
    n, k = idx.shape
    if n_epochs is None:
        n_epochs = default_n_epochs(n)
    rho, sigma = smooth_knn(dist, dtype)
    a = memberships(idx, dist, rho, sigma)
    rows = np.repeat(np.arange(n, dtype=np.int64), k - 1)
    cols = idx[:, 1:].astype(np.int64).ravel()
    av = a.ravel()
    keep = rows != cols
    rows, cols, av = rows[keep], cols[keep], av[keep]
    key = rows * n + cols
    if np.unique(key).size != key.size:
        raise ValueError("a row of idx lists a vertex twice")
    order = np.argsort(key)
    skey, sa = key[order], av[order]
    rkey = cols * n + rows  # the reciprocal direction; an absent one counts as 0
    p = np.minimum(np.searchsorted(skey, rkey), skey.size - 1)
    rec = np.where(skey[p] == rkey, sa[p], _F32(0)).astype(_F32)
    w = fuzzy_union(av, rec)
    ukey, first = np.unique(np.concatenate([key, rkey]), return_index=True)
    uw = np.concatenate([w, w])[first]
    thr = _F32(uw.max()) / _F32(n_epochs)
    live = uw >= thr
    ukey, uw = ukey[live], uw[live]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(ukey // n, minlength=n))]).astype(np.int64)
    return row_ptr, (ukey % n).astype(np.int32), uw.astype(_F32)


def prune_threshold(w: np.ndarray, n_epochs: int) -> np.float32:
    return _F32(np.max(w)) / _F32(n_epochs)


def layout_state(w: np.ndarray, negative_sample_rate: int = 5) -> dict:
    """Per directed edge, float32: ``eps = max(w) / w``, ``epn = eps / negative_sample_rate``,
    ``next = eps``, ``nneg = epn``."""
    w = np.asarray(w, _F32)
    eps = (_F32(w.max()) / w).astype(_F32)
    epn = (eps / _F32(negative_sample_rate)).astype(_F32)
    return {"eps": eps, "epn": epn, "next": eps.copy(), "nneg": epn.copy()}


def mix(x):
    """The 32-bit mixer of the negative sampler (uint32 in, uint32 out; arrays or scalars)."""
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def negative_vertex(e, seed: int, ep: int, p: int, n: int):
    """``mix(mix(mix(e ^ seed) + ep) + p) % n`` on uint32."""
    with np.errstate(over="ignore"):
        r = mix(mix(mix(np.asarray(e, np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)) + np.uint32(ep)) + np.uint32(p))
    return (r % np.uint32(n)).astype(np.int64)


def epoch_alpha(ep: int, n_epochs: int, lr: float = 1.0) -> np.float32:
    """``lr`` rounded to float32, the product in float64, rounded to float32."""
    return _F32(float(_F32(lr)) * (1.0 - ep / n_epochs))


def layout_epoch(Y: np.ndarray, graph, state: dict, ep: int, n_epochs: int, a: float, b: float, seed: int,
                 gamma: float = 1.0, lr: float = 1.0, dtype=np.float32, return_counts: bool = False):
    """ONE synchronous epoch: ``Y [n, 2]`` -> new ``Y`` (in ``dtype``) and the new state.  ``a``, ``b``,
    ``gamma`` and ``alpha`` enter rounded to float32; forces are evaluated in ``dtype`` (``d2^(b-1)`` as
    ``d2^b / d2``); the schedule is float32 whatever ``dtype`` is."""
    row_ptr, col, _ = graph
    n = Y.shape[0]
    dt = np.dtype(dtype).type
    Yd = np.asarray(Y).astype(dt)
    a, b, gamma = dt(_F32(a)), dt(_F32(b)), dt(_F32(gamma))
    alpha = dt(epoch_alpha(ep, n_epochs, lr))
    head = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    epf = _F32(ep)
    eps, epn, nxt, nneg = (np.asarray(state[s], _F32) for s in ("eps", "epn", "next", "nneg"))
    act = np.nonzero(nxt <= epf)[0]
    delta = np.zeros((n, 2), dt)
    four = dt(4)

    def clip(v):
        return np.clip(v, -four, four)

    j = head[act]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = Yd[j] - Yd[col[act]]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        pw = np.power(d2, b)
        c = np.where(d2 > 0, dt(-2) * a * b * (pw / d2) / (a * pw + dt(1)), dt(0))
        np.add.at(delta, j, dt(2) * clip(c[:, None] * d) * alpha)
        m = np.maximum(((epf - nneg[act]).astype(_F32) / epn[act]).astype(_F32).astype(np.int64), 0)
        for p in range(int(m.max()) if m.size else 0):
            sel = m > p
            e, js = act[sel], j[sel]
            v = negative_vertex(e, seed, ep, p, n)
            d = Yd[js] - Yd[v]
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            pw = np.power(d2, b)
            c = dt(2) * gamma * b / ((dt(0.001) + d2) * (a * pw + dt(1)))
            ok = (v != js) & (d2 > 0)
            np.add.at(delta, js[ok], clip(c[ok, None] * d[ok]) * alpha)
    new = {"eps": eps, "epn": epn, "next": nxt.copy(), "nneg": nneg.copy()}
    new["next"][act] = (nxt[act] + eps[act]).astype(_F32)
    new["nneg"][act] = (nneg[act] + (m.astype(_F32) * epn[act]).astype(_F32)).astype(_F32)
    out = (Yd + delta).astype(dt)
    if return_counts:
        full = np.zeros(nxt.size, np.int64)
        full[act] = m
        return out, new, full
    return out, new


def umap_layout(Y0: np.ndarray, graph, n_epochs: int, a: float, b: float, seed: int = 42, gamma: float = 1.0,
                lr: float = 1.0, negative_sample_rate: int = 5, dtype=np.float32, stop: int | None = None,
                return_state: bool = False):
    """The loop over ``ep = 0 .. n_epochs - 1`` (``stop``: return what epoch ``stop`` would read)."""
    Y = np.asarray(Y0).astype(dtype)
    st = layout_state(graph[2], negative_sample_rate)
    for ep in range(n_epochs if stop is None else stop):
        Y, st = layout_epoch(Y, graph, st, ep, n_epochs, a, b, seed, gamma, lr, dtype)
    return (Y, st) if return_state else Y


def pca_init(x: np.ndarray) -> np.ndarray:
    """The first two principal axes, each column of V signed so that its largest-magnitude entry is
    positive, each axis mapped affinely to [0, 10] -> float32 [n, 2]."""
    x = np.asarray(x, np.float64)
    xc = x - x.mean(0, keepdims=True)
    evals, evecs = np.linalg.eigh(xc.T @ xc)
    V = evecs[:, ::-1][:, :2]
    V = V * np.sign(V[np.abs(V).argmax(0), np.arange(2)])[None, :]
    p = xc @ V
    lo, hi = p.min(0), p.max(0)
    return (10.0 * (p - lo) / np.where(hi > lo, hi - lo, 1.0)).astype(_F32)


def umap_fit(x: np.ndarray, params=None, dtype=np.float32) -> np.ndarray:
    """Everything chained: table, graph, PCA initialisation (or ``params.init`` as an ``[n, 2]`` array),
    layout.  ``params`` is a ``search.umap.UMAPParams`` (defaults when None) -> float32 ``[n, 2]``."""
    if params is None:
        from .umap import UMAPParams

        params = UMAPParams()
    x = np.asarray(x)
    check_umap_limits(x.shape[0], params.n_neighbors, params.metric)
    if not np.isfinite(x).all():
        raise ValueError("non-finite input")
    n = x.shape[0]
    n_epochs = params.n_epochs or default_n_epochs(n)
    a, b = umap_ab(params.spread, params.min_dist)
    idx, dist = knn_table(x, params.n_neighbors, params.metric)
    graph = fuzzy_graph(idx, dist, n_epochs)
    if isinstance(params.init, str):
        if params.init != "pca":
            raise ValueError('init must be "pca" or an [n, 2] array')
        Y0 = pca_init(x)
    else:
        Y0 = np.asarray(params.init, _F32)
        if Y0.shape != (n, 2):
            raise ValueError("init array must be [n, 2]")
    Y = umap_layout(Y0, graph, n_epochs, a, b, params.seed, params.repulsion_strength, params.learning_rate,
                    params.negative_sample_rate, dtype)
    return np.asarray(Y, _F32)


def check_umap_limits(n: int, n_neighbors: int, metric: str = "cosine") -> None:
    if metric not in UMAP_METRICS:
        raise ValueError(f"metric must be one of {UMAP_METRICS}")
    if not 2 <= n_neighbors <= 64:
        raise ValueError("n_neighbors must be in 2..64")
    if n <= n_neighbors:
        raise ValueError(f"need more points ({n}) than n_neighbors ({n_neighbors})")
    if n >= 2 ** 31 // n_neighbors:
        raise ValueError("too many points: n * n_neighbors must stay below 2^31")


# ---------------------------------------------------------------------------------------------------
# UMAP transform: new points onto a fitted layout (oracle of search/umap.py's umap_transform_gpu)
# ---------------------------------------------------------------------------------------------------
TRANSFORM_EPOCHS = 100
TRANSFORM_MAX_DRAWS = 4096  # negative samples of one slot in one epoch; unreachable from a schedule run from its start


def transform_n_epochs(params=None) -> int:
    """``params.transform_epochs``, 100 when None: never a function of the number of queries."""
    e = getattr(params, "transform_epochs", None)
    e = TRANSFORM_EPOCHS if e is None else int(e)
    if e < 1:
        raise ValueError("transform_epochs must be at least 1")
    return e


def check_transform_limits(m: int, n: int, k: int, metric: str = "cosine") -> None:
    if metric not in UMAP_METRICS:
        raise ValueError(f"metric must be one of {UMAP_METRICS}")
    if not 1 <= k <= 64:
        raise ValueError("n_neighbors must be in 1..64")
    if k > n:
        raise ValueError(f"need at least n_neighbors ({k}) training points, not {n}")
    if n >= 2 ** 31 // 64 or m >= 2 ** 31 // k:
        raise ValueError("too many points: n * 64 and m * n_neighbors must stay below 2^31")


def knn_query_table(q: np.ndarray, x: np.ndarray, k: int, metric: str = "cosine", dtype=np.float64):
    """``q [m, d]`` against the training rows ``x [n, d]`` -> ``idx [m, k]`` int32, ``dist [m, k]`` float32: the
    ``k`` nearest training rows, ascending (ties by index).  No self column: a query is not a training row.
    The distance formulas are ``knn_table``'s."""
    q, x = np.asarray(q, dtype), np.asarray(x, dtype)
    if q.ndim != 2 or x.ndim != 2 or q.shape[1] != x.shape[1]:
        raise ValueError(f"q {q.shape} and x {x.shape} must be [m, d] and [n, d]")
    check_transform_limits(q.shape[0], x.shape[0], k, metric)
    if not (np.isfinite(q).all() and np.isfinite(x).all()):
        raise ValueError("non-finite input")
    if metric == "cosine":
        qn, xn = np.sqrt((q * q).sum(1)), np.sqrt((x * x).sum(1))
        if (qn == 0).any() or (xn == 0).any():
            raise ValueError("cosine metric: zero-norm row")
        d = np.maximum(0, 1 - (q / qn[:, None]) @ (x / xn[:, None]).T)
    else:
        d = np.sqrt(np.maximum(0, (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2 * (q @ x.T)))
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(d, order, 1).astype(_F32).reshape(q.shape[0], k)


def smooth_knn_query(dist: np.ndarray, dtype=np.float64, n_iter: int = 64):
    """``dist [m, k]`` (no self column) -> ``rho [m]``, ``sigma [m]`` in ``dtype``.  ``rho_i`` is the row's minimum,
    zero included; ``sigma_i`` the bisection of ``smooth_knn`` over ALL k columns towards ``log2(k)``, floored at
    1e-3 of the row's own mean."""
    d = np.asarray(dist, _F32).astype(dtype)
    m, k = d.shape
    one = dtype(1)
    target = dtype(np.log2(dtype(k)))
    rho = np.zeros(m, dtype)
    sigma = np.zeros(m, dtype)
    for i in range(m):
        row = d[i]
        r = row.min()
        gap = row - r
        lo, hi, mid = dtype(0), dtype(np.inf), one
        for _ in range(n_iter):
            psum = np.where(gap > 0, np.exp(-(np.maximum(gap, 0) / mid)), one).sum(dtype=dtype)
            if abs(psum - target) < SMOOTH_K_TOLERANCE:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / dtype(2)
            else:
                lo = mid
                mid = mid * dtype(2) if np.isinf(hi) else (lo + hi) / dtype(2)
        rho[i] = r
        sigma[i] = max(mid, dtype(MIN_K_DIST_SCALE) * row.mean(dtype=dtype))
    return rho, sigma


def memberships_query(dist: np.ndarray, rho: np.ndarray, sigma: np.ndarray) -> np.ndarray:
    """``w [m, k]`` (float32), computed in ``rho.dtype``: 1 where ``d - rho <= 0`` or ``sigma == 0``, else
    ``exp(-(d - rho) / sigma)``.  Not symmetrised: these are the edge weights of the transform."""
    dt = rho.dtype.type
    gap = np.asarray(dist, _F32).astype(dt) - rho[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where((gap <= 0) | (sigma[:, None] == 0), dt(1), np.exp(-(np.maximum(gap, 0) / sigma[:, None])))
    return w.astype(_F32)


def transform_state(w: np.ndarray, n_epochs: int, negative_sample_rate: int = 5) -> dict:
    """Per slot, float32, as ``layout_state`` with the row maximum 1: ``eps = 1 / w``, ``epn = eps /
    negative_sample_rate``, ``next = eps``, ``nneg = epn``; ``live`` is False where ``w < 1 / n_epochs`` (such a
    slot never fires)."""
    w = np.asarray(w, _F32)
    with np.errstate(divide="ignore"):
        eps = (_F32(1) / w).astype(_F32)
        epn = (eps / _F32(negative_sample_rate)).astype(_F32)
    return {"eps": eps, "epn": epn, "next": eps.copy(), "nneg": epn.copy(), "live": w >= _F32(1) / _F32(n_epochs)}


def transform_init(idx: np.ndarray, w: np.ndarray, Y_train: np.ndarray) -> np.ndarray:
    """The start of a query: the mean of its neighbours' training positions weighted by ``w`` over all k slots
    (the later pruned ones included), summed in float64 -> float32 ``[m, 2]``."""
    w64 = np.asarray(w, _F32).astype(np.float64)
    Yn = np.asarray(Y_train, _F32).astype(np.float64)[np.asarray(idx, np.int64)]
    return ((w64[:, :, None] * Yn).sum(1) / w64.sum(1)[:, None]).astype(_F32)


def transform_key(idx: np.ndarray) -> np.ndarray:
    """The sampler key of every slot, ``uint32(idx[i, 0]) * 64 + slot``: intrinsic to the query."""
    idx = np.asarray(idx)
    return (idx[:, :1].astype(np.uint32) * np.uint32(64) + np.arange(idx.shape[1], dtype=np.uint32)[None, :]).astype(np.uint32)


def transform_epoch(Y: np.ndarray, Y_train: np.ndarray, idx: np.ndarray, state: dict, ep: int, n_epochs: int, a: float,
                    b: float, seed: int, gamma: float = 1.0, lr: float = 1.0, dtype=np.float32,
                    return_counts: bool = False):
    """ONE synchronous epoch of the transform: ``layout_epoch`` where only the queries ``Y [m, 2]`` move and the
    training positions are fixed.  The attractive term carries factor 1 (the edge exists in one direction),
    ``alpha = epoch_alpha(ep, n_epochs, float32(lr) / 4)``, a negative sample is the TRAINING vertex
    ``negative_vertex(transform_key, seed, ep, p, n_train)``, skipped at ``d2 == 0``; there is no self to exclude."""
    dt = np.dtype(dtype).type
    Yd = np.asarray(Y).astype(dt)
    Yt = np.asarray(Y_train, _F32).astype(dt)
    n = Yt.shape[0]
    idx = np.asarray(idx, np.int64)
    m, k = idx.shape
    a, b, gamma = dt(_F32(a)), dt(_F32(b)), dt(_F32(gamma))
    alpha = dt(epoch_alpha(ep, n_epochs, _F32(lr) / _F32(4)))
    epf = _F32(ep)
    eps, epn, nxt, nneg = (np.asarray(state[s], _F32).reshape(-1) for s in ("eps", "epn", "next", "nneg"))
    head = np.repeat(np.arange(m, dtype=np.int64), k)
    col = idx.reshape(-1)
    key = transform_key(idx).reshape(-1)
    act = np.nonzero(np.asarray(state["live"], bool).reshape(-1) & (nxt <= epf))[0]
    delta = np.zeros((m, 2), dt)
    four = dt(4)

    def clip(v):
        return np.clip(v, -four, four)

    j = head[act]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = Yd[j] - Yt[col[act]]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        pw = np.power(d2, b)
        c = np.where(d2 > 0, dt(-2) * a * b * (pw / d2) / (a * pw + dt(1)), dt(0))
        np.add.at(delta, j, clip(c[:, None] * d) * alpha)
        cnt = np.maximum(((epf - nneg[act]).astype(_F32) / epn[act]).astype(_F32).astype(np.int64), 0)
        cnt = np.minimum(cnt, TRANSFORM_MAX_DRAWS)
        for p in range(int(cnt.max()) if cnt.size else 0):
            sel = cnt > p
            js = j[sel]
            v = negative_vertex(key[act[sel]], seed, ep, p, n)
            d = Yd[js] - Yt[v]
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            pw = np.power(d2, b)
            c = dt(2) * gamma * b / ((dt(0.001) + d2) * (a * pw + dt(1)))
            ok = d2 > 0
            np.add.at(delta, js[ok], clip(c[ok, None] * d[ok]) * alpha)
    new_next, new_nneg = nxt.copy(), nneg.copy()
    new_next[act] = (nxt[act] + eps[act]).astype(_F32)
    new_nneg[act] = (nneg[act] + (cnt.astype(_F32) * epn[act]).astype(_F32)).astype(_F32)
    new = {"eps": state["eps"], "epn": state["epn"], "live": state["live"], "next": new_next.reshape(m, k),
           "nneg": new_nneg.reshape(m, k)}
    out = (Yd + delta).astype(dt)
    if return_counts:
        full = np.zeros(m * k, np.int64)
        full[act] = cnt
        return out, new, full.reshape(m, k)
    return out, new


def umap_transform_layout(Y0: np.ndarray, Y_train: np.ndarray, idx: np.ndarray, w: np.ndarray, n_epochs: int, a: float,
                          b: float, seed: int = 42, gamma: float = 1.0, lr: float = 1.0, negative_sample_rate: int = 5,
                          dtype=np.float32, stop: int | None = None, return_state: bool = False):
    """The loop over ``ep = 0 .. n_epochs - 1`` (``stop``: return what epoch ``stop`` would read)."""
    Y = np.asarray(Y0).astype(dtype)
    st = transform_state(w, n_epochs, negative_sample_rate)
    for ep in range(n_epochs if stop is None else stop):
        Y, st = transform_epoch(Y, Y_train, idx, st, ep, n_epochs, a, b, seed, gamma, lr, dtype)
    return (Y, st) if return_state else Y


def umap_transform(q: np.ndarray, x_train: np.ndarray, Y_train: np.ndarray, params=None, dtype=np.float32) -> np.ndarray:
    """New points ``q [m, d]`` onto the layout ``Y_train [n, 2]`` of ``x_train [n, d]``: query table, smooth-kNN,
    memberships, weighted-mean start, layout.  ``params`` is a ``search.umap.UMAPParams`` (defaults when None);
    ``dtype`` is the precision of the forces (table and memberships follow the float64 rule) -> float32 ``[m, 2]``."""
    if params is None:
        from .umap import UMAPParams

        params = UMAPParams()
    q, x_train = np.asarray(q), np.asarray(x_train)
    Y_train = np.asarray(Y_train, _F32)
    if q.ndim != 2 or x_train.ndim != 2 or q.shape[1] != x_train.shape[1]:
        raise ValueError(f"q {q.shape} and x_train {x_train.shape} must be [m, d] and [n, d]")
    if Y_train.shape != (x_train.shape[0], 2):
        raise ValueError("Y_train must be [n, 2]")
    n_epochs = transform_n_epochs(params)
    check_transform_limits(q.shape[0], x_train.shape[0], params.n_neighbors, params.metric)
    if not np.isfinite(Y_train).all():
        raise ValueError("non-finite training positions")
    if q.shape[0] == 0:
        if not np.isfinite(x_train).all():
            raise ValueError("non-finite input")
        return np.zeros((0, 2), _F32)
    a, b = umap_ab(params.spread, params.min_dist)
    idx, dist = knn_query_table(q, x_train, params.n_neighbors, params.metric)
    rho, sigma = smooth_knn_query(dist)
    w = memberships_query(dist, rho, sigma)
    Y0 = transform_init(idx, w, Y_train)
    Y = umap_transform_layout(Y0, Y_train, idx, w, n_epochs, a, b, params.seed, params.repulsion_strength,
                              params.learning_rate, params.negative_sample_rate, dtype)
    return np.asarray(Y, _F32)
