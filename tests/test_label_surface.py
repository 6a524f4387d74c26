"""The surface oracle ``reference.label_surface`` / ``surface_stats`` / ``surface_to_obj`` on the
cases of ``label_surface_cases``: the literals of the rule and the identities every mesh must hold
(voxel counts from the mesh, signed volume of the corner mesh, cancelling directed edges, the
specified order, the surface-net formula bit for bit)."""
import numpy as np
import pytest

import label_surface_cases as sc
from bioengine_worker_amd.cellpose import reference as ref

DTYPES = {"corner": np.int32, "verts": np.float32, "vert_label": np.int32, "quads": np.int32, "quad_label": np.int32,
          "label_verts": np.int64, "label_quads": np.int64, "faces": np.int64, "voxels": np.int64}


def bound(name) -> int:
    n = sc.nlab(name)
    return (int(sc.volume(name).max()) if n is None else n - 1)


def counts(name) -> np.ndarray:
    K = bound(name)
    return np.bincount(sc.volume(name).ravel(), minlength=K + 1)[1:K + 1]


def corner_dets(s: dict) -> np.ndarray:
    p = s["corner"].astype(np.int64)[s["quads"]]  # [F, 4, 3]
    det = lambda a, b, c: np.einsum("ni,ni->n", a, np.cross(b, c))
    return det(p[:, 0], p[:, 1], p[:, 2]) + det(p[:, 0], p[:, 2], p[:, 3])


@pytest.mark.parametrize("name", sc.CASES)
def test_shapes_and_dtypes(name):
    s, K = sc.oracle(name), bound(name)
    assert set(s) == set(DTYPES)
    for k, dt in DTYPES.items():
        assert s[k].dtype == dt, k
    V, F = s["verts"].shape[0], s["quads"].shape[0]
    assert s["corner"].shape == (V, 3) and s["verts"].shape == (V, 3) and s["vert_label"].shape == (V,)
    assert s["quads"].shape == (F, 4) and s["quad_label"].shape == (F,)
    assert s["label_verts"].shape == s["label_quads"].shape == (K + 1,)
    assert s["faces"].shape == (K, 3) and s["voxels"].shape == (K,)
    assert s["label_verts"][0] == 0 == s["label_quads"][0] and s["label_verts"][-1] == V and s["label_quads"][-1] == F


@pytest.mark.parametrize("name", sc.CASES)
def test_mesh_identities(name):
    s, L, K = sc.oracle(name), sc.volume(name), bound(name)
    want = counts(name)
    assert np.array_equal(s["voxels"], want)
    # signed volume of the corner mesh, per label
    det = np.zeros(K, np.int64)
    np.add.at(det, s["quad_label"] - 1, corner_dets(s))
    assert np.array_equal(det, 6 * want)
    # faces per axis add up to the label's quads
    assert np.array_equal(s["faces"].sum(1), np.diff(s["label_quads"]))
    # every vertex is used, by quads of its own label only
    used = np.zeros(s["verts"].shape[0], bool)
    used[s["quads"].ravel()] = True
    assert used.all()
    assert np.array_equal(s["vert_label"][s["quads"]], np.repeat(s["quad_label"][:, None], 4, 1))
    # directed edges of a label cancel in pairs; every undirected edge is used 2 or 4 times
    q = s["quads"].astype(np.int64)
    a, b = q.ravel(), np.roll(q, -1, 1).ravel()
    V = max(s["verts"].shape[0], 1)
    fwd, cnt = np.unique(a * V + b, return_counts=True)
    bwd, cntb = np.unique(b * V + a, return_counts=True)
    assert np.array_equal(fwd, bwd) and np.array_equal(cnt, cntb)
    und = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)[1]
    assert np.isin(und, (2, 4)).all()
    # quads are unit squares of the lattice
    p = s["corner"].astype(np.int64)[s["quads"]]
    assert (np.abs(np.roll(p, -1, 1) - p).sum(2) == 1).all()
    assert L.shape == sc.volume(name).shape


@pytest.mark.parametrize("name", sc.CASES)
def test_order(name):
    s, L = sc.oracle(name), sc.volume(name)
    Z, H, W = L.shape
    NC = (Z + 1) * (H + 1) * (W + 1)
    c = s["corner"].astype(np.int64)
    vkey = s["vert_label"].astype(np.int64) * NC + (c[:, 0] * (H + 1) + c[:, 1]) * (W + 1) + c[:, 2]
    assert (np.diff(vkey) > 0).all()  # (label, corner raster), no duplicates
    # a quad's voxel and side from its corners: the plane axis, the side from the winding
    p = c[s["quads"]]
    lo = p.min(1)
    axis = (p.max(1) == lo).argmax(1)
    step = (p[:, 1] - p[:, 0]).argmax(1)  # s = 1 starts along b = a + 1, s = 0 along c = a + 2
    side = (step == (axis + 1) % 3).astype(np.int64)
    vox = lo.copy()
    vox[np.arange(vox.shape[0]), axis] -= side  # the plane is a = v_a + s
    assert (vox >= 0).all() and (vox < np.array(L.shape)).all()
    assert np.array_equal(L[vox[:, 0], vox[:, 1], vox[:, 2]], s["quad_label"])
    qkey = (s["quad_label"].astype(np.int64) * L.size + (vox[:, 0] * H + vox[:, 1]) * W + vox[:, 2]) * 6 + 2 * axis + side
    assert (np.diff(qkey) > 0).all()  # (label, voxel raster, 2a + s), no duplicates
    assert np.array_equal(np.bincount(s["quad_label"] - 1, minlength=s["faces"].shape[0] * 1)[:s["faces"].shape[0]],
                          s["faces"].sum(1))
    assert np.array_equal(s["label_verts"][1:], np.searchsorted(s["vert_label"], np.arange(1, s["faces"].shape[0] + 1), "right"))
    assert np.array_equal(s["label_quads"][1:], np.searchsorted(s["quad_label"], np.arange(1, s["faces"].shape[0] + 1), "right"))


#: the 12 edges of the 2 x 2 x 2 block of voxel centres: (low end, high end, midpoint offset in half voxels)
EDGES = []
for _a in range(3):
    _o1, _o2 = [ax for ax in range(3) if ax != _a]
    for _d1 in (0, 1):
        for _d2 in (0, 1):
            _lo, _hi, _mid = [0, 0, 0], [0, 0, 0], [0, 0, 0]
            _lo[_o1] = _hi[_o1] = _d1
            _lo[_o2] = _hi[_o2] = _d2
            _hi[_a] = 1
            _mid[_o1], _mid[_o2] = 2 * _d1 - 1, 2 * _d2 - 1
            EDGES.append((tuple(_lo), tuple(_hi), tuple(_mid)))


def net_offsets_loop(L: np.ndarray, corners, labels):
    """The surface-net sums of every vertex, written out edge by edge in plain Python: shares no code
    with the oracle.  Returns nsum [V, 3] and ncross [V]."""
    Z, H, W = L.shape
    P = np.zeros((Z + 2, H + 2, W + 2), np.int64)  # a zero border: outside the array counts as 0
    P[1:-1, 1:-1, 1:-1] = L
    P = P.tolist()
    nsum, ncross = [], []
    for (cz, cy, cx), l in zip(corners.tolist(), labels.tolist()):
        s, n = [0, 0, 0], 0
        for lo, hi, mid in EDGES:  # voxel (c - 1 + d) is P[c + d]
            if (P[cz + lo[0]][cy + lo[1]][cx + lo[2]] == l) != (P[cz + hi[0]][cy + hi[1]][cx + hi[2]] == l):
                n += 1
                s[0] += mid[0]
                s[1] += mid[1]
                s[2] += mid[2]
        nsum.append(s)
        ncross.append(n)
    return np.array(nsum, np.int64).reshape(-1, 3), np.array(ncross, np.int64)


@pytest.mark.parametrize("name", sc.CASES)
def test_verts_are_the_formula_bit_for_bit(name):
    """Every vertex of every case against the edge-by-edge loop."""
    s, L = sc.oracle(name), sc.volume(name)
    nsum, ncross = net_offsets_loop(L, s["corner"], s["vert_label"])
    assert ((ncross >= 3) & (ncross <= 12)).all()
    want = (s["corner"].astype(np.float64) + nsum.astype(np.float64) / (2 * ncross).astype(np.float64)[:, None]).astype(np.float32)
    assert want.shape == s["verts"].shape
    bad = np.flatnonzero((want.view(np.uint32) != s["verts"].view(np.uint32)).any(1))
    assert bad.size == 0, (name, bad[:5])
    seen = set(ncross.tolist())
    if name == "rand":
        # the cuts of the cube graph: 3 |S| - 2 e(S), so 10 and 11 crossing edges do not exist
        assert seen == {3, 4, 5, 6, 7, 8, 9, 12}
    if name == "single":
        assert seen == {3}


def test_literals():
    s = sc.oracle("single")
    assert s["quads"].shape[0] == 6 and s["verts"].shape[0] == 8
    third = np.float32(np.float64(1) + np.float64(2) / np.float64(6)), np.float32(np.float64(2) + np.float64(-2) / np.float64(6))
    assert set(np.unique(s["verts"]).tolist()) == {float(third[0]), float(third[1])}
    assert np.allclose(s["verts"], np.where(s["corner"] == 1, 1 + 1 / 3, 2 - 1 / 3), atol=1e-6)
    st = sc.stats("single")
    assert st["area"][0] == pytest.approx(6 / 9, rel=1e-6) and st["area_voxel"][0] == 6.0 and st["volume"][0] == 1.0
    assert st["n_verts"][0] == 8 and st["n_quads"][0] == 6
    d = sc.oracle("diag")
    assert d["quads"].shape[0] == 18 and d["verts"].shape[0] == 23
    assert d["label_quads"].tolist() == [0, 12, 18] and d["label_verts"].tolist() == [0, 15, 23]  # 2 x 8 - 1 shared
    assert d["faces"].tolist() == [[4, 4, 4], [2, 2, 2]] and d["voxels"].tolist() == [2, 1]
    f = sc.oracle("full")
    assert f["faces"].tolist() == [[24, 16, 12]] and f["verts"].shape[0] == 3 * 4 * 5 - 1 * 2 * 3
    c = f["corner"][f["quads"]]
    on_border = ((c == 0).all(1) | (c == np.array([2, 3, 4])).all(1)).any(1)
    assert on_border.all()
    for name, (F, V) in sc.BALL_COUNTS.items():
        b = sc.oracle(name)
        assert (b["quads"].shape[0], b["verts"].shape[0]) == (F, V) and V - F == 2
    assert sc.oracle("empty")["quads"].shape == (0, 4) and sc.oracle("empty")["label_verts"].tolist() == [0]
    n = sc.oracle("nolab")
    assert n["verts"].shape == (0, 3) and n["faces"].shape == (0, 3) and n["label_quads"].tolist() == [0]
    cells = sc.oracle("cells")
    assert cells["faces"].shape == (11, 3) and cells["voxels"][3] == 0 and int(sc.volume("cells").max()) == 12
    assert (cells["voxels"][[0, 1, 2, 4]] > 0).all() and int(cells["quad_label"].max()) <= 11


@pytest.mark.parametrize("name", ("ball6", "ball10"))
def test_ball_area_ratio(name):
    r = int(name[4:])
    st = sc.stats(name)
    assert abs(st["area"][0] / (4 * np.pi * r * r) - sc.BALL_RATIO[name]) < 1e-5
    assert 1.45 < st["area_voxel"][0] / (4 * np.pi * r * r) < 1.55
    assert st["volume"][0] == float(sc.volume(name).sum())
    assert 0 < st["mesh_volume"][0] < st["volume"][0]  # the nets pull the surface inward
    assert 0.9 < st["sphericity"][0] < 1.0


def test_stats_spacing_and_empty_labels():
    s = sc.oracle("cells")
    sp = (2.5, 1.0, 0.5)
    st = ref.surface_stats(s, sp)
    f = s["faces"].astype(np.float64)
    assert np.array_equal(st["area_voxel"], f[:, 0] * 1.0 * 0.5 + f[:, 1] * 2.5 * 0.5 + f[:, 2] * 2.5 * 1.0)
    assert np.array_equal(st["volume"], s["voxels"] * (2.5 * 1.0 * 0.5))
    for absent in (3, 10):  # labels 4 and 11 are absent
        assert np.isnan(st["sphericity"][absent]) and st["area"][absent] == 0 and st["n_quads"][absent] == 0
    assert np.isfinite(np.delete(st["sphericity"], (3, 10))).all()
    # the corner mesh scaled by spacing has the voxel-face area and the voxel volume exactly
    cm = dict(s, verts=s["corner"].astype(np.float32))
    ct = ref.surface_stats(cm, sp)
    assert np.allclose(ct["area"], ct["area_voxel"], rtol=1e-12) and np.allclose(ct["mesh_volume"], ct["volume"], rtol=1e-12)
    e = ref.surface_stats(sc.oracle("nolab"))
    assert all(v.shape == (0,) and v.dtype == np.float64 for v in e.values())


def parse_obj(text: str):
    groups, verts, faces = [], [], []
    for line in text.splitlines():
        t = line.split()
        if t[0] == "o":
            groups.append(t[1])
        elif t[0] == "v":
            verts.append([float(v) for v in t[1:]])
        elif t[0] == "f":
            faces.append([int(v) for v in t[1:]])
    return groups, np.array(verts, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 4)


@pytest.mark.parametrize("smooth", (True, False))
def test_obj_round_trip(smooth):
    s = sc.oracle("cells")
    sp = (2.0, 1.0, 1.0)
    text = ref.surface_to_obj(s, spacing=sp, smooth=smooth)
    groups, v, f = parse_obj(text)
    present = [l for l in range(1, 12) if s["label_quads"][l] > s["label_quads"][l - 1]]
    assert groups == [f"label_{l}" for l in present] and 4 not in present
    assert v.shape[0] == s["verts"].shape[0] and f.shape[0] == s["quads"].shape[0]
    assert f.min() == 1 and f.max() == v.shape[0]
    src = s["verts" if smooth else "corner"].astype(np.float64)
    assert np.array_equal(v, src[:, ::-1] * np.array([1.0, 1.0, 2.0]))  # repr round-trips floats exactly
    # outward normals: positive signed volume in the (x, y, z) frame
    p = v[f - 1]
    det = lambda a, b, c: np.einsum("ni,ni->n", a, np.cross(b, c))
    assert (det(p[:, 0], p[:, 1], p[:, 2]) + det(p[:, 0], p[:, 2], p[:, 3])).sum() > 0
    # the stored order again (the other diagonal of a non-planar quad): the oracle's signed volume, mirrored
    p = v[f[:, ::-1] - 1]
    vol = -(det(p[:, 0], p[:, 1], p[:, 2]) + det(p[:, 0], p[:, 2], p[:, 3])).sum() / 6
    want = ref.surface_stats(s if smooth else dict(s, verts=s["corner"].astype(np.float32)), sp)["mesh_volume"].sum()
    assert vol == pytest.approx(want, rel=1e-9)
    # a subset of labels is re-indexed from 1
    g2, v2, f2 = parse_obj(ref.surface_to_obj(s, labels=[5, 2]))
    n5, n2 = (int(s["label_verts"][l] - s["label_verts"][l - 1]) for l in (5, 2))
    assert g2 == ["label_5", "label_2"] and v2.shape[0] == n5 + n2 and f2.min() == 1 and f2.max() == n5 + n2
    assert f2[: int(s["label_quads"][5] - s["label_quads"][4])].max() == n5
    assert ref.surface_to_obj(sc.oracle("empty")) == ""


def test_value_errors():
    with pytest.raises(ValueError, match="expects"):
        ref.label_surface(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="integer"):
        ref.label_surface(np.zeros((2, 2, 2), np.float32))
    s = sc.oracle("single")
    for bad in ((1, 1), (1, 0, 1), (1, -1, 1), (1, np.inf, 1), (1, np.nan, 1), "abc", None, (1, 1, 1, 1)):
        with pytest.raises(ValueError, match="spacing"):
            ref.surface_stats(s, bad)
        with pytest.raises(ValueError, match="spacing"):
            ref.surface_to_obj(s, bad)
    with pytest.raises(ValueError, match="labels"):
        ref.surface_to_obj(s, labels=[2])
    with pytest.raises(ValueError, match="labels"):
        ref.surface_to_obj(s, labels=[0])


def test_nlab_and_dtypes():
    L = sc.volume("cells")
    full = ref.label_surface(L)  # K = 12
    low = sc.oracle("cells")     # K = 11
    assert full["faces"].shape == (12, 3) and full["voxels"][11] == (L == 12).sum() > 0
    n = low["quads"].shape[0]
    assert np.array_equal(full["quads"][:n], low["quads"]) and np.array_equal(full["verts"][:low["verts"].shape[0]], low["verts"])
    # the label above the bound still bounds its neighbours: masking it out changes nothing below it
    assert np.array_equal(low["faces"], full["faces"][:11])
    high = ref.label_surface(L, nlab=20)
    assert high["faces"].shape == (19, 3) and np.array_equal(high["quads"], full["quads"]) and not high["voxels"][12:].any()
    for dt in (np.uint8, np.uint16, np.int64):
        got = ref.label_surface(L.astype(dt), nlab=12)
        for k in DTYPES:
            assert got[k].dtype == low[k].dtype and np.array_equal(got[k], low[k]), (dt, k)
