"""Label surfaces through the apps: ``infer(return_surfaces=True)`` of the Cellpose app in the
stack modes, each ``surface_format``, its ``ValueError``s and unchanged items without the flag; and
``em.volume.analyze_volume(surface_stats=True)`` of the FIB-SEM app's analysis.  Runs on whatever
device the app picks (the CPU without a GPU, where the numpy oracle meshes) with the random
cyto3-architecture CPnet."""
import asyncio
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from bioengine_worker_amd.cellpose import reference as ref

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"
KW = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}
MESH_KEYS = {"corner", "verts", "vert_label", "quads", "quad_label", "label_verts", "label_quads", "faces", "voxels"}
STAT_KEYS = {"label", "area_voxel", "area", "mesh_volume", "volume", "sphericity", "n_verts", "n_quads"}


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_surface_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


def stack():
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    return np.ascontiguousarray(synthetic_cells(5, 32, 40, ncells=4, seed=1)[:, 0])  # [Z, H, W] uint16


def same_item(a: dict, b: dict) -> None:
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])) if k == "output" else a[k] == b[k], k


def test_infer_surfaces_in_stack_modes(app):
    vol = stack()

    async def main():
        plain = await app.infer(input_arrays=[vol], stitch_threshold=0.25, **KW)
        stats = await app.infer(input_arrays=[vol], stitch_threshold=0.25, return_surfaces=True, **KW)
        mesh = await app.infer({"input_arrays": [vol], "stitch_threshold": 0.25, "return_surfaces": True,
                                "surface_format": "mesh", **KW})
        mesh_js = await app.infer(input_arrays=[vol], stitch_threshold=0.25, return_surfaces=True, surface_format="mesh",
                                  json_safe=True, **KW)
        planes = await app.infer(input_arrays=[vol], z_axis=0, return_surfaces=True, **KW)
        obj = await app.infer(input_arrays=[vol], do_3D=True, anisotropy=2.0, return_surfaces=True, surface_format="obj",
                              model="cyto3", niter=20)
        obj_stats = await app.infer(input_arrays=[vol], do_3D=True, anisotropy=2.0, return_surfaces=True, model="cyto3",
                                    niter=20)
        off = await app.infer(input_arrays=[vol], stitch_threshold=0.25, return_surfaces=False, surface_format="obj", **KW)
        return plain, stats, mesh, mesh_js, planes, obj, obj_stats, off

    plain, stats, mesh, mesh_js, planes, obj, obj_stats, off = asyncio.run(main())
    # without the flag the item is what it was
    assert set(plain[0]) - {"weights"} == {"input_path", "output"}
    same_item(plain[0], off[0])
    masks = np.asarray(stats[0]["output"])
    assert masks.shape == vol.shape and masks.max() > 0
    assert np.array_equal(masks, plain[0]["output"])
    want = ref.label_surface(masks)
    table = ref.surface_stats(want)
    # "stats": the table as lists
    got = stats[0]["surfaces"]
    assert set(got) == STAT_KEYS and all(isinstance(v, list) for v in got.values())
    for k in STAT_KEYS:
        assert np.allclose(got[k], table[k], rtol=1e-9, equal_nan=True), k
    assert got["volume"] == np.bincount(masks.ravel())[1:].astype(float).tolist()
    # "mesh": arrays, or lists under json_safe
    m = mesh[0]["surfaces"]
    assert set(m) == MESH_KEYS
    for k in MESH_KEYS:
        assert isinstance(m[k], np.ndarray) and m[k].dtype == want[k].dtype and np.array_equal(m[k], want[k]), k
    mj = mesh_js[0]["surfaces"]
    assert set(mj) == MESH_KEYS and all(isinstance(v, list) for v in mj.values())
    for k in MESH_KEYS:  # the same request: the same labels, as lists
        assert mj[k] == want[k].tolist(), k
    # z_axis alone (no stitching): the planes' labels as they are, meshed as one volume
    pm = np.asarray(planes[0]["output"])
    assert planes[0]["surfaces"]["volume"] == np.bincount(pm.ravel())[1:].astype(float).tolist()
    # "obj": text, scaled by (anisotropy, 1, 1)
    text = obj[0]["surfaces"]
    m3 = np.asarray(obj[0]["output"])
    assert isinstance(text, str) and text == ref.surface_to_obj(ref.label_surface(m3), spacing=(2.0, 1.0, 1.0))
    t3 = ref.surface_stats(ref.label_surface(m3), (2.0, 1.0, 1.0))
    assert np.allclose(obj_stats[0]["surfaces"]["area"], t3["area"], rtol=1e-9)
    assert np.allclose(obj_stats[0]["surfaces"]["volume"], 2.0 * np.bincount(m3.ravel(), minlength=1)[1:])


def test_infer_surface_errors(app):
    vol = stack()

    async def main():
        with pytest.raises(ValueError, match="surface_format"):
            await app.infer(input_arrays=[vol], stitch_threshold=0.25, return_surfaces=True, surface_format="ply", **KW)
        with pytest.raises(ValueError, match="surface_format"):
            await app.infer({"input_arrays": [vol], "z_axis": 0, "surface_format": "stl", **KW})
        with pytest.raises(ValueError, match="return_surfaces needs a z-stack"):
            await app.infer(input_arrays=[vol[0]], return_surfaces=True, **KW)
        with pytest.raises(ValueError, match="return_surfaces needs a z-stack"):
            await app.infer({"input_arrays": [vol[0]], "return_surfaces": True, **KW})

    asyncio.run(main())


def test_runner_surfaces_on_the_host():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    L = np.zeros((4, 6, 7), np.int32)
    L[1:3, 1:4, 2:6] = 1
    L[0, 5, 0] = 3
    out = CellposeRunner.surfaces(None, L, spacing=(2.0, 1.0, 0.5))
    want = ref.label_surface(L)
    assert set(out) == {"mesh", "stats"} and set(out["mesh"]) == MESH_KEYS and set(out["stats"]) == STAT_KEYS
    for k in MESH_KEYS:
        assert out["mesh"][k].dtype == want[k].dtype and np.array_equal(out["mesh"][k], want[k]), k
    st = ref.surface_stats(want, (2.0, 1.0, 0.5))
    for k in STAT_KEYS:
        assert np.array_equal(out["stats"][k], st[k], equal_nan=True), k
    assert out["stats"]["area_voxel"][0] == 2 * (3 * 4 * 0.5 + 2 * 4 * 1.0 + 2 * 3 * 2.0)
    t = torch.from_numpy(L)
    t.label_bound = 4
    assert np.array_equal(CellposeRunner.surfaces(None, t)["mesh"]["quads"], want["quads"])
    for bad in ((1, 1), (0, 1, 1), (1, float("inf"), 1), "x"):
        with pytest.raises(ValueError, match="spacing"):
            CellposeRunner.surfaces(None, L, spacing=bad)
    with pytest.raises(ValueError, match="expects"):
        CellposeRunner.surfaces(None, L[0])


def blobs() -> np.ndarray:
    p = np.zeros((9, 40, 44), np.float32)
    zz, yy, xx = np.mgrid[0:9, 0:40, 0:44]
    for cz, cy, cx in ((2, 12, 12), (5, 26, 30), (0, 8, 36)):  # the last one is cut by the volume border
        p += np.exp(-((zz - cz) ** 2 / 4 + (yy - cy) ** 2 / 30 + (xx - cx) ** 2 / 30))
    return p / p.max()


def test_em_analyze_volume_surface_stats():
    from bioengine_worker_amd.em import volume as vol

    v = torch.from_numpy(blobs())
    kw = dict(predict=vol.probability_identity, tile=64, overlap=16, batch=2, threshold=0.5, min_voxels=20,
              norm_range=(0.0, 1.0))
    plain = vol.analyze_volume(v, **kw)
    surf = vol.analyze_volume(v, surface_stats=True, spacing_nm=(8.0, 4.0, 4.0), return_mesh=True, **kw)
    base = {"label", "voxels", "centroid_z", "centroid_y", "centroid_x"}
    assert set(plain["instances"]) == base and "mesh_obj" not in plain
    assert set(surf["instances"]) == base | {"surface_area_nm2", "surface_area_voxel_nm2", "sphericity"}
    for k in base:
        assert surf["instances"][k] == plain["instances"][k], k
    assert surf["n_instances"] == plain["n_instances"] == 3 == len(surf["instances"]["sphericity"])
    labels = surf["labels_slab_t"].numpy()
    want = ref.surface_stats(ref.label_surface(labels), (8.0, 4.0, 4.0))
    keep = np.asarray(surf["instances"]["label"]) - 1
    assert surf["instances"]["surface_area_nm2"] == want["area"][keep].tolist()
    assert surf["instances"]["surface_area_voxel_nm2"] == want["area_voxel"][keep].tolist()
    assert surf["instances"]["sphericity"] == want["sphericity"][keep].tolist()
    a, av = np.array(surf["instances"]["surface_area_nm2"]), np.array(surf["instances"]["surface_area_voxel_nm2"])
    assert (a > 0).all() and (a < av).all() and (np.array(surf["instances"]["sphericity"]) > 0.3).all()
    # faces on the volume border count as surface: the cut instance is closed at z = 0
    s = ref.label_surface(labels)
    cut = int(labels[0, 8, 36])
    assert cut > 0 and (s["corner"][s["quads"][s["quad_label"] == cut]][:, :, 0] == 0).all(1).any()
    assert surf["mesh_obj"] == ref.surface_to_obj(s, spacing=(8.0, 4.0, 4.0), labels=(keep + 1).tolist())
    assert surf["mesh_obj"].count("\no label_") + 1 == 3
    only_mesh = vol.analyze_volume(v, return_mesh=True, **kw)
    assert set(only_mesh["instances"]) == base and only_mesh["mesh_obj"].startswith("o label_")
    with pytest.raises(ValueError, match="spacing"):
        vol.analyze_volume(v, surface_stats=True, spacing_nm=(0.0, 4.0, 4.0), **kw)


def test_fibsem_app_analyze_volume(tmp_path, monkeypatch):
    """The FIB-SEM app's own parameters: nm spacing from ``pixel_size_nm`` / ``z_size_nm``, the
    refusal with ``n_gpus > 1``, and the single-process path on a probability volume."""
    import base64
    import io

    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("TMPDIR", str(tmp_path))
    main_py = ROOT / "apps" / "fibsem-mito-analysis" / "analysis_deployment.py"
    spec = importlib.util.spec_from_file_location("em_app_surface_test", main_py)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cls = mod.MitoAnalysisDeployment.func_or_class
    app = object.__new__(cls)  # validation and the probability path need no model
    app._pipe, app.tile_batch, app.model_id = None, 2, "none"
    buf = io.BytesIO()
    np.save(buf, (blobs() * 255).astype(np.uint8))
    b64 = base64.b64encode(buf.getvalue()).decode()
    kw = dict(volume_npy_b64=b64, tile_size=64, overlap=16, input_is_probability=True, min_voxels=20)

    async def main():
        for flag in ({"surface_stats": True}, {"return_mesh": True}):
            with pytest.raises(ValueError, match="n_gpus = 1"):
                await app.analyze_volume(n_gpus=2, **flag, **kw)
        with pytest.raises(ValueError, match="positive and finite"):
            await app.analyze_volume(surface_stats=True, z_size_nm=0.0, **kw)
        plain = await app.analyze_volume(return_labels=True, **kw)
        surf = await app.analyze_volume(surface_stats=True, return_mesh=True, pixel_size_nm=4.0, z_size_nm=8.0, **kw)
        iso = await app.analyze_volume(surface_stats=True, pixel_size_nm=4.0, **kw)
        return plain, surf, iso

    plain, surf, iso = asyncio.run(main())
    base = {"label", "voxels", "centroid_z", "centroid_y", "centroid_x"}
    assert set(plain["instances"]) == base and "mesh_obj" not in plain
    assert set(surf["instances"]) == base | {"surface_area_nm2", "surface_area_voxel_nm2", "sphericity"}
    labels = np.load(io.BytesIO(base64.b64decode(plain["labels_npy_b64"])))
    s = ref.label_surface(labels)
    keep = np.asarray(surf["instances"]["label"]) - 1
    assert surf["instances"]["surface_area_nm2"] == ref.surface_stats(s, (8.0, 4.0, 4.0))["area"][keep].tolist()
    assert iso["instances"]["surface_area_nm2"] == ref.surface_stats(s, (4.0, 4.0, 4.0))["area"][keep].tolist()
    assert surf["mesh_obj"] == ref.surface_to_obj(s, spacing=(8.0, 4.0, 4.0), labels=(keep + 1).tolist())
