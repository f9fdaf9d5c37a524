"""mesh.save_textured_obj on a CPU Mesh / Atlas made of numpy arrays (no GPU): the OBJ, its .mtl and the PNGs are parsed
back.  The textures are 8-bit here: the float -> 8-bit conversion is the visualisation suite's and runs on the device
(tests/test_gpu_atlas.py)."""
import os

import numpy as np
import pytest

import atlas_ref as ar
from nrc_amd import mesh

R = 5


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * 0.5
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    n = (v - v.mean(axis=0)) / np.linalg.norm(v - v.mean(axis=0), axis=1, keepdims=True)
    return v, t, n.astype(np.float32)


def cpu_atlas(T, keys):
    cols, rows, W, H = ar.layout(T, R)
    rng = np.random.Generator(np.random.PCG64(5))
    owner = ar.texels(T, R)[0].reshape(H, W)
    tex = {k: rng.integers(0, 256, size=(H, W) if k in ("roughness", "metalness") else (H, W, 3)).astype(np.uint8) for k in keys}
    return mesh.Atlas(width=W, height=H, cell=R, uvs=ar.uvs(T, R), coverage=(owner >= 0).astype(np.uint8), textures=tex)


def parse_obj(path):
    v, vn, vt, f, other = [], [], [], [], []
    for line in open(path):
        kind, *rest = line.split()
        if kind in ("v", "vn", "vt"):
            {"v": v, "vn": vn, "vt": vt}[kind].append([float(x) for x in rest])
        elif kind == "f":
            f.append([[int(x) if x else 0 for x in c.split("/")] for c in rest])
        else:
            other.append((kind, rest))
    return np.asarray(v), np.asarray(vn), np.asarray(vt), np.asarray(f, np.int64), other


@pytest.mark.parametrize("with_normals", [True, False])
def test_textured_obj_round_trips(tmp_path, with_normals):
    from PIL import Image
    v, t, n = tetrahedron()
    m = mesh.Mesh(vertices=v, triangles=t, normals=n if with_normals else None)
    atlas = cpu_atlas(len(t), ("albedo", "roughness", "metalness", "normals_pred"))
    path = str(tmp_path / "tet.obj")
    paths = mesh.save_textured_obj(path, m, atlas)
    pv, pvn, pvt, f, other = parse_obj(path)
    assert ("mtllib", ["tet.mtl"]) in other and ("usemtl", ["atlas"]) in other
    assert np.array_equal(pv.astype(np.float32), v)
    assert pvt.shape == (3 * len(t), 2) and np.array_equal(pvt.astype(np.float32).reshape(-1, 3, 2), atlas.uvs)
    assert f.shape == (len(t), 3, 3 if with_normals else 2)
    assert np.array_equal(f[..., 0] - 1, t)                                           # 1-based vertex indices
    assert np.array_equal(f[..., 1], 1 + np.arange(3 * len(t)).reshape(-1, 3))        # three vt of its own per triangle
    if with_normals:
        assert np.array_equal(pvn.astype(np.float32), n) and np.array_equal(f[..., 2], f[..., 0])
    else:
        assert pvn.size == 0
    mtl = dict(line.split(None, 1) for line in open(str(tmp_path / "tet.mtl")).read().splitlines())
    assert mtl["newmtl"] == "atlas"
    assert (mtl["map_Kd"], mtl["map_Pr"], mtl["map_Pm"], mtl["norm"]) == \
        ("tet_albedo.png", "tet_roughness.png", "tet_metalness.png", "tet_normals_pred.png")
    assert set(paths) == set(atlas.textures)
    for k, p in paths.items():
        assert os.path.dirname(p) == str(tmp_path) and os.path.basename(p) == mtl[{"albedo": "map_Kd", "roughness": "map_Pr",
                                                                                   "metalness": "map_Pm", "normals_pred": "norm"}[k]]
        img = np.asarray(Image.open(p))
        assert img.shape == (atlas.height, atlas.width, 3) and img.dtype == np.uint8
        assert np.array_equal(img, np.broadcast_to(atlas.textures[k].reshape(atlas.height, atlas.width, -1), img.shape)), k


def test_maps_choose_the_pictures_and_the_diffuse_colour(tmp_path):
    v, t, n = tetrahedron()
    m = mesh.Mesh(vertices=v, triangles=t, normals=n)
    atlas = cpu_atlas(len(t), ("cache_diffuse", "roughness", "albedo"))
    paths = mesh.save_textured_obj(str(tmp_path / "a.obj"), m, atlas, maps=("cache_diffuse", "roughness"))
    assert set(paths) == {"cache_diffuse", "roughness"} and not os.path.exists(str(tmp_path / "a_albedo.png"))
    mtl = open(str(tmp_path / "a.mtl")).read()
    assert "map_Kd a_cache_diffuse.png" in mtl and "map_Pr a_roughness.png" in mtl and "map_Pm" not in mtl and "norm" not in mtl


def test_refusals(tmp_path):
    v, t, n = tetrahedron()
    m = mesh.Mesh(vertices=v, triangles=t, normals=n)
    with pytest.raises(ValueError, match="three uvs per triangle"):
        mesh.save_textured_obj(str(tmp_path / "b.obj"), m, cpu_atlas(len(t) + 1, ("albedo",)))
    atlas = cpu_atlas(len(t), ("albedo",))
    atlas.textures["albedo"] = atlas.textures["albedo"].astype(np.float32) / 255          # float, and no handle to convert it
    with pytest.raises(ValueError, match="needs `rc`"):
        mesh.save_textured_obj(str(tmp_path / "c.obj"), m, atlas)


def test_missing_pillow_is_a_runtime_error(tmp_path, monkeypatch):
    """As vis.save_suite: without the pillow package the writer says so, before it writes anything."""
    import sys
    v, t, n = tetrahedron()
    monkeypatch.setitem(sys.modules, "PIL", None)                       # `from PIL import Image` raises ImportError
    with pytest.raises(RuntimeError, match="pillow"):
        mesh.save_textured_obj(str(tmp_path / "d.obj"), mesh.Mesh(vertices=v, triangles=t, normals=n), cpu_atlas(len(t), ("albedo",)))
    assert not list(tmp_path.iterdir())
