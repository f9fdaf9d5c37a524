"""The reconstructed surface as geometry, extracted on the device: the contract of the reference's mesh
script (internal/mesh_network.py:48-72, 134-139: a linspace lattice in `ij` order, the density on it, nan_to_num, a
threshold, an OBJ file) with this project's own triangulation, marching tetrahedra on the Kuhn decomposition of every cell.

    query_points      the handle's fields at arbitrary points          rc_query_points
    density_lattice   the density of a sampler level on a lattice      rc_density_lattice
    isosurface        vertices, normals and triangles of any lattice   rc_isosurface, two passes, one host sync
    extract_mesh      lattice -> isosurface -> attributes at the vertices
    save_obj          `v` (optionally with colours), `vn` and 1-based `f a//a b//b c//c` lines
    atlas_layout, atlas_uvs, atlas_points   the per-triangle texture atlas of a mesh   rc_atlas_*
    bake_atlas        the fields at texel density on every triangle    rc_bake_atlas
    save_textured_obj `v` / `vn` / `vt` lines, faces `f a/ta/a ...`, an .mtl and one PNG per map

`rc` is a rc_ext.RadianceCache.  The lattice, the field and the mesh stay in HBM; only the two counts {V, T} of an
extraction (and save_obj's arrays) go to the host.

Not built: capping the surface where it leaves the box (the mesh is closed only where the surface stays inside), mesh
simplification or vertex welding beyond the one vertex per lattice edge, chart-based unwrapping and mip-safe padding of
the atlas, PLY or glTF writers, and a marching-cubes variant.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import numpy as np

KEYS = ("density", "normals_pred", "normals", "albedo", "roughness", "metalness")
_MATERIAL = {"albedo": slice(0, 3), "roughness": 3, "metalness": 4}       # columns of the material row, as the material pass splits it
# the view-independent part of the cache's own colour (rc_query_cache_diffuse): the shader's two diffuse heads and their sum
DIFFUSE_KEYS = ("ambient_diffuse", "indirect_diffuse", "cache_diffuse")
_DIFFUSE = {"ambient_diffuse": slice(0, 3), "indirect_diffuse": slice(3, 6)}
_COLOURS = ("albedo",) + DIFFUSE_KEYS                                     # written through the suite's sRGB conversion


@dataclass
class Mesh:
    vertices: object                       # [V, 3] float32 cuda tensor
    triangles: object                      # [T, 3] int32 cuda tensor, indices into vertices
    normals: Optional[object] = None       # [V, 3] float32: -normalize(lattice gradient of the field), towards lower values
    attributes: Dict[str, object] = field(default_factory=dict)     # query_points at the vertices


def query_points(rc, points, keys: Sequence[str] = ("density",), level: Optional[int] = None) -> Dict[str, object]:
    """The fields of `rc` at points [n, 3] (world coordinates) -> {key: cuda tensor} for keys among "density" [n]
    (sampler level `level`, None: the last), "normals_pred" and "normals" [n, 3] (last level, unrectified), "albedo"
    [n, 3], "roughness" [n] and "metalness" [n] (the material head; not on a time-resolved handle)."""
    unknown = [k for k in keys if k not in KEYS + DIFFUSE_KEYS]
    if unknown:
        raise ValueError(f"query_points: unknown keys {unknown}; known: {KEYS + DIFFUSE_KEYS}")
    outputs = [k for k in ("density", "normals_pred", "normals") if k in keys]
    if any(k in _MATERIAL for k in keys):
        outputs.append("material")
    raw = rc.query_points(points, outputs, level) if outputs else {}
    if any(k in DIFFUSE_KEYS for k in keys):
        raw["diffuse"] = rc.query_cache_diffuse(points)
    return {k: _split(raw, k, lambda x, cols: x[:, cols]) for k in keys}


def _split(raw, key, take):
    """One key of KEYS + DIFFUSE_KEYS out of the library's rows or planes; take(x, columns) slices the channel axis."""
    if key in _MATERIAL:
        return take(raw["material"], _MATERIAL[key]).contiguous()
    if key == "cache_diffuse":
        return take(raw["diffuse"], slice(0, 3)) + take(raw["diffuse"], slice(3, 6))
    if key in _DIFFUSE:
        return take(raw["diffuse"], _DIFFUSE[key]).contiguous()
    return raw[key]


def density_lattice(rc, lo, hi, dims, level: Optional[int] = None):
    """The density of sampler level `level` (None: the last) with nan_to_num applied on the [nx, ny, nz] lattice over
    the box lo .. hi (`ij` order, iz fastest): point i of axis a at lo[a] + float32(i) * ((hi[a] - lo[a]) / float32(n_a - 1)),
    which is linspace up to its last bits.  Generated and evaluated on the device, slab by slab."""
    return rc.density_lattice(lo, hi, dims, level)


def isosurface(rc, field, iso: float, lo, hi, normals: bool = True):
    """(vertices [V, 3], normals [V, 3] or None, triangles [T, 3] int32) of the surface field == iso of a [nx, ny, nz]
    float32 lattice over the box lo .. hi; a point is inside when field >= iso and the triangles face the lower values.
    Two calls of rc_isosurface (count, then extract) with one host synchronisation between them, for the counts."""
    return rc.isosurface(field, iso, lo, hi, normals)


def extract_mesh(rc, iso: float, lo, hi, dims, level: Optional[int] = None, attributes: Sequence[str] = ()) -> Mesh:
    """density_lattice -> isosurface -> query_points at the vertices for each of `attributes` (KEYS).  `iso` has no
    default: the reference script's 0.1 belongs to another model's density."""
    f = density_lattice(rc, lo, hi, dims, level)
    vertices, normals, triangles = isosurface(rc, f, iso, lo, hi, normals=True)
    attrs = query_points(rc, vertices, tuple(attributes)) if len(attributes) and vertices.shape[0] else \
        {k: vertices.new_empty((0, 3) if k in ("normals_pred", "normals", "albedo") else (0,)) for k in attributes}
    return Mesh(vertices=vertices, triangles=triangles, normals=normals, attributes=attrs)


def save_obj(path: str, mesh: Mesh, colors=None) -> None:
    """Wavefront OBJ on the host: `v x y z` (or `v x y z r g b` with colors [V, 3], for which albedo is the usual choice),
    `vn x y z` when the mesh has normals, and 1-based `f a//a b//b c//c` (`f a b c` without normals)."""
    host = lambda x: np.asarray(x.detach().cpu() if hasattr(x, "detach") else x)
    v = host(mesh.vertices).astype(np.float32).reshape(-1, 3)
    t = host(mesh.triangles).astype(np.int64).reshape(-1, 3) + 1
    n = None if mesh.normals is None else host(mesh.normals).astype(np.float32).reshape(-1, 3)
    if colors is not None:
        c = host(colors).astype(np.float32).reshape(-1, 3)
        if c.shape != v.shape:
            raise ValueError("save_obj: colors must have one row per vertex")
        v = np.concatenate([v, c], axis=1)
    lines = ["v " + " ".join(repr(float(x)) for x in row) for row in v]
    if n is not None:
        lines += ["vn " + " ".join(repr(float(x)) for x in row) for row in n]
        lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in t]
    else:
        lines += ["f %d %d %d" % (a, b, c) for a, b, c in t]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


# -- the texture atlas ------------------------------------------------------------------------------
@dataclass
class Atlas:
    width: int
    height: int
    cell: int                              # r: two triangles share one cell of r x r texels
    uvs: object                            # [T, 3, 2] float32: (u, v) of every triangle corner, v measured from the bottom
    coverage: object                       # [H, W] uint8: 1 where a triangle owns the texel
    textures: Dict[str, object] = field(default_factory=dict)     # key -> [H, W] or [H, W, 3] float32 (8-bit: uint8)


def atlas_layout(T: int, r: int):
    """(cols, rows, W, H) of the atlas of T triangles with cells of r x r texels (rc_atlas_layout)."""
    from . import rc_ext
    return rc_ext.atlas_layout(T, r)


def atlas_uvs(rc, T: int, r: int):
    """[T, 3, 2] float32 cuda: u = X / W, v = 1 - Y / H of every triangle corner (rc_atlas_uvs)."""
    return rc.atlas_uvs(T, r)


def atlas_points(rc, mesh: Mesh, r: int, first: int = 0, count: Optional[int] = None):
    """(points [count, 3], owner [count] int32) of the texels with linear index y W + x from `first` on (count None: all
    that follow): the world point of each texel centre on its triangle's plane, (0, 0, 0) and owner -1 for an empty texel."""
    return rc.atlas_points(mesh.vertices, mesh.triangles, r, first, count)


def bake_atlas(rc, mesh: Mesh, r: int, keys: Sequence[str] = ("albedo", "roughness", "metalness", "normals_pred"),
               level: Optional[int] = None) -> Atlas:
    """The fields `keys` (KEYS + DIFFUSE_KEYS) of `rc` at every texel of the mesh's atlas, baked on the device: a texel
    holds query_points at its point bit for bit, 0 where no triangle owns it."""
    unknown = [k for k in keys if k not in KEYS + DIFFUSE_KEYS]
    if unknown:
        raise ValueError(f"bake_atlas: unknown keys {unknown}; known: {KEYS + DIFFUSE_KEYS}")
    outputs = [k for k in ("density", "normals_pred", "normals") if k in keys]
    if any(k in _MATERIAL for k in keys):
        outputs.append("material")
    if any(k in DIFFUSE_KEYS for k in keys):
        outputs.append("diffuse")
    T = int(mesh.triangles.shape[0])
    raw = rc.bake_atlas(mesh.vertices, mesh.triangles, r, outputs + ["coverage"], level)
    H, W = (int(d) for d in raw["coverage"].shape)
    return Atlas(width=W, height=H, cell=int(r), uvs=atlas_uvs(rc, T, r), coverage=raw["coverage"],
                 textures={k: _split(raw, k, lambda x, cols: x[..., cols]) for k in keys})


_MTL_MAPS = (("map_Kd", ("albedo", "cache_diffuse")), ("map_Pr", ("roughness",)), ("map_Pm", ("metalness",)),
             ("norm", ("normals_pred",)))


def atlas_images(atlas: Atlas, maps: Optional[Sequence[str]] = None, rc=None) -> Dict[str, np.ndarray]:
    """The 8-bit pictures [H, W, 3] of the atlas' textures `maps` (None: all) on the host.  A float texture (a cuda tensor
    or a host array) goes through the visualisation suite's own conversion on the device of `rc` (rc_vis_images: colours
    as its sRGB pictures, normals as 0.5 n + 0.5, scalars clipped to [0, 1]; vis.py); a uint8 texture is taken as it is
    and needs no handle."""
    keys = list(atlas.textures) if maps is None else list(maps)
    H, W = atlas.height, atlas.width
    host = lambda x: np.asarray(x.detach().cpu() if hasattr(x, "detach") else x)
    out, items, item_keys = {}, [], []
    for k in keys:
        tex = atlas.textures[k]
        if str(tex.dtype).endswith("uint8"):
            img = host(tex)
            out[k] = np.broadcast_to(img.reshape(H, W, -1), (H, W, 3)).copy()
            continue
        if rc is None:
            raise ValueError(f"atlas_images: the float texture {k!r} needs `rc` for the suite's 8-bit conversion")
        if k in _COLOURS:
            items.append(dict(src=tex, op="srgb", channels=3, u8=True))
        elif k in ("normals", "normals_pred"):
            items.append(dict(src=tex, op="matte", channels=3, divide=2.0, offset=0.5, u8=True))
        else:
            items.append(dict(src=tex, op="matte", channels=1, u8=True))
        item_keys.append(k)
    if items:
        for k, o in zip(item_keys, rc.vis_images(items, H, W)):
            out[k] = host(o["u8"])
    return {k: out[k] for k in keys}


def save_textured_obj(path: str, mesh: Mesh, atlas: Atlas, maps: Optional[Sequence[str]] = None, rc=None) -> Dict[str, str]:
    """Wavefront OBJ with a material: `v`, `vn` (when the mesh has normals), three `vt u v` per triangle and 1-based faces
    `f a/ta/a b/tb/b c/tc/c` (`f a/ta ...` without normals); beside it <stem>.mtl (map_Kd: albedo, else cache_diffuse;
    map_Pr roughness; map_Pm metalness; norm normals_pred -- world-space normals, not tangent-space) and one
    <stem>_<map>.png per texture of `maps` (None: all of the atlas), written with PIL; float textures are converted to 8
    bits on the device of `rc` (atlas_images).  Returns the paths by map."""
    import os
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("save_textured_obj writes PNGs with PIL (the pillow package), which is not installed") from e
    host = lambda x: np.asarray(x.detach().cpu() if hasattr(x, "detach") else x)
    v = host(mesh.vertices).astype(np.float32).reshape(-1, 3)
    t = host(mesh.triangles).astype(np.int64).reshape(-1, 3) + 1
    n = None if mesh.normals is None else host(mesh.normals).astype(np.float32).reshape(-1, 3)
    uv = host(atlas.uvs).astype(np.float32).reshape(-1, 2)
    if uv.shape[0] != 3 * t.shape[0]:
        raise ValueError("save_textured_obj: the atlas holds three uvs per triangle of another mesh")
    images = atlas_images(atlas, maps, rc)
    stem = os.path.splitext(path)[0]
    base = os.path.basename(stem)
    paths = {}
    for k, img in images.items():
        paths[k] = f"{stem}_{k}.png"
        Image.fromarray(img).save(paths[k])
    mtl = ["newmtl atlas", "Kd 1 1 1"]
    for statement, candidates in _MTL_MAPS:
        k = next((c for c in candidates if c in images), None)
        if k is not None:
            mtl.append(f"{statement} {base}_{k}.png")
    with open(stem + ".mtl", "w") as fh:
        fh.write("\n".join(mtl) + "\n")
    lines = [f"mtllib {base}.mtl", "usemtl atlas"]
    lines += ["v " + " ".join(repr(float(x)) for x in row) for row in v]
    if n is not None:
        lines += ["vn " + " ".join(repr(float(x)) for x in row) for row in n]
    lines += ["vt " + " ".join(repr(float(x)) for x in row) for row in uv]
    if n is not None:
        lines += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, 3 * i + 1, a, b, 3 * i + 2, b, c, 3 * i + 3, c) for i, (a, b, c) in enumerate(t)]
    else:
        lines += ["f %d/%d %d/%d %d/%d" % (a, 3 * i + 1, b, 3 * i + 2, c, 3 * i + 3) for i, (a, b, c) in enumerate(t)]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return paths
