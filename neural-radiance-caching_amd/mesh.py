"""The reconstructed surface as geometry, extracted on the device: the contract of the reference's mesh
script (internal/mesh_network.py:48-72, 134-139: a linspace lattice in `ij` order, the density on it, nan_to_num, a
threshold, an OBJ file) with this project's own triangulation, marching tetrahedra on the Kuhn decomposition of every cell.

    query_points      the handle's fields at arbitrary points          rc_query_points
    density_lattice   the density of a sampler level on a lattice      rc_density_lattice
    isosurface        vertices, normals and triangles of any lattice   rc_isosurface, two passes, one host sync
    extract_mesh      lattice -> isosurface -> attributes at the vertices
    save_obj          `v` (optionally with colours), `vn` and 1-based `f a//a b//b c//c` lines

`rc` is a rc_ext.RadianceCache.  The lattice, the field and the mesh stay in HBM; only the two counts {V, T} of an
extraction (and save_obj's arrays) go to the host.

Not built: capping the surface where it leaves the box (the mesh is closed only where the surface stays inside), mesh
simplification or vertex welding beyond the one vertex per lattice edge, texture atlases, PLY or glTF writers, and a
marching-cubes variant.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import numpy as np

KEYS = ("density", "normals_pred", "normals", "albedo", "roughness", "metalness")
_MATERIAL = {"albedo": slice(0, 3), "roughness": 3, "metalness": 4}       # columns of the material row, as the material pass splits it


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
    unknown = [k for k in keys if k not in KEYS]
    if unknown:
        raise ValueError(f"query_points: unknown keys {unknown}; known: {KEYS}")
    outputs = [k for k in ("density", "normals_pred", "normals") if k in keys]
    if any(k in _MATERIAL for k in keys):
        outputs.append("material")
    raw = rc.query_points(points, outputs, level)
    return {k: (raw["material"][:, _MATERIAL[k]].contiguous() if k in _MATERIAL else raw[k]) for k in keys}


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
