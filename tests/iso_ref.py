"""numpy restatement of rc_isosurface: marching tetrahedra on the Kuhn decomposition of a lattice, written
from the rule and vectorised.  Returns the same three arrays in the same order as the device call.

Lattice: field [nx, ny, nz] float32, iz fastest; point i of an axis sits at lo + float32(i) * ((hi - lo) / float32(n - 1)),
every operation in float32.  A point is inside when f >= iso (a NaN is outside).

Every float operation below is a single float32 operation in the order of the kernels (which are built with
-ffp-contract=off), so vertices and normals agree with the device up to the last bits."""
import itertools

import numpy as np

F = np.float32
PERMS = list(itertools.permutations(range(3)))            # xyz, xzy, yxz, yzx, zxy, zyx
DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def tet_vertices(k):
    """v0..v3 of tetrahedron k as integer offsets."""
    a, b, _ = PERMS[k]
    e = np.eye(3, dtype=np.int64)
    return [np.zeros(3, np.int64), e[a], e[a] + e[b], np.ones(3, np.int64)]


def case_triangles(k, mask):
    """The oriented triangles of tetrahedron k with inside mask `mask` (bit i: v_i inside): a list of triangles, each three
    (i, j) pairs with i < j naming the edge (v_i, v_j) a corner sits on; and whether the rule's order was swapped."""
    v = tet_vertices(k)
    ins = [i for i in range(4) if (mask >> i) & 1]
    out = [i for i in range(4) if not (mask >> i) & 1]
    if len(ins) in (0, 4):
        return [], False
    if len(ins) == 1 or len(ins) == 3:
        a = ins[0] if len(ins) == 1 else out[0]
        rest = out if len(ins) == 1 else ins
        tris = [[(a, rest[0]), (a, rest[1]), (a, rest[2])]]
    else:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    towards = np.mean([v[i] for i in out], axis=0) - np.mean([v[i] for i in ins], axis=0)
    oriented, flipped = [], False
    for tri in tris:
        q = [(v[i] + v[j]) / 2.0 for i, j in tri]
        if np.dot(np.cross(q[1] - q[0], q[2] - q[0]), towards) < 0:
            tri = [tri[0], tri[2], tri[1]]
            flipped = True
        oriented.append([(min(i, j), max(i, j)) for i, j in tri])
    return oriented, flipped


def edge_of(k, pair):
    """Tetrahedron edge (i, j), i < j -> (offset of its owner, its number 0..6 among the owner's edges)."""
    v = tet_vertices(k)
    i, j = pair
    return v[i], DIRS.index(tuple(int(x) for x in v[j] - v[i]))


def iso_tables():
    """The table of csrc/rc_iso_table.h in the words of isocheck's output."""
    code = lambda o: int(o[0]) | int(o[1]) << 1 | int(o[2]) << 2
    t = {"vert": {}, "edge": {}, "case": {}}
    for k in range(6):
        t["vert"][k] = [code(v) for v in tet_vertices(k)]
        for e, pair in enumerate(PAIRS):
            owner, num = edge_of(k, pair)
            t["edge"][(k, e)] = (code(owner), num)
        for m in range(16):
            tris, flipped = case_triangles(k, m)
            pairs = [0] * 6
            vref = [0] * 6
            for ti, tri in enumerate(tris):
                for c, pair in enumerate(tri):
                    owner, num = edge_of(k, pair)
                    pairs[3 * ti + c] = PAIRS.index(pair)
                    vref[3 * ti + c] = code(owner) | num << 3
            t["case"][(k, m)] = (len(tris), int(flipped), pairs, vref)
    return t


def lattice_axis(lo, hi, n):
    """Positions of an axis: lo + float32(i) * ((hi - lo) / float32(n - 1)), and the spacing."""
    step = (F(hi) - F(lo)) / F(n - 1)
    return F(lo) + np.arange(n, dtype=F) * step, step


def _gradient(f, steps):
    """Central differences on the lattice, one-sided at the border, divided by the spacing: [3][nx, ny, nz]."""
    g = []
    for ax in range(3):
        n = f.shape[ax]
        i = np.arange(n)
        ip, im = np.minimum(i + 1, n - 1), np.maximum(i - 1, 0)
        shape = [1, 1, 1]
        shape[ax] = n
        den = ((ip - im).astype(F) * steps[ax]).reshape(shape)
        g.append(((np.take(f, ip, axis=ax) - np.take(f, im, axis=ax)) / den).astype(F))
    return g


def isosurface(field, iso, lo, hi, normals=True):
    """(vertices [V, 3] float32, normals [V, 3] float32 or None, triangles [T, 3] int32)."""
    f = np.ascontiguousarray(field, dtype=F)
    nx, ny, nz = f.shape
    dims = (nx, ny, nz)
    iso = F(iso)
    inside = f >= iso
    axes, steps = zip(*[lattice_axis(lo[a], hi[a], dims[a]) for a in range(3)])
    with np.errstate(all="ignore"):
        # one vertex per owned edge whose endpoints differ, numbered by (owner's linear index, edge number)
        cross = np.zeros((nx, ny, nz, 7), dtype=bool)
        for e, (dx, dy, dz) in enumerate(DIRS):
            cross[:nx - dx, :ny - dy, :nz - dz, e] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
        flat = cross.reshape(-1)
        vid = (np.cumsum(flat, dtype=np.int64) - 1).reshape(nx, ny, nz, 7)
        where = np.flatnonzero(flat)
        p, e = where // 7, where % 7
        i0 = np.stack(np.unravel_index(p, dims), axis=1)
        i1 = i0 + np.asarray(DIRS, dtype=np.int64)[e]
        f0, f1 = f[tuple(i0.T)], f[tuple(i1.T)]
        t = ((iso - f0) / (f1 - f0)).astype(F)
        t = np.fmin(np.fmax(t, F(0)), F(1))               # a NaN becomes 0, as fmaxf / fminf make it
        P0 = np.stack([axes[a][i0[:, a]] for a in range(3)], axis=1)
        P1 = np.stack([axes[a][i1[:, a]] for a in range(3)], axis=1)
        vertices = (P0 + t[:, None] * (P1 - P0)).astype(F)
        vnormals = None
        if normals:
            g = _gradient(f, steps)
            g0 = np.stack([g[a][tuple(i0.T)] for a in range(3)], axis=1)
            g1 = np.stack([g[a][tuple(i1.T)] for a in range(3)], axis=1)
            gi = (g0 + t[:, None] * (g1 - g0)).astype(F)
            ln = np.sqrt((gi[:, 0] * gi[:, 0] + gi[:, 1] * gi[:, 1]) + gi[:, 2] * gi[:, 2]).astype(F)
            vnormals = np.where((ln > 0)[:, None], -(gi / ln[:, None]), F(0)).astype(F)

    # triangles: cells in linear order, tetrahedra 0..5, the rule's order
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    tris = np.zeros((cx, cy, cz, 6, 2, 3), dtype=np.int64)
    count = np.zeros((cx, cy, cz, 6), dtype=np.int64)
    ci = np.stack(np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij"), axis=-1)
    for k in range(6):
        v = tet_vertices(k)
        m = np.zeros((cx, cy, cz), dtype=np.int64)
        for i in range(4):
            m |= inside[v[i][0]:v[i][0] + cx, v[i][1]:v[i][1] + cy, v[i][2]:v[i][2] + cz].astype(np.int64) << i
        ntri = np.zeros(16, np.int64)
        owner = np.zeros((16, 2, 3, 3), np.int64)
        num = np.zeros((16, 2, 3), np.int64)
        for mask in range(16):
            case, _ = case_triangles(k, mask)
            ntri[mask] = len(case)
            for ti, tri in enumerate(case):
                for c, pair in enumerate(tri):
                    owner[mask, ti, c], num[mask, ti, c] = edge_of(k, pair)
        count[..., k] = ntri[m]
        for ti in range(2):
            for c in range(3):
                o = ci + owner[m, ti, c]
                tris[..., k, ti, c] = vid[o[..., 0], o[..., 1], o[..., 2], num[m, ti, c]]
    keep = np.arange(2)[None, None, None, None, :] < count[..., None]
    triangles = tris[keep].astype(np.int32).reshape(-1, 3)
    return vertices, vnormals, triangles
