"""The texture atlas on the GPU: rc_atlas_uvs, rc_atlas_points and rc_bake_atlas against the numpy
restatement of tests/atlas_ref.py and against rc_query_points / rc_query_cache_diffuse at the texels' points.

Meshes: one triangle (the cell's second half empty), three triangles (odd, cols 2, rows 1), a tetrahedron, and the 24^3
extract_mesh of tests/test_gpu_extract_mesh.py at r = 4 and r = 7.  uvs and owners are exact; the points lie within 2 ulp of
the box extent (the bound of tests/test_gpu_isosurface.py for vertices: the restatement and the kernel round the same
fp32 expression, a compiler may still fuse nothing here, -ffp-contract=off); a baked texel is the query at its point bit for
bit and exactly 0 where no triangle owns it.  No test passes a triangle index outside the vertex array."""
import numpy as np
import pytest
import torch

import atlas_ref as ar
import common
from nrc_amd import mesh, rc_ext

pytestmark = pytest.mark.gpu
LO, HI, DIMS = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (24, 24, 24)
KEYS = ("density", "normals_pred", "normals", "albedo", "roughness", "metalness", "ambient_diffuse", "indirect_diffuse",
        "cache_diffuse")
RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def rc():
    return common.make_rc(weights=common.weights_material_np())


def small_mesh(name):
    rng = np.random.Generator(np.random.PCG64(11))
    if name == "one":
        v, t = rng.uniform(-0.9, 0.9, size=(3, 3)), [[0, 1, 2]]
    elif name == "three":
        v, t = rng.uniform(-0.9, 0.9, size=(5, 3)), [[0, 1, 2], [2, 1, 3], [4, 0, 3]]
    else:
        v, t = np.array([[0.7, 0.7, 0.7], [-0.7, -0.7, 0.7], [-0.7, 0.7, -0.7], [0.7, -0.7, -0.7]]), [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
    return mesh.Mesh(vertices=torch.from_numpy(np.asarray(v, np.float32)).cuda(), triangles=torch.tensor(t, dtype=torch.int32).cuda())


_MESHES = {}


def get_mesh(rc, name):
    if name not in _MESHES:
        if name == "extracted":
            field = mesh.density_lattice(rc, LO, HI, DIMS)
            _MESHES[name] = mesh.extract_mesh(rc, float(field.median()), LO, HI, DIMS)
        else:
            _MESHES[name] = small_mesh(name)
    return _MESHES[name]


CASES = [("one", 4), ("one", 7), ("three", 5), ("tetrahedron", 8), ("extracted", 4), ("extracted", 7)]


@pytest.mark.parametrize("name,r", CASES)
def test_layout_uvs_owner_and_points(rc, name, r):
    m = get_mesh(rc, name)
    v, t = m.vertices.cpu().numpy(), m.triangles.cpu().numpy()
    T = len(t)
    cols, rows, W, H = ar.layout(T, r)
    assert mesh.atlas_layout(T, r) == (cols, rows, W, H)
    if name == "three":
        assert (cols, rows) == (2, 1)
    if name == "extracted":
        assert T > 1000 and W * H > 64 * 1024
    uvs = mesh.atlas_uvs(rc, T, r)
    points, owner = mesh.atlas_points(rc, m, r)
    torch.cuda.synchronize()
    assert uvs.shape == (T, 3, 2) and np.array_equal(uvs.cpu().numpy(), ar.uvs(T, r))
    ref_p, ref_o = ar.points(v, t, r)
    assert owner.dtype == torch.int32 and np.array_equal(owner.cpu().numpy(), ref_o)
    assert int((owner >= 0).sum()) == ar.owned_count(T, r)
    p = points.cpu().numpy()
    assert np.all(p[ref_o < 0] == 0.0)
    err = np.abs(p.astype(np.float64) - ref_p.astype(np.float64)).max()
    bound = 2 * np.spacing(np.float32(max(np.abs(LO).max(), np.abs(HI).max())))
    print(f"{name} r={r}: T={T}, atlas {W}x{H}, max |point - restatement| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    if name == "one":
        assert int((owner == -1).sum()) == r * (r - 1) // 2                     # the empty second half


@pytest.mark.parametrize("name,r", [("three", 5), ("extracted", 7)])
def test_ranges_equal_the_whole_atlas(rc, name, r):
    m = get_mesh(rc, name)
    W, H = mesh.atlas_layout(int(m.triangles.shape[0]), r)[2:]
    points, owner = mesh.atlas_points(rc, m, r)
    for first, count in ((0, 1), (W - 3, 2 * W + 5), (W * H - 37, 37), (W * H // 2 + 1, 67)):
        first, count = max(first, 0), min(count, W * H - max(first, 0))
        p, o = mesh.atlas_points(rc, m, r, first, count)
        assert torch.equal(p, points[first:first + count]) and torch.equal(o, owner[first:first + count]), (first, count)


@pytest.fixture(scope="module")
def baked(rc):
    out = {}
    for name, r in (("one", 4), ("three", 5), ("tetrahedron", 8), ("extracted", 4), ("extracted", 7)):
        out[name, r] = mesh.bake_atlas(rc, get_mesh(rc, name), r, KEYS)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,r", [("one", 4), ("three", 5), ("tetrahedron", 8), ("extracted", 4), ("extracted", 7)])
def test_bake_is_the_query_at_the_texel_points(rc, baked, name, r):
    m, atlas = get_mesh(rc, name), baked[name, r]
    T = int(m.triangles.shape[0])
    W, H = mesh.atlas_layout(T, r)[2:]
    assert (atlas.width, atlas.height, atlas.cell) == (W, H, r) and set(atlas.textures) == set(KEYS)
    assert torch.equal(atlas.uvs, mesh.atlas_uvs(rc, T, r))
    points, owner = mesh.atlas_points(rc, m, r)
    cov = atlas.coverage.reshape(-1)
    assert atlas.coverage.dtype == torch.uint8 and atlas.coverage.shape == (H, W)
    assert torch.equal(cov.bool(), owner >= 0) and int(cov.sum()) == ar.owned_count(T, r)
    q = mesh.query_points(rc, points, KEYS)
    for k in KEYS:
        tex = atlas.textures[k]
        assert tex.dtype == torch.float32 and tuple(tex.shape[:2]) == (H, W), k
        flat = tex.reshape(W * H, -1)
        assert torch.equal(flat[cov.bool()], q[k].reshape(W * H, -1)[cov.bool()]), k
        assert bool((flat[~cov.bool()] == 0).all()), k
    assert float(atlas.textures["albedo"].abs().max()) > 0 and float(atlas.textures["cache_diffuse"].abs().max()) > 0


def test_two_bakes_are_bitwise_equal_and_chunks_do_not_show(rc, baked):
    m = get_mesh(rc, "extracted")
    again = mesh.bake_atlas(rc, m, 7, KEYS)
    for k in KEYS:
        assert torch.equal(again.textures[k], baked["extracted", 7].textures[k]), k
    assert torch.equal(again.coverage, baked["extracted", 7].coverage)
    # a subset of the planes, and a level other than the last, go through other launches and give the same / the level's density
    albedo = mesh.bake_atlas(rc, m, 7, ("albedo",))
    assert torch.equal(albedo.textures["albedo"], again.textures["albedo"])
    diffuse = mesh.bake_atlas(rc, m, 7, ("cache_diffuse",))
    assert torch.equal(diffuse.textures["cache_diffuse"], again.textures["cache_diffuse"])
    points, owner = mesh.atlas_points(rc, m, 7)
    low = mesh.bake_atlas(rc, m, 7, ("density", "indirect_diffuse"), level=0)
    q = mesh.query_points(rc, points, ("density",), level=0)["density"]
    own = owner >= 0
    assert torch.equal(low.textures["density"].reshape(-1)[own], q[own])
    assert torch.equal(low.textures["indirect_diffuse"], again.textures["indirect_diffuse"])


def test_default_keys_and_8bit_pictures(rc, tmp_path):
    """bake_atlas' default keys, and the 8-bit conversion of save_textured_obj against the suite's restatement."""
    import vis_ref
    m = get_mesh(rc, "tetrahedron")
    m = mesh.Mesh(vertices=m.vertices, triangles=m.triangles, normals=torch.nn.functional.normalize(m.vertices, dim=1))
    atlas = mesh.bake_atlas(rc, m, 8)
    assert tuple(atlas.textures) == ("albedo", "roughness", "metalness", "normals_pred")
    images = mesh.atlas_images(atlas, rc=rc)
    H, W = atlas.height, atlas.width
    for k, img in images.items():
        assert img.shape == (H, W, 3) and img.dtype == np.uint8, k
        x = atlas.textures[k].cpu().numpy().reshape(H, W, -1)
        if k == "albedo":
            y = vis_ref.item("srgb", x, dtype=np.float32)[0]
        elif k == "normals_pred":
            y = vis_ref.item("matte", x, divide=2.0, offset=0.5, dtype=np.float32)[0]
        else:
            y = vis_ref.item("matte", x, dtype=np.float32)[0]
        diff = np.abs(img.astype(np.int32) - vis_ref.to_u8(y).astype(np.int32))
        assert diff.max() <= 1 and (diff > 0).mean() <= 0.01, (k, diff.max(), (diff > 0).mean())      # a rounding tie apart at most
    from PIL import Image
    paths = mesh.save_textured_obj(str(tmp_path / "tet.obj"), m, atlas, rc=rc)
    assert set(paths) == set(atlas.textures)
    for k, p in paths.items():
        assert np.array_equal(np.asarray(Image.open(p)), images[k]), k
    host = mesh.Atlas(width=W, height=H, cell=8, uvs=atlas.uvs.cpu().numpy(), coverage=atlas.coverage.cpu().numpy(),
                      textures={k: v.cpu().numpy() for k, v in atlas.textures.items()})      # float arrays on the host
    for k, img in mesh.atlas_images(host, rc=rc).items():
        assert np.array_equal(img, images[k]), k
    text = open(str(tmp_path / "tet.obj")).read().splitlines()
    assert sum(l.startswith("vt ") for l in text) == 12 and sum(l.startswith("f ") for l in text) == 4


def test_refusals(rc):
    m = get_mesh(rc, "three")
    v, t = m.vertices, m.triangles
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.full((4096,), -7.0, device="cuda")
    own = torch.full((1024,), -7, dtype=torch.int32, device="cuda")
    pts = lambda T, r, first, count, vp=v.data_ptr(), V=5, tp=t.data_ptr(): rc.lib.rc_atlas_points(
        rc._h, vp, V, tp, T, r, first, count, buf.data_ptr(), own.data_ptr(), st)
    assert pts(3, 5, 0, 50) == 0
    assert pts(3, 3, 0, 1) == RC_ERR_INVALID_ARG and pts(3, 65, 0, 1) == RC_ERR_INVALID_ARG and pts(0, 5, 0, 1) == RC_ERR_INVALID_ARG
    assert pts(3, 5, -1, 1) == RC_ERR_INVALID_ARG and pts(3, 5, 0, -1) == RC_ERR_INVALID_ARG
    assert pts(3, 5, 0, 51) == RC_ERR_INVALID_ARG and pts(3, 5, 50, 1) == RC_ERR_INVALID_ARG          # W H = 50
    assert pts(3, 5, 0, 1, vp=None) == RC_ERR_INVALID_ARG and pts(3, 5, 0, 1, tp=None) == RC_ERR_INVALID_ARG
    assert pts(3, 5, 0, 1, V=0) == RC_ERR_INVALID_ARG
    assert pts(2 ** 31 - 1, 4, 0, 1) == RC_ERR_UNSUPPORTED
    buf.fill_(-7.0)
    assert pts(3, 5, 50, 0) == 0 and pts(3, 5, 0, 0) == 0                                               # count == 0: nothing launched
    assert rc.lib.rc_atlas_uvs(rc._h, 3, 5, None, st) == RC_ERR_INVALID_ARG
    assert rc.lib.rc_atlas_uvs(rc._h, 3, 2, buf.data_ptr(), st) == RC_ERR_INVALID_ARG
    out = rc_ext.rc_atlas_outputs()
    out.density = buf.data_ptr()
    import ctypes as C
    bake = lambda T, r, level, o=out: rc.lib.rc_bake_atlas(rc._h, v.data_ptr(), 5, t.data_ptr(), T, r, level, None if o is None else C.byref(o), st)
    assert bake(3, 3, -1) == RC_ERR_INVALID_ARG and bake(3, 5, 3) == RC_ERR_INVALID_ARG and bake(3, 5, -1, None) == RC_ERR_INVALID_ARG
    assert bake(2 * 4096 * 4096 + 1, 4, -1) == RC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())
    out.normals_pred = buf.data_ptr()
    assert bake(3, 5, 0) == RC_ERR_UNSUPPORTED                                                          # normals on another level than the last
    with pytest.raises(ValueError):
        mesh.bake_atlas(rc, m, 5, ("rgb",))
    with pytest.raises(rc_ext.RcError) as e:
        mesh.bake_atlas(rc, m, 65)
    assert e.value.code == RC_ERR_INVALID_ARG
    cache_only = common.make_rc()
    with pytest.raises(rc_ext.RcError) as e:
        mesh.bake_atlas(cache_only, m, 5, ("albedo",))
    assert e.value.code == -3                                                                           # RC_ERR_MISSING_WEIGHT
    d = mesh.bake_atlas(cache_only, m, 5, ("cache_diffuse", "density"))                                 # needs no material weights
    assert bool(torch.isfinite(d.textures["cache_diffuse"]).all())
