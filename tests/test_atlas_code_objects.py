"""The textured export's code, read from the gfx950 code objects and the binding (no GPU needed): rc_atlas_layout,
rc_atlas_uvs, rc_atlas_points, rc_query_cache_diffuse and rc_bake_atlas are exported and bound with the header's argument
counts, the ABI version did not move, and the kernels of rc_atlas.hip use no scratch and no MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

KERNELS = {"k_atlas_uvs", "k_atlas_points", "k_atlas_store", "k_shader_diffuse_points"}
EXPORTS = (("rc_atlas_layout", 3), ("rc_atlas_uvs", 5), ("rc_atlas_points", 11), ("rc_query_cache_diffuse", 5),
           ("rc_bake_atlas", 9))


def test_atlas_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name, nargs in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
        restype, argtypes = rc_ext._PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    points = rc_ext._PROTOTYPES["rc_atlas_points"][1]
    assert [points[i] for i in (2, 4, 6, 7)] == [ctypes.c_int64] * 4 and points[5] is ctypes.c_int32
    assert rc_ext._PROTOTYPES["rc_atlas_layout"][1][0] is ctypes.c_int64
    assert len(rc_ext._PROTOTYPES["rc_query_points"][1]) == 9                  # untouched
    assert [k for k, _ in rc_ext.rc_atlas_outputs._fields_] == ["density", "normals_pred", "normals", "material", "diffuse", "coverage"]
    for method in ("query_cache_diffuse", "atlas_uvs", "atlas_points", "bake_atlas"):
        assert callable(getattr(rc_ext.RadianceCache, method)), method
    lib.rc_abi_version.restype = ctypes.c_int
    assert lib.rc_abi_version() == 5 == rc_ext.RC_ABI_VERSION


def test_mesh_module_has_the_atlas():
    from nrc_amd import mesh

    for name in ("atlas_layout", "atlas_uvs", "atlas_points", "bake_atlas", "atlas_images", "save_textured_obj", "Atlas"):
        assert hasattr(mesh, name), name
    assert mesh.KEYS == ("density", "normals_pred", "normals", "albedo", "roughness", "metalness")
    assert mesh.DIFFUSE_KEYS == ("ambient_diffuse", "indirect_diffuse", "cache_diffuse")


def test_atlas_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = [v for v in product.values() if v["base"] in KERNELS]
    assert sorted(v["base"] for v in ks) == sorted(KERNELS), sorted(v["base"] for v in ks)
    for v in ks:
        assert v["scratch"] == 0, (v["base"], v["scratch"])
        assert not v["mfma"], (v["base"], v["mfma"])
