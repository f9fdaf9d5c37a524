"""The surface export's code, read from the gfx950 code objects and the binding (no GPU needed): rc_query_points,
rc_density_lattice and rc_isosurface are exported and bound with the header's argument counts, the ABI version did not
move, and the new kernels of rc_mesh.hip use no scratch and no MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

KERNELS = {"k_rows_to_soa", "k_soa_to_rows", "k_lattice_points", "k_nan_to_num", "k_iso_classify", "k_iso_scan_tiles",
           "k_iso_scan_groups", "k_iso_vertices", "k_iso_triangles"}


def test_mesh_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name, nargs in (("rc_query_points", 9), ("rc_density_lattice", 9), ("rc_isosurface", 15)):
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
        restype, argtypes = rc_ext._PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    iso = rc_ext._PROTOTYPES["rc_isosurface"][1]
    assert iso[5] is ctypes.c_float and iso[10] is ctypes.c_int64 and iso[12] is ctypes.c_int64
    assert rc_ext._PROTOTYPES["rc_query_points"][1][2] is ctypes.c_int64
    for method in ("query_points", "density_lattice", "isosurface", "isosurface_into"):
        assert callable(getattr(rc_ext.RadianceCache, method)), method
    lib.rc_abi_version.restype = ctypes.c_int
    assert lib.rc_abi_version() == 5 == rc_ext.RC_ABI_VERSION


def test_mesh_module_is_part_of_the_package():
    import nrc_amd
    from nrc_amd import mesh

    assert nrc_amd.mesh is mesh
    for name in ("query_points", "density_lattice", "isosurface", "extract_mesh", "save_obj", "Mesh"):
        assert hasattr(mesh, name), name


def test_mesh_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = [v for v in product.values() if v["base"] in KERNELS]
    assert sorted(v["base"] for v in ks) == sorted(KERNELS), sorted(v["base"] for v in ks)
    for v in ks:
        assert v["scratch"] == 0, (v["base"], v["scratch"])
        assert not v["mfma"], (v["base"], v["mfma"])
