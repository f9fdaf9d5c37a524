"""rc_render_transient_slices' code, read from the gfx950 code objects (no GPU needed): the export is there and bound
with its struct pointer types, the ABI version did not move, and k_transient_slice is in the product and uses no scratch
(and no MFMA: its head values are plain fp32 dot products)."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

KERNELS = {"k_transient_slice"}


def test_transient_slice_export_is_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    assert hasattr(lib, "rc_render_transient_slices")
    assert "rc_render_transient_slices" in rc_ext.EXPORTS
    restype, argtypes = rc_ext._PROTOTYPES["rc_render_transient_slices"]
    assert restype is ctypes.c_int and len(argtypes) == 9
    assert argtypes[1] is ctypes.POINTER(rc_ext.rc_rays)
    assert argtypes[6] is ctypes.POINTER(rc_ext.rc_transient_slices)
    assert argtypes[7] is ctypes.POINTER(rc_ext.rc_transient_outputs)
    s = rc_ext.rc_transient_slices
    assert rc_ext.RC_TSLICE_MAX == 8 and s.t.size == 4 * rc_ext.RC_TSLICE_MAX
    assert [f for f, _ in s._fields_] == ["count", "t", "rgb", "direct", "indirect"]
    lib.rc_abi_version.restype = ctypes.c_int
    assert lib.rc_abi_version() == 5 == rc_ext.RC_ABI_VERSION


def test_transient_slice_kernel_uses_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = [v for v in product.values() if v["base"] in KERNELS]
    assert sorted(v["base"] for v in ks) == sorted(KERNELS), sorted(v["base"] for v in ks)
    for v in ks:
        assert v["scratch"] == 0, (v["base"], v["scratch"])
        assert not v["mfma"], (v["base"], v["mfma"])
