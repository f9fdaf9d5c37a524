"""rc_probe_rays' and rc_vmf_panorama's code, read from the gfx950 code objects (no GPU needed): both exports are there and
bound with their struct pointer types, the ABI version did not move, and the two kernels use no scratch and no MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

KERNELS = {"k_probe_rays", "k_vmf_panorama"}


def test_probe_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in ("rc_probe_rays", "rc_vmf_panorama"):
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    restype, argtypes = rc_ext._PROTOTYPES["rc_probe_rays"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert argtypes[1] is ctypes.POINTER(rc_ext.rc_probe_view) and argtypes[10] is ctypes.POINTER(rc_ext.rc_cast_outputs)
    restype, argtypes = rc_ext._PROTOTYPES["rc_vmf_panorama"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    lib.rc_abi_version.restype = ctypes.c_int
    assert lib.rc_abi_version() == 5 == rc_ext.RC_ABI_VERSION


def test_probe_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = [v for v in product.values() if v["base"] in KERNELS]
    assert sorted(v["base"] for v in ks) == sorted(KERNELS), sorted(v["base"] for v in ks)
    for v in ks:
        assert v["scratch"] == 0, (v["base"], v["scratch"])
        assert not v["mfma"], (v["base"], v["mfma"])
