"""rc_eval_shift_invariant's code, read from the gfx950 code objects (no GPU needed): the export is there and bound, its
three kernels exist (both instantiations of the two templated ones), none of them uses scratch or an MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

KERNELS = {"k_si_metric", "k_si_select", "k_si_finish"}


def test_eval_si_export_is_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    assert hasattr(lib, "rc_eval_shift_invariant")
    assert "rc_eval_shift_invariant" in rc_ext.EXPORTS
    restype, argtypes = rc_ext._PROTOTYPES["rc_eval_shift_invariant"]
    assert restype is ctypes.c_int and argtypes[1] is ctypes.POINTER(rc_ext.rc_eval_si_images)


def test_eval_si_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = [v for v in product.values() if v["base"] in KERNELS]
    assert {v["base"] for v in ks} == KERNELS, sorted(v["base"] for v in ks)
    assert sum(v["base"] == "k_si_metric" for v in ks) == 2 and sum(v["base"] == "k_si_select" for v in ks) == 2
    for v in ks:
        assert v["scratch"] == 0, (v["base"], v["scratch"])
        assert not v["mfma"], (v["base"], v["mfma"])
