"""rc_eval_image's code, read from the gfx950 code objects (no GPU needed): the export is there and bound, its four
kernels exist, none of them uses scratch or an MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

KERNELS = {"k_eval_bins", "k_eval_pixels", "k_eval_ssim", "k_eval_finish"}


def test_eval_export_is_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    assert hasattr(lib, "rc_eval_image")
    assert "rc_eval_image" in rc_ext.EXPORTS


def test_eval_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = {v["base"]: v for v in product.values() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
