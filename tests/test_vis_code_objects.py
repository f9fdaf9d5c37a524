"""The visualisation calls' code, read from the gfx950 code objects (no GPU needed): the four exports are there and bound,
their kernels exist, none of them uses scratch or an MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

EXPORTS = ("rc_weighted_percentile", "rc_image_max", "rc_vis_images", "rc_vis_turbo_lut")
KERNELS = {"k_vis_select_begin", "k_vis_select_hist", "k_vis_select_narrow", "k_vis_select_neighbours",
           "k_vis_select_finish", "k_vis_max", "k_vis_max_finish", "k_vis_bins", "k_vis_items"}


def test_vis_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name


def test_vis_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = {v["base"]: v for v in product.values() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
