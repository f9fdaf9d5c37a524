"""The relighting calls' code, read from the gfx950 code objects (no GPU needed): the five exports are there and bound,
their kernels exist, none of them uses scratch or an MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

EXPORTS = ("rc_set_env_image", "rc_env_tables", "rc_env_lookup", "rc_env_pick", "rc_render_relight")
KERNELS = {"k_env_pad", "k_env_lookup", "k_env_tables_sum", "k_env_tables", "k_env_logp", "k_env_pick", "k_env_pick_finish",
           "k_env_sample", "k_albedo_ratio"}


def test_relight_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name


def test_relight_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = {v["base"]: v for v in product.values() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
