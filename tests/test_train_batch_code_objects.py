"""rc_cast_rays_multi / rc_train_batch's code, on the code objects of tests/test_code_objects.py: the
library exports the two entry points under the unchanged ABI version, both kernels are there for gfx950, neither uses
scratch or the matrix pipe, and the single-camera kernel they share their per-pixel body with is still scratch-free."""
import ctypes

from test_code_objects import product  # noqa: F401  (product: fixture)

EXPORTS = ("rc_cast_rays_multi", "rc_train_batch")
KERNELS = {"k_cast_rays_multi", "k_train_batch"}


def test_exports():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert lib.rc_abi_version() == rc_ext.RC_ABI_VERSION == 5


def test_kernels_are_there_without_scratch(product):
    ks = {v["base"]: v for v in product.values() if v["base"] in KERNELS | {"k_cast_rays", "k_prng_fill"}}
    assert set(ks) == KERNELS | {"k_cast_rays", "k_prng_fill"}, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
        assert v["agpr"] == 0 and v["vgpr"] <= 128, (name, v["vgpr"], v["agpr"])      # streaming kernels: full occupancy
