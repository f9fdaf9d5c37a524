"""rc_prng_fill_segments' code, on the code objects of tests/test_code_objects.py: the library exports
the two entry points, k_prng_fill_segments is there for gfx950 as a streaming kernel -- no scratch, no matrix pipe, no
AGPRs and at most 128 VGPRs (full occupancy) -- and k_prng_fill beside it is still one as well.  Register and
scratch metadata only."""
import ctypes

from test_code_objects import product  # noqa: F401  (product: fixture)

EXPORTS = ("rc_material_randoms_plan", "rc_prng_fill_segments")
KERNELS = {"k_prng_fill_segments", "k_prng_fill"}


def test_exports():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert lib.rc_abi_version() == rc_ext.RC_ABI_VERSION


def test_kernels_are_streaming_kernels(product):
    ks = {v["base"]: v for v in product.values() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
        assert v["agpr"] == 0 and v["vgpr"] <= 128, (name, v["vgpr"], v["agpr"])
        print(name, {k: v[k] for k in ("vgpr", "agpr", "scratch")})
    assert ks["k_prng_fill"]["vgpr"] == 42          # its row on the parent commit: the new kernel beside it changed nothing
