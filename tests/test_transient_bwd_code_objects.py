"""rc_transient_data_backward's exports and kernels, read from the gfx950 code objects (no GPU needed): the new kernels
exist, use no scratch and no bf16 MFMA (the recompute is fp32 whatever the forward's arithmetic), k_transient_bins_bwd runs
its recompute on the fp32 matrix instruction, and the products of the head layers go through k_gemm_tile."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture: the product library's code objects)

EXPORTS = ("rc_transient_head_grad_size", "rc_transient_head_grad_layout", "rc_transient_data_backward")
KERNELS = {"k_transient_loss", "k_transient_bins_bwd", "k_gemm_tile"}
MFMA = "v_mfma_f32_32x32x2_f32"


def test_exports_and_abi_version():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert lib.rc_abi_version() == 5 == rc_ext.RC_ABI_VERSION
    assert rc_ext.RC_LAYOUT_TRANSIENT_HEADS == -5


def test_kernels(product):  # noqa: F811
    ks = {}
    for v in product.values():
        if v["base"] in KERNELS:
            ks.setdefault(v["base"], []).append(v)
    assert set(ks) == KERNELS, sorted(ks)
    for name, vs in ks.items():
        for v in vs:
            assert v["scratch"] == 0, (name, v["scratch"])
            assert not any("bf16" in op for op in v["mfma"]), name
    assert not ks["k_transient_loss"][0]["mfma"]
    bwd = ks["k_transient_bins_bwd"][0]
    # 64 + 32 k-steps of a tile at the least (more if the tile loop is unrolled), every one the fp32 instruction
    assert bwd["mfma"].count(MFMA) >= 96 and set(bwd["mfma"]) == {MFMA}, bwd["mfma"][:4]
    assert all(MFMA in v["mfma"] for v in ks["k_gemm_tile"])
