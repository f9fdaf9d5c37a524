"""The loss family's exports and kernels, read from the gfx950 code objects (no GPU needed): k_transient_loss_kinds and
k_dtof_to_itof exist, use no scratch (their row sums are reduced one row at a time) and no matrix instruction;
k_transient_loss is still there beside them."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture: the product library's code objects)

EXPORTS = ("rc_transient_data_backward_kind", "rc_dtof_to_itof")
NEW_KERNELS = {"k_transient_loss_kinds", "k_dtof_to_itof"}


def test_exports_and_abi_version():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS + ("rc_transient_data_backward",):
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert lib.rc_abi_version() == 5 == rc_ext.RC_ABI_VERSION


def test_kernels(product):  # noqa: F811
    ks = {}
    for v in product.values():
        if v["base"] in NEW_KERNELS | {"k_transient_loss"}:
            ks.setdefault(v["base"], []).append(v)
    assert set(ks) == NEW_KERNELS | {"k_transient_loss"}, sorted(ks)
    for name, vs in ks.items():
        for v in vs:
            assert v["scratch"] == 0, (name, v["scratch"])
            assert not v["mfma"], (name, v["mfma"][:4])
