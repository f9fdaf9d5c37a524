"""The mask loss's code, read from the gfx950 code objects (no GPU needed): the two exports are there and bound, the
code object of rc_mask.hip holds exactly its two kernels (the loss's fixed-order sum reuses k_interlevel_reduce of
rc_interlevel.hip), and neither uses scratch or an MFMA."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

EXPORTS = ("rc_backward_mask_rays", "rc_mask_backward")
KERNELS = {"k_backward_mask_rays", "k_mask_loss_bwd"}
REUSED = "k_interlevel_reduce"


def test_mask_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert {k for k, _ in rc_ext.rc_mask_loss._fields_} == {"charb_padding", "weight_opaque", "weight_empty", "zero_masks"}


def test_mask_kernels_are_the_two_and_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = {v["base"]: (co, v) for (co, _), v in product.items() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    cos = {co for co, _ in ks.values()}
    assert len(cos) == 1, cos                                   # one translation unit
    (co,) = cos
    assert {v["base"] for (c, _), v in product.items() if c == co} == KERNELS     # and nothing else in it
    assert sum(v["base"] == REUSED for v in product.values()) == 1                # the reduce kernel is the existing one
    for name, (_, v) in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
