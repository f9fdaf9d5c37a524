"""The code of rc_normals_backward and rc_geometry_smoothness_backward, read from the gfx950 code objects (no GPU needed):
both exports are there and bound, the code object of rc_normals_bwd.hip holds exactly its four kernels (the weight-gradient
contraction and the loss's fixed-order sum reuse k_wgrad / k_grad_reduce / k_interlevel_reduce), none uses scratch, and the
per-point kernel runs on the fp32 matrix pipe alone."""
import ctypes

from test_code_objects import product  # noqa: F401  (fixture)

EXPORTS = ("rc_normals_backward", "rc_geometry_smoothness_backward")
# kernel -> the MFMA opcode it must contain (None: no MFMA at all)
KERNELS = {"k_normals_bwd": "v_mfma_f32_32x32x2_f32", "k_grid_scatter_jac": None, "k_gsmooth_points": None, "k_gsmooth_loss": None}
REUSED = ("k_wgrad", "k_grad_reduce", "k_interlevel_reduce")
# k_normals_bwd's layers: forward 17 + 33 steps of two tiles, W1^T 32 x 2, W0^T 32 x 1, the two forward layers once more
PER_POINT_MFMAS = 2 * (17 * 2 + 33 * 2) + 32 * 2 + 32


def test_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert [k for k, _ in rc_ext.rc_geometry_smoothness._fields_] == ["noise", "weight_normals", "weight_normals_pred", "weight_density"]


def test_kernels_are_found_and_use_no_scratch(product):  # noqa: F811
    mine = {k: v for k, v in product.items() if v["base"] in KERNELS}
    assert {v["base"] for v in mine.values()} == set(KERNELS), sorted(v["base"] for v in mine.values())
    cos = {co for co, _ in mine}
    assert len(cos) == 1, cos                                   # one translation unit
    (co,) = cos
    assert {v["base"] for (c, _), v in product.items() if c == co} == set(KERNELS)     # and nothing else in it
    for name in REUSED:                                         # the existing kernels, not twins of them
        assert sum(v["base"] == name for v in product.values()) == 1, name
    assert sum(v["base"] == "k_grid_scatter_jac" for v in mine.values()) == 2          # F = 4 and F = 1
    for (_, sym), v in mine.items():
        assert v["scratch"] == 0, (sym, v["scratch"])
        assert not any("bf16" in op for op in v["mfma"]), sym
        if KERNELS[v["base"]] is None:
            assert not v["mfma"], (sym, v["mfma"])


def test_per_point_kernel_runs_on_the_fp32_matrix_pipe(product):  # noqa: F811
    (v,) = [v for v in product.values() if v["base"] == "k_normals_bwd"]
    assert set(v["mfma"]) == {KERNELS["k_normals_bwd"]}, set(v["mfma"])
    assert len(v["mfma"]) == PER_POINT_MFMAS, len(v["mfma"])
    assert v["vgpr"] < 512                                      # no need for the split form's whole-register-file fence
