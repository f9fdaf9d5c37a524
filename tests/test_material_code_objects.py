"""rc_material_smoothness_backward's code: the library exports the new entry points, and its kernels use no scratch and no
bf16 MFMA (the backward runs in fp32; the split-bf16 form is fenced to the forward shaders)."""
import ctypes

import pytest

from test_code_objects import code_objects

MATERIAL_KERNELS = {"k_material_smoothness_points", "k_material_smoothness_bwd", "k_material_smoothness_reduce",
                    "k_grid_l2_bwd", "k_grid_l2_reduce"}
NAMES = ("rc_material_grad_size", "rc_material_grad_layout", "rc_material_smoothness_backward", "rc_material_regularizer")


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    from nrc_amd import rc_ext
    return rc_ext.library_path(), code_objects(rc_ext.library_path(), tmp_path_factory.mktemp("material"))


def test_exports(product):
    lib = ctypes.CDLL(product[0])
    for name in NAMES:
        assert hasattr(lib, name), name
    from nrc_amd import rc_ext
    for name in NAMES:
        assert name in rc_ext.EXPORTS, name


def test_kernels_have_no_scratch_and_no_bf16_mfma(product):
    ks = {v["base"]: v for v in product[1].values() if v["base"] in MATERIAL_KERNELS}
    assert set(ks) == MATERIAL_KERNELS, sorted(set(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not any("bf16" in op for op in v["mfma"]), name
    for name in ("k_material_smoothness_bwd", "k_material_smoothness_reduce"):
        assert not ks[name]["mfma"], name                        # plain fp32, no MFMA at all
