"""rc_data_backward's code: the library exports the new entry points, and its kernels use no scratch and no bf16 MFMA
(the split-bf16 form is fenced to the forward shaders; the backward runs the exact fp32 MFMA chain)."""
import ctypes

import pytest

from test_code_objects import code_objects

DATA_KERNELS = {"k_data_loss_bwd", "k_gemm", "k_sum_parts", "k_stage_feature", "k_shader_glue_fwd", "k_shader_out_bwd",
                "k_shader_glue_bwd", "k_split_feature"}


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    from nrc_amd import rc_ext
    return rc_ext.library_path(), code_objects(rc_ext.library_path(), tmp_path_factory.mktemp("data"))


def test_exports(product):
    lib = ctypes.CDLL(product[0])
    for name in ("rc_shader_grad_size", "rc_shader_grad_layout", "rc_data_backward"):
        assert hasattr(lib, name), name


def test_kernels_have_no_scratch_and_no_bf16_mfma(product):
    ks = {v["base"]: v for v in product[1].values() if v["base"] in DATA_KERNELS}
    assert set(ks) == DATA_KERNELS, sorted(set(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not any("bf16" in op for op in v["mfma"]), name
    assert any(op == "v_mfma_f32_32x32x2_f32" for op in ks["k_gemm"]["mfma"])
