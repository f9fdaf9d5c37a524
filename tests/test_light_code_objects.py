"""rc_light_sampling_backward's code: the library exports the new entry points, and its kernel uses no scratch and no bf16
MFMA (the backward runs in fp32; the split-bf16 form is fenced to the forward shaders)."""
import ctypes

import pytest

from test_code_objects import code_objects

LIGHT_KERNELS = {"k_light_sampling_loss_bwd", "k_gemm", "k_sum_parts", "k_grid_l2_bwd", "k_grid_l2_reduce"}


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    from nrc_amd import rc_ext
    return rc_ext.library_path(), code_objects(rc_ext.library_path(), tmp_path_factory.mktemp("light"))


def test_exports(product):
    lib = ctypes.CDLL(product[0])
    for name in ("rc_light_grad_size", "rc_light_grad_layout", "rc_light_sampling_backward", "rc_light_regularizer"):
        assert hasattr(lib, name), name
    from nrc_amd import rc_ext
    for name in ("rc_light_grad_size", "rc_light_grad_layout", "rc_light_sampling_backward", "rc_light_regularizer"):
        assert name in rc_ext.EXPORTS, name


def test_kernels_have_no_scratch_and_no_bf16_mfma(product):
    ks = {v["base"]: v for v in product[1].values() if v["base"] in LIGHT_KERNELS}
    assert set(ks) == LIGHT_KERNELS, sorted(set(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not any("bf16" in op for op in v["mfma"]), name
