"""rc_material_data_backward's code: the library exports the new entry point, and its kernels use no scratch and no bf16
MFMA (the backward runs in fp32, no MFMA at all)."""
import ctypes

import pytest

from test_code_objects import code_objects

DATA_KERNELS = {"k_material_data_bwd", "k_material_data_head_bwd"}
NAMES = ("rc_material_data_backward",)


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    from nrc_amd import rc_ext
    return rc_ext.library_path(), code_objects(rc_ext.library_path(), tmp_path_factory.mktemp("material_data"))


def test_exports(product):
    lib = ctypes.CDLL(product[0])
    from nrc_amd import rc_ext
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name


def test_kernels_have_no_scratch_and_no_mfma(product):
    ks = {v["base"]: v for v in product[1].values() if v["base"] in DATA_KERNELS}
    assert set(ks) == DATA_KERNELS, sorted(set(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], name
