"""rc_adam_update's code: the library exports the optimizer entry points, and its kernels use no scratch and no MFMA
(streaming element-wise code with 16-byte loads and stores)."""
import ctypes

import pytest

from test_code_objects import code_objects

OPTIM_KERNELS = {"k_adam", "k_adam_sumsq", "k_adam_norm"}


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    from nrc_amd import rc_ext
    return rc_ext.library_path(), code_objects(rc_ext.library_path(), tmp_path_factory.mktemp("optim"))


def test_exports(product):
    lib = ctypes.CDLL(product[0])
    for name in ("rc_adam_update", "rc_load_params_flat"):
        assert hasattr(lib, name), name


def test_kernels_have_no_scratch_and_no_mfma(product):
    ks = {v["base"]: v for v in product[1].values() if v["base"] in OPTIM_KERNELS}
    assert set(ks) == OPTIM_KERNELS, sorted(set(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
