"""rc_adam_update's code: the library exports the optimizer entry points, and its kernels use no scratch and no MFMA
(the TRAINING["optimizer"] row of tests/test_code_objects.py, on that module's code objects)."""
from test_code_objects import check_training_exports, check_training_kernels, product  # noqa: F401  (product: fixture)


def test_exports():
    check_training_exports("optimizer")


def test_kernels_have_no_scratch_and_no_mfma(product):
    check_training_kernels(product, "optimizer")
