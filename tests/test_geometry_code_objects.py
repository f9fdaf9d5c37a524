"""rc_geometry_backward's code: the library exports the entry points, and its kernels use no scratch and no bf16 MFMA
(the TRAINING["geometry"] row of tests/test_code_objects.py, on that module's code objects)."""
from test_code_objects import check_training_exports, check_training_kernels, product  # noqa: F401  (product: fixture)


def test_exports():
    check_training_exports("geometry")


def test_kernels_have_no_scratch_and_no_bf16_mfma(product):
    check_training_kernels(product, "geometry")
