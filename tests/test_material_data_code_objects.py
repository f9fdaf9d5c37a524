"""rc_material_data_backward's code: the library exports the entry point, and its kernels use no scratch and no MFMA
(the TRAINING["material_data"] row of tests/test_code_objects.py, on that module's code objects)."""
from test_code_objects import check_training_exports, check_training_kernels, product  # noqa: F401  (product: fixture)


def test_exports():
    check_training_exports("material_data")


def test_kernels_have_no_scratch_and_no_mfma(product):
    check_training_kernels(product, "material_data")
