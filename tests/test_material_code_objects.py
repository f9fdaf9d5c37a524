"""rc_material_smoothness_backward's code: the library exports the entry points, and its kernels use no scratch and no
bf16 MFMA, the backward and the reduction no MFMA at all (the TRAINING["material"] row of tests/test_code_objects.py, on
that module's code objects)."""
from test_code_objects import check_training_exports, check_training_kernels, product  # noqa: F401  (product: fixture)


def test_exports():
    check_training_exports("material")


def test_kernels_have_no_scratch_and_no_bf16_mfma(product):
    check_training_kernels(product, "material")
