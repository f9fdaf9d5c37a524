"""rc_material_data_backward_env's code, on the code objects of tests/test_code_objects.py: the library
exports the new entry points, the new kernels are there, none of them uses scratch or a bf16 MFMA, the tiled GEMM runs
v_mfma_f32_32x32x2_f32 from operands it reads out of LDS, and the per-ray kernel has no MFMA at all."""
import ctypes
import os
import re
import shutil
import subprocess

from test_code_objects import LLVM, _base_name, product  # noqa: F401  (product: fixture)

EXPORTS = ("rc_envmap_grad_size", "rc_envmap_grad_layout", "rc_material_data_backward_env")
KERNELS = {"k_material_data_env_bwd", "k_envmap_stage", "k_envmap_out_bwd", "k_gemm_tile"}


def test_exports():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert lib.rc_abi_version() == rc_ext.RC_ABI_VERSION == 5


def test_kernels_have_no_scratch_and_no_bf16_mfma(product):
    ks = {v["base"]: v for v in product.values() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not any("bf16" in op for op in v["mfma"]), name
    assert "v_mfma_f32_32x32x2_f32" in ks["k_gemm_tile"]["mfma"]
    assert set(ks["k_gemm_tile"]["mfma"]) == {"v_mfma_f32_32x32x2_f32"}
    for name in ("k_material_data_env_bwd", "k_envmap_stage", "k_envmap_out_bwd"):
        assert not ks[name]["mfma"], (name, ks[name]["mfma"])
    # the old call's kernels are as test_material_data_code_objects pins them, beside the new instantiation of their body
    old = {v["base"]: v for v in product.values() if v["base"] in ("k_material_data_bwd", "k_material_data_head_bwd")}
    assert len(old) == 2 and all(not v["mfma"] and v["scratch"] == 0 for v in old.values())


def test_tiled_gemm_reads_its_operands_from_lds(tmp_path):
    """k_gemm_tile's ISA: LDS reads (ds_read*) and writes, 16-byte global loads, no scalar-indexed registers."""
    from nrc_amd import rc_ext

    so = tmp_path / "lib.so"
    shutil.copy(rc_ext.library_path(), so)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    bodies = []                                                   # one per instantiation (128 x 128 and 64 x 64 tiles)
    for co in sorted(p for p in tmp_path.iterdir() if p.name.endswith("gfx950")):
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.M | re.S):
            if _base_name(m.group(1)) == "k_gemm_tile":
                bodies.append(m.group(2))
    assert len(bodies) == 2
    counts = []
    for body in bodies:
        ops = re.findall(r"^\s*([a-z_0-9]+)", body, re.M)
        assert sum(op.startswith("ds_read") for op in ops) >= 2, "no LDS reads"
        assert any(op.startswith("ds_write") for op in ops)
        assert "global_load_dwordx4" in ops
        assert not any(op.startswith("s_set_gpr_idx") for op in ops)
        counts.append(ops.count("v_mfma_f32_32x32x2_f32"))
    # a step of 16 k is 8 MFMAs per tile of a wave: 4 tiles (128 x 128) and 1 tile (64 x 64), the loop unrolled
    assert sorted(counts) == [8, 32], counts
