"""The time-resolved cache stage's sampler side, read from the gfx950 code objects (no GPU needed): the seven exports are
there and bound without a change of the ABI version, the code object of rc_transient_sampler.hip holds exactly its one
kernel, which runs on 64-lane waves, uses no scratch, no LDS and no MFMA; the losses' fixed-order sums and the density
backward reuse the existing kernels."""
import ctypes
import re
import shutil
import subprocess

from test_code_objects import LLVM, _base_name, product  # noqa: F401  (fixture, helpers)

EXPORTS = ("rc_transient_sampler_grad_size", "rc_transient_sampler_grad_layout", "rc_transient_interlevel_backward",
           "rc_transient_geometry_backward", "rc_transient_mask_backward", "rc_transient_density_regularizer",
           "rc_transient_data_backward_sampler")
KERNELS = {"k_transient_weights_bwd"}
REUSED = ("k_interlevel_reduce", "k_interlevel_bwd", "k_geometry_loss_bwd", "k_mask_loss_bwd", "k_grid_l2_bwd", "k_density_bwd",
          "k_points_aos")


def test_exports_and_layout_id():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name
    assert rc_ext.RC_LAYOUT_TRANSIENT_SAMPLER == -6
    assert rc_ext._GRAD_LAYOUTS["transient_sampler"][2] == -6 and rc_ext._LAYOUT_KEYS[-6] == "transient_sampler"
    assert lib.rc_abi_version() == rc_ext.RC_ABI_VERSION          # additive: the existing exports keep their version


def test_kernel_set_scratch_and_mfma(product):  # noqa: F811
    ks = {v["base"]: (co, v) for (co, _), v in product.items() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    (co, v), = ks.values()
    assert {x["base"] for (c, _), x in product.items() if c == co} == KERNELS     # nothing else in its translation unit
    assert v["scratch"] == 0 and not v["mfma"] and v["agpr"] == 0, v
    assert v["vgpr"] <= 64, v["vgpr"]                              # a per-ray scan kernel: full occupancy
    for name in REUSED:            # one translation unit each, not the new one: the new calls launch the existing kernels
        cos = {c for (c, _), x in product.items() if x["base"] == name}
        assert len(cos) == 1 and co not in cos, (name, cos)


def test_wave_size_and_lds(tmp_path):
    from nrc_amd import rc_ext

    so = tmp_path / "lib.so"
    shutil.copy(rc_ext.library_path(), so)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    found = 0
    for co in sorted(p for p in tmp_path.iterdir() if p.name.endswith("gfx950")):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        if "amdhsa.kernels:" not in notes:
            continue
        for entry in re.split(r"^  - ", notes.split("amdhsa.kernels:", 1)[1], flags=re.M)[1:]:
            kv = dict(re.findall(r"^\s*\.(name|wavefront_size|group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)",
                                 "    " + entry, re.M))
            if _base_name(kv.get("name", "")) in KERNELS:
                found += 1
                assert int(kv["wavefront_size"]) == 64, kv
                assert int(kv["group_segment_fixed_size"]) == 0, kv
                assert int(kv["max_flat_workgroup_size"]) == 256, kv          # four rays, one wave each
    assert found == 1
