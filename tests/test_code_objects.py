"""The register-file fence of the split-form kernels, read from the gfx950 code objects (no GPU needed).

The split form (rc_dev_mlp.h: fp32 operands as three bf16 pieces, six products on v_mfma_f32_32x32x16_bf16) gives
launch-to-launch differences of ~1e-3 when a wave of another workgroup or kernel shares its SIMD (INSTABILITY there).
What keeps that from happening is split_exclusive_simd(): the wave names v255/a255 and so allocates all 512 registers of
its SIMD.  Only compiler behaviour holds that, so it is checked here on what the compiler made: every kernel of the
product library with a bf16 MFMA in its ISA has .vgpr_count 512 and no scratch.  The kernels are found from the ISA, so
a new split kernel is covered without editing a list.  The fp32-MFMA variant (make variant-f32) has no bf16 MFMA at all.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
LLVM = "/opt/rocm/llvm/bin"
SPLIT_KERNELS = {"k_cache_fused", "k_cache_shader", "k_envmap", "k_transient_shader", "k_transient_bins"}


def _base_name(mangled):
    """The kernel's identifier in its Itanium-mangled name (the same for every instantiation of a template):
    _ZN12_GLOBAL__N_113k_cache_fusedILb1E... -> k_cache_fused.  Reads the nested name's <length><identifier> parts."""
    i = 2 + (mangled[2:3] == "N")
    while i < len(mangled) and mangled[i].isdigit():
        j = i
        while mangled[j].isdigit():
            j += 1
        ident = mangled[j:j + int(mangled[i:j])]
        if ident.startswith("k_"):
            return ident
        i = j + len(ident)
    return mangled


def _kernel_metadata(notes):
    """{kernel: {key: value}} from the AMDGPU metadata note (llvm-readelf --notes)."""
    body = notes.split("amdhsa.kernels:", 1)[1]
    body = re.split(r"^amdhsa\.target:", body, flags=re.M)[0]
    out = {}
    for entry in re.split(r"^  - ", body, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*\.(vgpr_count|agpr_count|private_segment_fixed_size|name):\s+(\S+)", "    " + entry, re.M))
        if "name" in kv:
            out[kv["name"]] = kv
    return out


def _mfma_by_symbol(disasm):
    """{symbol: [MFMA opcodes]} from llvm-objdump -d."""
    out, cur = {}, None
    for line in disasm.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = m.group(1)
            out.setdefault(cur, [])
            continue
        m = re.match(r"^\s*(v_mfma_\w+)", line)
        if m and cur is not None:
            out[cur].append(m.group(1))
    return out


def code_objects(lib_path, tmp_path):
    """{(code object, kernel): vgpr/agpr count, scratch, MFMA opcodes} over every gfx950 code object in the library."""
    assert os.path.exists(lib_path), lib_path
    work = tmp_path / os.path.basename(os.path.dirname(lib_path))
    work.mkdir()
    so = work / "lib.so"
    shutil.copy(lib_path, so)           # --offloading writes the extracted bundles next to its input
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(so)], check=True, capture_output=True, cwd=work)
    cos = sorted(p for p in work.iterdir() if p.name.endswith("gfx950"))
    assert cos, "no gfx950 code object in " + lib_path
    kernels = {}
    for co in cos:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        if "amdhsa.kernels:" not in notes:
            continue
        disasm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
        mfma = _mfma_by_symbol(disasm)
        for name, kv in _kernel_metadata(notes).items():
            assert name in mfma, (co.name, name)
            # anonymous-namespace kernels of different translation units may share a name: key by code object too
            kernels[(co.name, name)] = dict(vgpr=int(kv["vgpr_count"]), agpr=int(kv["agpr_count"]),
                                 scratch=int(kv["private_segment_fixed_size"]), mfma=mfma[name])
    for (_, name), kv in kernels.items():
        kv["base"] = _base_name(name)
    return kernels


_PRODUCT = []


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    # built and extracted once per session: the per-entry-point modules (test_*_code_objects.py) import this fixture
    if not _PRODUCT:
        import __graft_entry__ as g
        g.build()
        from nrc_amd import rc_ext
        _PRODUCT.append(code_objects(rc_ext.library_path(), tmp_path_factory.mktemp("product")))
    return _PRODUCT[0]


@pytest.fixture(scope="module")
def variant_f32(tmp_path_factory):
    # the library tests/test_gpu_f32_build.py runs the GPU suite against; a failed build fails the test
    r = subprocess.run(["make", "-C", CSRC, "-j16", "variant-f32"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return code_objects(os.path.join(ROOT, "build", "f32", "librc_hip.so"), tmp_path_factory.mktemp("f32"))


def test_parser_sees_every_kernel(product):
    """A parsing failure must not pass as 'no split kernel found': the known split kernels are there, with MFMAs."""
    bases = {v["base"] for v in product.values()}
    assert SPLIT_KERNELS <= bases, sorted(bases)
    assert len(product) >= 20, len(product)
    assert sum(len(v["mfma"]) for v in product.values()) > 1000


def test_every_bf16_mfma_kernel_owns_its_simd(product):
    split = {k: v for k, v in product.items() if any("bf16" in op for op in v["mfma"])}
    assert SPLIT_KERNELS <= {v["base"] for v in split.values()}, sorted(v["base"] for v in split.values())
    bad = {f'{v["base"]} {k[1]} ({k[0]})': (v["vgpr"], v["scratch"], sum("bf16" in op for op in v["mfma"]))
           for k, v in split.items() if v["vgpr"] != 512 or v["scratch"] != 0}
    assert not bad, ("kernels with bf16 MFMAs that do not allocate the whole register file of their SIMD "
                     "(kernel: vgpr_count, scratch bytes, bf16 MFMAs)", bad)


def test_fp32_variant_has_no_bf16_mfma(variant_f32):
    assert "k_cache_fused_team" in {v["base"] for v in variant_f32.values()}
    assert sum(len(v["mfma"]) for v in variant_f32.values()) > 1000
    bf16 = {f'{v["base"]} {k[1]} ({k[0]})': sum("bf16" in op for op in v["mfma"]) for k, v in variant_f32.items()
            if any("bf16" in op for op in v["mfma"])}
    assert not bf16, bf16


# The training entry points' code, one row per tests/test_<entry>_code_objects.py: its exports (in the library and in
# rc_ext.EXPORTS), its exact kernel set, the kernels with no MFMA at all and the MFMA opcode a kernel must contain.  Every
# kernel of a row uses no scratch and no bf16 MFMA: the split-bf16 form is fenced to the forward shaders, the backwards
# run in fp32.
TRAINING = {
    "data": (("rc_shader_grad_size", "rc_shader_grad_layout", "rc_data_backward"),
             {"k_data_loss_bwd", "k_gemm", "k_sum_parts", "k_stage_feature", "k_shader_glue_fwd", "k_shader_out_bwd",
              "k_shader_glue_bwd", "k_split_feature"},
             set(), {"k_gemm": "v_mfma_f32_32x32x2_f32"}),
    "geometry": (("rc_geometry_backward", "rc_density_regularizer"),
                 {"k_geometry_loss_bwd", "k_stage_hidden", "k_grid_l2_bwd", "k_grid_l2_reduce"}, set(), {}),
    "light": (("rc_light_grad_size", "rc_light_grad_layout", "rc_light_sampling_backward", "rc_light_regularizer"),
              {"k_light_sampling_loss_bwd", "k_gemm", "k_sum_parts", "k_grid_l2_bwd", "k_grid_l2_reduce"}, set(), {}),
    "material": (("rc_material_grad_size", "rc_material_grad_layout", "rc_material_smoothness_backward",
                  "rc_material_regularizer"),
                 {"k_material_smoothness_points", "k_material_smoothness_bwd", "k_material_smoothness_reduce",
                  "k_grid_l2_bwd", "k_grid_l2_reduce"},
                 {"k_material_smoothness_bwd", "k_material_smoothness_reduce"}, {}),
    "material_data": (("rc_material_data_backward",), {"k_material_data_bwd", "k_material_data_head_bwd"},
                      {"k_material_data_bwd", "k_material_data_head_bwd"}, {}),
    # streaming element-wise code with 16-byte loads and stores
    "optimizer": (("rc_adam_update", "rc_load_params_flat"), {"k_adam", "k_adam_sumsq", "k_adam_norm"},
                  {"k_adam", "k_adam_sumsq", "k_adam_norm"}, {}),
}


def check_training_exports(entry):
    import ctypes

    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in TRAINING[entry][0]:
        assert hasattr(lib, name), name
        assert name in rc_ext.EXPORTS, name


def check_training_kernels(product, entry):
    _, kernels, no_mfma, has_op = TRAINING[entry]
    ks = {v["base"]: v for v in product.values() if v["base"] in kernels}
    assert set(ks) == kernels, sorted(set(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not any("bf16" in op for op in v["mfma"]), name
        if name in no_mfma:
            assert not v["mfma"], (name, v["mfma"])
    for name, op in has_op.items():
        assert op in ks[name]["mfma"], (name, op)
