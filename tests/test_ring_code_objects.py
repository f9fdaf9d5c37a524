"""The weight ring's pieces and the directional-encoding constants, read from the gfx950 code objects (no GPU needed).

k_cache_fused and k_cache_shader run one wave per SIMD with in-order issue, so every instruction between the MFMAs of
the shader is on the ray's chain.  Two things are written to stay off it and only compiler behaviour holds them, so
they are checked on what the compiler made, for every instantiation of the two kernels:

  * the shader reads nothing from global memory but its weight stream (LDS-DMA, `global_load_lds_*`): between the first
    and the last v_mfma_f32_32x32x16_bf16 there is no other `global_load_*`.  The IDE polynomial coefficients are
    compile-time constants (rc_ide_coef.h); as a table in global memory they were 121 per-lane loads of a wave-uniform
    address and as many waits.
  * a piece of the ring costs its load and a two-instruction address setup (rc_dev_mlp.h ws_issue_piece: one 32-bit
    vector add for the source, one scalar move for M0): between two `global_load_lds_dwordx4` with no workgroup barrier
    between them -- the pieces of one seam -- there is no 64-bit vector add (`v_lshl_add_u64`, `v_add_co` /
    `v_addc_co`) and no `v_readfirstlane_b32`.
  * .vgpr_count 512, no scratch, and a static LDS segment within the 160 KiB of a CU.
"""
import re
import subprocess

import pytest

from test_code_objects import LLVM, product  # noqa: F401  (fixture)
from test_fused_lookup_code_objects import kernel_streams

KERNELS = ("k_cache_fused", "k_cache_shader")
BF16 = "v_mfma_f32_32x32x16_bf16"
LDS_BYTES = 163840
_ADDRESS = re.compile(r"^(v_lshl_add_u64|v_readfirstlane_b32|v_add_co_|v_addc_co_)")


def is_piece(ins):
    return ins.startswith("global_load_lds_dwordx4")


@pytest.fixture(scope="module")
def ring_streams(product, tmp_path_factory):  # noqa: F811
    from nrc_amd import rc_ext

    work = tmp_path_factory.mktemp("ring")
    streams = kernel_streams(rc_ext.library_path(), work)
    want = {k for k, v in product.items() if v["base"] in KERNELS}
    assert len(want) >= 7, sorted(want)          # k_cache_fused: GRAD x {plain, FRONT, EXPORT}; k_cache_shader
    assert want <= set(streams), sorted(want - set(streams))
    lds = {}
    for co in sorted(p for p in work.iterdir() if p.name.endswith("gfx950")):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        if "amdhsa.kernels:" not in notes:
            continue
        for entry in re.split(r"^  - ", notes.split("amdhsa.kernels:", 1)[1], flags=re.M)[1:]:
            kv = dict(re.findall(r"^\s*\.(group_segment_fixed_size|name):\s+(\S+)", "    " + entry, re.M))
            if "name" in kv:
                lds[(co.name, kv["name"])] = int(kv["group_segment_fixed_size"])
    return {k: dict(stream=streams[k], lds=lds[k], **product[k]) for k in sorted(want)}


def test_the_shader_loads_nothing_but_its_weight_stream(ring_streams):
    bad, seen = {}, 0
    for k, v in ring_streams.items():
        s = v["stream"]
        at = [i for i, ins in enumerate(s) if ins.startswith(BF16)]
        if not at:                               # FRONT ends in front of the shader
            continue
        seen += 1
        loads = [ins for ins in s[at[0]:at[-1] + 1] if ins.startswith("global_load_") and not ins.startswith("global_load_lds")]
        if loads:
            bad[k[1]] = (len(loads), loads[:4])
    assert seen >= 5, seen                       # k_cache_fused GRAD x {plain, EXPORT}, k_cache_shader
    assert not bad, ("global loads between the first and the last bf16 MFMA (count, first four)", bad)


def test_a_piece_of_the_ring_needs_no_vector_address_arithmetic(ring_streams):
    bad, pieces = {}, 0
    for k, v in ring_streams.items():
        s = v["stream"]
        at = [i for i, ins in enumerate(s) if is_piece(ins)]
        assert len(at) >= 16, (k[1], len(at))     # at least a few chunks: FRONT without the backward has 32
        pieces += len(at)
        hits = []
        for lo, hi in zip(at, at[1:]):
            seg = s[lo + 1:hi]
            if any(ins.startswith("s_barrier") for ins in seg):
                continue                         # pieces of two seams: whatever the kernel does between them
            hits += [ins for ins in seg if _ADDRESS.match(ins)]
        if hits:
            bad[k[1]] = (len(hits), hits[:4])
    print("pieces", pieces)
    assert not bad, ("address instructions between the pieces of one seam (count, first four)", bad)


def test_registers_scratch_and_lds(ring_streams):
    bad = {k[1]: (v["vgpr"], v["scratch"], v["lds"]) for k, v in ring_streams.items()
           if v["vgpr"] != 512 or v["scratch"] != 0 or v["lds"] > LDS_BYTES}
    assert not bad, ("(vgpr_count, scratch bytes, static LDS bytes)", bad)
