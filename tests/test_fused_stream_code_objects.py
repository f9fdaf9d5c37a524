"""The length of the fused kernel's weight stream, read from the gfx950 code object (no GPU needed).

k_cache_fused<true> pulls its stream through the LDS ring in chunks of 64 fragments: one workgroup barrier per chunk and
four 1-KiB LDS-DMA pieces per chunk and wave, all of them on the ray's chain.  With the output rows packed as tables
(rc_pack_host.h pack_dot_rows, kRcFusedRows) the stream is shorter than the fragment form's 3452 fragments = 54 chunks,
so the split build's kernel must hold exactly what the fragment count `hostcheck --rows` prints implies -- ceil(NF / 64)
`s_barrier` and ceil(NF / 16) `global_load_lds_dwordx4` (a wave issues its 1-KiB piece of every group of four pieces that
starts inside the stream, rc_dev_mlp.h ws_issue: 4 ceil(NF / 64) unless the last chunk ends early) -- both below the
fragment form's 54 and 216, and the same MFMAs as before: the table form changes where the output rows' weights lie, not a product.
"""
import os
import re
import subprocess

import pytest

from test_code_objects import CSRC, LLVM, product  # noqa: F401  (fixture)
from test_fused_lookup_code_objects import kernel_streams

PARENT_BARRIERS, PARENT_PIECES = 54, 216
BF16_32, BF16_16, F32 = 1305, 14, 496


@pytest.fixture(scope="module")
def grad_kernel(product, tmp_path_factory):  # noqa: F811
    from nrc_amd import rc_ext

    streams = kernel_streams(rc_ext.library_path(), tmp_path_factory.mktemp("fused_stream"))
    want = [k for k, v in product.items() if v["base"] == "k_cache_fused" and "k_cache_fusedILb1ELb0ELb0E" in k[1]]
    assert len(want) == 1, want                  # GRAD, neither FRONT nor EXPORT
    return streams[want[0]]


@pytest.fixture(scope="module")
def fragments():
    r = subprocess.run(["make", "-C", CSRC, "hostcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(CSRC, "hostcheck"), "--rows"], capture_output=True, text=True)      # the offsets only
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^layout rows=(\d) NF_FUSED=(\d+)$", r.stdout, re.M)
    assert m, r.stdout
    return int(m.group(1)), int(m.group(2))


def test_barriers_and_pieces_are_what_the_fragment_count_implies(grad_kernel, fragments):
    rows, nf = fragments
    chunks = -(-nf // 64)
    barriers = sum(ins.startswith("s_barrier") for ins in grad_kernel)
    pieces = sum(ins.startswith("global_load_lds_dwordx4") for ins in grad_kernel)
    print(f"NF_FUSED {nf}, chunks {chunks}, s_barrier {barriers}, global_load_lds_dwordx4 {pieces}")
    assert rows == 1
    assert barriers == chunks and pieces == -(-nf // 16) and 4 * chunks - 3 <= pieces <= 4 * chunks, (barriers, pieces, chunks)
    assert barriers < PARENT_BARRIERS and pieces < PARENT_PIECES


def test_mfma_counts_are_unchanged(grad_kernel):
    ops = [ins.split()[0] for ins in grad_kernel if ins.startswith("v_mfma_")]
    count = {op: ops.count(op) for op in set(ops)}
    assert count.get("v_mfma_f32_32x32x16_bf16") == BF16_32, count
    assert count.get("v_mfma_f32_16x16x32_bf16") == BF16_16, count
    assert sum(n for op, n in count.items() if "bf16" not in op) == F32, count
