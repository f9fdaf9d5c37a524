"""The fused cache kernel's table loads, read from the gfx950 code objects (no GPU needed).

k_cache_fused runs one wave per SIMD with in-order issue: a `s_waitcnt vmcnt` between the loads of two grid levels is a
whole memory round trip on the ray's chain.  The lookups of proposal levels 0 and 1 are written to put all their loads in
flight first (6 cell-table loads of 16 bytes for the 3 dense levels, 8 corner loads for each hashed level) and to combine
afterwards.  Only compiler behaviour holds that, so it is checked on what the compiler made, for every instantiation:

  * the instruction stream is cut at the MFMAs: level 0's lookup lies before the first MFMA, level 1's in the first gap
    between two MFMAs that holds a table load (behind the level-0 density MLP);
  * in each segment the longest run of global loads (LDS-DMA `global_load_lds` aside) with no `s_waitcnt` that carries a
    vmcnt field between them is >= 30 (6 + 8 * 3) for level 0, >= 38 (6 + 8 * 4) for level 1;
  * no vector memory load follows the kernel's last global store (a load there also waits for every output store to be
    acknowledged).

The parent of this test (level kinds read at run time from RcGridLevel::dense) FAILS the run-length check: the hashed arm of
every level opened with `s_waitcnt vmcnt(0)` and the longest run was 10 in both lookups, in all six instantiations.
"""
import os
import re
import shutil
import subprocess

import pytest

from test_code_objects import LLVM, product  # noqa: F401  (fixture)

KERNEL = "k_cache_fused"
MIN_RUN = {"level 0": 6 + 8 * 3, "level 1": 6 + 8 * 4}
_LOAD = re.compile(r"^(global|flat|buffer|scratch)_load_")


def kernel_streams(lib_path, work):
    """{(code object, symbol): [instruction text]} for every function symbol of every gfx950 code object in the library."""
    so = work / "lib.so"
    shutil.copy(lib_path, so)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(so)], check=True, capture_output=True, cwd=work)
    out = {}
    for co in sorted(p for p in work.iterdir() if p.name.endswith("gfx950")):
        disasm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in disasm.splitlines():
            m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
            if m:
                cur = out.setdefault((co.name, m.group(1)), [])
                continue
            if cur is not None and line.startswith(("\t", " ")):
                text = line.split("//")[0].strip()
                if text:
                    cur.append(text)
    return out


def is_table_load(ins):
    return ins.startswith("global_load_") and not ins.startswith("global_load_lds")


def waits_for_loads(ins):
    # a decoded s_waitcnt names the counters it waits on; one the disassembler left as a number counts as a wait too
    return ins.startswith("s_waitcnt") and not ins.startswith("s_waitcnt_") and ("vmcnt" in ins or "cnt(" not in ins)


def longest_load_run(seg):
    """Most table loads issued back to back in `seg` with no wait on the vector-memory counter between them."""
    best = run = 0
    for ins in seg:
        if is_table_load(ins):
            run += 1
            best = max(best, run)
        elif waits_for_loads(ins):
            run = 0
    return best


def lookup_segments(stream):
    """The instructions of the level-0 and the level-1 lookup: the stream cut at its MFMAs."""
    at = [i for i, ins in enumerate(stream) if ins.startswith("v_mfma_")]
    assert len(at) > 100, len(at)
    seg0 = stream[:at[0]]
    for lo, hi in zip(at, at[1:]):
        if any(is_table_load(ins) for ins in stream[lo + 1:hi]):
            return {"level 0": seg0, "level 1": stream[lo + 1:hi]}
    raise AssertionError("no table load between two MFMAs")


def load_runs_by_gap(stream):
    """Report helper for any MFMA kernel: longest load run of every MFMA-free stretch that holds a table load."""
    at = [-1] + [i for i, ins in enumerate(stream) if ins.startswith("v_mfma_")] + [len(stream)]
    return [(longest_load_run(stream[lo + 1:hi]), sum(map(is_table_load, stream[lo + 1:hi])))
            for lo, hi in zip(at, at[1:]) if any(is_table_load(ins) for ins in stream[lo + 1:hi])]


@pytest.fixture(scope="module")
def fused_streams(product, tmp_path_factory):  # noqa: F811
    from nrc_amd import rc_ext

    streams = kernel_streams(rc_ext.library_path(), tmp_path_factory.mktemp("fused_lookup"))
    want = {k for k, v in product.items() if v["base"] == KERNEL}
    assert len(want) >= 6, sorted(want)          # GRAD x {plain, FRONT, EXPORT}
    assert want <= set(streams), sorted(want - set(streams))
    return {k: streams[k] for k in sorted(want)}


def test_lookup_loads_of_levels_0_and_1_go_out_in_one_batch(fused_streams):
    runs = {k[1]: {name: longest_load_run(seg) for name, seg in lookup_segments(s).items()} for k, s in fused_streams.items()}
    print(runs)
    bad = {k: r for k, r in runs.items() if any(r[name] < MIN_RUN[name] for name in MIN_RUN)}
    assert not bad, ("longest run of table loads without a vmcnt wait in the lookup of (level 0, level 1); wanted "
                     f"{MIN_RUN}", bad)


def test_no_vector_load_behind_the_last_store(fused_streams):
    bad = {}
    for k, s in fused_streams.items():
        stores = [i for i, ins in enumerate(s) if ins.startswith("global_store_")]
        assert stores, k
        late = [ins for ins in s[stores[-1] + 1:] if _LOAD.match(ins)]
        if late:
            bad[k[1]] = late
    assert not bad, bad
