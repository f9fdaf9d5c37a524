"""The fused cache kernel's scalar loads, read from the gfx950 code objects (no GPU needed).

k_cache_fused runs one wave per SIMD with in-order issue: a scalar load that is waited for right behind its issue is a
scalar-cache round trip on the ray's chain.  The kernel reads the scalars of each phase from a compact per-phase record
of its arguments (rc_fused_common.h: RcLookupRec, RcResampleRec, RcShadeRec), a few wide `s_load`s issued one phase ahead
and named by one empty asm behind the work that covers them.  Only compiler behaviour holds that, so it is checked on
what the compiler made, for all six instantiations of the product library (GRAD x {plain, FRONT, EXPORT}):

  * a lookup's table loads -- the last 30 (6 + 8 * 3), 38 (6 + 8 * 4) and 64 (two rounds of 4 * 8) vector loads in front
    of the density MLP of level 0, 1 and 2; what precedes them in those stretches are the ray record and the jitter value
    -- have no `s_load_` between the first and the last of them;
  * the scalar wait groups (an `s_waitcnt` with an lgkmcnt field that closes at least one `s_load_`) are fewer than in the
    parent's library and within the ceiling this change reached:

        instantiation     parent   ceiling        `s_load_` parent -> now
        plain GRAD          39        6                 75 -> 35
        plain               40        6                 74 -> 36
        EXPORT GRAD         40        6                 76 -> 36
        EXPORT              41        6                 75 -> 37
        FRONT GRAD          39        8                 76 -> 38
        FRONT               33        9                 73 -> 38

    (FRONT keeps the power-ladder scalars of its resampler where they were);
  * `.vgpr_count` is 512 and scratch is 0.

The parent of this test FAILS the first point with 4, 9 and 8 (GRAD: 10) `s_load_` inside the lookups of levels 0, 1 and 2
in every instantiation, and the second by its own counts.
"""
import re

import pytest

from test_code_objects import product  # noqa: F401  (fixture)
from test_fused_lookup_code_objects import KERNEL, is_table_load, kernel_streams

LOOKUP_LOADS = (6 + 8 * 3, 6 + 8 * 4, 2 * 4 * 8)
# (GRAD, FRONT, EXPORT) -> (scalar wait groups of the parent's library, ceiling)
WAIT_GROUPS = {(1, 0, 0): (39, 6), (0, 0, 0): (40, 6), (1, 0, 1): (40, 6), (0, 0, 1): (41, 6), (1, 1, 0): (39, 8), (0, 1, 0): (33, 9)}


def instantiation(symbol):
    m = re.search(r"k_cache_fusedILb([01])ELb([01])ELb([01])E", symbol)
    assert m, symbol
    return tuple(int(x) for x in m.groups())


def scalar_wait_groups(stream):
    pending = groups = 0
    for ins in stream:
        if ins.startswith("s_load_"):
            pending += 1
        elif ins.startswith("s_waitcnt") and not ins.startswith("s_waitcnt_") and ("lgkmcnt" in ins or "cnt(" not in ins):
            groups += pending > 0
            pending = 0
    return groups


def lookup_stretches(stream):
    """The instructions from the first to the last table load of the three lookups: the stream cut at its MFMAs, the
    first three MFMA-free stretches that hold at least a lookup's loads, the last LOOKUP_LOADS[i] loads of each."""
    at = [-1] + [i for i, ins in enumerate(stream) if ins.startswith("v_mfma_")] + [len(stream)]
    out = []
    for lo, hi in zip(at, at[1:]):
        idx = [i for i in range(lo + 1, hi) if is_table_load(stream[i])]
        if len(out) < 3 and len(idx) >= LOOKUP_LOADS[len(out)]:
            out.append(stream[idx[-LOOKUP_LOADS[len(out)]]:idx[-1] + 1])
    assert len(out) == 3, len(out)
    return out


@pytest.fixture(scope="module")
def fused_streams(product, tmp_path_factory):  # noqa: F811
    from nrc_amd import rc_ext

    streams = kernel_streams(rc_ext.library_path(), tmp_path_factory.mktemp("fused_scalar_batches"))
    want = {k for k, v in product.items() if v["base"] == KERNEL}
    assert len(want) >= 6, sorted(want)          # GRAD x {plain, FRONT, EXPORT}
    assert want <= set(streams), sorted(want - set(streams))
    got = {instantiation(k[1]): streams[k] for k in sorted(want)}
    assert set(got) == set(WAIT_GROUPS), sorted(got)
    return got


def test_no_scalar_load_between_the_table_loads_of_a_lookup(fused_streams):
    got = {k: [sum(ins.startswith("s_load_") for ins in seg) for seg in lookup_stretches(s)] for k, s in fused_streams.items()}
    print(got)
    assert all(n == [0, 0, 0] for n in got.values()), got


def test_fewer_scalar_wait_groups_than_the_parent(fused_streams):
    got = {k: scalar_wait_groups(s) for k, s in fused_streams.items()}
    print(got, {k: sum(ins.startswith("s_load_") for ins in s) for k, s in fused_streams.items()})
    bad = {k: n for k, n in got.items() if not (n < WAIT_GROUPS[k][0] and n <= WAIT_GROUPS[k][1])}
    assert not bad, ("(GRAD, FRONT, EXPORT): scalar wait groups; (parent, ceiling) are", WAIT_GROUPS, bad)


def test_kernel_keeps_its_registers_and_no_scratch(product):  # noqa: F811
    ks = {k: v for k, v in product.items() if v["base"] == KERNEL}
    assert len(ks) >= 6
    bad = {k[1]: (v["vgpr"], v["scratch"]) for k, v in ks.items() if v["vgpr"] != 512 or v["scratch"] != 0}
    assert not bad, bad
