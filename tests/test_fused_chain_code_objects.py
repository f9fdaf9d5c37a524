"""Scalar round trips in the fused cache kernel's tail, read from the gfx950 code objects (no GPU needed).

k_cache_fused runs one wave per SIMD with in-order issue, so every scalar round trip between two output stores is on the ray's
critical path.  For all six instantiations of the product library
(GRAD x {plain, FRONT, EXPORT}):

  * between the first and the last `global_store_` of the kernel at most two `s_load_` occur: the output pointers of the
    compositing tail (and the workspace pointers of FRONT / EXPORT) are fetched as one batch in front of the first store;
  * the kernel keeps `.vgpr_count 512` and zero scratch (read as tests/test_code_objects.py reads them).

The parent of this test FAILS the first point with 15 / 14 (plain, GRAD / no GRAD), 23 / 22 (EXPORT) and 2 / 3 (FRONT)
`s_load_` between the first and the last store.

The table loads of the three lookups keep the `v[lo:hi], off` address form.  The scalar-base form with 32-bit byte
offsets (137 `v_lshl_add_u64` fewer in k_cache_fused<true>) was built and measured with this change and was SLOWER in every
alternated round (profiles/r10_chain_addressing_ab.txt), so no check asks for it.
"""
import pytest

from test_code_objects import product  # noqa: F401  (fixture)
from test_fused_lookup_code_objects import KERNEL, kernel_streams


@pytest.fixture(scope="module")
def fused_streams(product, tmp_path_factory):  # noqa: F811
    from nrc_amd import rc_ext

    streams = kernel_streams(rc_ext.library_path(), tmp_path_factory.mktemp("fused_chain"))
    want = {k for k, v in product.items() if v["base"] == KERNEL}
    assert len(want) >= 6, sorted(want)          # GRAD x {plain, FRONT, EXPORT}
    assert want <= set(streams), sorted(want - set(streams))
    return {k: streams[k] for k in sorted(want)}


def test_tail_fetches_its_pointers_in_front_of_the_first_store(fused_streams):
    got = {}
    for k, s in fused_streams.items():
        stores = [i for i, ins in enumerate(s) if ins.startswith("global_store_")]
        assert len(stores) >= 2, k
        got[k[1]] = sum(ins.startswith("s_load_") for ins in s[stores[0]:stores[-1]])
    print(got)
    assert all(n <= 2 for n in got.values()), got


def test_kernel_keeps_its_registers_and_no_scratch(product):  # noqa: F811
    ks = {k: v for k, v in product.items() if v["base"] == KERNEL}
    assert len(ks) >= 6
    bad = {k[1]: (v["vgpr"], v["scratch"]) for k, v in ks.items() if v["vgpr"] != 512 or v["scratch"] != 0}
    assert not bad, bad
