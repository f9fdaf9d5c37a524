"""tests/gemm_ref.py on the CPU: the fp64 reference of RcGemmArgs against literal loops, the rounding bound against an fp32
and a bf16-operand emulation of the kernels' sum, the mutation guards (each wrong reading of the contract changes the
reference on every case it applies to), the table of production descriptors against the host files' call sites, and the
driver's cross-compile.  tests/test_gpu_gemm.py runs the same cases on the device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_ref as G

CUS = 256                                    # an MI355X; the cases' K of the 128 x 128 instantiation follows it


@pytest.fixture(scope="module")
def built():
    return G.build_cases(CUS)


def _logical_changed(c, bufs, mutation):
    want, got = G.reference(c, bufs), G.reference(c, bufs, mutation)
    return any(not np.array_equal(G.c_view(c, want["C"], z).view(np.uint32), G.c_view(c, got["C"], z).view(np.uint32))
               for z in range(c["kparts"]))


def test_reference_matches_a_triple_loop(built):
    bufs, cases = built
    keys = ["edge/33x33x17", "edge/1x129x5", "edge/129x1x0", "layout/Ann01", "layout/Abc10", "layout/Amc11", "layout/C70.2",
            "layout/beyondK", "epilogue/bias1relu1mask1acc1", "epilogue/bias0relu1mask0acc1"]
    for key in keys:
        c = [c for c in cases if c["name"].startswith(key)][-1]           # the last: the shortest K slices
        name = c["name"]
        assert np.array_equal(G.reference(c, bufs)["C"].view(np.uint32), G.triple_loop(c, bufs).view(np.uint32)), name


def test_exact_family_is_exact_and_canaries_hold(built):
    bufs, cases = built
    for c in cases:
        if c["family"] != "exact":
            continue
        assert G.exact_precondition(c)
        A, B, bias, _ = G.operand_views(c, bufs)
        for v in (A, B) + ((bias,) if bias is not None else ()):
            assert np.array_equal(v * 8, np.round(v * 8)) and np.abs(v).max(initial=0) <= 1       # no canary among them either
        if c["accumulate"]:
            assert not G.is_canary(G.c_view(c, bufs[c["c_buf"]], c["kparts"] - 1)).any()
        else:
            assert G.is_canary(bufs[c["c_buf"]]).all()                     # the old C is never to be read
    c = next(c for c in cases if c["name"] == "edge/33x33x17")
    ref = G.reference(c, bufs)
    assert np.array_equal(ref["parts"][0], G.c_view(c, ref["C"], 0).astype(np.float64))     # fp64 result is an fp32 number
    outside = np.ones(ref["C"].size, bool)
    outside[c["c_off"] + (np.arange(33)[:, None] * c["sci"] + np.arange(33)[None, :] * c["scj"]).ravel()] = False
    assert G.is_canary(ref["C"][outside]).all() and not np.isnan(ref["C"][~outside]).any()


def test_rounding_bound_holds_the_fp32_emulation_and_rejects_bf16(built):
    bufs, cases = built
    rounding = [c for c in cases if c["family"] == "round"]
    assert len(rounding) == 12
    for c in rounding:
        ref, bound = G.reference(c, bufs)["parts"], G.rounding_bound(c, bufs)
        err = np.abs(G.emulate_f32(c, bufs) - ref)
        assert (err <= 0.5 * bound).all(), (c["name"], float((err / bound).max()))
        err16 = np.abs(G.emulate_f32(c, bufs, truncate_bf16=True)[0] - ref[0])
        assert (err16 / bound[0]).max() >= 10.0, (c["name"], float((err16 / bound[0]).max()))


@pytest.mark.parametrize("mutation", G.MUTATIONS)
def test_mutation_changes_every_case_it_applies_to(built, mutation):
    bufs, cases = built
    applies = {"drop_last_k": lambda c: c["K"] >= 1, "bias_jm1": lambda c: c["bias_buf"] >= 0, "mask_ge": lambda c: c["mask_buf"] >= 0,
               "relu_first": lambda c: c["relu"] and c["accumulate"], "b_shift": lambda c: c["K"] >= 1}[mutation]
    n = 0
    for c in cases:
        if c["family"] == "exact" and c["group"] not in ("biglayout", "biglayout5", "big") and applies(c):
            assert _logical_changed(c, bufs, mutation), (mutation, c["name"])
            n += 1
    assert n >= 4, n                                                     # relu_first: the four epilogue cases with both
    if mutation in ("drop_last_k", "bias_jm1", "b_shift"):               # one case each of the large groups
        for key in ("big/4097x1025x19/ragged", "biglayout/Akc10"):
            c = next(c for c in cases if c["name"].startswith(key))
            assert _logical_changed(c, bufs, mutation), (mutation, c["name"])


def test_every_call_site_is_listed():
    """A new dense_* call (or hand-built descriptor) in the five host files fails here until gemm_ref.PRODUCTION restates it."""
    listed = {(f, line) for f, line, _ in G.PRODUCTION}
    assert not listed & G.NOT_CALL_SITES
    assert G.call_sites() == listed | G.NOT_CALL_SITES
    # the lambdas' calls: one entry each; the light head's loops: three layers per line
    assert len(G.PRODUCTION) == 73
    kinds = [d[0] for _, _, d in G.PRODUCTION]
    assert kinds.count("fwd") == 23 and kinds.count("dx") == 25 and kinds.count("wgrad") == 25


def test_cases_cover_the_issue(built):
    bufs, cases = built
    groups = {}
    for c in cases:
        groups.setdefault(c["group"], []).append(c)
    assert len(groups["prod"]) == 23 + 25 + 2 * 25
    assert {(c["M"], c["N"], c["K"]) for c in groups["edge"]} == {(m, n, k) for m, n in G.EDGE_MN for k in G.EDGE_K}
    assert all(c["bias_buf"] >= 0 for c in groups["edge"])
    pairs = G.layout_variants()
    forms = {(k, l, o) for k in G.KINDS for l in (0, 1) for o in (0, 1)}
    assert {a for a, _ in pairs} == forms and {b for _, b in pairs} == forms
    assert {(a[0], b[0]) for a, b in pairs} == {(x, y) for x in G.KINDS for y in G.KINDS}
    assert {c["kslice"] for c in groups["layout"]} == {37, 16, 12, 5}
    assert any(c["scj"] != 1 for c in groups["layout"]) and any(c["mask_buf"] >= 0 and c["smj"] != 1 for c in groups["layout"])
    assert len({(c["bias_buf"] >= 0, c["relu"], c["mask_buf"] >= 0, c["accumulate"]) for c in groups["epilogue"]}) == 16
    for c in groups["epilogue"]:
        if c["mask_buf"] >= 0:
            m = G.operand_views(c, bufs)[3]
            assert {v.tobytes() for v in m.ravel()} == {v.tobytes() for v in G.MASK_VALUES}
    assert {(c["K"], c["kslice"]) for c in groups["biglayout"]} == {(4 * CUS + 3, 4), (4 * CUS + 3, 5)}
    assert len(groups["biglayout"]) == 2 * (len(groups["layout"]) - 1) // 4
    assert all(G.big_instantiation(c, CUS) for c in groups["big"] + groups["biglayout5"])
    assert all(G.big_instantiation(c, CUS) == (c["kslice"] == 4) for c in groups["biglayout"])
    assert sorted((c["K"], G.big_instantiation(c, CUS)) for c in groups["round"]) == sorted(
        (k, b) for k in (27, 96, 129) for b in (False, True) for _ in range(2))
    # every sliced case of the small groups has its slices as launches of their own
    sliced = [c for c in groups["prod"] + groups["layout"] if c["kparts"] > 1 and c["name"] != "layout/beyondK"]
    assert {(c["parent"], c["slice"]) for c in groups["unsliced"]} == {(c["name"], z) for c in sliced for z in range(c["kparts"])}


def test_case_file_round_trip(built, tmp_path):
    bufs, cases = built
    path = tmp_path / "cases.bin"
    G.write_case_file(path, bufs[:40], [])
    head = np.fromfile(path, np.int64, 4)
    assert list(head) == [G.MAGIC_CASES, 40, 0, len(G.FIELDS)]
    table = np.fromfile(path, np.int64, 80, offset=32).reshape(40, 2)
    stored = table[:, 0] >= 0
    assert os.path.getsize(path) == 32 + 640 + 4 * int(table[stored, 1].sum())
    n = int(np.flatnonzero(stored)[3])
    got = np.fromfile(path, np.float32, int(table[n, 1]), offset=32 + 640 + 4 * int(table[n, 0]))
    assert np.array_equal(got.view(np.uint32), bufs[n].view(np.uint32))
    assert all(G.is_canary(bufs[i]).all() for i in np.flatnonzero(~stored))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_driver_cross_compiles():
    r = subprocess.run(["make", "-C", G.CSRC, "-j16", "gemmcheck", "ARCH=gfx950"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(G.ROOT, "build", "gemmcheck"))
