"""k_gemm (csrc/rc_data.hip) and k_gemm_tile (csrc/rc_envmap_bwd.hip) on the device, directly against RcGemmArgs' contract:
the cases of tests/gemm_ref.py (every production descriptor of the five host files, tile edges and K tails, operand layouts,
the 16 epilogues, both tile instantiations) through tests/gemm_check.hip, which links the library's own objects.  The
driver runs once, as a child process under a time limit; the tests below only read its result file.

Exact family: operands are multiples of 1/8, every sum is exact in fp32 in any order, so C, every K-slice partial and the
sums of k_sum_parts equal the fp64 reference bit for bit.  Rounding family: uniform operands, held to
2 (K + 2) 2^-24 (sum |a||b| + |bias| + |old C|) per element.  Every float of a result buffer that is not a logical element
is a canary NaN and has to come back bitwise unchanged."""
import os
import subprocess
import time

import numpy as np
import pytest

import gemm_ref as G

pytestmark = pytest.mark.gpu
EXE = os.path.join(G.ROOT, "build", "gemmcheck")


class Run:
    def __init__(self, bufs, cases, res):
        self.bufs, self.cases, self.res = bufs, cases, res
        self._ref = {}

    def ref(self, n):
        if n not in self._ref:
            self._ref[n] = G.reference(self.cases[n], self.bufs)
        return self._ref[n]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    t0 = time.time()
    r = subprocess.run(["make", "-C", G.CSRC, "-j16", "gemmcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE, "--info"], capture_output=True, text=True, timeout=60)          # no case runs: the CU count
    assert r.returncode == 0 and r.stdout.startswith("cus "), r.stdout + r.stderr
    cus = int(r.stdout.split()[1])
    bufs, cases = G.build_cases(cus)
    d = tmp_path_factory.mktemp("gemmcheck")
    G.write_case_file(d / "cases.bin", bufs, cases)
    t1 = time.time()
    r = subprocess.run([EXE, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gemmcheck ok" in r.stdout, r.stdout + r.stderr
    res = G.Results(d / "results.bin", bufs, cases)
    assert res.cus == cus
    print(f"\ngemmcheck: {len(cases)} cases, {cus} CUs, build + cases {t1 - t0:.1f} s, driver {time.time() - t1:.1f} s "
          f"(its own clock {res.wall_us * 1e-6:.2f} s)")
    return Run(bufs, cases, res)


def _same(x, y):
    return np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _logical(c, size):
    """Boolean map of the C buffer's logical elements (all parts)."""
    m = np.zeros(size, bool)
    at = (np.arange(c["M"], dtype=np.int64)[:, None] * c["sci"] + np.arange(c["N"], dtype=np.int64)[None, :] * c["scj"]).ravel()
    for z in range(c["kparts"]):
        m[c["c_off"] + z * c["spart"] + at] = True
    return m


def test_exact_family_equals_fp64_bit_for_bit(run):
    bad = []
    for n, c in enumerate(run.cases):
        if c["family"] != "exact":
            continue
        assert G.exact_precondition(c)
        ref = run.ref(n)
        for which, kernel in enumerate(("k_gemm", "k_gemm_tile")):
            if not _same(run.res.C(n, which), ref["C"]):
                bad.append((kernel, c["name"], "C"))
            if ref["G"] is not None and not _same(run.res.G(n, which), ref["G"]):
                bad.append((kernel, c["name"], "sums"))
    assert not bad, (len(bad), bad[:20])


def test_rounding_family_within_the_bound(run):
    worst = {}
    for n, c in enumerate(run.cases):
        if c["family"] != "round":
            continue
        ref, bound = run.ref(n)["parts"], G.rounding_bound(c, run.bufs)
        for which, kernel in enumerate(("k_gemm", "k_gemm_tile")):
            got = run.res.C(n, which)
            ratio = max(float((np.abs(G.c_view(c, got, z).astype(np.float64) - ref[z]) / bound[z]).max()) for z in range(c["kparts"]))
            worst[(c["name"], kernel)] = ratio
            print(f"{c['name']:32s} {kernel:12s} error / bound = {ratio:.4f}")
    assert len(worst) == 24
    assert all(r <= 1.0 for r in worst.values()), {k: r for k, r in worst.items() if r > 1.0}


def test_canaries_unchanged_and_no_nan(run):
    bad = []
    for n, c in enumerate(run.cases):
        for which in range(2):
            got = run.res.C(n, which)
            m = _logical(c, got.size)
            if not G.is_canary(got[~m]).all():
                bad.append((which, c["name"], "canary of C"))
            if np.isnan(got[m]).any():
                bad.append((which, c["name"], "NaN in C"))
            g = run.res.G(n, which)
            if g is not None:
                lo, hi = c["g_off"], c["g_off"] + c["spart"]
                if not (G.is_canary(g[:lo]).all() and G.is_canary(g[hi:]).all()):
                    bad.append((which, c["name"], "canary of the sums"))
                if np.isnan(g[lo:hi]).any():
                    bad.append((which, c["name"], "NaN in the sums"))
    assert not bad, (len(bad), bad[:20])


def test_both_kernels_agree_bit_for_bit(run):
    """rc_envmap_bwd.hip: "the sum over k runs in k_gemm's order"."""
    bad = []
    for n, c in enumerate(run.cases):
        if not _same(run.res.C(n, 0), run.res.C(n, 1)):
            bad.append((c["name"], "C"))
        if c["g_buf"] >= 0 and not _same(run.res.G(n, 0), run.res.G(n, 1)):
            bad.append((c["name"], "sums"))
    assert not bad, (len(bad), bad[:20])


def test_partials_equal_unsliced_launches(run):
    index = {c["name"]: n for n, c in enumerate(run.cases)}
    bad, seen = [], 0
    for n, d in enumerate(run.cases):
        if d["group"] != "unsliced":
            continue
        p = index[d["parent"]]
        for which in range(2):
            part = G.c_view(run.cases[p], run.res.C(p, which), d["slice"])
            if not _same(np.ascontiguousarray(part), np.ascontiguousarray(G.c_view(d, run.res.C(n, which), 0))):
                bad.append((which, d["name"]))
        seen += 1
    sliced = [c for c in run.cases if c["group"] in ("prod", "layout") and c["kparts"] > 1 and c["name"] != "layout/beyondK"]
    assert seen == sum(c["kparts"] for c in sliced) > 0 and not bad, (seen, len(bad), bad[:20])


def test_coverage_of_panel_modes_and_instantiations(run):
    """panel_mode and the big * kparts >= CUs predicate of rc_launch_gemm_tile restated from the reported alignments and CU
    count: the cases reached all four load modes for A and for B on both instantiations, each with ragged M, N and K."""
    reached = set()
    for n, c in enumerate(run.cases):
        al = run.res.align[n, 1]
        big = G.big_instantiation(c, run.res.cus)
        tile = 128 if big else 64
        last = G.slice_bounds(c, c["kparts"] - 1)
        ragged = c["M"] % tile and c["N"] % tile and (last[1] - last[0]) % 16 and c["K"] > 0
        if not ragged:
            continue
        reached.add((big, "A", G.panel_mode(al[0], c["sai"], c["sak"], c["kslice"])))
        reached.add((big, "B", G.panel_mode(al[1], c["sbj"], c["sbk"], c["kslice"])))
    assert reached == {(big, op, mode) for big in (False, True) for op in "AB" for mode in range(4)}, sorted(reached)
    # both launchers saw the same operands, and every production descriptor ran on both
    assert np.array_equal(run.res.align[:, 0] >= 0, run.res.align[:, 1] >= 0)
    assert sum(c["group"] == "prod" for c in run.cases) == sum(2 if d[0] == "wgrad" else 1 for _, _, d in G.PRODUCTION)
    assert (run.res.align[:, :, :3] >= 0).all()
