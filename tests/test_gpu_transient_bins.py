"""k_shadow_rays, k_transient_bins, k_transient_slice and k_transient_bins_bwd on the device, directly against their argument
structs' contracts: the cases of tests/transient_bins_ref.py (windows at the ends of tiles and of the histogram, empty
windows, every exposure / threshold pair, integral, fractional, negative and oversized shifts, the direct spill, asymmetric
taps of every code path, the flags and clamps, 1 to 9 rays in blocks of 4, null output pointers) through
tests/transient_check.hip, which links the library's own rc_transient.o, rc_transient_slice.o and rc_transient_bwd.o -- once
from the split-form build and once from the fp32 build (`make transientcheck`).  Each driver runs once, as a child process
under a time limit; the tests below only read its result file.

Tolerances (derivations: tests/transient_bins_ref.py; the CPU side: tests/test_transient_bins_ref.py): every output to a
bound derived from the fp64 reference's own sums of absolute products, with the head constant of the build under test;
softplus_bins to 4 x the allowance measured on the CPU.  Bins outside a sample's window, tiles outside a workgroup's range,
killed samples, dz outside the live tiles and the shadow rays' copies and clamps are held to equality.  Every float of an
output buffer that is not a logical element, every output a launch was not asked for and every row of the backward's
per-sample outputs outside its chunk is a canary NaN and has to come back bitwise unchanged.

Measured on one MI355X (profiles/transient_contract.txt has every figure), worst error / tolerance in the split and the fp32
build: bins 0.47 / 0.47 (out_direct, out_rgb), slices 0.28 / 0.28, backward 0.69 / 0.69 (dz_irr), shadow rays 0.38 / 0.38; no
launch of either build failed a check."""
import os
import subprocess
import time

import numpy as np
import pytest

import transient_bins_ref as M

pytestmark = pytest.mark.gpu
TARGETS = {"split": (os.path.join(M.ROOT, "build", "transientcheck"), M.c_split),
           "f32": (os.path.join(M.ROOT, "build", "f32", "transientcheck"), M.c_f32)}


class Run:
    def __init__(self, cs, got, wall, c):
        self.cs, self.got, self.wall, self.c = cs, got, wall, c
        self._res = {}

    def result(self, li):
        """(failures, error / tolerance per slot) of launch li, computed once."""
        if li not in self._res:
            ref, tol = M.expected(self.cs, li, dev=self.got, c=self.c)
            self._res[li] = M.check(self.cs, li, self.got, ref, tol)
        return self._res[li]

    def logical(self, li, slot):
        L = self.cs.launches[li]
        if L["bufs"][slot] < 0:
            return None
        shape = M.out_shape(L["kernel"], slot, L["ints"])
        return self.got[L["bufs"][slot]][M.GUARD:M.GUARD + int(np.prod(shape))].reshape(shape)


def run_driver(exe, cs, case_file, result_file, timeout=180):
    r = subprocess.run([exe, str(case_file), str(result_file)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "transientcheck ok" in r.stdout, r.stdout + r.stderr
    return M.read_results(result_file, cs)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    t0 = time.time()
    r = subprocess.run(["make", "-C", M.CSRC, "-j16", "transientcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cs = M.build_cases()
    d = tmp_path_factory.mktemp("transientcheck")
    M.write_case_file(d / "cases.bin", cs)
    t1 = time.time()
    out = {}
    for name, (exe, c) in TARGETS.items():                   # a driver that fails ends everything: nothing else is launched
        got, wall = run_driver(exe, cs, d / "cases.bin", d / f"results_{name}.bin")
        out[name] = Run(cs, got, wall, c)
    print(f"\ntransientcheck: {len(cs.launches)} launches, build + cases {t1 - t0:.1f} s, two drivers {time.time() - t1:.1f} s "
          f"(their launches {out['split'].wall:.2f} s and {out['f32'].wall:.2f} s); softplus allowance measured "
          f"{cs.softplus_allowance():.3e} -> 4 x = {4 * cs.softplus_allowance():.3e} of 1 + softplus")
    return out


def family(run, kernel, fam=None, label=""):
    bad, worst, seen = [], {}, 0
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] != kernel or (fam is not None and L["family"] != fam):
            continue
        b, ratio = run.result(li)
        bad += [(L["name"],) + x for x in b]
        for slot, r in ratio.items():
            if r > worst.get(slot, (-1.0, ""))[0]:
                worst[slot] = (r, L["name"])
        seen += 1
    for slot, (r, name) in sorted(worst.items()):
        print(f"{label:6s}{kernel:9s} {fam or '':9s} {slot:28s} worst error / tolerance = {r:.4f}  ({name})")
    return bad, seen


def count(cs, kernel, fam):
    return sum(1 for L in cs.launches if L["kernel"] == kernel and L["family"] == fam)


@pytest.mark.parametrize("target", list(TARGETS))
def test_shadow_rays(runs, target):
    bad, seen = family(runs[target], "shadow", label=target)
    assert seen == 12 and not bad, (seen, len(bad), bad[:20])


@pytest.mark.parametrize("fam", M.FAMILIES)
@pytest.mark.parametrize("kernel", ["bins", "slice"])
@pytest.mark.parametrize("target", list(TARGETS))
def test_forward(runs, target, kernel, fam):
    """No element over tolerance, the exact zeros exact, the canaries unchanged: per build, kernel and family."""
    run = runs[target]
    bad, seen = family(run, kernel, fam, target)
    assert seen == count(run.cs, kernel, fam) and seen >= 4 and not bad, (seen, len(bad), bad[:20])


@pytest.mark.parametrize("fam", ["window", "shift", "direct", "flags", "rays"])
@pytest.mark.parametrize("target", list(TARGETS))
def test_backward(runs, target, fam):
    """dz of both heads, the heads' inputs in reference order, d_tib, d_direct, d_weights against fp64 autograd; exact zeros
    outside the live tiles and for killed, clamped and weightless samples; canaries in the rows outside the chunk."""
    run = runs[target]
    bad, seen = family(run, "bins_bwd", fam, target)
    assert seen == count(run.cs, "bins_bwd", fam) and seen >= 2 and not bad, (seen, len(bad), bad[:20])
    if fam == "rays":
        chunks = {(L["ints"]["r0"], L["ints"]["C"]) for L in run.cs.launches if L["kernel"] == "bins_bwd" and L["ints"]["n_rays"] == 9}
        assert {(3, 5), (8, 1), (0, 9)} <= chunks


@pytest.mark.parametrize("target", list(TARGETS))
def test_windows_are_exact_zeros_outside(runs, target):
    """The unshifted composites are exactly zero outside the union of the ray's kept bins, and not all zero inside it."""
    run = runs[target]
    seen = 0
    for li, (lo, hi) in run.cs.window_specs.items():
        L = run.cs.launches[li]
        keep = M.decisions(L["scene"])["keep"].any(1)                    # [n, 700] bins any sample of the ray keeps
        assert keep[:, lo:hi + 1].all() and not keep[:, :lo].any() and not keep[:, hi + 1:].any()
        for slot in ("out_ti_diffuse", "out_ti_specular"):
            v = run.logical(li, slot)
            assert (v[~keep] == 0).all() and (v[keep] > 0).all(), (L["name"], slot)
        seen += 1
    assert seen == 8


@pytest.mark.parametrize("target", list(TARGETS))
def test_slice_equals_interpolated_histograms(runs, target):
    """k_transient_slice against k_transient_bins on the same buffers: w v[ceil t] + (1 - w) v[floor t] of the histograms the
    bins kernel wrote, to the 4e-5 of test_slices_vs_full_render_and_extras_bitwise (there on histograms below 1; here
    relative to the largest of the entries read where that exceeds 1).  The direct part is held to equality as well: the
    expression in float32, in that order, from the twin's out_direct ("the direct slice is bitwise the full
    render's", here on asymmetric taps and every form of the filter)."""
    run = runs[target]
    worst, seen, exact_seen = 0.0, 0, 0
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] != "slice" or L.get("twin") is None:
            continue
        for slot in M.SLICE_OUT:
            s, h = run.logical(li, slot), run.logical(L["twin"], slot)
            if s is None or h is None:
                continue
            if slot == "out_direct":
                # the two kernels share the scatter and the filter (rc_dev_transient.h): float32, in the kernel's order
                tf = np.asarray(L["t"], np.float32)
                w = (tf - np.floor(tf))[None, :, None]
                exact = w * h[:, np.ceil(tf).astype(int)] + (np.float32(1.0) - w) * h[:, np.floor(tf).astype(int)]
                assert exact.dtype == np.float32 and np.array_equal(s.view(np.uint32), exact.view(np.uint32)), (L["name"], slot)
                exact_seen += 1
            h = h.astype(np.float64)
            t = np.asarray(L["t"], np.float32).astype(np.float64)
            mag = np.maximum(np.abs(h[:, np.floor(t).astype(int)]), np.abs(h[:, np.ceil(t).astype(int)]))
            d = np.abs(s.astype(np.float64) - M.slice_of(h, L["t"])) / np.maximum(1.0, mag)
            worst = max(worst, float(d.max()))
            assert d.max() <= 4e-5, (L["name"], slot, float(d.max()))
            seen += 1
    print(f"{target}: max |slice - interpolated histogram| = {worst:.3e} (bound 4e-5) over {seen} outputs")
    assert seen >= 3 * 55 and exact_seen >= 55


@pytest.mark.parametrize("target", list(TARGETS))
def test_sums_of_the_histograms(runs, target):
    """out_rgb is the float32 sum of out_direct and out_indirect; the per-ray sums equal the histograms' sums over the bins
    (702 u sum |.|: 700 additions in any order); integrated = direct + indirect in float32."""
    run = runs[target]
    seen = 0
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] != "bins":
            continue
        g = {s: run.logical(li, s) for s in ("out_rgb", "out_direct", "out_indirect", "out_direct_rgb", "out_indirect_rgb", "out_integrated_rgb")}
        if any(v is None for v in g.values()):
            continue
        assert np.array_equal(g["out_rgb"], g["out_direct"] + g["out_indirect"]), L["name"]
        assert np.array_equal(g["out_integrated_rgb"], g["out_direct_rgb"] + g["out_indirect_rgb"]), L["name"]
        for h, s in (("out_direct", "out_direct_rgb"), ("out_indirect", "out_indirect_rgb")):
            h64 = g[h].astype(np.float64)
            assert (np.abs(g[s] - h64.sum(1)) <= (M.BINS + 2) * M.U * np.abs(h64).sum(1)).all(), (L["name"], s)
        seen += 1
    assert seen >= 55


@pytest.mark.parametrize("target", list(TARGETS))
def test_null_outputs_and_wall_time(runs, target):
    run = runs[target]
    assert {L["kernel"] for L in run.cs.launches} == set(M.KERNELS)
    assert all(not run.result(li)[0] for li in range(len(run.cs.launches)))
    none = [L for L in run.cs.launches if L["name"].startswith("pointers/none")]
    assert len(none) == 2 and all(b < 0 for L in none for s, b in L["bufs"].items() if s in M.SLOTS[L["kernel"]][3])
    assert run.wall < 5.0, run.wall
