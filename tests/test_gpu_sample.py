"""The per-ray kernels of csrc/rc_sample.hip on the device, directly against their argument structs' contracts: the cases of
tests/sample_ref.py (bins and samples at and around the 16-lane row boundaries, 1 to 9 rays in blocks of 4 waves, every
optional pointer null and set) through tests/sample_check.hip, which links the library's own rc_sample.o.  The driver runs
once, as a child process under a time limit; the tests below only read its result file.

Tolerances (derivations: tests/sample_ref.py; the CPU side: tests/test_sample_ref.py).  Measured floors, max |float32
restatement - fp64| over a family's cases (Cases.floors() measures them on the CPU of the machine that runs the test; the
figures are the record), and the device's tolerance of 4 x floor:
  k_sample_intervals  rounding family 3.64e-6 -> 1.46e-5;  flat family 2.60e-6 -> 1.04e-5;  exact family: the restatement's bits
  k_sample_level      sdist 1.15e-5 -> 4.6e-5; tdist and means: that times the slope of s -> t, + the map's own rounding
  k_composite         percentiles 3.54e-7 -> 1.42e-6
Alpha weights, acc, the sums of products, filt_weight, distance_mean and the ladder values are held to derived bounds; picks,
gathered values, copied acc and every claim of "the same bits" to equality.  Every float of an output buffer that is not a
logical element, and every output a launch was not asked for, is a canary NaN and has to come back bitwise unchanged."""
import os
import subprocess
import time

import numpy as np
import pytest

import sample_ref as R

pytestmark = pytest.mark.gpu
EXE = os.path.join(R.ROOT, "build", "samplecheck")


class Run:
    def __init__(self, cs, got, wall):
        self.cs, self.got, self.wall = cs, got, wall
        self._res = {}

    def result(self, li):
        """(failures, error / tolerance per slot) of launch li, computed once."""
        if li not in self._res:
            ref, tol = R.expected(self.cs, li, dev=self.got)
            self._res[li] = R.check(self.cs, li, self.got, ref, tol)
        return self._res[li]

    def logical(self, li, slot):
        L = self.cs.launches[li]
        size = int(np.prod(R.out_shape(L["kernel"], slot, L["ints"])))
        return self.got[L["bufs"][slot]][R.GUARD:R.GUARD + size]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    t0 = time.time()
    r = subprocess.run(["make", "-C", R.CSRC, "-j16", "samplecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cs = R.build_cases()
    d = tmp_path_factory.mktemp("samplecheck")
    R.write_case_file(d / "cases.bin", cs)
    t1 = time.time()
    r = subprocess.run([EXE, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "samplecheck ok" in r.stdout, r.stdout + r.stderr
    got, wall = R.read_results(d / "results.bin", cs)
    print(f"\nsamplecheck: {len(cs.launches)} launches, build + cases {t1 - t0:.1f} s, driver {time.time() - t1:.1f} s "
          f"(its launches {wall:.2f} s)")
    return Run(cs, got, wall)


def _family(run, kernels, family=None):
    bad, worst, seen = [], {}, 0
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] not in kernels or (family is not None and L["family"] != family):
            continue
        b, ratio = run.result(li)
        bad += [(L["name"],) + x for x in b]
        for slot, r in ratio.items():
            if r > worst.get((L["kernel"], slot), (-1.0, ""))[0]:
                worst[(L["kernel"], slot)] = (r, L["name"])
        seen += 1
    for k, (r, name) in sorted(worst.items()):
        print(f"{k[0]:10s} {k[1]:28s} worst error / tolerance = {r:.4f}  ({name})")
    return bad, seen


def test_sample_intervals_exact_family_bit_for_bit(run):
    bad, seen = _family(run, ("intervals",), "exact")
    assert seen == 64 and not bad, (len(bad), bad[:20])


def test_sample_intervals_rounding_family(run):
    bad, seen = _family(run, ("intervals",), "round")
    assert seen == 2 * len(R.pairs()) and not bad, (len(bad), bad[:20])


def test_sample_intervals_flat_family(run):
    bad, seen = _family(run, ("intervals",), "flat")
    assert seen == 2 * sum(P >= 3 for P, _ in R.pairs()) + 5 * 4 * 2 and not bad, (len(bad), bad[:20])


def test_ladder_bounds(run):
    bad, seen = _family(run, ("ladder",))
    assert seen >= 5 and not bad, (len(bad), bad[:20])


def test_sample_level(run):
    bad, seen = _family(run, ("level",))
    assert seen >= len(R.pairs()) and not bad, (len(bad), bad[:20])


def test_sample_level_sorts_inverted_posts(run):
    """The launches whose clipped posts are out of order (tests/test_sample_ref.py pins which pairs: the last alone, the first
    alone, all of them): the ballot has to see the inversion and the rank sort has to run -- sdist sorted in [0, 1] and sdist,
    tdist and means within the level family's bounds (R.check holds all of it)."""
    seen = 0
    for li, L in enumerate(run.cs.launches):
        if "inversions" in L:
            bad, ratio = run.result(li)
            assert not bad and {"sdist", "tdist", "means"} <= set(ratio), (L["name"], bad[:5])
            s = run.logical(li, "sdist").reshape(L["ints"]["n"], -1)
            assert (np.diff(s, axis=-1) >= 0).all() and s.min() >= 0 and s.max() <= 1, L["name"]
            seen += 1
    assert seen == 16


def test_sample_level_on_ladder_bounds_bit_for_bit(run):
    """One (near, far) and no normals: the launch on k_ladder_bounds' s_bounds equals the per-ray computation."""
    seen = 0
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] == "level" and "twin" in L:
            for slot in ("sdist", "tdist", "means"):
                assert np.array_equal(run.logical(li, slot).view(np.uint32), run.logical(L["twin"], slot).view(np.uint32)), (L["name"], slot)
            seen += 1
    assert seen >= 8


def test_resample(run):
    bad, seen = _family(run, ("resample",))
    assert seen == 5 * len(R.SAMPLES) and not bad, (len(bad), bad[:20])


def test_composite(run):
    bad, seen = _family(run, ("composite",))
    assert seen == 7 * len(R.SAMPLES) and not bad, (len(bad), bad[:20])


def test_composite_reduction_paths_bit_for_bit(run):
    """k_composite: "Either way each sum is added up in the same order: same bits" -- the outputs a launch shares with the
    launch that asked for every pointer, without resampling (Sf = S) and with it (Sf = 1: rgb and acc)."""
    seen, bad = 0, []
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] != "composite" or "twin" not in L:
            continue
        T = run.cs.launches[L["twin"]]
        ref, _ = R.expected(run.cs, li, dev=run.got)
        for slot in R.SLOTS["composite"][3]:
            if L["bufs"][slot] >= 0 and T["bufs"][slot] >= 0 and slot in ref:
                if not np.array_equal(run.logical(li, slot).view(np.uint32), run.logical(L["twin"], slot).view(np.uint32)):
                    bad.append((L["name"], slot))
                seen += 1
    assert seen >= (4 * 2 + 2) * len(R.SAMPLES) and not bad, bad[:20]
    assert sum(L["kernel"] == "composite" and L["ints"]["Sf"] == 1 and "twin" in L for L in run.cs.launches) == len(R.SAMPLES)


def test_composite_pick(run):
    bad, seen = _family(run, ("pick",))
    assert seen == len(R.SAMPLES) + 4 and not bad, (len(bad), bad[:20])
    pairs = 0
    for li, L in enumerate(run.cs.launches):                             # rc_internal.h: "Same values, bit for bit"
        if L["kernel"] == "pick" and "twin" in L:
            for a, b in (("out_rgb", "out_rgb"), ("out_acc", "out_acc")):
                assert np.array_equal(run.logical(li, a).view(np.uint32), run.logical(L["twin"], b).view(np.uint32)), (L["name"], a)
            pairs += 1
    assert pairs == len(R.SAMPLES)


def test_every_launch_was_checked_and_wall_time(run):
    kinds = {L["kernel"] for L in run.cs.launches}
    assert kinds == set(R.KERNELS)
    assert all(not run.result(li)[0] for li in range(len(run.cs.launches)))
    assert run.wall < 5.0, run.wall
