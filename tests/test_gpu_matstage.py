"""The material stage's forward kernels of csrc/rc_material.hip on the device, directly against their argument structs'
contracts: the cases of tests/matstage_ref.py (waves with 64 and with 3 live lanes, Ks != Kd, vMF shares other than Kd -
round(Kd / 2), 1 to 9 rays in blocks of 4 waves, S around the wave size, the MH_PTS = 16 instantiation, every optional
pointer null and set, the clamps) through tests/matstage_check.hip, which links the library's own rc_material.o.  The driver
runs once, as a child process under a time limit; the tests below only read its result file.

Tolerances (derivations: tests/matstage_ref.py; the CPU side: tests/test_matstage_ref.py): the heads, the composite and the
integrator to derived bounds; the sampler's directions, pdfs and MIS weights to 4 x the floor MatCases.floors() measures on
the CPU of the machine that runs the test (the figures are the record: regular family 9.2e-6 local, 9.1e-6 global, pdf 4.3e-6
on the scale 1 + pdf, weight 2.1e-5 -> 3.7e-5, 3.6e-5, 1.7e-5, 8.4e-5; edge family 1.5e-6, 1.9e-6, 3.5e-6, 7.3e-6; the
ill-conditioned family, kappa <= eps on the sampled lobe, against the float32 restatement at the regular tolerance);
sec_origins / near / far / lights, local_view, zero pdfs and zero weights, the
drawn lobe, and every claim of "the same bits" to equality.  Every float of an output buffer that is not a logical element,
and every output a launch was not asked for, is a canary NaN and has to come back bitwise unchanged."""
import os
import subprocess
import time

import numpy as np
import pytest

import matstage_ref as M

pytestmark = pytest.mark.gpu
EXE = os.path.join(M.ROOT, "build", "matstagecheck")


class Run:
    def __init__(self, cs, got, wall):
        self.cs, self.got, self.wall = cs, got, wall
        self._res = {}

    def result(self, li):
        """(failures, error / tolerance per slot) of launch li, computed once."""
        if li not in self._res:
            ref, tol = M.expected(self.cs, li, dev=self.got)
            self._res[li] = M.check(self.cs, li, self.got, ref, tol)
        return self._res[li]

    def logical(self, li, slot):
        L = self.cs.launches[li]
        size = int(np.prod(M.out_shape(L["kernel"], slot, L["ints"])))
        return self.got[L["bufs"][slot]][M.GUARD:M.GUARD + size]

    def same_bits(self, a, sa, b, sb):
        return np.array_equal(self.logical(a, sa).view(np.uint32), self.logical(b, sb).view(np.uint32))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    t0 = time.time()
    r = subprocess.run(["make", "-C", M.CSRC, "-j16", "matstagecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cs = M.build_cases()
    d = tmp_path_factory.mktemp("matstagecheck")
    M.write_case_file(d / "cases.bin", cs)
    t1 = time.time()
    r = subprocess.run([EXE, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "matstagecheck ok" in r.stdout, r.stdout + r.stderr
    got, wall = M.read_results(d / "results.bin", cs)
    print(f"\nmatstagecheck: {len(cs.launches)} launches, build + cases {t1 - t0:.1f} s, driver {time.time() - t1:.1f} s "
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
        print(f"{k[0]:10s} {k[1]:30s} worst error / tolerance = {r:.4f}  ({name})")
    return bad, seen


def test_material_head(run):
    bad, seen = _family(run, ("mhead",))
    assert seen == len(M.RAYS) + 8 + 1 + 3 + 2 and not bad, (seen, len(bad), bad[:20])


def test_material_head_of_8211_points_equals_launches_of_up_to_8192(run):
    """k_material_head<16> (the launcher's choice above 8192 points; the last block holds 3): "sums run in the same order as
    the one-point form" -- the same bits as k_material_head<4> on the same points."""
    li = next(i for i, L in enumerate(run.cs.launches) if "parts" in L)
    parts = np.concatenate([run.logical(p, "mat") for p in run.cs.launches[li]["parts"]])
    assert run.cs.launches[li]["ints"]["n"] == 8211 and parts.size == 8211 * 5
    assert np.array_equal(run.logical(li, "mat").view(np.uint32), parts.view(np.uint32))


def test_light_head(run):
    bad, seen = _family(run, ("lhead",))
    assert seen == len(M.RAYS) + 8 + 1 + 3 and not bad, (seen, len(bad), bad[:20])
    for li, L in enumerate(run.cs.launches):
        if L.get("edge") == "clamps":                                    # the constants of the contract, held exactly
            v, lg = run.logical(li, "vmf").reshape(3, 128, 5), run.logical(li, "vmf_logit").reshape(3, 128)
            assert (v[:, ::2, 3] == 50.0).all() and (lg[:, ::2] == -50.0).all()
        if L.get("edge") == "equal_logits":
            assert (run.logical(li, "vmf").reshape(3, 128, 5)[..., 4] == np.float32(1.0 / 128)).all()


def test_shading_heads_equal_the_two_separate_launches(run):
    bad, seen = _family(run, ("heads",))
    assert seen == 8 + 2 + 2 and not bad, (seen, len(bad), bad[:20])
    pairs = 0
    for li, L in enumerate(run.cs.launches):
        for slot, (other, oslot) in L.get("twins", {}).items():
            assert run.same_bits(li, slot, other, oslot), (L["name"], slot)
            pairs += 1
    assert pairs == 8 * 3 + 1 + 2


@pytest.mark.parametrize("family", ["regular", "edges", "illcond"])
def test_brdf_sample(run, family):
    bad, seen = _family(run, ("sample",), family)
    assert seen == {"regular": 2 * len(M.SPLITS) + 1 + 3 + 2, "edges": 5, "illcond": 1}[family] and not bad, (seen, len(bad), bad[:20])


def test_brdf_sample_draws_the_lobe_the_keys_name(run):
    """argmax(logit + gumbel) on the raw logits, the lowest index among equal keys: the drawn launch equals, bit for bit, the
    launch that is handed the fp64-expected lobe; vmf_lobe outside [0, 127] is clamped."""
    seen = 0
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] != "sample" or "twin" not in L:
            continue
        if "winner" in L:
            ref, _ = M.expected(run.cs, li, dev=run.got)
            assert np.array_equal(ref["_lobe"], L["winner"]), L["name"]
        for slot in M.SLOTS["sample"][3]:
            assert run.same_bits(li, slot, L["twin"], slot), (L["name"], slot)
        seen += 1
    assert seen == len(M.SPLITS) + 2


def test_last_ray_does_not_depend_on_the_block_it_falls_in(run):
    """The same point as ray 0 of 1, ray 4 of 5 and ray 8 of 9: wave 0 of a block whose other waves are the clamped tail, and
    wave 0 of the second and third block, give the same bits in k_brdf_sample and k_material_integrate."""
    (s1, i1), (s5, i5), (s9, i9) = run.cs.lastray
    K = 10
    for s, n in ((s5, 5), (s9, 9)):
        for slot in ("samples", "local_view"):
            a = run.logical(s1, slot).reshape(1, -1)[-1]
            b = run.logical(s, slot).reshape(n, -1)[-1]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (n, slot)
        a, b = run.logical(s1, "sec_dirs").reshape(K, 3), run.logical(s, "sec_dirs").reshape(n * K, 3)
        rows = np.r_[(n - 1) * 5 + np.arange(5), n * 5 + (n - 1) * 5 + np.arange(5)]
        assert np.array_equal(a.view(np.uint32), b[rows].view(np.uint32)), n
    for i, n in ((i5, 5), (i9, 9)):
        for k in M.MOUT_INTEGRATE:
            a = run.logical(i1, "out_" + k).reshape(1, -1)[-1]
            b = run.logical(i, "out_" + k).reshape(n, -1)[-1]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (n, k)


def test_material_composite_all(run):
    bad, seen = _family(run, ("composite",))
    assert seen == 2 * (len(M.S_COMPOSITE) + 6) and not bad, (seen, len(bad), bad[:20])
    assert {L["ints"]["n"] for L in run.cs.launches if L["kernel"] == "composite"} == set(M.N_COMPOSITE)


@pytest.mark.parametrize("family", ["regular", "edges"])
def test_material_integrate(run, family):
    bad, seen = _family(run, ("integrate",), family)
    want = 3 * len(M.SPLITS) + len(M.S_INTEGRATE) + len(M.MOUT_INTEGRATE) + 3 + 2 if family == "regular" else 3
    assert seen == want and not bad, (seen, len(bad), bad[:20])


def test_material_integrate_does_not_depend_on_the_null_pointers(run):
    seen = 0
    for li, L in enumerate(run.cs.launches):
        if L["kernel"] != "integrate" or "twin" not in L:
            continue
        ref, _ = M.expected(run.cs, li, dev=run.got)
        for slot in M.SLOTS["integrate"][3]:
            if L["bufs"][slot] >= 0 and slot in ref:
                assert run.same_bits(li, slot, L["twin"], slot), (L["name"], slot)
                seen += 1
    assert seen >= 2 * len(M.SPLITS) + len(M.MOUT_INTEGRATE)


def test_every_launch_was_checked_and_wall_time(run):
    assert {L["kernel"] for L in run.cs.launches} == set(M.KERNELS)
    assert all(not run.result(li)[0] for li in range(len(run.cs.launches)))
    assert run.wall < 5.0, run.wall
