"""tests/sample_ref.py on the CPU: its fp64 references against oracle/spec_np.py where they overlap, the case table against
the shape list, the derived bounds against the float32 restatement (inside) and a bfloat16-cut variant (outside), the measured
floors of the resampled posts and percentiles, the mutation guards (each plausible kernel mistake fails the checker that
the GPU test uses, on at least one case), the file formats and the driver's cross-compile.  tests/test_gpu_sample.py runs the
same cases on the device.

Measured floors, max |float32 restatement - fp64| over a family's cases (Cases.floors() measures them on the machine that
runs the test; the figures here are the record test_post_floors holds them near):
  k_sample_intervals  rounding family 3.64e-6, flat family 2.60e-6      -> device tolerance 1.46e-5 and 1.04e-5
  k_sample_level      sdist 1.15e-5                                    -> 4.6e-5
  k_composite         percentiles 3.54e-7                               -> 1.42e-6"""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import sample_ref as R
from oracle import spec_np as spec


@pytest.fixture(scope="module")
def cs():
    return R.build_cases()


@pytest.fixture(scope="module")
def refs(cs):
    """Per launch: (fp64 reference, float32 restatement, what the device is held to, its tolerances), computed once."""
    out = []
    for li in range(len(cs.launches)):
        ref, tol = R.expected(cs, li)
        out.append((R.reference(cs, li), R.reference(cs, li, np.float32), ref, tol))
    return out


def _by(cs, kernel):
    return [(li, L) for li, L in enumerate(cs.launches) if L["kernel"] == kernel]


def _val(cs, L, slot, shape, dtype=np.float32):
    return cs.value(L["bufs"][slot]).view(dtype).reshape(shape).astype(np.float64 if dtype == np.float32 else np.int64)


def test_out_names_follow_the_abi():
    text = open(os.path.join(R.ROOT, "include", "rc_abi.h")).read()
    names = re.findall(r"^\s*RC_OUT_([A-Z0-9_]+)\b", text[text.index("RC_OUT_RGB = 0"):], re.M)
    assert [n.lower() for n in names[:names.index("COUNT")]] == list(R.OUT_NAMES)
    head = open(os.path.join(R.CSRC, "rc_internal.h")).read()
    assert "RC_SH_RGB = 0, RC_SH_AD = 3, RC_SH_ID = 6, RC_SH_IS = 9, RC_SH_TINT = 12, RC_SHADE_CH = 15" in head
    assert (R.SH_RGB, R.SH_AD, R.SH_ID, R.SH_IS, R.SH_TINT, R.SHADE_CH) == (0, 3, 6, 9, 12, 15)


def test_reference_agrees_with_spec_np(cs, refs):
    seen = set()
    for li, L in enumerate(cs.launches):
        i, f, ref = L["ints"], L["flts"], refs[li][0]
        n, S = i.get("n", 0), i.get("S", 0)
        if L["kernel"] == "intervals" and L["family"] != "exact":
            P = i["P"]
            t, lg = _val(cs, L, "t", (n, P + 1)), _val(cs, L, "logits", (n, P))
            jit = _val(cs, L, "jitter", (n,)) if L["bufs"]["jitter"] >= 0 else [None] * n
            for r in range(n):
                with np.errstate(invalid="ignore"):
                    want = spec.sample_intervals_ray(None if jit[r] is None else float(jit[r]), t[r], lg[r], S)
                assert np.abs(ref["out"][r] - want).max() <= 1e-12, L["name"]
            seen.add("intervals")
        elif L["kernel"] == "ladder":
            x = np.array([f["near"], min(f["far"], f["far_clamp"])])
            assert np.allclose(ref["out"], spec.power_ladder(x, f["p"], f["premult"]), rtol=1e-14, atol=0)
            seen.add("ladder")
        elif L["kernel"] == "level":
            if "prev_weights" in ref:
                P = i["P"]
                want = spec.alpha_weights(_val(cs, L, "prev_density", (n, P)), _val(cs, L, "prev_tdist", (n, P + 1)),
                                          _val(cs, L, "directions", (n, 3)))
                assert np.allclose(ref["prev_weights"], want, rtol=1e-12, atol=1e-300), L["name"]
            if i["use_raydist"]:
                p, pm = f["raydist_p"], f["raydist_premult"]
                if L["bufs"]["s_bounds"] < 0:
                    assert np.allclose(ref["_s_far"], spec.power_ladder(ref["_far"], p, pm), rtol=1e-14)
                want = spec.power_ladder_inverse(ref["_y"], p, pm)
                assert np.allclose(ref["tdist"], want, rtol=1e-12, atol=1e-15), L["name"]
                seen.add("inverse ladder")
            o, d = _val(cs, L, "origins", (n, 3)), _val(cs, L, "directions", (n, 3))
            if "means" in ref:                                           # spec_np.sampler's lines, render.py:49-59
                t0, t1 = ref["tdist"][:, :-1], ref["tdist"][:, 1:]
                s_, d_ = t0 + t1, t1 - t0
                tm = s_ * (0.5 + d_ ** 2 / np.maximum(spec.EPS ** 2, 3 * s_ ** 2 + d_ ** 2))
                want = (o[:, None, :] + d[:, None, :] * tm[..., None]).reshape(n * S, 3).T
                assert np.allclose(ref["means"], want, rtol=1e-12, atol=1e-15), L["name"]
            seen.add("level")
        elif L["kernel"] == "resample":
            want_w = spec.alpha_weights(_val(cs, L, "density", (n, S)), _val(cs, L, "tdist", (n, S + 1)), _val(cs, L, "directions", (n, 3)))
            assert np.allclose(ref["weights"], want_w, rtol=1e-12, atol=1e-300), L["name"]
            if L["bufs"]["gumbel"] >= 0:
                ind, fw = spec.pick(None, want_w, gumbel=_val(cs, L, "gumbel", (n, S)))
            else:
                ind, fw = spec.pick(None, want_w, inds=np.clip(_val(cs, L, "inds_in", (n,), np.int32), 0, S - 1))
            assert np.array_equal(ind, ref["inds_out"]) and np.allclose(ref["filt_weight"], fw, rtol=1e-12, atol=1e-300), L["name"]
            seen.add("resample")
        elif L["kernel"] == "composite" and i["Sf"] == S and L["name"].startswith("comp/all"):
            t = _val(cs, L, "tdist", (n, S + 1))
            w = spec.alpha_weights(_val(cs, L, "density", (n, S)), t, _val(cs, L, "directions", (n, 3)))
            sh = _val(cs, L, "shade", (R.SHADE_CH, n, S))
            ch = lambda c: np.moveaxis(sh[c:c + 3], 0, -1)
            means = np.moveaxis(_val(cs, L, "means", (3, n, S)), 0, -1)
            per = {"rgb": ch(R.SH_RGB), "direct_rgb": ch(R.SH_AD), "indirect_diffuse_rgb": ch(R.SH_ID),
                   "indirect_specular_rgb": ch(R.SH_IS), "albedo_rgb": ch(R.SH_TINT), "diffuse_rgb": ch(R.SH_AD) + ch(R.SH_ID),
                   "indirect_rgb": ch(R.SH_ID) + ch(R.SH_IS), "means": means,
                   "normals_pred": np.moveaxis(_val(cs, L, "normals_pred", (3, n, S)), 0, -1),
                   "ray_dists": np.linalg.norm(_val(cs, L, "origins", (n, 3))[:, None] - means, axis=-1, keepdims=True),
                   "light_dists": np.linalg.norm(_val(cs, L, "lights", (n, 3))[:, None] - means, axis=-1, keepdims=True)}
            cfg = types.SimpleNamespace(percentiles=(f["pct0"], f["pct1"], f["pct2"]))
            with np.errstate(invalid="ignore", divide="ignore"):
                want = spec.integrate(cfg, per, w, w, t, f["bg"])
            for k in ("rgb", "acc", "distance_mean", "distance_percentile_5", "distance_median", "distance_percentile_95",
                      "direct_rgb", "indirect_diffuse_rgb", "indirect_specular_rgb", "albedo_rgb", "diffuse_rgb", "indirect_rgb",
                      "means", "normals_pred", "ray_dists", "light_dists"):
                assert np.allclose(ref["out_" + k], np.asarray(want[k]).reshape(ref["out_" + k].shape), rtol=1e-11, atol=1e-13), (L["name"], k)
            seen.add("composite")
    assert seen == {"intervals", "ladder", "level", "inverse ladder", "resample", "composite"}


def test_cases_cover_the_shape_list(cs):
    for kernel in ("intervals", "level"):
        got = {(L["ints"]["P"], L["ints"]["S"]) for _, L in _by(cs, kernel)}
        want = {(P, S) for P in (1, 64) for S in R.SAMPLES} | {(P, S) for S in (32, 64) for P in R.BINS} | {(S, S) for S in R.SAMPLES}
        assert want | set(R.PRODUCTION) <= got and got <= {(P, S) for P in R.BINS for S in R.SAMPLES}, kernel
        assert {L["ints"]["n"] for _, L in _by(cs, kernel)} == set(R.RAYS)
    for kernel in ("resample", "composite"):
        assert {L["ints"]["S"] for _, L in _by(cs, kernel)} == set(R.SAMPLES)
        assert {L["ints"]["n"] for _, L in _by(cs, kernel)} == set(R.RAYS)
    assert all(L["ints"]["S"] >= 2 for L in cs.launches if "S" in L["ints"])
    fams = {L["family"] for _, L in _by(cs, "intervals")}
    assert fams == {"exact", "round", "flat"}
    for li, L in _by(cs, "intervals"):
        n, P = L["ints"]["n"], L["ints"]["P"]
        if L["family"] == "exact":
            t, lg = _val(cs, L, "t", (n, P + 1)), _val(cs, L, "logits", (n, P))
            assert P & (P - 1) == 0 and np.array_equal(t * 1024, np.round(t * 1024)) and (lg == lg[:, :1]).all()
        if L["bufs"]["jitter"] >= 0:
            j = _val(cs, L, "jitter", (n,))
            assert j.min() >= 0 and j.max() < 1 and (j[0] == 0 or n == 1) and j[-1] == 1 - 2.0 ** -24
    assert {L["ints"]["P"] for _, L in _by(cs, "intervals") if L["family"] == "exact"} == {1, 2, 16, 32, 64}
    lv = [L for _, L in _by(cs, "level")]
    assert {L["ints"]["S"] for L in lv if L["bufs"]["prev_sdist"] < 0} == set(R.SAMPLES)              # level 0 at every S
    later = [L for L in lv if L["bufs"]["prev_sdist"] >= 0]
    assert any(L["bufs"]["prev_weights"] >= 0 for L in later) and any(L["bufs"]["prev_weights"] < 0 for L in later)
    assert any(L["bufs"]["means"] < 0 for L in lv) and any(L["bufs"]["normals"] >= 0 for L in lv)
    assert any(L["bufs"]["s_bounds"] >= 0 for L in lv) and any(L["ints"]["secondary"] == 0 for L in lv)
    assert all("twin" in L for L in lv if L["bufs"]["s_bounds"] >= 0)
    rs = [L for _, L in _by(cs, "resample")]
    for key in ("gumbel", "inds_in", "acc_out", "src_out", "pts_out"):
        assert any(L["bufs"][key] >= 0 for L in rs) and any(L["bufs"][key] < 0 for L in rs), key
    for L in rs:
        if L["bufs"]["inds_in"] >= 0:
            raw = _val(cs, L, "inds_in", (L["ints"]["n"],), np.int32)
            assert (raw < 0).any() or (raw >= L["ints"]["S"]).any(), L["name"]
    cp = [L for _, L in _by(cs, "composite")]
    assert {L["ints"]["Sf"] == 1 for L in cp} == {True, False}
    for key in ("lights", "normals_grad", "weights"):
        assert any(L["bufs"][key] < 0 for L in cp) and any(L["bufs"][key] >= 0 for L in cp), key
    pk = [L for _, L in _by(cs, "pick")]
    assert any(L["bufs"]["out_rgb"] < 0 for L in pk) and any(L["bufs"]["out_acc"] < 0 for L in pk)
    assert sum("twin" in L for L in pk) == len(R.SAMPLES)


def test_gumbel_winner_leads_by_construction(cs, refs):
    """fp64 keys: the winner is the planned index and leads the runner-up by >= 1e-3 (the ties cases: by exactly 0, on
    identical logit bits, and the planned index is the lowest of the maxima)."""
    seen = 0
    for li, L in _by(cs, "resample"):
        if "winner" not in L:
            continue
        n, S = L["ints"]["n"], L["ints"]["S"]
        ref = refs[li][0]
        assert np.array_equal(ref["inds_out"], L["winner"]), L["name"]
        key = ref["_logit"] + _val(cs, L, "gumbel", (n, S))
        top = np.sort(key, axis=-1)
        if "ties" in L["name"]:
            assert (ref["weights"] == 0).all() and (np.argmax(key, axis=-1) == L["winner"]).all()
            assert ((key == top[:, -1:]).sum(axis=-1) >= 2).all()
            if S >= 50 and n > 1:
                assert set(np.flatnonzero(key[1] == top[1, -1])) == {17, 49}
        else:
            assert (top[:, -1] - top[:, -2] >= 1e-3).all(), L["name"]
            assert (top[:, -1] - top[:, -2]).min() < 3e-3
        seen += 1
    assert seen == 3 * len(R.SAMPLES)


def test_bounds_hold_the_float32_restatement(cs, refs):
    worst = {}
    for li, L in enumerate(cs.launches):
        r64, r32, ref, tol = refs[li]
        bad, ratio = R.check(cs, li, R.render(cs, li, r32), ref, tol)
        assert not bad, (L["name"], bad[:5])
        for slot, r in ratio.items():
            key = (L["kernel"], slot)
            worst[key] = max(worst.get(key, 0.0), r)
    # the derived bounds hold it with half to spare (tdist and means of k_sample_level rest on the measured floor of sdist)
    measured = {("intervals", "out"), ("level", "sdist"), ("level", "tdist"), ("level", "means"),
                ("composite", "out_distance_percentile_5"), ("composite", "out_distance_median"), ("composite", "out_distance_percentile_95")}
    derived = {k: v for k, v in worst.items() if k not in measured}
    assert len(derived) >= 25 and max(derived.values()) <= 0.5, worst


def test_bounds_reject_a_bfloat16_cut(cs, refs):
    """dd rounded to bfloat16 inside the alpha weights.  The weights of every launch with density leave their bound by a factor
    >= 10.  acc, filt_weight and distance_mean cannot move on a saturated ray (acc = 1 - exp(-sum dd) stays 1), so the
    criterion is per ray and on the contract alone: wherever the cut moves the fp64 value by >= 20 x the tolerance, the cut
    float32 restatement lies >= 10 x outside it; such rays exist for every output, picks given by inds_in included.  The
    ladder values rounded to bfloat16 leave their bound too."""
    seen = {}
    for li, L in enumerate(cs.launches):
        r64, _, ref, tol = refs[li]
        if L["kernel"] == "ladder":
            err = np.abs(R.bf16(r64["out"].astype(np.float32)).astype(np.float64) - r64["out"])
            assert (err / tol["out"]).max() >= 10, L["name"]
            continue
        if L["kernel"] not in ("resample", "composite") or "ties" in L["name"]:
            continue
        if not (_val(cs, L, "density", (L["ints"]["n"], L["ints"]["S"])) > 0).any():
            continue
        cut, cut64 = R.reference(cs, li, np.float32, cut=True), R.reference(cs, li, np.float64, cut=True)
        for slot in ("weights", "acc_out", "out_acc", "filt_weight", "out_distance_mean"):
            if slot not in r64:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.broadcast_to(tol[slot], r64[slot].shape)
                r = np.where(t > 0, np.abs(cut[slot].astype(np.float64) - r64[slot]) / t, 0.0)
                moved = np.where(t > 0, np.abs(cut64[slot] - r64[slot]) / t, 0.0) >= 20
            if slot == "weights":
                assert r.max() >= 10, (L["name"], slot, r.max())
            assert (r[moved] >= 10).all(), (L["name"], slot, r[moved].min())
            seen[slot] = seen.get(slot, 0) + int(moved.sum())
    print(seen)
    assert set(seen) == {"weights", "acc_out", "out_acc", "filt_weight", "out_distance_mean"} and min(seen.values()) >= 5, seen


def test_post_floors(cs):
    """The floors are measured on this machine's numpy (Cases.floors()), so the figures in the docstrings are a record, not a
    constant: what has to hold is that 4 x floor stays within the 1e-4 the golden test already holds, and that the floors
    are the size they were recorded at (within a factor of 2: another build of numpy may round its float32 exp differently)."""
    floors = cs.floors()
    print("measured floors", floors)
    recorded = {"round": 3.64e-6, "flat": 2.60e-6, "level": 1.15e-5, "pct": 3.54e-7}
    assert set(floors) == set(R.POST_FAMILIES) == set(recorded)
    for fam, v in floors.items():
        assert 0 < 4 * v <= 1e-4, (fam, v)
        assert 0.5 * recorded[fam] <= v <= 2 * recorded[fam], (fam, v)


def test_level_cases_reach_the_inversion_check(cs, refs):
    """k_sample_level sorts only when its ballot finds an inversion among the clipped posts.  The unsorted posts of the float32
    restatement: no inversion on the ordinary level launches (the copy path), every pair on the descending ones, and on the
    "inv" launches rays whose only inversion is the last pair (S - 1, S) and rays whose only one is the first pair (0, 1)."""
    kinds = {"none": 0, "all": 0, "last only": 0, "first only": 0}
    for li, L in _by(cs, "level"):
        raw = R.reference(cs, li, np.float32, "no_sort")["sdist"]
        inv = raw[:, :-1] > raw[:, 1:]
        S = L["ints"]["S"]
        if "inversions" not in L:
            assert not inv.any(), L["name"]
            kinds["none"] += 1
            continue
        assert inv.any(axis=-1).all(), L["name"]
        if L["inversions"] == "all":
            assert inv.sum(axis=-1).min() >= S - 2, L["name"]
            kinds["all"] += 1
        for row in inv:
            if row.sum() == 1 and row[S - 1]:
                kinds["last only"] += 1
            if row.sum() == 1 and row[0]:
                kinds["first only"] += 1
        ref = refs[li][0]["sdist"]
        assert (np.diff(ref, axis=-1) >= 0).all() and ref.min() >= 0 and ref.max() <= 1
    print(kinds)
    assert kinds["none"] >= 60 and kinds["all"] == 8 and kinds["last only"] >= 6 and kinds["first only"] >= 6, kinds


def test_exact_family_is_exact(cs, refs):
    """The float32 restatement of an exact case has exact CDF posts k / P (so any order of the sums gives them) and agrees with
    fp64 to the rounding of u and of the interpolation."""
    for li, L in _by(cs, "intervals"):
        if L["family"] != "exact":
            continue
        r64, r32, ref, tol = refs[li]
        assert tol["out"] == 0.0 and ref["out"].dtype == np.float32
        assert np.abs(r32["out"].astype(np.float64) - r64["out"]).max() <= 4e-7, L["name"]


APPLIES = {"side_left": ("intervals", "level"), "last_post_not_reflected": ("intervals", "level"), "no_sort": ("intervals", "level"),
           "inversion_check_misses_last": ("level",), "inversion_check_misses_first": ("level",),
           "cdf_end_not_one": ("composite",), "scan_restart_16": ("intervals", "level", "resample", "composite"),
           "scan_restart_32": ("intervals", "level", "resample", "composite"),
           "scan_restart_48": ("intervals", "level", "resample", "composite"), "lane63_dropped": ("intervals", "resample", "composite"),
           "no_excl_shift": ("level", "resample", "composite"), "tie_high": ("resample",), "inds_unclamped": ("resample",),
           "pct_filtered": ("composite",), "bg_filtered_acc": ("composite",), "clamped_wave_store": ("intervals", "level", "composite")}


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutation_is_caught(cs, refs, mutation):
    """A device with this mistake (its float32 arithmetic otherwise the restatement's) fails R.check on at least one launch of
    EVERY kernel the mistake applies to."""
    caught, tried = {k: [] for k in APPLIES[mutation]}, 0
    for li, L in enumerate(cs.launches):
        if L["kernel"] not in APPLIES[mutation]:
            continue
        _, _, ref, tol = refs[li]
        bad, _ = R.check(cs, li, R.render(cs, li, R.reference(cs, li, np.float32, mutation), mutation), ref, tol)
        tried += 1
        if bad:
            caught[L["kernel"]].append((L["name"], bad[0][:2]))
    print(mutation, "caught on", {k: len(v) for k, v in caught.items()}, "of", tried, [v[:2] for v in caught.values()])
    assert all(caught.values()), (mutation, {k: len(v) for k, v in caught.items()})
    assert set(APPLIES) == set(R.MUTATIONS)


def test_case_file_round_trip(cs, tmp_path):
    path = tmp_path / "cases.bin"
    R.write_case_file(path, cs)
    nf = 1 + R.N_INT + R.N_FLT + R.N_BUF
    head = np.fromfile(path, np.int64, 4)
    assert list(head) == [R.MAGIC_CASES, len(cs.bufs), len(cs.launches), nf]
    table = np.fromfile(path, np.int64, 2 * len(cs.bufs), offset=32).reshape(-1, 2)
    stored = table[:, 0] >= 0
    assert np.array_equal(stored, np.array(cs.stored)) and np.array_equal(table[:, 1], [b.size for b in cs.bufs])
    base = 32 + 16 * len(cs.bufs) + 8 * nf * len(cs.launches)
    assert os.path.getsize(path) == base + 4 * int(table[stored, 1].sum())
    rec = np.fromfile(path, np.int64, nf * len(cs.launches), offset=32 + 16 * len(cs.bufs)).reshape(-1, nf)
    for li in (0, len(cs.launches) // 2, len(cs.launches) - 1):
        L = cs.launches[li]
        si, sf, sb, _ = R.SLOTS[L["kernel"]]
        assert rec[li, 0] == R.KERNELS.index(L["kernel"])
        assert [rec[li, 1 + j] for j in range(len(si))] == [L["ints"][s] for s in si]
        got = rec[li, 1 + R.N_INT:1 + R.N_INT + len(sf)].astype(np.uint32).view(np.float32)
        assert np.array_equal(got, np.array([L["flts"][s] for s in sf], np.float32))
        assert [rec[li, 1 + R.N_INT + R.N_FLT + j] for j in range(len(sb))] == [L["bufs"][s] for s in sb]
    n = int(np.flatnonzero(stored)[7])
    got = np.fromfile(path, np.float32, int(table[n, 1]), offset=base + 4 * int(table[n, 0]))
    assert np.array_equal(got.view(np.uint32), cs.bufs[n].view(np.uint32))
    assert all(R.is_canary(cs.bufs[i]).all() for i in np.flatnonzero(~stored))
    assert all(R.is_canary(b[:R.GUARD]).all() and R.is_canary(b[-R.GUARD:]).all() for b in cs.bufs)
    # a result file as the driver writes it
    outs = [i for i, s in enumerate(cs.stored) if not s]
    res = tmp_path / "results.bin"
    with open(res, "wb") as fh:
        np.array([R.MAGIC_RESULTS, len(outs), len(cs.launches), 1234], np.int64).tofile(fh)
        for i in outs:
            cs.bufs[i].tofile(fh)
    got, wall = R.read_results(res, cs)
    assert sorted(got) == outs and wall == pytest.approx(1234e-6) and all(R.is_canary(v).all() for v in got.values())


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_driver_cross_compiles():
    r = subprocess.run(["make", "-C", R.CSRC, "-j16", "samplecheck", "ARCH=gfx950"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(R.ROOT, "build", "samplecheck"))
