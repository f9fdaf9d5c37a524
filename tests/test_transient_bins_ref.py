"""The CPU side of tests/test_gpu_transient_bins.py: the references, cases and tolerances of tests/transient_bins_ref.py
checked against each other and against the project's independent oracle, and shown to bite.

  * the float32 restatement of every launch stays inside the bounds derived for the fp32 build (the tighter of the two);
  * no float32 decision of any case is a near tie; the backward cases keep every pre-clamp value clear of rgb_max;
  * on the cornell settings the restatement agrees with oracle/transient_ref.py (zero_invalid_bins, shift_map_coordinates,
    shift_direct, gauss_filter) and with scipy.signal.convolve(mode="same") for every tap count used;
  * the case table holds what the families promise (windows, exposures, thresholds, tap counts, ray counts, chunks);
  * each mutated reference leaves the tolerance (of the looser, split-form build) on a launch of the family meant to catch
    it."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal
import torch

import nrc_amd
import transient_bins_ref as M
from oracle import transient_ref

B, S = M.BINS, M.S


@pytest.fixture(scope="module")
def cs():
    return M.build_cases()


def _check(cs, li, ref_out, c):
    ref, tol = M.expected(cs, li, c=c)
    return M.check(cs, li, M.render(cs, li, ref_out), ref, tol)


def test_float32_restatement_is_inside_the_bounds(cs):
    allow = cs.softplus_allowance()
    print(f"\nsoftplus_bins: max |float32 form - fp64| / (1 + fp64) = {allow:.3e} over {len(cs.scenes)} scenes -> the device's "
          f"allowance 4 x = {4 * allow:.3e}; the head bound beside it: c_f32(129) = {M.c_f32(M.K_SLF):.3e}, c_split(129) = "
          f"{M.c_split(M.K_SLF):.3e} of sum |x w|")
    assert 2.0 ** -26 < allow < 2.0 ** -21         # an ulp or so of a value of 1: a measurement, not a guess
    worst = {}
    for li, L in enumerate(cs.launches):
        bad, ratio = _check(cs, li, M.reference(cs, li, np.float32), M.c_f32)
        assert not bad, (L["name"], L["kernel"], bad[:5])
        for s, r in ratio.items():
            worst[(L["kernel"], s)] = max(worst.get((L["kernel"], s), 0.0), r)
    for k, r in sorted(worst.items()):
        print(f"{k[0]:9s} {k[1]:28s} float32 restatement: worst error / tolerance = {r:.4f}")
    # the bounds are no formality: the restatement uses a fair share of them somewhere in every kernel
    for kernel in M.KERNELS:
        assert max(r for (k, _), r in worst.items() if k == kernel) > 0.1, kernel


def test_no_decision_is_a_near_tie(cs):
    for sc in cs.scenes:
        assert M.near_ties(sc) == 0
    ties = 0
    for sc in cs.scenes:                             # the exact ties the cases do hold: float32 and fp64 agree on them
        D = M.decisions(sc)
        ties += int((D["low"] == D["high"]).sum())
    assert ties >= 96 + 4 * 32                       # direct/integral's 96 samples, the tied half of the four dyadic compare cases
    bwd = [L for L in cs.launches if L["kernel"] == "bins_bwd"]
    assert len(bwd) == 20
    for sc in {id(L["scene"]): L["scene"] for L in bwd}.values():
        assert M.clamp_margin(sc) > 0.0


def test_layout_of_the_activations():
    """layout_feat against the inverse k_transient_bins_bwd applies (x_slf / x_irr in reference column order): step s, half h
    of sample j holds column 32 (s >> 4) + (s & 3) + 8 ((s & 15) >> 2) + 4 h."""
    rng = np.random.default_rng(3)
    for F in (128, 64):
        x = rng.normal(size=(2, S, F)).astype(np.float32)
        f = M.layout_feat(x)
        assert f.shape == (2, F // 2, 64)
        back = np.zeros_like(x)
        for s in range(F // 2):
            for lane in range(64):
                back[:, lane & 31, 32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2) + 4 * (lane >> 5)] = f[:, s, lane]
        assert np.array_equal(back, x)


def _cornell_scene(rng, n=3):
    """Random geometry at the cornell settings; light_dist, cam_dist and ray_dist are the oracle's own float32 norms."""
    cfg = nrc_amd.cornell_transient_config()
    t = cfg.transient
    means = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, S, 3)).astype(np.float32))
    rays = {"lights": torch.from_numpy(rng.uniform(-2.5, 2.5, (n, 3)).astype(np.float32)),
            "origins": torch.from_numpy(rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32))}
    rays["cam_origins"] = rays["origins"] + torch.from_numpy(rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32))
    ld = torch.linalg.norm(rays["lights"][:, None] - means, dim=-1)
    rd = torch.linalg.norm(rays["origins"][:, None] - means, dim=-1)
    cam = rd + torch.linalg.norm(rays["origins"] - rays["cam_origins"], dim=-1)[:, None]
    P = dict(M.CORNELL, max_dists=float(np.float32((t.n_bins - 1) * t.exposure_time)))
    P.pop("max_bin")
    assert (P["exposure"], P["thr"], P["light_near"], bool(P["light_zero"]), P["shift"]) == \
        (t.exposure_time, t.bin_zero_threshold_light, t.light_near, t.light_zero, t.transient_shift)
    assert (P["irradiance_bias"], P["slf_rgb_bias"], P["indirect_scale"], P["rgb_max"]) == \
        (t.irradiance_bias, t.slf_rgb_bias, t.indirect_scale, t.rgb_max)
    ts = np.zeros((M.TS_COUNT, n * S), np.float32)
    ts[M.TS_DD:M.TS_DD + 6] = rng.uniform(0.0, 0.6, (6, n * S))
    ts[M.TS_TIB:M.TS_TIB + 3] = rng.uniform(0.05, 0.95, (3, n * S))
    ts[M.TS_LDIST], ts[M.TS_RDIST], ts[M.TS_CAMDIST] = ld.numpy().ravel(), rd.numpy().ravel(), cam.numpy().ravel()
    w = rng.uniform(0.0, 0.06, (n, S)).astype(np.float32)
    ws = M.WSet(rng, 0.18)
    x_slf = np.maximum(rng.normal(0.3, 0.5, (n, S, 128)), 0.0).astype(np.float32)
    x_irr = np.maximum(rng.normal(0.3, 0.5, (n, S, 64)), 0.0).astype(np.float32)
    taps = transient_ref.gauss_filter(t.tfilter_sigma).numpy()
    return M.Scene(ws, x_slf, x_irr, ts, w, P, taps), cfg, rays, means


def test_agrees_with_the_oracle_on_the_cornell_settings():
    for seed in range(5, 25):                        # geometry without a near tie, so that the fp64 oracle decides as float32 does
        sc, cfg, rays, means = _cornell_scene(np.random.default_rng(seed))
        if M.near_ties(sc) == 0:
            break
    n = sc.n
    # zero_invalid_bins: the float32 decisions are the oracle's (the same comparisons on the same float32 numbers)
    ones = torch.ones(n, S, B, 3)
    kept, _ = transient_ref.zero_invalid_bins(cfg, rays, means, ones, ones)
    keep = M.decisions(sc)["keep"]
    assert np.array_equal(kept[..., 0].numpy() != 0, keep) and 0.02 < keep.mean() < 0.98
    assert M.near_ties(sc) == 0                    # (so the fp64 oracle decides the same way)
    with torch.no_grad():
        r = M.forward(sc)
    # shift_map_coordinates on the per-sample histograms, fp64
    val = r["_val"].reshape(n * S, B, 3)
    move = torch.from_numpy(sc.ts(M.TS_RDIST).astype(np.float64).ravel()) + float(np.float32(sc.P["shift"]))
    ind = transient_ref.shift_map_coordinates(val, move, float(np.float32(sc.P["exposure"])), B).reshape(n, S, B, 3).sum(1)
    assert float(ind.abs().max()) > 1e-4 and torch.allclose(ind, r["out_indirect"], rtol=1e-12, atol=1e-15)
    # the scatter form the mutated references are built on: the same sum, with the float32 d in its weights (an ulp of d <= 700)
    assert np.allclose(M.shift_scatter(sc, r["_val"].numpy()), r["out_indirect"].numpy(), rtol=0, atol=1e-4 * float(ind.abs().max()))
    # shift_direct, then the temporal filter as the oracle's integrator applies it
    d = r["_d_dir"]
    assert float(d.min()) >= 0 and float(d.max()) < 2 * B and float(d.max()) > B      # a spill, nothing beyond the next ray
    dh = transient_ref.shift_direct(d, r["_direct"], r["_w"], B)
    assert torch.allclose(dh, r["_dh"], rtol=1e-12, atol=1e-15) and float(dh[1:, :40].abs().max()) > 0
    f = transient_ref.gauss_filter(cfg.transient.tfilter_sigma).to(torch.float64)
    half = (f.numel() - 1) // 2
    y = torch.nn.functional.conv1d(dh.permute(0, 2, 1).reshape(n * 3, 1, B), torch.flip(f, [0]).reshape(1, 1, -1), padding=half)
    assert torch.allclose(y.reshape(n, 3, B).permute(0, 2, 1), r["out_direct"], rtol=1e-10, atol=1e-14)
    assert np.array_equal(M._gauss(3.0).view(np.uint32), transient_ref.gauss_filter(3.0).numpy().view(np.uint32)) or \
        np.allclose(M._gauss(3.0), transient_ref.gauss_filter(3.0).numpy(), rtol=3e-7, atol=0)
    # the slice of the trainer's light-in-flight frame
    t = np.array([0.0, 166.5, 699.0, 12.25], np.float32)
    h = r["out_rgb"].numpy()
    for i, tt in enumerate(t):
        lo, hi, w = int(np.floor(tt)), int(np.ceil(tt)), float(tt) - np.floor(tt)
        assert np.allclose(M.slice_of(h, t)[:, i], w * h[:, hi] + (1 - w) * h[:, lo], rtol=0, atol=0)


def test_filter_is_scipy_convolve_same(cs):
    """conv_same = scipy.signal.convolve(x, taps[None, :, None], mode="same") for every tap vector of the cases (asymmetric;
    odd and even counts) and an even count of four."""
    rng = np.random.default_rng(7)
    x = rng.normal(size=(2, B, 3))
    x[:, 20:680] = 0.0                               # energy at both ends: the zero padding is what is read
    seen = set()
    for taps in [sc.taps for sc in cs.scenes if sc.taps is not None] + [np.array([0.4, 0.3, 0.2, 0.1], np.float32)]:
        t64 = taps.astype(np.float64)
        want = scipy.signal.convolve(x, t64[None, :, None], mode="same")
        assert np.allclose(M.conv_same(torch.from_numpy(x), t64).numpy(), want, rtol=1e-12, atol=1e-15)
        seen.add(len(taps))
        if len(taps) != 25 or not np.array_equal(taps, taps[::-1]):
            assert not np.allclose(M.conv_same(torch.from_numpy(x), t64, "taps_reversed").numpy(), want, atol=1e-6)
    assert seen == {3, 4, 25, 31, 32, 33, 49}


def test_case_table_holds_what_the_families_promise(cs):
    bins = [L for L in cs.launches if L["kernel"] == "bins"]
    assert sorted(cs.window_specs.values()) == sorted([(0, 0), (0, 31), (31, 32), (32, 63), (33, 671), (640, 698), (699, 699), (0, 699)])
    for li, (lo, hi) in cs.window_specs.items():
        wl, wh = M.windows(M.decisions(cs.launches[li]["scene"])["keep"])
        assert wl.min() == lo and wh.max() == hi and ((wl == lo) & (wh == hi)).any(1).all()
    by = {L["name"]: L for L in bins}
    wl, wh = M.windows(M.decisions(by["window/empty_workgroup"]["scene"])["keep"])
    assert (wl[:4] > wh[:4]).all() and (wl[4] <= wh[4]).any()
    wl, wh = M.windows(M.decisions(by["window/empty_ray"]["scene"])["keep"])
    assert (wl[2] > wh[2]).all() and all((wl[r] <= wh[r]).any() for r in (0, 1, 3))
    wl, wh = M.windows(M.decisions(by["window/disjoint"]["scene"])["keep"])
    assert (wl[0].min(), wh[0].max(), wl[1].min(), wh[1].max()) == (5, 20, 600, 690) and (wl[2:] > wh[2:]).all()
    cmp_ = [L for L in bins if L["family"] == "compare"]
    assert {(round(L["flts"]["exposure"], 6), L["ints"]["bin_zero_threshold_light"]) for L in cmp_} >= \
        {(round(float(np.float32(e)), 6), t) for e in (2.0 ** -7, 0.01, 0.037) for t in (0, 1, 100, 699)}
    sh = {L["name"]: M.decisions(L["scene"]) for L in bins if L["family"] == "shift"}
    assert (sh["shift/below"]["d_ind"] < 0).all() and (sh["shift/past"]["d_ind"] > B).all()
    below = by["shift/below"]["scene"]
    assert -below.P["shift"] > below.ts(M.TS_RDIST).max() and M.windows(sh["shift/below"]["keep"])[1].max() == B - 1
    for k in ("shift/zero", "shift/int+", "shift/int-"):
        assert (sh[k]["d_ind"] == np.round(sh[k]["d_ind"])).all()
    assert (sh["shift/int-"]["d_ind"] < 0).any() and (sh["shift/frac-"]["d_ind"] < 0).any()
    assert (np.ptp(sh["shift/coincide"]["d_ind"], axis=1) == 0).all()
    dr = {L["name"]: M.decisions(L["scene"]) for L in bins if L["family"] == "direct"}
    assert (dr["direct/spill"]["low"] >= B).any() and (dr["direct/spill"]["low"] < B).any() and (dr["direct/spill"]["high"] < 2 * B).all()
    assert by["direct/spill/one_ray"]["ints"]["n_rays"] == 1
    assert (dr["direct/integral"]["low"] == dr["direct/integral"]["high"]).all()
    assert (dr["direct/negative"]["high"] <= 0).all() and (dr["direct/negative"]["d_dir"] < -1).all()
    far = dr["direct/far"]["d_dir"]
    assert far.max() > 2.9e9 and far.min() < -2.9e9
    assert {L["ints"]["n_taps"] for L in bins if L["family"] == "taps"} == {0, 3, 25, 31, 32, 33, 49}
    assert sorted(L["ints"]["n_rays"] for L in bins if L["family"] == "rays") == [1, 3, 4, 5, 9]
    assert {L["ints"]["count"] for L in cs.launches if L["kernel"] == "slice"} == {1, M.TSLICE_MAX}
    for L in cs.launches:
        if L["kernel"] == "slice":
            t = L["t"]
            assert t.min() >= 0 and t.max() <= B - 1
            if len(t) == M.TSLICE_MAX:
                assert 0.0 in t and 699.0 in t and (t == np.round(t)).sum() >= 3 and (t != np.round(t)).sum() >= 3
    zw = by["flags/zero_weights"]["scene"].weights
    assert (zw[1] == 0).all() and (zw[0] == 0).any() and (zw[0] != 0).any()
    clamped = M.scene_ref(by["flags/rgb_max/wide"]["scene"])
    with torch.no_grad():
        r = M.forward(by["flags/rgb_max/wide"]["scene"])
    share = float(((r["_diff_pre"] > 0.1) & torch.from_numpy(clamped["D"]["keep"])[..., None]).float().mean())
    assert 0.1 < share < 0.9                         # rgb_max clamps a good share of the bins
    shadow = [L for L in cs.launches if L["kernel"] == "shadow"]
    assert {(L["ints"]["n"], L["ints"]["samples_per_ray"]) for L in shadow} == {(n, s) for n in (1, 255, 256, 257) for s in (1, 5, 32)}
    for L in shadow:
        if L["ints"]["n"] > 7:
            r64 = M.shadow(np.float64, L["args"])
            assert (r64["_dist"] == 0).any() and ((r64["_dist"] > 0) & (r64["_dist"] < 1e-5)).any()
            assert (r64["far"] == np.float32(0.05)).any() and (r64["far"] == 4.0).any()
    bw = [L["ints"] for L in cs.launches if L["kernel"] == "bins_bwd"]
    assert {i["n_rays"] for i in bw} >= {1, 5, 9} and any(i["C"] < i["n_rays"] and i["r0"] > 0 for i in bw)


@pytest.mark.parametrize("mut", sorted(M.MUTATIONS))
def test_mutated_reference_leaves_the_tolerance(cs, mut):
    """The mutated reference, rendered as the device would leave it, fails the check of the family meant to catch it -- under
    the looser of the two builds' bounds -- on the bins kernel or on the slices taken from it."""
    fam = M.MUTATIONS[mut]
    caught = []
    for li, L in enumerate(cs.launches):
        if L["family"] != fam or L["kernel"] not in ("bins", "slice"):
            continue
        bad, _ = _check(cs, li, M.reference(cs, li, np.float64, mut=mut), M.c_split)
        if bad:
            caught.append((L["name"], bad[0][0], bad[0][1], round(float(bad[0][2]), 2)))
    print(f"\n{mut}: caught on {len(caught)} launches of family {fam!r}, e.g. {caught[:3]}")
    assert any(k == "bins" for k in [cs.launches[i]["kernel"] for i, L in enumerate(cs.launches) if L["name"] in {c[0] for c in caught}]), mut
    if mut not in ("win_lo_off", "win_hi_off", "thr_ignored", "light_zero_ignored", "clamp_omitted", "zero_weight_contributes"):
        return
    # a mutation of what both kernels share is seen through the slices too
    assert any("/slice" in c[0] for c in caught), mut


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_driver_cross_compiles():
    """The split-form driver against the library's own objects (the fp32 one needs the objects of `make variant-f32`, which
    the GPU test builds)."""
    exe = os.path.join(M.ROOT, "build", "transientcheck")
    r = subprocess.run(["make", "-C", M.CSRC, "-j16", "../../build/transientcheck", "ARCH=gfx950"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(exe)
