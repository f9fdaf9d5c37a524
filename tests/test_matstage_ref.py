"""tests/matstage_ref.py on the CPU: its fp64 references against oracle/spec_np.py where they compute the same thing, the case
table against the shape list, the regular family's margins (asserted on the fp64 reference: no element of the device run is
excused), the derived bounds against the float32 restatement (inside, with half to spare) and a bfloat16-cut variant
(outside), the measured floors of the sampler, the mutation guards (each plausible kernel mistake fails the checker that the
GPU test uses, on a named case), the file formats and the driver's cross-compile.  tests/test_gpu_matstage.py runs the same
cases on the device.

Measured floors of k_brdf_sample, max |float32 restatement - fp64| over a family's launches (MatCases.floors() measures them
on the machine that runs the test; the figures here are the record test_sampler_floors holds them near):
  regular  local directions 9.2e-6, global 9.1e-6, pdf / (1 + pdf) 4.3e-6, MIS weight 2.1e-5, mixture pdf 7.8e-7
  edges    local 1.5e-6, global 1.9e-6, pdf 3.5e-6, MIS weight 7.3e-6, mixture pdf 5.7e-7
(the regular family's worst lanes are vMF samples of a lobe with kappa near 1e-2: w = 1 + log(arg) / kappa carries the ulp
of arg a hundredfold)."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import matstage_ref as M
from oracle import spec_np as spec

RECORDED = {("regular", "local"): 9.2e-6, ("regular", "global"): 9.1e-6, ("regular", "pdf"): 4.3e-6, ("regular", "weight"): 2.1e-5,
            ("regular", "mix"): 7.8e-7, ("edges", "local"): 1.5e-6, ("edges", "global"): 1.9e-6, ("edges", "pdf"): 3.5e-6,
            ("edges", "weight"): 7.3e-6, ("edges", "mix"): 5.7e-7}


@pytest.fixture(scope="module")
def cs():
    return M.build_cases()


@pytest.fixture(scope="module")
def refs(cs):
    """Per launch: (fp64 reference, float32 restatement, what the device is held to, its tolerances), computed once."""
    out = []
    for li in range(len(cs.launches)):
        ref, tol = M.expected(cs, li)
        out.append((M.reference(cs, li), M.reference(cs, li, np.float32), ref, tol))
    return out


def _by(cs, kernel):
    return [(li, L) for li, L in enumerate(cs.launches) if L["kernel"] == kernel]


def _val(cs, L, slot, shape, dtype=np.float32):
    return cs.value(L["bufs"][slot]).view(dtype).reshape(shape).astype(np.float64 if dtype == np.float32 else np.int64)


def test_names_follow_the_headers():
    text = open(os.path.join(M.ROOT, "include", "rc_abi.h")).read()
    names = re.findall(r"\bRC_MOUT_([A-Z0-9_]+)\b", text[text.index("RC_MOUT_RGB = 0"):text.index("} rc_mat_output_id")])
    assert [n.lower().replace("f_0", "F_0") for n in names if n != "COUNT"] == list(M.MOUT)
    head = open(os.path.join(M.CSRC, "rc_internal.h")).read()
    for name in ("RC_MAT_CH", "RC_VMF_CH", "RC_SMP_CH"):
        assert f"enum {{ {name} = 5 }}" in head
    assert (M.MAT_CH, M.VMF_CH, M.SMP_CH) == (5, 5, 5)
    assert len(M.SLOTS["integrate"][2]) <= M.N_BUF and all(len(s[0]) <= M.N_INT and len(s[1]) <= M.N_FLT for s in M.SLOTS.values())


def test_reference_agrees_with_spec_np(cs, refs, monkeypatch):
    rng = np.random.default_rng(5)
    f64 = np.float64
    # tangent_frame, to_local, to_global
    n = M._unit(rng.normal(size=(64, 3)))
    n = n[np.abs(np.abs(n[:, 2]) - 0.9) > 1e-3]
    fr, want = M.make_frame(f64, n), spec.tangent_frame(n)
    assert all(np.abs(a - b).max() <= 1e-14 for a, b in zip(fr, want))
    assert {bool(v) for v in np.abs(n[:, 2]) < 0.9} == {True, False}
    d = rng.normal(size=n.shape)
    assert np.abs(M.to_local(d, fr) - spec.to_local(d, want)).max() <= 1e-14
    assert np.abs(M.to_global(d, fr) - spec.to_global(d, want)).max() <= 1e-14
    # ggx_ndf, vmf_density, mixture_pdf
    c, a = rng.uniform(0, 1, size=50), rng.uniform(0.05, 1, size=50)
    assert np.allclose(M.ggx_d(f64, c, a), spec.ggx_ndf(c, a), rtol=1e-14, atol=0)
    mu = M._unit(rng.normal(size=(4, 128, 3)))
    kap = np.exp(rng.uniform(np.log(1e-2), np.log(49), size=(4, 128)))
    kap[:, 3], kap[:, 77] = 0.0, M.EPS
    lg = rng.uniform(-3, 3, size=(4, 128))
    e = np.exp(lg - lg.max(-1, keepdims=True))
    vmf = np.concatenate([mu, kap[..., None], (e / e.sum(-1, keepdims=True))[..., None]], axis=-1)
    gd = M._unit(rng.normal(size=(4, 9, 3)))
    assert np.allclose(M.mixture(f64, gd, vmf), spec.mixture_pdf(gd, (mu, kap, lg)), rtol=1e-12, atol=0)
    one = np.concatenate([mu[:, :1], kap[:, :1, None], np.ones((4, 1, 1))], axis=-1)
    one = np.concatenate([one, np.zeros((4, 127, 5))], axis=1)
    one[:, 1:, 3] = 1.0
    assert np.allclose(M.mixture(f64, gd, one), spec.vmf_density(gd, mu[:, :1], kap[:, :1]), rtol=1e-12, atol=0)
    # brdf_lobe and mc_estimate through k_material_integrate's reference (filt_weight 1, bg 0)
    seen = 0
    for li, L in _by(cs, "integrate"):
        if not (L["name"].startswith("integrate/all/") or L["name"].startswith("edges/integrate")):
            continue
        i, f = L["ints"], L["flts"]
        nn, Ks, Kd, S = i["n"], i["Ks"], i["Kd"], i["S"]
        K = Ks + Kd
        arr = {k: cs.value(L["bufs"][k]) for k in M.SLOTS["integrate"][2][:11]}
        arr["filt_weight"] = np.ones(nn, np.float32)
        arr["lights"] = None
        got = M.material_integrate(f64, Ks, Kd, S, arr, dict(f, bg=0.0))
        mat = arr["mat"].reshape(nn, 5).astype(f64)
        m = dict(albedo=mat[:, 0:3], roughness=mat[:, 3:4], metalness=mat[:, 4:5], F_0=np.full((nn, 1), f["f0"]))
        smp = arr["samples"].reshape(nn, K, 5).astype(f64)
        wo = np.broadcast_to(arr["local_view"].reshape(nn, 1, 3).astype(f64), (nn, K, 3))
        blk = lambda v, c_: (v[:nn * Ks].reshape(nn, Ks, c_), v[nn * Ks:].reshape(nn, Kd, c_))
        rgb, acc, env = (blk(arr[k].astype(f64).reshape(nn * K, c_), c_) for k, c_ in (("sec_rgb", 3), ("sec_acc", 1), ("sec_env", 3)))
        for j, (kind, sl) in enumerate((("specular", slice(0, Ks)), ("diffuse", slice(Ks, K)))):
            wi = smp[:, sl, 0:3]
            lobe = spec.brdf_lobe(wi, wo[:, sl], m, kind)
            rad = np.maximum(spec.nan0(rgb[j]), 0.0)
            with np.errstate(invalid="ignore"):
                en = np.nan_to_num(np.maximum(env[j], 0.0) * (1.0 - acc[j]), nan=0.0)
            ind, irr_i = spec.mc_estimate(rad, lobe, wi, smp[:, sl, 3:4], smp[:, sl, 4:5], f["rgb_max"])
            dr, irr_d = spec.mc_estimate(en, lobe, wi, smp[:, sl, 3:4], smp[:, sl, 4:5], f["rgb_max"])
            assert np.allclose(got[f"out_indirect_{kind}_rgb"], ind, rtol=1e-11, atol=1e-14), (L["name"], kind)
            assert np.allclose(got[f"out_direct_{kind}_rgb"], dr, rtol=1e-11, atol=1e-14), (L["name"], kind)
            if kind == "diffuse":
                assert np.allclose(got["out_lighting_irradiance"], 0.5 * (irr_i + irr_d), rtol=1e-11, atol=1e-14), L["name"]
        seen += 1
    assert seen == len(M.SPLITS) + 3
    # material_params and light_lobes from the grid features on (the hash encoding and the contraction are not these kernels')
    feats = {}
    monkeypatch.setattr(spec, "hash_encoding", lambda w, prefix, g, x, **kw: feats[prefix.rsplit("/", 1)[-1]])
    monkeypatch.setattr(spec, "contract", lambda x, radius: x)
    W = M._weights(np.random.default_rng(M.build_cases.__defaults__[0]))
    w = {}
    for path, k, shape in (("MaterialShader/bottleneck_layer", "0", (32, 128)), ("MaterialShader/pred_brdf_layer", "1", (128, 10))):
        w[f"params/{path}/kernel"], w[f"params/{path}/bias"] = W["w" + k].reshape(shape), W["b" + k]
    for path, k, shape in (("LightSampler/layers_0", "0", (32, 64)), ("LightSampler/layers_1", "1", (64, 64)),
                           ("LightSampler/output_layer", "2", (64, 640))):
        w[f"params/{path}/kernel"], w[f"params/{path}/bias"] = W["l_w" + k].reshape(shape), W["l_b" + k]
    cfg = types.SimpleNamespace(material_grid=None, light_grid=None, contract_radius=1.0, min_roughness=0.25, default_F_0=0.04,
                                num_vmf=128, vmf_scale=2.0)
    feat, pts, nz = M._lhead_inputs(rng, 6, W)
    feats["material_grid"] = feats["light_grid"] = feat.astype(f64)
    mine = M.material_head(f64, feat, W["w0"], W["b0"], W["w1"], W["b1"], 0.25)["mat"]
    want = spec.material_params(w, cfg, pts.astype(f64))
    assert np.allclose(mine, np.concatenate([want["albedo"], want["roughness"], want["metalness"]], axis=-1), rtol=1e-12, atol=0)
    mine = M.light_head(f64, feat, W["l_w0"], W["l_b0"], W["l_w1"], W["l_b1"], W["l_w2"], W["l_b2"], pts, nz, 2.0)
    mean, kappa, logit = spec.light_lobes(w, cfg, pts.astype(f64), nz)
    assert np.allclose(mine["vmf"][..., 0:3], mean, rtol=1e-11, atol=1e-13) and np.allclose(mine["vmf"][..., 3], kappa, rtol=1e-12)
    assert np.allclose(mine["vmf_logit"], logit, rtol=1e-12, atol=1e-13)
    e = np.exp(logit - logit.max(-1, keepdims=True))
    assert np.allclose(mine["vmf"][..., 4], e / e.sum(-1, keepdims=True), rtol=1e-12, atol=0)


def test_cases_cover_the_shape_list(cs):
    sm, ig = [L for _, L in _by(cs, "sample")], [L for _, L in _by(cs, "integrate")]
    for Ls in (sm, ig):
        assert {L["ints"]["n"] for L in Ls} == set(M.RAYS)
    assert {(L["ints"]["Ks"], L["ints"]["Kd"], L["ints"]["Kc"]) for L in sm} == set(M.SPLITS)
    assert {(L["ints"]["Ks"], L["ints"]["Kd"]) for L in ig} == {s[:2] for s in M.SPLITS}
    assert {L["ints"]["S"] for L in ig} == set(M.S_INTEGRATE)
    assert any(L["ints"]["Ks"] + L["ints"]["Kd"] == 64 for L in sm) and any(L["ints"]["Ks"] + L["ints"]["Kd"] == 3 for L in sm)
    cp = [L for _, L in _by(cs, "composite")]
    assert {L["ints"]["S"] for L in cp} == set(M.S_COMPOSITE) and {L["ints"]["n"] for L in cp} == set(M.N_COMPOSITE)
    mh = [L for _, L in _by(cs, "mhead")]
    assert set(M.RAYS) | {8211} <= {L["ints"]["n"] for L in mh} and {L["flts"]["min_roughness"] for L in mh} == {0.0, 0.25}
    assert set(M.RAYS) <= {L["ints"]["n"] for _, L in _by(cs, "lhead")}
    hd = {(L["ints"]["n"], L["ints"]["ln"]) for _, L in _by(cs, "heads")}
    assert {(m, l_) for m in (1, 3, 4, 5) for l_ in (1, 2)} | {(3, 0), (0, 2)} <= hd
    # every optional pointer null in one launch and set in another
    for key in ("lights", "vmf_lobe", "vmf_lobe_gumbel"):
        assert any(L["bufs"][key] < 0 for L in sm) and any(L["bufs"][key] >= 0 for L in sm), key
    assert all((L["bufs"]["vmf_lobe"] < 0) == (L["bufs"]["vmf_lobe_gumbel"] >= 0) for L in sm)
    for key in ("lights",) + tuple("out_" + k for k in M.MOUT):
        assert any(L["bufs"][key] < 0 for L in ig) and any(L["bufs"][key] >= 0 for L in ig), key
    for key in M.SLOTS["composite"][3]:
        assert any(L["bufs"][key] < 0 for L in cp) and any(L["bufs"][key] >= 0 for L in cp), key
    # a later launch reads an earlier launch's output
    assert sum(not cs.stored[L["bufs"]["vmf"]] for L in sm) == 2 and sum(not cs.stored[L["bufs"]["samples"]] for L in ig) >= 60


def test_regular_family_holds_its_margins(cs, refs):
    """Asserted on the fp64 reference, so the conditions hold without the device: every branch of the regular family is away
    from its threshold, and no element is excused."""
    seen, lead = 0, []
    for li, L in _by(cs, "sample"):
        if L["family"] != "regular":
            continue
        m = refs[li][0]["_margins"]
        assert M.margins_hold(m), (L["name"], m)
        assert m["wo.n"] >= 0.05 and m["wo.h"] >= 0.02 and m["wi+wo"] >= 0.1 and m["z"] >= 1e-3 and m["mis"] >= 1e-3
        assert m["u1"] <= 1 - 1e-3 and 1e-2 <= m["kappa_lo"] and m["kappa_hi"] < 50 and m["nz"] >= 1e-3 and m["mean_z"] >= 1e-2
        if L["bufs"]["vmf_lobe"] < 0:
            assert 2e-3 <= m["lead"], (L["name"], m["lead"])
            lead.append(m["lead"])
            assert np.array_equal(refs[li][0]["_lobe"], L["winner"]), L["name"]
        seen += 1
    assert seen == 2 * len(M.SPLITS) + 6 and min(lead) < 3e-3
    for li, L in _by(cs, "integrate"):
        if L["family"] == "regular":
            assert np.abs(refs[li][0]["_z"]).min() >= 1e-3, L["name"]
    for li, L in _by(cs, "lhead") + _by(cs, "heads"):
        if "_mnorm" in refs[li][0]:
            assert refs[li][0]["_mnorm"].min() >= 0.1, L["name"]


def test_both_precisions_take_the_same_side(cs, refs):
    """Every sampler launch, the edge family included: the fp64 reference and the float32 restatement agree on the sign of
    every local z, on wn <= 0, on the drawn lobe, and so on where pdf and weight are exactly 0."""
    for li, L in _by(cs, "sample"):
        r64, r32 = refs[li][0], refs[li][1]
        if L["family"] != "illcond":
            assert np.array_equal(r64["samples"][..., 2] > 0, r32["samples"][..., 2] > 0), L["name"]
            assert np.array_equal(r64["samples"][..., 3:] == 0, r32["samples"][..., 3:] == 0), L["name"]
        assert np.array_equal(r64["_wn"] <= 0, r32["_wn"] <= 0), L["name"]
        assert np.array_equal(r64["_lobe"], r32["_lobe"]), L["name"]
        assert np.isfinite(r32["samples"]).all() and np.isfinite(r32["sec_dirs"]).all(), L["name"]


def test_edge_cases_reach_their_clamps(cs, refs):
    by_name = {L["name"]: li for li, L in enumerate(cs.launches)}
    r = refs[by_name["edges/sample"]][0]
    smp = r["samples"]
    assert (smp[0, :4, 3] == 0).all() and (smp[1, :4, 3] == 0).any()        # view along -n, view in the tangent plane: wn <= 0
    assert np.allclose(smp[:, 4, 2], np.sqrt(1e-5), rtol=1e-12)              # the cosine lane with u1 = 1
    assert (smp[6, 6:, 2] < 0).all() and (smp[6, 6:, 4] == 0).all()          # every vMF sample below the surface: weight 0
    assert (smp[8, 6:, 2] < 0).all() and (smp[7, 6:, 2] > 0).all()           # lobe means (0, 0, -1) and (0, 0, 1)
    L = cs.launches[by_name["edges/sample"]]
    nz = _val(cs, L, "nrm", (9, 3))[2:5, 2]
    f9 = np.float32(0.9)
    assert list(nz) == [float(f9), float(np.nextafter(f9, np.float32(0))), float(np.nextafter(f9, np.float32(1)))]
    d = refs[by_name["edges/lobe/drawn"]][0]
    assert list(d["_lobe"][:5]) == [17, 3, 0, 101, 20]
    key = d["_key"]
    assert key[0, 17] == key[0, 81] == key[0].max() and key[1, 3] == key[1, 40] == key[1].max() and (key[2] == key[2, 0]).all()
    ill = refs[by_name["illcond/sample"]]
    assert np.abs(ill[1]["samples"][:, 6:, :3].astype(np.float64) - ill[0]["samples"][:, 6:, :3]).max() >= 0.1   # fp64 is not the contract
    assert ill[2]["samples"].dtype == np.float64 and np.array_equal(ill[2]["samples"].astype(np.float32), ill[1]["samples"])
    for name in ("clip", "noclip"):
        li = by_name["edges/integrate/" + name]
        r = refs[li][0]
        assert np.isfinite(np.concatenate([np.ravel(v) for k, v in r.items() if k.startswith("out_")])).all()
        assert (r["out_indirect_diffuse_rgb"][3] == 0).all() and (r["out_direct_diffuse_rgb"][3] == 0).all()   # every z <= 0
        assert (refs[li][3]["out_indirect_diffuse_rgb"][3] == 0).all()                                      # held exactly
        assert (r["out_specular_rgb"][4] == 0).all() and (r["out_rgb"][4] != 0).all()                     # filt_weight 0: bg only
    r, tol = refs[by_name["edges/integrate/below"]][0], refs[by_name["edges/integrate/below"]][3]
    for k in ("diffuse_rgb", "direct_diffuse_rgb", "indirect_diffuse_rgb", "lighting_irradiance"):
        assert (r["out_" + k] == 0).all() and (tol["out_" + k] == 0).all(), k     # the whole launch: exactly zero, held exactly
    assert (r["out_specular_rgb"] > 0).any()
    a, b = (refs[by_name["edges/integrate/" + k]][0]["out_indirect_rgb"] for k in ("clip", "noclip"))
    assert (a < b).any()                                                                                  # rgb_max clips
    for name, what in (("lhead/clamps", None), ("lhead/equal_logits", None)):
        r = refs[by_name[name]]
        if name == "lhead/clamps":
            assert (r[0]["vmf"][:, ::2, 3] == 50.0).all() and (r[0]["vmf_logit"][:, ::2] == -50.0).all()
            assert (r[3]["vmf"][:, ::2, 3] == 0).all() and (r[3]["vmf_logit"][:, ::2] == 0).all()           # held exactly
            assert (r[0]["vmf"][:, 1::2, 3] < 50.0).all() and (r[3]["vmf"][:, 1::2, 3] > 0).all()
        else:
            assert (r[1]["vmf"][..., 4] == np.float32(1.0 / 128)).all()


def test_sampler_floors(cs):
    """The floors are measured on this machine's numpy (MatCases.floors()), so the figures in the docstrings are a record, not
    a constant: 4 x floor stays within the 1e-4 the oracle tests hold (RGB_TOL), and the floors are the size they were
    recorded at (within a factor of 2: another build of numpy may round its float32 exp, log, sin and cos differently)."""
    floors = cs.floors()
    print("measured floors", floors)
    assert set(floors) == set(RECORDED) == {(f, q) for f in M.FAMILIES for q in M.QUANTITIES}
    for key, v in floors.items():
        assert 0 < 4 * v <= 1e-4, (key, v)
        assert 0.5 * RECORDED[key] <= v <= 2 * RECORDED[key], (key, v)


def test_bounds_hold_the_float32_restatement(cs, refs):
    worst = {}
    for li, L in enumerate(cs.launches):
        r64, r32, ref, tol = refs[li]
        bad, ratio = M.check(cs, li, M.render(cs, li, r32), ref, tol)
        assert not bad, (L["name"], bad[:5])
        for slot, r in ratio.items():
            key = (L["kernel"], slot)
            worst[key] = max(worst.get(key, 0.0), r)
    derived = {k: v for k, v in worst.items() if k[0] != "sample"}           # the sampler rests on the measured floors
    print(worst)
    assert len(derived) == 1 + 2 + 3 + 4 + 16 and max(derived.values()) <= 0.5, worst
    assert max(v for k, v in worst.items() if k[0] == "sample") <= 0.25 + 1e-12


def test_bounds_reject_a_bfloat16_cut(cs, refs):
    """Both operands of every dense layer rounded to bfloat16: every output of every head launch leaves its bound
    (the bound is the worst case of 2 (K + 2) u sum |a| |b| through three layers, so the factor is 2.6 at the least and 6
    in the median, not the 2^15 between the two formats)."""
    worst = []
    for li, L in enumerate(cs.launches):
        if L["kernel"] not in ("mhead", "lhead", "heads"):
            continue
        r64, _, _, tol = refs[li]
        cut, cut64 = M.reference(cs, li, np.float32, cut=True), M.reference(cs, li, np.float64, cut=True)
        for slot in ("mat", "vmf", "vmf_logit"):
            if slot not in r64 or np.array_equal(cut64[slot], r64[slot]):  # (equal logits from a zero column: nothing to cut)
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(tol[slot] > 0, np.abs(cut[slot].astype(np.float64) - r64[slot]) / tol[slot], 0.0)
            assert r.max() > 1, (L["name"], slot, r.max())
            worst.append(r.max())
    print(sorted(worst)[:5], np.median(worst))
    assert len(worst) == 19 + 2 * 17 + (8 * 3 + 1 + 2 + 2 * 3) - 2 and min(worst) > 1


# mutation -> {kernel it applies to: a case that has to catch it}
APPLIES = {
    "kc_off_by_one": {"sample": "sample/given/Ks4Kd4Kc2n5"},
    "diffuse_offset_rKs": {"sample": "sample/given/Ks2Kd3Kc1n3", "integrate": "integrate/all/Ks2Kd3Kc1n3S31"},
    "mis_no_2": {"sample": "sample/given/Ks1Kd2Kc1n1"},
    "mis_light_pdf_local": {"sample": "sample/given/Ks16Kd16Kc8n3"},
    "weight_not_zeroed": {"sample": "edges/sample"},                 # (in k_material_integrate the lobes vanish at z <= 0 anyway)
    "wn_not_zeroing": {"sample": "edges/sample"},
    "tie_high": {"sample": "edges/lobe/drawn"},
    "argmax_log_softmax": {"sample": "edges/lobe/drawn"},
    "mixture_upper_half_dropped": {"sample": "sample/given/Ks32Kd32Kc16n4"},
    "sinh_neighbour": {"sample": "sample/given/Ks1Kd63Kc32n5"},
    "softmax_max_not_subtracted": {"lhead": "lhead/large_logits"},
    "rough_metal_swapped": {"mhead": "mhead/n1"},
    "min_roughness_not_squared": {"mhead": "mhead/n3"},
    "mean_over_K": {"integrate": "integrate/all/Ks61Kd3Kc1n9S33"},
    "lane63_dropped": {"integrate": "integrate/S64"},
    "bg_filtered_acc": {"integrate": "integrate/S1"},
    "occ_scale_missing": {"integrate": "integrate/all/Ks1Kd2Kc1n1S1"},
    "tail_wave_store": {"sample": "sample/lastray/n5", "integrate": "integrate/lastray/n9"},
}


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_mutation_is_caught(cs, refs, mutation):
    """A device with this mistake (its float32 arithmetic otherwise the restatement's) fails M.check on the named launch of
    EVERY kernel the mistake applies to."""
    assert set(APPLIES) == set(M.MUTATIONS)
    caught = {k: [] for k in APPLIES[mutation]}
    for li, L in enumerate(cs.launches):
        if L["kernel"] not in APPLIES[mutation]:
            continue
        _, _, ref, tol = refs[li]
        bad, _ = M.check(cs, li, M.render(cs, li, M.reference(cs, li, np.float32, mutation), mutation), ref, tol)
        if bad:
            caught[L["kernel"]].append(L["name"])
    print(mutation, "caught on", {k: (len(v), v[:3]) for k, v in caught.items()})
    for kernel, name in APPLIES[mutation].items():
        assert name in caught[kernel], (mutation, kernel, name, caught[kernel][:10])


def test_case_file_round_trip(cs, tmp_path):
    path = tmp_path / "cases.bin"
    M.write_case_file(path, cs)
    nf = 1 + M.N_INT + M.N_FLT + M.N_BUF
    head = np.fromfile(path, np.int64, 4)
    assert list(head) == [M.MAGIC_CASES, len(cs.bufs), len(cs.launches), nf] and M.MAGIC_CASES != M.R.MAGIC_CASES
    rec = np.fromfile(path, np.int64, nf * len(cs.launches), offset=32 + 16 * len(cs.bufs)).reshape(-1, nf)
    for li in (0, len(cs.launches) // 2, len(cs.launches) - 1):
        L = cs.launches[li]
        si, sf, sb, _ = M.SLOTS[L["kernel"]]
        assert rec[li, 0] == M.KERNELS.index(L["kernel"])
        assert [rec[li, 1 + j] for j in range(len(si))] == [L["ints"][s] for s in si]
        got = rec[li, 1 + M.N_INT:1 + M.N_INT + len(sf)].astype(np.uint32).view(np.float32)
        assert np.array_equal(got, np.array([L["flts"][s] for s in sf], np.float32))
        assert [rec[li, 1 + M.N_INT + M.N_FLT + j] for j in range(len(sb))] == [L["bufs"][s] for s in sb]
    assert all(M.is_canary(b[:M.GUARD]).all() and M.is_canary(b[-M.GUARD:]).all() for b in cs.bufs)
    outs = [i for i, s in enumerate(cs.stored) if not s]
    res = tmp_path / "results.bin"
    with open(res, "wb") as fh:
        np.array([M.MAGIC_RESULTS, len(outs), len(cs.launches), 1234], np.int64).tofile(fh)
        for i in outs:
            cs.bufs[i].tofile(fh)
    got, wall = M.read_results(res, cs)
    assert sorted(got) == outs and wall == pytest.approx(1234e-6) and all(M.is_canary(v).all() for v in got.values())


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_driver_cross_compiles():
    r = subprocess.run(["make", "-C", M.CSRC, "-j16", "matstagecheck", "ARCH=gfx950"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(M.ROOT, "build", "matstagecheck"))
