"""Relighting under an explicit environment image on the GPU: rc_env_lookup, rc_env_tables and rc_env_pick
against the numpy restatement of tests/relight_ref.py, rc_render_relight against rc_render_material and against the oracle's
material stage with the image lookup (and, in RC_RELIGHT_ENV, the environment sampler) hooked in, RC_PASS_ENV_IMAGE on
secondary rays, the albedo ratio and the Python interface.

Stages with device trigonometry are held to DESIGN §6's floor rule, per channel:
    max|HIP - fp64| <= 3 max|fp32 numpy - fp64| + 5e-7 max|value|
Every figure that is asserted is printed first."""
import dataclasses

import numpy as np
import pytest
import torch

import common
import nrc_amd
import relight_ref as R
from nrc_amd import model as M
from nrc_amd import prng, rc_ext, relight
from test_gpu_mlp_floor import adversarial_dirs, floor_stats

pytestmark = pytest.mark.gpu
K_FLOOR, EPS_FLOOR = 3.0, 5e-7
TOL = 1e-4                                   # DESIGN §6's material bound
PASSES = ("cache", "light", "material")
SIZES = ((4, 8), (5, 7))
DIRECT = ("direct_rgb", "direct_diffuse_rgb", "direct_specular_rgb")
INDIRECT = ("indirect_rgb", "indirect_diffuse_rgb", "indirect_specular_rgb", "indirect_occ")
MAT_KEYS = ("rgb", "acc", "direct_rgb", "indirect_rgb", "diffuse_rgb", "specular_rgb", "direct_diffuse_rgb",
            "direct_specular_rgb", "indirect_diffuse_rgb", "indirect_specular_rgb", "indirect_occ", "lighting_irradiance",
            "material_albedo", "material_roughness", "material_metalness", "material_F_0", "means", "normals_to_use",
            "ray_dists", "light_dists")


def image(H, W, seed=0, lo=0.05, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(H, W, 3)).astype(np.float32)


def floor_check(name, hip, b32, b64, scale=None):
    err, floor, _, mx = floor_stats(hip, b32, b64, b64)
    mx = mx if scale is None else np.full_like(mx, scale)
    bound = K_FLOOR * floor + EPS_FLOOR * mx
    print(f"{name}: HIP-fp64 {err}, fp32-fp64 {floor}, ratio to the bound {err / np.maximum(bound, 1e-300)}")
    assert (err <= bound).all(), (name, err, floor, bound)


@pytest.fixture(scope="module")
def rc():
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h.load_weights(common.weights_material_np(True))
    return h


def lookup_dirs(n, seed):
    """adversarial_dirs of test_gpu_mlp_floor.py (axes = the poles of the lookup's axis -y, +-0, grazing) plus the seam phi = +-pi."""
    seam = np.asarray([(-1, 0, 0.0), (-1, 0, -0.0), (-1, 0, 1e-7), (-1, 0, -1e-7), (-0.6, 0.8, 1e-30), (-0.6, -0.8, -1e-30),
                       (-1, 1e-4, -2.0 ** -24), (-2.0 ** -24, 1, -2.0 ** -24)], np.float64)
    seam = np.where(seam == 0, seam, seam / np.linalg.norm(seam, axis=-1, keepdims=True)).astype(np.float32)
    return np.concatenate([seam, adversarial_dirs(n - len(seam), seed=seed)])


# ---------------------------------------------------------------------------------------------
# 1. lookup
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_lookup_at_the_fp32_floor(rc, H, W):
    img = image(H, W, seed=H)
    env = relight.EnvImage(rc, img)
    d = lookup_dirs(4097, seed=W)
    hip = env.lookup(d).cpu().numpy()
    floor_check(f"env lookup {H}x{W}", hip, R.lookup(img, d, np.float32), R.lookup(img, d.astype(np.float64)), scale=float(img.max()))
    # a non-finite direction: a NaN colour, RC_OK, nothing else disturbed
    bad = d[:5].copy()
    bad[1, 0], bad[3, 2] = np.nan, np.inf
    out = env.lookup(bad).cpu().numpy()
    assert np.isnan(out[1]).all() and np.isnan(out[3]).all()
    assert np.array_equal(out[[0, 2, 4]], hip[[0, 2, 4]])
    assert env.lookup(np.zeros((0, 3), np.float32)).shape == (0, 3)


# ---------------------------------------------------------------------------------------------
# 2. tables
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_tables_at_the_fp32_floor(rc, H, W):
    img = image(H, W, seed=10 + H)
    got = [t.cpu().numpy() for t in rc.env_tables(img, 2.5)]
    again = [t.cpu().numpy() for t in rc.env_tables(img, 2.5)]
    b32, b64 = R.tables(img, 2.5, np.float32), R.tables(img, 2.5)
    for name, g, a, x32, x64 in zip(("pmf", "pdf", "dirs"), got, again, b32, b64):
        assert np.array_equal(g, a), name                               # fixed-order sum: bitwise repeatable
        c = 3 if name == "dirs" else 1
        floor_check(f"env tables {H}x{W} {name}", g.reshape(-1, c), x32.reshape(-1, c), x64.reshape(-1, c))
    assert abs(float(got[0].astype(np.float64).sum()) - 1.0) <= 1e-6
    # scale multiplies rgb only: pmf is invariant up to rounding
    one = rc.env_tables(img, 1.0)[0].cpu().numpy()
    d = np.abs(one - got[0]).max()
    print(f"pmf(scale 1) - pmf(scale 2.5): {d:.3e}")
    assert d <= 4 * np.finfo(np.float32).eps * got[0].max()


# ---------------------------------------------------------------------------------------------
# 3. picks
# ---------------------------------------------------------------------------------------------
def test_picks_are_row_maxima(rc):
    env = relight.EnvImage(rc, image(5, 7, seed=0))
    pmf = env.pmf.cpu().numpy()
    same = total = 0
    for seed in (1, 2, 3):
        for T in (1, 7, 256):
            key = prng.PRNGKey(seed)
            got = env.picks(key, T).cpu().numpy()
            assert np.array_equal(got, env.picks(key, T).cpu().numpy())     # order-free maxima: bitwise repeatable
            s = R.pick_scores(key, pmf, T)
            gap = s.max(1) - s[np.arange(T), got]
            print(f"picks seed {seed} T {T}: worst gap to the host maximum {gap.max():.3e}, equal {np.mean(got == s.argmax(1)):.4f}")
            assert got.min() >= 0 and got.max() < 35 and gap.max() <= 1e-5
            if T == 256:
                same += int((got == s.argmax(1)).sum())
                total += T
    assert same >= 0.99 * total, (same, total)


def test_picks_single_texel_and_histogram(rc):
    img = np.zeros((5, 7, 3), np.float32)
    img[3, 4] = (0.2, 0.5, 0.1)
    env = relight.EnvImage(rc, img)
    for seed in range(4):
        assert (env.picks(prng.PRNGKey(seed), 256).cpu().numpy() == 3 * 7 + 4).all()
    # 256 picks x 16 keys follow pmf: chi-square at the 1e-4 level, seeds fixed
    from scipy import stats
    env = relight.EnvImage(rc, image(5, 7, seed=0))
    pmf = env.pmf.cpu().numpy().astype(np.float64)
    counts = np.zeros(35)
    for seed in range(100, 116):
        counts += np.bincount(env.picks(prng.PRNGKey(seed), 256).cpu().numpy(), minlength=35)
    expect = pmf / pmf.sum() * counts.sum()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    crit = float(stats.chi2.isf(1e-4, 34))
    print(f"chi-square {chi2:.2f} (critical {crit:.2f} at 1e-4, 34 dof), smallest expected count {expect.min():.1f}")
    assert expect.min() >= 5 and chi2 <= crit


# ---------------------------------------------------------------------------------------------
# material stage: shared inputs
# ---------------------------------------------------------------------------------------------
def stage_inputs(n):
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    return cfg, nrc_amd.synthetic_rays(n, seed=77), material_ref.draw_randoms(cfg, n, seed=3)


def np_dict(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---------------------------------------------------------------------------------------------
# 4. BRDF mode against rc_render_material
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 256])
def test_brdf_mode_against_render_material(rc, n):
    cfg, rays, rnd = stage_inputs(n)
    c0, m0 = (np_dict(t) for t in rc.render_material(rays.hot_fields(), rnd))
    e1, e2 = image(4, 8, seed=1), image(4, 8, seed=2)
    a, b = np.float32(0.75), np.float32(1.5)
    mix = (a * e1 + b * e2).astype(np.float32)
    res = {}
    for name, img in (("e1", e1), ("e2", e2), ("mix", mix), ("zero", np.zeros_like(e1))):
        relight.EnvImage(rc, img)
        c, m = rc.render_relight(rays.hot_fields(), rnd, "brdf")
        res[name] = (np_dict(c), np_dict(m))
    for name, (c, m) in res.items():
        for k in c0:                                                     # same rays, same trace
            assert np.array_equal(c[k], c0[k]), (name, k)
        for k in INDIRECT + ("acc", "means", "normals_to_use", "material_albedo", "material_roughness", "ray_dists"):
            assert np.array_equal(m[k], m0[k]), (name, k)
        assert max(float(np.abs(m[k]).max()) for k in DIRECT + ("rgb",)) < 0.5 * cfg.rgb_max      # rgb_max never clips
    z = res["zero"][1]
    for k in DIRECT:
        assert float(np.abs(z[k]).max()) == 0.0, k
    bgw = np.maximum(np.float32(0.0), np.float32(1.0) - z["acc"]) * np.float32(cfg.bg_intensity)
    assert np.array_equal(z["rgb"], z["indirect_rgb"] + bgw[:, None])
    assert float(np.abs(res["e1"][1]["direct_rgb"]).max()) > 1e-3                                  # the image is seen
    for k in DIRECT:
        want = a * res["e1"][1][k] + b * res["e2"][1][k]
        d = float(np.abs(res["mix"][1][k] - want).max())
        print(f"linearity n={n} {k}: {d:.3e} of {float(np.abs(want).max()):.3e}")
        assert d <= 2e-5 * float(np.abs(want).max()), k


# ---------------------------------------------------------------------------------------------
# 5. / 6. against the oracle's material stage with the hooks
# ---------------------------------------------------------------------------------------------
def oracle_stage(monkeypatch, img, n, dtype, rnd, samplers=None, ratio=None):
    from oracle import cache_ref, material_ref
    cfg, rays, _ = stage_inputs(n)
    monkeypatch.setattr(cache_ref, "model_env_map_rgb", lambda w, c, d: R.lookup_torch(img, d))
    if samplers is not None:
        monkeypatch.setattr(material_ref, "sample_specular", samplers[0])
        monkeypatch.setattr(material_ref, "sample_diffuse", samplers[1])
    with torch.no_grad():
        return material_ref.material_forward(common.to_torch(common.weights_material_np(True), dtype), cfg,
                                             common.rays_torch(rays, dtype), rnd)


def with_picks(rnd, ref):
    return dict(rnd, gumbel=None, spec_gumbel=None, diff_gumbel=None,
                resample_inds=ref["inds"][:, 0].numpy().astype(np.int32),
                spec_resample_inds=ref["debug"]["specular"]["inds"].numpy().astype(np.int32),
                diff_resample_inds=ref["debug"]["diffuse"]["inds"].numpy().astype(np.int32))


def check_outputs(name, mres, ref, ref64=None):
    """Every output key within TOL; a key beyond it is held to 3 x the fp32 oracle's distance from the fp64 oracle (ref64:
    a callable that computes it when needed)."""
    r = ref["render"]
    over = {}
    for k in MAT_KEYS:
        a = mres[k].cpu().numpy()
        d = float(np.abs(a - r[k].numpy().reshape(a.shape)).max())
        print(f"{name} {k}: {d:.3e}")
        if d > TOL:
            over[k] = (a, d)
    if over:
        r64 = ref64()["render"]
        for k, (a, d) in over.items():
            floor = float(np.abs(r[k].numpy().astype(np.float64) - r64[k].numpy()).max())
            d64 = float(np.abs(a - r64[k].numpy().reshape(a.shape)).max())
            print(f"{name} {k}: beyond {TOL}: HIP-fp64 {d64:.3e}, fp32-fp64 oracle {floor:.3e}, ratio {d64 / max(floor, 1e-300):.2f}")
            assert d64 <= 3.0 * floor, (name, k, d, d64, floor)


@pytest.mark.parametrize("n", [65, 256])
def test_brdf_mode_against_the_oracle(rc, monkeypatch, n):
    cfg, rays, rnd = stage_inputs(n)
    img = image(5, 7, seed=21, lo=0.0, hi=1.0)
    ref = oracle_stage(monkeypatch, img, n, torch.float32, rnd)
    rnd_p = with_picks(rnd, ref)
    relight.EnvImage(rc, img)
    cres, mres = rc.render_relight(rays.hot_fields(), rnd_p, "brdf")
    torch.cuda.synchronize()
    assert np.array_equal(rc.workspace("inds", np.int32)[:n], rnd_p["resample_inds"])
    check_outputs(f"brdf n={n}", mres, ref, lambda: oracle_stage(monkeypatch, img, n, torch.float64, dict(rnd_p, gumbel=rnd["gumbel"])))
    assert np.abs(cres["rgb"].cpu().numpy() - ref["render"]["cache_rgb"].numpy()).max() <= 1e-5


@pytest.mark.parametrize("n", [1, 65, 256])
def test_env_mode_against_the_oracle(rc, monkeypatch, n):
    cfg, rays, rnd = stage_inputs(n)
    Ks, Kd = relight.leg_counts(cfg)
    # an even height: with an odd one the tables' middle row (latitude 0) lies ON the lookup's seam phi = +-pi, where the
    # sign of a 1e-8 rounding residue picks texel column 0 or the zero padding (tests/test_relight.py pins that; DESIGN
    # "Oddities"), and no two precisions agree there
    H, W = 4, 8
    img = image(H, W, seed=22, lo=0.4, hi=1.0)
    env = relight.EnvImage(rc, img)
    pmf, pdf, dirs = (t.cpu().numpy() for t in (env.pmf, env.pdf, env.dirs))
    assert 0.02 <= pdf.min() and pdf.max() <= 5.0, (pdf.min(), pdf.max())
    Ts, Td = relight.expected_T(n, Ks), relight.expected_T(n, Kd)
    assert (Ts == 256) == (n == 256)
    ps, pd = R.picks(prng.PRNGKey(31), pmf, Ts), R.picks(prng.PRNGKey(32), pmf, Td)
    samplers = R.oracle_env_samplers(ps, pd, Ks, Kd, pdf, dirs)
    ref = oracle_stage(monkeypatch, img, n, torch.float32, rnd, samplers)
    rnd_p = with_picks(rnd, ref)
    lean = {k: v for k, v in rnd_p.items() if k not in ("spec_u1", "spec_u2", "cos_u1", "cos_u2", "vmf_noise", "vmf_lobe", "vmf_v", "vmf_tmp")}
    cres, mres = rc.render_relight(rays.hot_fields(), lean, "env", ps, pd)        # the BRDF / vMF tensors are not needed
    torch.cuda.synchronize()
    # the sampler's own outputs on the HIP path's normals: directions, pdf, weight at the floor
    K = Ks + Kd
    nrm = rc.workspace("m_nrm")[:3 * n].reshape(n, 3)
    smp = rc.workspace("sec_samples")[:n * K * 5].reshape(n, K, 5)
    sdir = rc.workspace("sec_dirs")[:3 * n * K].reshape(n * K, 3)
    for leg, picks_T, k0, k1, r0 in (("spec", ps, 0, Ks, 0), ("diff", pd, Ks, K, n * Ks)):
        Kl = k1 - k0
        l64, g64, p64, w64 = R.env_samples(nrm, picks_T, Kl, pdf, dirs, np.float64)
        l32, g32, p32, w32 = R.env_samples(nrm, picks_T, Kl, pdf, dirs, np.float32)
        floor_check(f"env n={n} {leg} local dirs", smp[:, k0:k1, :3].reshape(-1, 3), l32.reshape(-1, 3), l64.reshape(-1, 3), scale=1.0)
        floor_check(f"env n={n} {leg} traced dirs", sdir[r0:r0 + n * Kl], g32.reshape(-1, 3), g64.reshape(-1, 3), scale=1.0)
        assert np.array_equal(smp[:, k0:k1, 3], p32)                      # a table entry, max(., 0)
        clear = np.abs(l64[..., 2]) > 1e-6                                 # the horizon test away from the horizon
        assert np.array_equal(smp[:, k0:k1, 4][clear], w64[clear].astype(np.float32))
    check_outputs(f"env n={n}", mres, ref, lambda: oracle_stage(monkeypatch, img, n, torch.float64, dict(rnd_p, gumbel=rnd["gumbel"]), samplers))


# ---------------------------------------------------------------------------------------------
# 7. secondary pass
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000])
def test_secondary_pass_composites_the_image(rc, n):
    env = relight.EnvImage(rc, image(5, 7, seed=41))
    rays, rnd = common.secondary_case(n, seed=5)
    sec = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY
    out = np_dict(rc.render_rays(rays, rnd, sec | rc_ext.RC_PASS_ENV_IMAGE, outputs=["rgb", "acc", "env_map_rgb"]))
    base = np_dict(rc.render_rays(rays, rnd, sec | rc_ext.RC_PASS_NO_ENVMAP, outputs=["rgb", "acc"]))
    assert np.array_equal(out["env_map_rgb"], env.lookup(rays["viewdirs"]).cpu().numpy())
    assert np.array_equal(out["acc"], base["acc"])
    back = out["rgb"] - out["env_map_rgb"] * (np.float32(1.0) - out["acc"])[:, None]
    d = np.abs(back - base["rgb"])
    print(f"secondary n={n}: worst |rgb - env (1 - acc) - rgb_no_env| in ulps of rgb {float((d / np.spacing(np.abs(out['rgb']))).max()):.2f}")
    assert (d <= np.spacing(np.abs(out["rgb"]))).all()
    # use_env_map = False wins over the image
    both = np_dict(rc.render_rays(rays, rnd, sec | rc_ext.RC_PASS_NO_ENVMAP | rc_ext.RC_PASS_ENV_IMAGE, outputs=["rgb", "env_map_rgb"]))
    assert np.array_equal(both["rgb"], base["rgb"]) and float(np.abs(both["env_map_rgb"]).max()) == 0.0
    env.unbind()
    with pytest.raises(rc_ext.RcError, match="RC_PASS_ENV_IMAGE"):
        rc.render_rays(rays, rnd, sec | rc_ext.RC_PASS_ENV_IMAGE, outputs=["rgb"])


# ---------------------------------------------------------------------------------------------
# 8. albedo ratio
# ---------------------------------------------------------------------------------------------
def test_albedo_ratio(rc):
    n = 65
    cfg, rays, rnd = stage_inputs(n)
    S = cfg.sampling_strategy[-1][2]
    relight.EnvImage(rc, image(4, 8, seed=51))
    c0, m0 = (np_dict(t) for t in rc.render_relight(rays.hot_fields(), rnd, "brdf"))
    torch.cuda.synchronize()
    mat_all = rc.workspace("m_mat_all")[:n * S * 5].reshape(n, S, 5).astype(np.float64)      # the per-sample material, unscaled
    wts = rc.workspace("weights2")[:n * S].reshape(n, S).astype(np.float64)
    c1, m1 = (np_dict(t) for t in rc.render_relight(rays.hot_fields(), rnd, "brdf", albedo_ratio=(1.0, 1.0, 1.0)))
    for k in m0:
        assert np.array_equal(m0[k], m1[k]), k
    _, mz = rc.render_relight(rays.hot_fields(), rnd, "brdf", albedo_ratio=(0.0, 0.0, 0.0))
    assert float(mz["material_albedo"].abs().max()) == 0.0
    ratio = np.asarray([0.5, 1.7, 3.0], np.float32)
    _, mr = rc.render_relight(rays.hot_fields(), rnd, "brdf", albedo_ratio=ratio)
    want = (wts[..., None] * np.clip(mat_all[..., :3] * ratio.astype(np.float64), 0.0, 1.0)).sum(1)
    d = float(np.abs(mr["material_albedo"].cpu().numpy() - want).max())
    clipped = float((mat_all[..., :3] * ratio > 1.0).mean())
    print(f"albedo ratio: |material_albedo - sum w clip(a r)| {d:.3e}; {clipped:.3f} of the samples clip")
    assert d <= 1e-6 and 0.0 < clipped < 1.0
    assert np.abs(mr["material_albedo"].cpu().numpy() - m0["material_albedo"]).max() > 1e-3
    assert np.array_equal(mr["material_roughness"].cpu().numpy(), m0["material_roughness"])


# ---------------------------------------------------------------------------------------------
# 9. interface
# ---------------------------------------------------------------------------------------------
class _Dataset:
    camtype = "perspective"
    mesh = None
    albedo_ratio = None


def test_interface_forms_and_end_to_end():
    cfg = nrc_amd.hotdog_config(render_chunk_size=63)
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_material_np(True))
    img = image(5, 7, seed=61)
    env = relight.EnvImage(m.rc, img, scale=2.5)
    n = 17
    rays = nrc_amd.synthetic_rays(n, seed=9)
    key = prng.PRNGKey(7)
    render_rngs = prng.split(key, 1)                                      # the per-device key array of the trainer
    one = m.apply(None, key, rays, passes=PASSES, env_map=env, albedo_ratio=(0.9, 0.8, 0.7))["render"]
    plain = m.apply(None, key, rays, passes=PASSES)["render"]
    assert set(one.keys()) == set(plain.keys())                           # _apply_material's key set is unchanged
    arrays = dict(env_map=(img * np.float32(2.5)).reshape(1, 35, 1, 3), env_map_w=7, env_map_h=5,
                  env_map_pmf=env.pmf.cpu().numpy().reshape(1, 35, 1), env_map_pdf=env.pdf.cpu().numpy().reshape(1, 35, 1),
                  env_map_dirs=env.dirs.cpu().numpy().reshape(1, 35, 1, 3))
    two = m.apply(None, key, rays, passes=PASSES, albedo_ratio=(0.9, 0.8, 0.7), **arrays)["render"]
    for k in one:
        assert torch.equal(one[k], two[k]), k
    # compute_relight_metrics: the environment sampler, from the same key
    m_env = M.Model(dataclasses.replace(cfg, compute_relight_metrics=True), 0)
    m_env.load_variables(common.weights_material_np(True))
    env_e = relight.EnvImage(m_env.rc, img, scale=2.5)
    via_apply = m_env.apply(None, key, rays, passes=PASSES, env_map=env_e)["render"]
    via_relight = relight.relight(m_env, rays, key, env_e, mode="env")["render"]
    for k in via_apply:
        assert torch.equal(via_apply[k], via_relight[k]), k
    assert not torch.equal(via_apply["direct_rgb"], relight.relight(m_env, rays, key, env_e, mode="brdf")["render"]["direct_rgb"])
    # create_render_fn with a dataset that carries env_map, through render_image on a 9 x 7 view == the direct call
    data = _Dataset()
    data.env_map, data.albedo_ratio = env, (0.9, 0.8, 0.7)
    fn = M.bind_render_fn(M.create_render_fn(m, data))
    view = nrc_amd.synthetic_camera_rays(9, 7)
    pic, _ = M.render_image(fn, rng=render_rngs, rays=view, config=cfg, passes=PASSES, verbose=False)
    flat = view.tree_map(lambda r: np.asarray(r).reshape(63, -1))
    direct = m.apply(None, prng.random_split(render_rngs[0])[0], flat, passes=PASSES, env_map=env, albedo_ratio=(0.9, 0.8, 0.7))["render"]
    for k in ("rgb", "direct_rgb", "material_albedo", "acc"):
        assert np.array_equal(np.asarray(pic[k]).reshape(63, -1), direct[k].cpu().numpy().reshape(63, -1)), k
    # the end-to-end use: a relit view scored against itself
    big = nrc_amd.synthetic_camera_rays(11, 12)
    cfg2 = nrc_amd.hotdog_config(render_chunk_size=132)
    pic2, _ = M.render_image(fn, rng=render_rngs, rays=big, config=cfg2, passes=PASSES, verbose=False)
    score = m.rc.eval_image(np.asarray(pic2["rgb"]), np.asarray(pic2["rgb"]))
    print(f"relit view against itself: psnr {score['psnr']}, mse {score['mse']}")
    assert score["mse"] == 0.0 and score["psnr"] == float("inf")


def _alloc_bytes():
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info()
    return free


def test_repeat_calls_allocate_nothing_and_refusals(rc):
    n = 65
    cfg, rays, rnd = stage_inputs(n)
    Ks, Kd = relight.leg_counts(cfg)
    img = image(5, 7, seed=71, lo=0.4)
    env = relight.EnvImage(rc, img)
    ps = env.picks(prng.PRNGKey(1), relight.expected_T(n, Ks))
    pd = env.picks(prng.PRNGKey(2), relight.expected_T(n, Kd))
    d = torch.from_numpy(lookup_dirs(64, 1)).cuda()
    out = torch.empty_like(d)
    tabs = rc.env_tables(img, 1.0)
    picks = torch.empty(256, dtype=torch.int32, device="cuda")
    key = (rc_ext.C.c_uint32 * 2)(1, 2)
    img_d = env.rgb

    def once():
        st = rc._stream()
        rc._check(rc.lib.rc_set_env_image(rc._h, img_d.data_ptr(), env.pmf.data_ptr(), env.pdf.data_ptr(), env.dirs.data_ptr(), 5, 7, st))
        rc._check(rc.lib.rc_env_tables(rc._h, img_d.data_ptr(), 5, 7, 1.0, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), st))
        rc._check(rc.lib.rc_env_lookup(rc._h, d.data_ptr(), 64, out.data_ptr(), st))
        rc._check(rc.lib.rc_env_pick(rc._h, key, 256, picks.data_ptr(), st))

    once()
    rc.render_relight(rays.hot_fields(), rnd, "env", ps, pd)
    before = _alloc_bytes()
    for _ in range(3):
        once()
    after = _alloc_bytes()
    assert after == before, (before, after)
    # refusals
    with pytest.raises(rc_ext.RcError, match="T_spec must be 1040"):
        rc.render_relight(rays.hot_fields(), rnd, "env", ps[:256], pd)
    with pytest.raises(rc_ext.RcError, match="T_diff must be 1040"):
        rc.render_relight(rays.hot_fields(), rnd, "env", ps, torch.cat([pd, pd]))
    rc.set_env_image(env.rgb)                                             # no tables
    with pytest.raises(rc_ext.RcError, match="tables"):
        rc.render_relight(rays.hot_fields(), rnd, "env", ps, pd)
    with pytest.raises(rc_ext.RcError, match="no pmf bound"):
        rc.env_pick(prng.PRNGKey(0), 4)
    rc.render_relight(rays.hot_fields(), rnd, "brdf")                     # the image alone serves the BRDF mode
    rc.set_env_image(None)
    with pytest.raises(rc_ext.RcError, match="no image bound"):
        rc.render_relight(rays.hot_fields(), rnd, "brdf")
    with pytest.raises(rc_ext.RcError, match="no image bound"):
        rc.env_lookup(d)
    with pytest.raises(rc_ext.RcError, match="together"):
        rc._check(rc.lib.rc_set_env_image(rc._h, img_d.data_ptr(), env.pmf.data_ptr(), None, None, 5, 7, rc._stream()))
    rc._env_bound = None
    # n = 0 / T = 0: RC_OK, nothing written
    assert rc.lib.rc_env_lookup(rc._h, None, 0, None, rc._stream()) == 0
    assert rc.lib.rc_env_pick(rc._h, key, 0, None, rc._stream()) == 0
    # a time-resolved handle refuses every call
    th = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    for call in (lambda: th.set_env_image(img), lambda: th.env_tables(img), lambda: th.env_lookup(d), lambda: th.env_pick(prng.PRNGKey(0), 4)):
        with pytest.raises(rc_ext.RcError, match="time-resolved"):
            call()
    a = rc_ext.rc_relight_args()
    assert th.lib.rc_render_relight(th._h, None, 0, None, None, 32, rc_ext.C.byref(a), None, None, th._stream()) == -5
