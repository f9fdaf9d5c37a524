"""Parity of the HIP path (through the C ABI) against the CPU oracle and the golden vectors.

Tolerances (BASELINE.json north_star): RGB L-inf <= 1e-4 in fp32.  Geometry extras that are sums of
O(1) positions/distances get 5e-4; raw hash-grid features of points far outside the scene (where the
contraction amplifies one-ulp coordinate differences by N = 2048) get 2e-3.
"""
import os

import numpy as np
import pytest
import torch

import common
import nrc_amd

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RGB_TOL = 1e-4
FUSED_TOL = 0.0     # fused and launch-per-stage plans run the same arithmetic in the same order: bitwise equal


@pytest.fixture(scope="module")
def rc():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h.load_weights(common.weights_np())
    return h


@pytest.fixture(scope="module")
def rc_shell():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h.load_weights(common.weights_np(4.0))
    return h


def _render(rc, n, jitter_seed=None, seed=20200823, fused=True, **kw):
    """The plain cache pass runs as ONE fused launch by default (rc_set_fused); `fused=False` selects the
    launch-per-stage plan, which leaves every intermediate in the workspace for inspection."""
    rays = nrc_amd.synthetic_rays(n, seed=seed)
    rnd = None if jitter_seed is None else {"jitter": common.jitters(n, seed=jitter_seed)}
    rc.set_fused(fused)
    try:
        out = rc.render_rays(rays.hot_fields(), rnd, **kw)
        torch.cuda.synchronize()
    finally:
        rc.set_fused(True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _staged_matches(rc, out, n, jitter_seed=None, tol=0.0, **kw):
    """Re-render with the launch-per-stage plan (fills the workspace) and compare with the fused result."""
    st = _render(rc, n, jitter_seed, fused=False, **kw)
    for k, v in out.items():
        d = np.abs(st[k] - v).max() if v.size else 0.0
        assert d <= tol, (k, d)
    return st


# ---------------------------------------------------------------------------------------------
# single operators
# ---------------------------------------------------------------------------------------------
def test_hashgrid_operator_vs_oracle_and_golden(rc):
    from oracle import hashgrid_ref, mathx
    g = dict(np.load(os.path.join(GOLD, "operators.npz")))
    cfg = nrc_amd.hotdog_config()
    wt = common.weights_torch()
    grids = [("params/Cache/Sampler/MLP_0/density_grid", cfg.proposal_grids[0]),
             ("params/Cache/Sampler/MLP_1/density_grid", cfg.proposal_grids[1]),
             ("params/Cache/Sampler/MLP_2/density_grid", cfg.proposal_grids[2]),
             ("params/Cache/Shader/appearance_grid", cfg.appearance_grid)]
    pts = g["points"]
    for gid, (prefix, gc) in enumerate(grids):
        out = rc.hashgrid_lookup(gid, pts).cpu().numpy()
        ref = hashgrid_ref.hash_encoding(wt, prefix, gc, mathx.contract_radius(torch.from_numpy(pts), 2.0)).numpy()
        assert out.shape == ref.shape == (pts.shape[0], gc.out_dim)
        assert np.abs(out - ref).max() <= 2e-3
        assert np.abs(out - g[f"grid{gid}"]).max() <= 2e-3


def test_hashgrid_inside_unit_ball_is_bit_exact(rc):
    """Where the contraction is the identity every step is exactly rounded fp32 -> bitwise equal."""
    from oracle import hashgrid_ref, mathx
    cfg = nrc_amd.hotdog_config()
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1.1, 1.1, size=(4096, 3)).astype(np.float32)      # |x/2| < 1
    wt = common.weights_torch()
    out = rc.hashgrid_lookup(2, pts).cpu().numpy()
    ref = hashgrid_ref.hash_encoding(wt, "params/Cache/Sampler/MLP_2/density_grid", cfg.proposal_grids[2],
                                     mathx.contract_radius(torch.from_numpy(pts), 2.0)).numpy()
    assert np.array_equal(out, ref)


def test_hashgrid_without_contraction_negative_and_outside_coords(rc):
    from oracle import hashgrid_ref
    cfg = nrc_amd.hotdog_config()
    pts = np.array([[-1.7, 0.3, 1.9], [-0.999, -0.999, -0.999], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0],
                    [-1.0, 0.5, 0.25], [1.499, -1.499, 0.001]], dtype=np.float32)
    out = rc.hashgrid_lookup(3, pts, apply_contraction=False).cpu().numpy()
    ref = hashgrid_ref.hash_encoding(common.weights_torch(), "params/Cache/Shader/appearance_grid",
                                     cfg.appearance_grid, torch.from_numpy(pts)).numpy()
    assert np.array_equal(out, ref)
    # dense levels (first 3 x F) of a point outside the bbox are exactly zero (zero padding)
    assert np.all(out[0, :12] == 0.0) and np.any(out[0, 12:] != 0.0)


def test_hashgrid_empty_and_single_point(rc):
    assert rc.hashgrid_lookup(0, np.zeros((0, 3), np.float32)).shape == (0, 6)
    assert rc.hashgrid_lookup(1, np.zeros((1, 3), np.float32)).shape == (1, 7)


def test_sample_intervals_operator(rc):
    from oracle import stepfun_ref
    g = dict(np.load(os.path.join(GOLD, "operators.npz")))
    t, lg, jit = g["si_t"], g["si_logits"], g["si_jitter"]
    out = rc.sample_intervals(t, lg, 32).cpu().numpy()
    ref = stepfun_ref.sample_intervals(None, torch.from_numpy(t), torch.from_numpy(lg), 32).numpy()
    # the CDF is a parallel wave scan here and a sequential cumsum in the oracle; a flat CDF segment
    # amplifies the few-ulp difference when it is inverted
    assert np.abs(out - ref).max() <= 5e-5 and np.abs(out - g["si_out_det"]).max() <= 1e-4
    out = rc.sample_intervals(t, lg, 32, jit).cpu().numpy()
    assert np.abs(out - g["si_out_jit"]).max() <= 1e-4
    assert np.all(np.diff(out, axis=-1) >= 0) and out.min() >= 0 and out.max() <= 1
    # single bin -> 64 samples (level 0 of the sampler)
    t1 = np.tile(np.array([[0.0, 1.0]], np.float32), (4, 1))
    out = rc.sample_intervals(t1, np.zeros((4, 1), np.float32), 64).cpu().numpy()
    assert np.abs(out - g["si_out_1bin"]).max() <= 1e-6


# ---------------------------------------------------------------------------------------------
# the hot path
# ---------------------------------------------------------------------------------------------
CHECK_3 = ("diffuse_rgb", "specular_rgb", "direct_rgb", "indirect_rgb", "albedo_rgb", "indirect_diffuse_rgb",
           "indirect_specular_rgb", "indirect_occ")


@pytest.mark.parametrize("jitter_seed", [None, 7])
def test_cache_render_256_vs_oracle_fp32(rc, jitter_seed):
    n = 256
    out = _render(rc, n, jitter_seed)
    ref = common.oracle_cache(n, jitter_seed=jitter_seed, want_grad_normals=False)
    r = {k: v.numpy() for k, v in ref["render"].items()}
    assert np.abs(out["rgb"] - r["rgb"]).max() <= RGB_TOL
    assert np.abs(out["acc"] - r["acc"]).max() <= RGB_TOL
    for k in CHECK_3:
        assert np.abs(out[k] - r[k]).max() <= RGB_TOL, k
    for k in ("means", "normals_pred"):
        assert np.abs(out[k] - r[k]).max() <= 5e-4, k
    for k in ("ray_dists", "light_dists"):
        assert np.abs(out[k] - r[k][:, 0]).max() <= 5e-4, k
    for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
        assert np.abs(out[k] - r[k]).max() <= 1e-3, k
    # intermediate stages (launch-per-stage plan; its outputs equal the fused kernel's)
    _staged_matches(rc, out, n, jitter_seed, tol=FUSED_TOL)
    for l, S in enumerate((64, 64, 32)):
        assert np.abs(rc.workspace(f"sdist{l}").reshape(n, S + 1) - ref["sampler"][l]["sdist"].numpy()).max() <= 5e-5
        assert np.abs(rc.workspace(f"tdist{l}").reshape(n, S + 1) - ref["sampler"][l]["tdist"].numpy()).max() <= 1e-4
        assert np.abs(rc.workspace(f"weights{l}").reshape(n, S) - ref["sampler"][l]["weights"].numpy()).max() <= 2e-4
    # level 0 sits on bit-identical sample positions -> the density MLP is compared tightly
    d0 = rc.workspace("density0").reshape(n, 64)
    assert np.abs(d0 - ref["sampler"][0]["density"].numpy()).max() <= 1e-4


@pytest.mark.parametrize("jitter_seed", [None, 7])
def test_intermediates_sit_at_the_fp32_noise_floor_of_the_oracle(rc, jitter_seed):
    """The keys the test above holds to looser-than-1e-4 bounds (geometry 5e-4, distances 1e-3, the samplers' step functions),
    measured against what fp32 arithmetic in the reference's OWN order loses: the fp64 oracle is the exact value, the fp32
    oracle's distance from it is the floor, and the HIP path may be no more than 3 x that floor away from the exact value
    (measured 0.6-1.4 x: profiles/r04_tolerance_floor.txt, tools/measure_tolerances.py).  An error of the kernels' own -- a
    wrong constant, a dropped term -- is orders of magnitude above the floor; a bound of 1e-3 would let one of 5e-4 through."""
    n = 256
    out = _render(rc, n, jitter_seed, fused=False)
    r32 = common.oracle_cache(n, jitter_seed=jitter_seed, want_grad_normals=False)
    r64 = common.oracle_cache(n, jitter_seed=jitter_seed, want_grad_normals=False, dtype=torch.float64)

    def check(name, a, b32, b64):
        a = a.astype(np.float64)
        b32, b64 = np.asarray(b32, np.float64).reshape(a.shape), np.asarray(b64, np.float64).reshape(a.shape)
        floor, err = np.abs(b32 - b64).max(), np.abs(a - b64).max()
        assert err <= 3.0 * floor + 1e-7, (name, err, floor)

    for k in ("rgb", "acc", "means", "normals_pred", "ray_dists", "light_dists", "distance_mean", "distance_median",
              "distance_percentile_5", "distance_percentile_95"):
        b32, b64 = r32["render"][k].numpy(), r64["render"][k].numpy()
        if k in ("ray_dists", "light_dists"): b32, b64 = b32[:, 0], b64[:, 0]
        check(k, out[k], b32, b64)
    for l, S in enumerate((64, 64, 32)):
        for w, cols in (("sdist", S + 1), ("tdist", S + 1), ("weights", S), ("density", S)):
            check(f"{w}{l}", rc.workspace(f"{w}{l}").reshape(n, cols), r32["sampler"][l][w].numpy(), r64["sampler"][l][w].numpy())


@pytest.mark.parametrize("name", ["hotdog_cache_256_det.npz", "hotdog_cache_256_jit.npz"])
def test_cache_render_vs_fp64_golden(rc, name):
    g = dict(np.load(os.path.join(GOLD, name)))
    n, js = int(g["meta"][0]), int(g["meta"][1])
    out = _render(rc, n, None if js < 0 else js)
    assert np.abs(out["rgb"] - g["render_rgb"]).max() <= RGB_TOL
    assert np.abs(out["acc"] - g["render_acc"]).max() <= RGB_TOL
    for k in CHECK_3:
        assert np.abs(out[k] - g["render_" + k]).max() <= 2e-4, k


def test_cache_render_shell_weights_saturated_rays(rc_shell):
    """Second weight set (+4 on the density bias): rays saturate, early samples dominate."""
    g = dict(np.load(os.path.join(GOLD, "hotdog_cache_64_shell.npz")))
    n, js = int(g["meta"][0]), int(g["meta"][1])
    out = _render(rc_shell, n, js)
    assert g["render_acc"].min() > 0.99
    assert np.abs(out["rgb"] - g["render_rgb"]).max() <= RGB_TOL
    assert np.abs(out["acc"] - g["render_acc"]).max() <= RGB_TOL
    ref = common.oracle_cache(n, jitter_seed=js, density_shift=4.0, want_grad_normals=False)["render"]
    assert np.abs(out["rgb"] - ref["rgb"].numpy()).max() <= RGB_TOL
    assert np.abs(out["distance_median"] - ref["distance_median"].numpy()).max() <= 1e-3


@pytest.mark.parametrize("n", [1, 3, 31, 33, 100, 1000])
def test_ragged_batch_sizes(rc, n):
    """n not a multiple of the 4-ray workgroups / 32-point MFMA tiles / 128-point MLP workgroups."""
    out = _render(rc, n, outputs=["rgb", "acc"])
    ref = common.oracle_cache(n, want_grad_normals=False)["render"]
    assert out["rgb"].shape == (n, 3)
    assert np.abs(out["rgb"] - ref["rgb"].numpy()).max() <= RGB_TOL
    assert np.abs(out["acc"] - ref["acc"].numpy()).max() <= RGB_TOL


@pytest.mark.parametrize("n,jitter_seed", [(1, None), (5, 2), (257, 11), (2048, 4)])
def test_fused_plan_equals_staged_plan(rc, n, jitter_seed):
    """Every output of the fused per-ray kernel against the launch-per-stage plan, incl. analytic normals."""
    out = _render(rc, n, jitter_seed)
    assert "normals" in out and "distance_median" in out
    _staged_matches(rc, out, n, jitter_seed, tol=FUSED_TOL)


@pytest.mark.parametrize("n,jitter_seed", [(1, None), (2, 3), (3, None), (64, 5), (1023, None), (4097, 8)])
def test_two_wave_fused_kernel_equals_the_one_wave_kernel(rc, n, jitter_seed):
    """rc_set_fused 1 (k_cache_fused_team: two wavefronts per ray, two rays per workgroup, csrc/rc_fused2.hip) against
    rc_set_fused 3 (k_cache_fused: one wavefront per ray): the same weight stream, the same MFMA order per accumulator,
    the same scans -- every output bitwise equal, odd ray counts (a workgroup with one live ray) included; with and
    without requesting the analytic normals (the GRAD / non-GRAD instantiations).
    A library built with the split-form shader (rc_mlp_arithmetic() == 1, the default) runs the one-wave kernel for mode 1
    as well: there the comparison is of that kernel with itself; it compares the two kernels in a
    RC_SPLIT_MFMA=0 build (RC_HIP_LIBRARY).  The real comparison runs in every GPU suite run: tests/test_gpu_f32_build.py
    runs this module against that build (make variant-f32) in a child process."""
    rays = nrc_amd.synthetic_rays(n, seed=900 + n)
    rnd = None if jitter_seed is None else {"jitter": common.jitters(n, seed=jitter_seed)}
    for outputs in (None, ["rgb", "acc", "distance_median", "normals_pred"]):
        res = {}
        for mode in (1, 3):
            rc.set_fused(mode)
            try:
                out = rc.render_rays(rays.hot_fields(), rnd, **({} if outputs is None else {"outputs": outputs}))
                torch.cuda.synchronize()
            finally:
                rc.set_fused(True)
            res[mode] = {k: v.clone() for k, v in out.items()}
        for k in res[1]:
            assert torch.equal(res[1][k], res[3][k]), (k, outputs)
            assert bool(torch.isfinite(res[1][k]).all()), k


def test_two_wave_fused_kernel_exports_the_samples_of_the_one_wave_kernel(rc_smooth):
    """The material stage's primary pass under rc_set_fused 1 (RC_SPLIT_MFMA=0: k_cache_fused_team with its sample
    export) against rc_set_fused 3 (k_cache_fused's EXPORT instantiation): the four exported buffers themselves (fence
    posts, densities, means, predicted normals of the last level, read back from the workspace) and every array
    render_material returns are bitwise equal; 5 rays (a workgroup with one live ray), fixed picks (the shading point
    then takes the exported mean and normal at the given index).  In the split build both modes run the one-wave kernel,
    as above."""
    from oracle import material_ref
    n = 5
    cfg = nrc_amd.hotdog_config()
    rays = nrc_amd.synthetic_rays(n, seed=905)
    rnd = material_ref.draw_randoms(cfg, n, seed=5)
    ks, kd = rnd["spec_u1"].shape[1], rnd["diff_jitter"][0].size // n
    rnd = dict(rnd, gumbel=None, spec_gumbel=None, diff_gumbel=None,
               resample_inds=np.array([3, 11, 16, 20, 29], np.int32),
               spec_resample_inds=((np.arange(n * ks) * 7 + 3) % 32).astype(np.int32),
               diff_resample_inds=((np.arange(n * kd) * 5 + 1) % 32).astype(np.int32))
    res = {}
    for mode in (1, 3):
        rc_smooth.set_fused(mode)
        try:
            cres, mres = rc_smooth.render_material(rays.hot_fields(), rnd)
            torch.cuda.synchronize()
        finally:
            rc_smooth.set_fused(True)
        res[mode] = {**{"cache:" + k: v.clone() for k, v in cres.items()}, **{"material:" + k: v.clone() for k, v in mres.items()}}
        for name, count in (("tdist2", n * 33), ("density2", n * 32), ("means2", 3 * n * 32), ("normals_pred", 3 * n * 32)):
            w = rc_smooth.workspace(name)
            assert w.size >= count, (name, w.size)
            res[mode]["export:" + name] = torch.from_numpy(w[:count].copy())
    assert res[1].keys() == res[3].keys() and len(res[1]) > 0
    for k in res[1]:
        assert torch.equal(res[1][k], res[3][k]), k
        assert bool(torch.isfinite(res[1][k]).all()), k


def test_empty_batch_is_a_noop(rc):
    rays = nrc_amd.synthetic_rays(4)
    f = {k: np.asarray(v)[:0] for k, v in rays.hot_fields().items()}
    out = rc.render_rays(f, None, outputs=["rgb"])
    assert out["rgb"].shape == (0, 3)


def test_full_size_batch_properties_1024(rc):
    """BASELINE configs[1] size; size-independent properties instead of an oracle run."""
    n = 1024
    out = _render(rc, n, jitter_seed=3)
    acc, rgb = out["acc"], out["rgb"]
    assert np.all(np.isfinite(rgb)) and acc.min() >= 0 and acc.max() <= 1 + 1e-6
    # rgb = direct + indirect + (1 - acc) * bg (bg = 1); diffuse + specular = direct + indirect
    assert np.abs(rgb - (out["direct_rgb"] + out["indirect_rgb"] + (1 - acc)[:, None])).max() <= 2e-6
    assert np.abs(out["diffuse_rgb"] + out["specular_rgb"] - out["direct_rgb"] - out["indirect_rgb"]).max() <= 2e-6
    assert np.abs(out["indirect_occ"] - acc[:, None]).max() <= 2e-6
    _staged_matches(rc, out, n, 3, tol=FUSED_TOL)
    for l, S in enumerate((64, 64, 32)):
        sd = rc.workspace(f"sdist{l}").reshape(n, S + 1)
        td = rc.workspace(f"tdist{l}").reshape(n, S + 1)
        assert np.all(np.diff(sd, axis=-1) >= 0) and sd.min() >= 0 and sd.max() <= 1
        assert td.min() >= 2.0 - 1e-6 and td.max() <= 6.0 + 1e-6
    w2 = rc.workspace("weights2").reshape(n, 32)
    assert np.abs(w2.sum(-1) - acc).max() <= 2e-6
    assert np.all(out["distance_percentile_5"] <= out["distance_median"] + 1e-6)
    assert np.all(out["distance_median"] <= out["distance_percentile_95"] + 1e-6)
    # linearity of the composite in the per-sample colours: sum_s w_s * shade_rgb_s + (1-acc)
    sh = rc.workspace("shade").reshape(15, n, 32)
    recon = (w2[None] * sh[0:3]).sum(-1).T + (1 - acc)[:, None]
    assert np.abs(recon - rgb).max() <= 5e-6


def test_determinism_and_graph_replay_equals_eager(rc):
    rays = nrc_amd.synthetic_rays(512)
    f = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in rays.hot_fields().items()}
    rc.set_graph_mode(0)
    a = rc.render_rays(f, None)
    torch.cuda.synchronize()
    a = {k: v.clone() for k, v in a.items()}
    rc.set_graph_mode(2)
    buf = rc.render_rays(f, None)             # captures
    b = rc.render_rays(f, None, out=buf)      # replays
    torch.cuda.synchronize()
    rc.set_graph_mode(1)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_errors_are_reported_not_fatal(rc):
    from nrc_amd import rc_ext
    rays = nrc_amd.synthetic_rays(8).hot_fields()
    with pytest.raises(rc_ext.RcError, match="resampling needs"):
        rc.render_rays(rays, None, pass_mask=rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE)
    with pytest.raises(rc_ext.RcError, match="unknown tensor"):
        rc.load_weights({"params/Nope/kernel": np.zeros((2, 2), np.float32)})
    with pytest.raises(rc_ext.RcError, match="bad shape"):
        rc.load_weights({"params/Cache/Shader/tint_layer/kernel": np.zeros((95, 3), np.float32)})
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    with pytest.raises(rc_ext.RcError, match="missing weight"):
        h.render_rays(rays, None)
    # the original handle is still usable
    out = rc.render_rays(rays, None, outputs=["rgb"])
    assert torch.isfinite(out["rgb"]).all()


# ---------------------------------------------------------------------------------------------
# host layer: Model.apply / render_image keep the reference's signatures and keys
# ---------------------------------------------------------------------------------------------
def test_model_apply_render_dict_matches_oracle_keys():
    from nrc_amd import model as M
    cfg = nrc_amd.hotdog_config()
    m = M.Model(cfg, 0)
    variables = {"params": {}}
    for k, v in common.weights_np().items():
        node = variables
        parts = k.split("/")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = v
    rays = nrc_amd.synthetic_rays(64)
    out = m.apply(variables, None, rays, train=False, passes=("cache",), compute_extras=True)["render"]
    ref = common.oracle_cache(64, want_grad_normals=True)["render"]
    assert set(out.keys()) == set(ref.keys())
    for k, v in ref.items():
        got = out[k].cpu().numpy()
        assert got.shape == tuple(v.shape), k
        if "normals" in k and "pred" not in k and "to_use" not in k:
            assert np.abs(got - v.numpy()).mean() <= 3e-3, k   # analytic normals: see test_analytic_normals
            continue
        tol = 1e-3 if ("dist" in k or k.endswith("means")) else RGB_TOL * (5 if "normals" in k else 1)
        assert np.abs(got - v.numpy()).max() <= tol, k


def test_render_image_matches_oracle_on_small_image():
    from nrc_amd import model as M
    cfg = nrc_amd.hotdog_config(render_chunk_size=256)
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_np())
    rays = nrc_amd.synthetic_camera_rays(18, 20)        # 360 rays -> chunks of 256 + 104 (padded)
    img, _ = M.render_image(M.bind_render_fn(M.create_render_fn(m)), None, rays, cfg, ("cache",), verbose=False)
    assert img["rgb"].shape == (18, 20, 3) and img["acc"].shape == (18, 20) and img["rgb"].dtype == np.float32
    from oracle import cache_ref
    flat = rays.tree_map(lambda r: np.asarray(r).reshape(360, -1))
    ref = cache_ref.cache_forward(common.weights_torch(), cfg, common.rays_torch(flat), None,
                                  want_grad_normals=False)["render"]
    err = np.abs(img["rgb"].reshape(360, 3) - ref["rgb"].numpy()).max()
    mse = float(np.mean((img["rgb"].reshape(360, 3) - ref["rgb"].numpy()) ** 2))
    psnr = -10.0 * np.log10(max(mse, 1e-30))
    assert err <= RGB_TOL and psnr >= 80.0, (err, psnr)


# ---------------------------------------------------------------------------------------------
# secondary rays (is_secondary=True): far clamp, near replacement, power-ladder distances,
# categorical resampling to one sample, bg = 0, model-level EnvMap composite
# ---------------------------------------------------------------------------------------------
def _oracle_secondary(rays, rnd, cfg=None, **kw):
    from oracle import cache_ref
    jit = [torch.from_numpy(j)[:, None] for j in rnd["jitter"]]
    cfg = nrc_amd.hotdog_config() if cfg is None else cfg
    return cache_ref.cache_forward(common.weights_torch(), cfg, common.rays_dict_torch(rays), jit,
                                   is_secondary=True, gumbel=torch.from_numpy(rnd["gumbel"]),
                                   want_grad_normals=False, **kw)


def test_secondary_rays_vs_oracle(rc):
    from nrc_amd import rc_ext
    n = 512
    rays, rnd = common.secondary_case(n, seed=5)
    ref = _oracle_secondary(rays, rnd)
    out = rc.render_rays(rays, rnd, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY)
    torch.cuda.synchronize()
    inds = rc.workspace("inds", np.int32)[:n]
    ref_inds = ref["filtered_sampler_inds"][:, 0].numpy()
    same = inds == ref_inds
    assert same.mean() >= 0.995          # a Gumbel near-tie may flip under fp32 noise; none expected
    r = ref["render"]
    for l in range(3):
        td = rc.workspace(f"tdist{l}").reshape(n, -1)
        assert np.abs(td - ref["sampler"][l]["tdist"].numpy()).max() <= 2e-4
        assert td.max() <= 2.0 + 1e-5 and td.min() >= 0.0          # far = min(far, env_map_distance)
    for k in ("rgb", "acc", "diffuse_rgb", "specular_rgb", "indirect_rgb", "direct_rgb"):
        v = out[k].cpu().numpy()
        assert np.abs(v[same] - r[k].numpy().reshape(v.shape)[same]).max() <= RGB_TOL, k
    assert np.abs(out["env_map_rgb"].cpu().numpy() - r["env_map_rgb"].numpy()).max() <= 1e-5
    no_env = (r["rgb_no_stopgrad"] - r["env_map_rgb"] * (1 - r["acc"][:, None])).numpy()
    assert np.abs(out["rgb_no_env"].cpu().numpy()[same] - no_env[same]).max() <= RGB_TOL
    assert np.abs(out["distance_median"].cpu().numpy() - r["distance_median"].numpy()).max() <= 1e-3


def test_power_ladder_mapping_of_the_secondary_rays_to_a_few_ulp_of_the_power(rc):
    """s -> t of the secondary rays' fence posts = math.inv_power_ladder (internal/math.py:319-341) with p = -1.5: the
    kernels evaluate its power with the hardware's log2 / exp2 around a split exponent (rc_dev_sample.h pow_pos) instead
    of the library's powf.  From the kernel's own float32 fence posts in s (workspace sdist) a float64 evaluation of the
    mapping must give the kernel's t with the power itself within 4 float32 ulp -- on all three levels, 512 rays."""
    from nrc_amd import rc_ext
    n = 512
    rays, rnd = common.secondary_case(n, seed=15)
    rays = {k: v for k, v in rays.items() if k != "normals"}          # no near replacement: one (near, far) for all rays
    rc.render_rays(rays, rnd, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY | rc_ext.RC_PASS_NO_ENVMAP, outputs=["rgb", "acc"])
    torch.cuda.synchronize()
    cfg = nrc_amd.hotdog_config()
    p, premult = np.float32(cfg.raydist_p), np.float32(cfg.raydist_premult)
    near = np.asarray(rays["near"], np.float32).reshape(-1)
    far = np.minimum(np.asarray(rays["far"], np.float32).reshape(-1), np.float32(cfg.env_map_distance))

    def ladder32(x):                                       # power_ladder in float32 as the kernel's k_ladder_bounds does
        x = np.float32(x) * premult
        xs = np.abs(x) / np.maximum(np.float32(1.17549435e-38), np.abs(p - np.float32(1)))
        y = np.abs(p - np.float32(1)) / p * (np.power(xs + np.float32(1), p, dtype=np.float32) - np.float32(1))
        return np.sign(x) * y

    for l, S in enumerate((64, 64, 32)):
        sd = rc.workspace(f"sdist{l}")[: n * (S + 1)].reshape(n, S + 1).astype(np.float64)
        td = rc.workspace(f"tdist{l}")[: n * (S + 1)].reshape(n, S + 1)
        # the rays of secondary_case share one (near, far): the bounds in s are two float32 numbers
        s_near, s_far = np.float64(ladder32(near[0])), np.float64(ladder32(far[0]))
        y = (sd * s_far + (1.0 - sd) * s_near).astype(np.float32).astype(np.float64)   # the kernel's float32 argument
        p64, pm1 = np.float64(p), abs(np.float64(p) - 1.0)
        c32 = np.float64(np.float32(1.0) / p)                                            # the exponent as float32, like the reference
        x32 = (np.float32(p64 / pm1) * y.astype(np.float32) + np.float32(1)).astype(np.float64)
        pw = np.power(x32, c32)
        want = pm1 * (pw - 1.0) / np.float64(premult)
        # t = pm1 (x^c - 1) / premult: an error of the power enters t in absolute terms (near t = 0 the subtraction cancels),
        # so the budget is in ulp OF THE POWER scaled by pm1 / premult -- 4: pow_pos's ~1.5 plus the two bounds in s, which
        # the kernel gets from the library's powf and this test from numpy's (each may differ by one ulp) -- plus 4 ulp of t
        # for the float32 steps around the power (measured worst case over the three levels: 3.03 of the 4)
        ulp_pw = np.spacing(pw.astype(np.float32)).astype(np.float64)
        ulp_t = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(td.astype(np.float64) - want)
        tol = 4.0 * ulp_pw * pm1 / np.float64(premult) + 4.0 * ulp_t
        assert (err <= tol).all(), (l, float((err / tol).max()))


def test_secondary_rays_without_envmap_and_given_indices(rc):
    from nrc_amd import rc_ext
    n = 200
    rays, rnd = common.secondary_case(n, seed=9)
    ref = _oracle_secondary(rays, rnd, use_env_map=False)
    # hand the oracle's picks over (filtered_sampler_inds): removes the only discontinuous step
    rnd2 = dict(jitter=rnd["jitter"], resample_inds=ref["filtered_sampler_inds"][:, 0].numpy().astype(np.int32))
    mask = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY | rc_ext.RC_PASS_NO_ENVMAP
    out = rc.render_rays(rays, rnd2, mask)
    torch.cuda.synchronize()
    r = ref["render"]
    assert np.abs(out["rgb"].cpu().numpy() - r["rgb"].numpy()).max() <= RGB_TOL
    assert np.abs(out["acc"].cpu().numpy() - r["acc"].numpy()).max() <= RGB_TOL
    assert float(out["env_map_rgb"].abs().max()) == 0.0
    assert np.array_equal(rc.workspace("inds", np.int32)[:n], rnd2["resample_inds"])


def test_primary_rays_with_forced_resampling(rc):
    """resample=True on primary rays (MaterialModel.resample_render, models.py:156-167): one shaded sample,
    acc / distances from the unfiltered weights, bg = 1.  White-noise tables: the Gumbel draw itself is checked
    (>= 99 % equal picks); the values are compared with the oracle's picks handed over (next test holds 1e-4)."""
    from nrc_amd import rc_ext
    from oracle import cache_ref
    n = 256
    rays = nrc_amd.synthetic_rays(n)
    rng = np.random.Generator(np.random.PCG64(3))
    g = rng.gumbel(size=(n, 32)).astype(np.float32)
    ref = cache_ref.cache_forward(common.weights_torch(), nrc_amd.hotdog_config(), common.rays_torch(rays), None,
                                  resample=True, gumbel=torch.from_numpy(g), want_grad_normals=False)
    out = rc.render_rays(rays.hot_fields(), {"gumbel": g}, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE)
    torch.cuda.synchronize()
    picks = ref["filtered_sampler_inds"][:, 0].numpy().astype(np.int32)
    same = rc.workspace("inds", np.int32)[:n] == picks
    assert same.mean() >= 0.99
    out = rc.render_rays(rays.hot_fields(), {"resample_inds": picks}, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE)
    torch.cuda.synchronize()
    assert np.array_equal(rc.workspace("inds", np.int32)[:n], picks)
    r = ref["render"]
    # ONE shaded sample per ray: the per-sample colour noise (1-ulp position differences amplified by the
    # random fine-level tables, ~3e-4 per sample) is not averaged over 32 samples here.
    v, b = out["rgb"].cpu().numpy(), r["rgb"].numpy()
    assert np.abs(v - b).max() <= 1e-3
    assert np.abs(v - b).mean() <= 2e-5
    assert np.abs(out["acc"].cpu().numpy() - r["acc"].numpy()).max() <= RGB_TOL
    assert np.abs(out["distance_median"].cpu().numpy() - r["distance_median"].numpy()).max() <= 1e-3


def test_analytic_normals(rc):
    """`normals` = -normalize(d raw_density / d x) (geometry.py:421-460): MLP backward on the matrix cores,
    trilinear Jacobian, contraction Jacobian.  The gradient of a trilinear interpolant is piecewise constant
    and JUMPS across cell faces (cells are 1/2048 wide on random tables), so a sample whose position differs
    by one ulp can land in another cell: the fp32 and fp64 oracles themselves disagree on ~1 % of the samples
    (max 1.8).  The check is therefore statistical per sample and loose on the composited value."""
    n = 256
    rays = nrc_amd.synthetic_rays(n)
    out = rc.render_rays(rays.hot_fields(), None, outputs=["normals", "rgb"])
    torch.cuda.synchronize()
    ref = common.oracle_cache(n, want_grad_normals=True)
    rc.set_fused(False)
    staged = rc.render_rays(rays.hot_fields(), None, outputs=["normals", "rgb"])
    torch.cuda.synchronize()
    rc.set_fused(True)
    assert torch.equal(staged["normals"], out["normals"]) and torch.equal(staged["rgb"], out["rgb"])
    ng = rc.workspace("normals_grad").reshape(3, n, 32).transpose(1, 2, 0)
    rn = ref["sampler"][2]["normals"].numpy()
    d = np.abs(ng - rn)
    assert np.median(d) <= 2e-4 and d.mean() <= 3e-3 and (d > 1e-2).mean() <= 0.03
    nrm = np.linalg.norm(ng, axis=-1)
    assert np.abs(nrm[nrm > 0] - 1).max() <= 1e-5
    assert np.abs(out["normals"].cpu().numpy() - ref["render"]["normals"].numpy()).max() <= 0.1
    assert np.abs(out["normals"].cpu().numpy() - ref["render"]["normals"].numpy()).mean() <= 3e-3
    # requesting the normals must not change rgb (normals_to_use = normals_pred)
    out2 = rc.render_rays(rays.hot_fields(), None, outputs=["rgb"])
    torch.cuda.synchronize()
    assert torch.equal(out["rgb"], out2["rgb"])


# ---------------------------------------------------------------------------------------------
# strict parity on a smooth field, and the material stage (config 3)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rc_smooth():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h.load_weights(common.weights_material_np(smooth=True))
    return h


def test_cache_render_smooth_field_is_tight(rc_smooth):
    """Same kernels, tables whose amplitude decays with level (equal gradient per level): without the
    chaotic amplification of the white-noise tables the HIP path agrees with the fp32 oracle to ~1e-6."""
    from oracle import cache_ref
    n = 256
    rays = nrc_amd.synthetic_rays(n)
    jit = common.jitters(n, seed=2)
    out = rc_smooth.render_rays(rays.hot_fields(), {"jitter": jit})
    torch.cuda.synchronize()
    ref = cache_ref.cache_forward(common.to_torch(common.weights_material_np(True)), nrc_amd.hotdog_config(),
                                  common.rays_torch(rays), [torch.from_numpy(j) for j in jit], want_grad_normals=False)["render"]
    assert np.abs(out["rgb"].cpu().numpy() - ref["rgb"].numpy()).max() <= 1e-5
    assert np.abs(out["acc"].cpu().numpy() - ref["acc"].numpy()).max() <= 1e-5
    assert np.abs(out["normals_pred"].cpu().numpy() - ref["normals_pred"].numpy()).max() <= 1e-4
    assert np.abs(out["distance_median"].cpu().numpy() - ref["distance_median"].numpy()).max() <= 1e-4


MAT_KEYS_3 = ("rgb", "direct_rgb", "indirect_rgb", "diffuse_rgb", "specular_rgb", "direct_diffuse_rgb",
              "direct_specular_rgb", "indirect_diffuse_rgb", "indirect_specular_rgb", "lighting_irradiance",
              "material_albedo", "means", "normals_to_use")


@pytest.mark.parametrize("smooth", [True, False])
def test_material_stage_vs_oracle(rc_smooth, smooth):
    """config 3: cache pass + resampled shading point + light sampler (128 vMF lobes) + GGX / cosine / vMF
    importance sampling with MIS + batched secondary trace (n*32 rays) + EnvMap + BRDF integration.
    The estimate is a ONE-sample-per-ray Monte-Carlo estimator built from one-sample secondary estimates:
    nothing averages the fp32 noise, and two discrete picks per path (categorical resampling on the primary
    and on every secondary ray) can flip on near-ties, so the check is statistical: tight on the bulk of the
    rays, loose on the maximum."""
    from nrc_amd import rc_ext
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    wn = common.weights_material_np(smooth)
    if smooth:
        rc = rc_smooth
    else:
        rc = rc_ext.RadianceCache(cfg, 0)
        rc.load_weights(wn)
    n = 128
    rays = nrc_amd.synthetic_rays(n, seed=77)
    rnd = material_ref.draw_randoms(cfg, n, seed=3)
    ref = material_ref.material_forward(common.to_torch(wn), cfg, common.rays_torch(rays), rnd)
    cres, mres = rc.render_material(rays.hot_fields(), rnd)
    torch.cuda.synchronize()
    same = rc.workspace("inds", np.int32)[:n] == ref["inds"][:, 0].numpy()
    assert same.mean() >= 0.98
    r = ref["render"]
    bulk, worst = (2e-5, 2e-3) if smooth else (3e-3, 5e-2)
    for k in MAT_KEYS_3 + ("acc", "indirect_occ", "material_roughness", "material_metalness", "material_F_0",
                           "ray_dists", "light_dists"):
        a = mres[k].cpu().numpy()
        b = r[k].numpy().reshape(a.shape)
        d = np.abs(a - b)[same]
        assert np.percentile(d, 95) <= bulk, (k, np.percentile(d, 95))
        assert d.max() <= worst, (k, d.max())
    # the cache_<k> keys are the plain cache pass
    assert np.abs(cres["rgb"].cpu().numpy() - r["cache_rgb"].numpy()).max() <= (1e-5 if smooth else RGB_TOL)
    assert np.abs(cres["acc"].cpu().numpy() - r["acc"].numpy()).max() <= (1e-5 if smooth else RGB_TOL)
    # per-stage intermediates on the smooth field
    if smooth:
        mat = rc.workspace("m_mat").reshape(n, 5)
        assert np.abs(mat[:, :3] - ref["material"]["albedo"].numpy())[same].max() <= 1e-4
        smp = rc.workspace("sec_samples").reshape(n, 32, 5)
        dd = ref["debug"]["diffuse"]
        assert np.abs(smp[:, 16:, :3] - dd["local_lightdirs"].numpy())[same].max() <= 1e-3
        assert np.abs(smp[:, 16:, 4] - dd["weight"][..., 0].numpy())[same].max() <= 1e-2
        ds = ref["debug"]["specular"]
        rel = np.abs(smp[:, :16, 3] - ds["pdf"][..., 0].numpy()) / (ds["pdf"][..., 0].numpy() + 1.0)
        assert rel[same].max() <= 5e-2


def test_forced_resampling_smooth_field_holds_1e4(rc_smooth):
    """Same pass on the smooth field with the oracle's picks handed over (rc_randoms.resample_inds): every output
    within the north-star 1e-4 L-inf (no percentile)."""
    from nrc_amd import rc_ext
    from oracle import cache_ref
    n = 256
    rays = nrc_amd.synthetic_rays(n)
    rng = np.random.Generator(np.random.PCG64(3))
    g = rng.gumbel(size=(n, 32)).astype(np.float32)
    jit = common.jitters(n, seed=4)
    ref = cache_ref.cache_forward(common.to_torch(common.weights_material_np(True)), nrc_amd.hotdog_config(),
                                  common.rays_torch(rays), [torch.from_numpy(j) for j in jit], resample=True,
                                  gumbel=torch.from_numpy(g), want_grad_normals=False)
    picks = ref["filtered_sampler_inds"][:, 0].numpy().astype(np.int32)
    mask = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE
    drawn = rc_smooth.render_rays(rays.hot_fields(), {"jitter": jit, "gumbel": g}, mask, outputs=["rgb"])
    torch.cuda.synchronize()
    assert (rc_smooth.workspace("inds", np.int32)[:n] == picks).mean() >= 0.99
    out = rc_smooth.render_rays(rays.hot_fields(), {"jitter": jit, "resample_inds": picks}, mask)
    torch.cuda.synchronize()
    r = ref["render"]
    for k in ("rgb", "acc", "diffuse_rgb", "specular_rgb", "direct_rgb", "indirect_rgb", "albedo_rgb", "means",
              "normals_pred", "distance_mean", "distance_median", "ray_dists"):
        a = out[k].cpu().numpy()
        d = np.abs(a - r[k].numpy().reshape(a.shape)).max()
        assert d <= RGB_TOL, (k, d)


MAT_ALL_KEYS = MAT_KEYS_3 + ("acc", "indirect_occ", "material_roughness", "material_metalness", "material_F_0",
                             "ray_dists", "light_dists")


def _material_with_picks(rc, rays, rnd, ref):
    """rc_render_material with the reference run's categorical picks handed over (rc_material_randoms.resample_inds /
    .sec_resample_inds): the two discrete steps per path can then not flip on a near-tie."""
    rnd2 = dict(rnd, gumbel=None, spec_gumbel=None, diff_gumbel=None,
                resample_inds=np.asarray(ref["inds"]).reshape(-1).astype(np.int32),
                spec_resample_inds=np.asarray(ref["spec_inds"]).reshape(-1).astype(np.int32),
                diff_resample_inds=np.asarray(ref["diff_inds"]).reshape(-1).astype(np.int32))
    cres, mres = rc.render_material(rays.hot_fields(), rnd2)
    torch.cuda.synchronize()
    return cres, mres


def test_material_stage_smooth_field_holds_1e4(rc_smooth):
    """SURVEY a21-a23 at the north-star tolerance: with the oracle's picks handed over, `rgb` and every material key
    agree with the fp32 oracle within 1e-4 L-inf on ALL rays (no percentile, no `same` mask), and so do the
    importance-sampling intermediates (directions, pdfs, MIS weights)."""
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    wn = common.weights_material_np(True)
    n = 128
    rays = nrc_amd.synthetic_rays(n, seed=77)
    rnd = material_ref.draw_randoms(cfg, n, seed=3)
    ref = material_ref.material_forward(common.to_torch(wn), cfg, common.rays_torch(rays), rnd)
    picks = dict(inds=ref["inds"][:, 0].numpy(), spec_inds=ref["debug"]["specular"]["inds"].numpy(),
                 diff_inds=ref["debug"]["diffuse"]["inds"].numpy())
    # the Gumbel draws themselves: nearly all picks equal (a near-tie may flip)
    rc_smooth.render_material(rays.hot_fields(), rnd)
    torch.cuda.synchronize()
    assert (rc_smooth.workspace("inds", np.int32)[:n] == picks["inds"]).mean() >= 0.98
    cres, mres = _material_with_picks(rc_smooth, rays, rnd, picks)
    rnd_p = dict(rnd, resample_inds=picks["inds"], spec_resample_inds=picks["spec_inds"], diff_resample_inds=picks["diff_inds"])
    ref64 = material_ref.material_forward(common.to_torch(wn, torch.float64), cfg, common.rays_torch(rays, torch.float64), rnd_p)
    assert np.array_equal(rc_smooth.workspace("inds", np.int32)[:n], picks["inds"])
    assert np.array_equal(rc_smooth.workspace("s:inds", np.int32)[:n * 32],
                          np.concatenate([picks["spec_inds"], picks["diff_inds"]]))
    r = ref["render"]
    for k in MAT_ALL_KEYS:
        a = mres[k].cpu().numpy()
        d = np.abs(a - r[k].numpy().reshape(a.shape)).max()
        assert d <= RGB_TOL, (k, d)
    assert np.abs(cres["rgb"].cpu().numpy() - r["cache_rgb"].numpy()).max() <= 1e-5
    # importance sampling intermediates (a21): local directions, pdf, MIS weight
    smp = rc_smooth.workspace("sec_samples").reshape(n, 32, 5)
    d_n = float(np.abs(rc_smooth.workspace("m_nrm").reshape(n, 3) - ref64["filtered"]["normals_to_use"][:, 0].numpy()).max()) + 1e-6
    assert d_n <= RGB_TOL
    for blk, name in ((slice(0, 16), "specular"), (slice(16, 32), "diffuse")):
        dd = ref["debug"][name]
        assert np.abs(smp[:, blk, :3] - dd["local_lightdirs"].numpy()).max() <= RGB_TOL
        pdf = dd["pdf"][..., 0].numpy()
        # pdf = D cos / (4 wo.h) (render_utils.py:501-531).  wo.h is a cancelling dot product (0.012 from terms of 0.055
        # on the worst sample: the view direction lies below the predicted normal's tangent plane), so the pdf inherits
        # the shading normal's own fp32 error d_n -- asserted <= 1e-4 above, measured here -- as d_n / (wo.h) relative:
        # the fp32 and fp64 ORACLES differ by 3.3e-2 where pdfs reach 1.8e3.  First-order bound with that measured d_n;
        # the estimator divides a lobe carrying the same factor by this pdf, so the OUTPUTS hold the plain 1e-4.
        d64 = ref64["debug"][name]
        p64 = d64["pdf"][..., 0].numpy()
        wi, wo = d64["local_lightdirs"].numpy(), d64["local_viewdirs"].numpy()
        hv = wi + wo
        hv = hv / np.maximum(np.linalg.norm(hv, axis=-1, keepdims=True), 1e-30)
        wdoth = np.maximum(np.abs((wo * hv).sum(-1)), 1e-12)
        cond = (4.0 * d_n / wdoth) if name == "specular" else 0.0
        assert (np.abs(smp[:, blk, 3] - p64) <= RGB_TOL * (1.0 + p64) + p64 * cond).all()
        assert np.abs(smp[:, blk, 4] - dd["weight"][..., 0].numpy()).max() <= RGB_TOL
    sec_rgb = rc_smooth.workspace("sec_rgb").reshape(n * 32, 3)
    ref_rgb = np.concatenate([ref["debug"]["specular"]["rgb"].numpy(), ref["debug"]["diffuse"]["rgb"].numpy()])
    # per-secondary-ray radiance: ONE shaded sample times w / p of its pick (not an output: the outputs above average
    # 16 of them per lobe and hold 1e-4)
    assert np.abs(sec_rgb - ref_rgb).max() <= 5e-4
    assert np.abs(sec_rgb - ref_rgb).mean() <= 1e-5


def test_material_stage_golden_fp64(rc_smooth):
    """tests/golden/hotdog_material_64_smooth.npz: the fp64 oracle's material stage (configs[2]) with its picks stored."""
    from oracle import material_ref
    g = np.load(os.path.join(GOLD, "hotdog_material_64_smooth.npz"))
    n, rays_seed, rnd_seed = (int(v) for v in g["meta"])
    cfg = nrc_amd.hotdog_config()
    rays = nrc_amd.synthetic_rays(n, seed=rays_seed)
    rnd = material_ref.draw_randoms(cfg, n, seed=rnd_seed)
    picks = dict(inds=g["inds"], spec_inds=g["spec_inds"], diff_inds=g["diff_inds"])
    cres, mres = _material_with_picks(rc_smooth, rays, rnd, picks)
    for k in MAT_ALL_KEYS:
        a = mres[k].cpu().numpy()
        d = np.abs(a - g["render_" + k].reshape(a.shape)).max()
        # colours at the north-star 1e-4; the geometry extras (unit normals from a normalised 3-vector of the MLP,
        # positions, distances) at the 5e-4 this file gives them against float64
        assert d <= (5e-4 if k in ("means", "normals_to_use", "ray_dists", "light_dists") else RGB_TOL), (k, d)
    assert np.abs(cres["rgb"].cpu().numpy() - g["render_cache_rgb"]).max() <= 1e-5


def _smooth_rc_at(K):
    from nrc_amd import rc_ext
    cfg = nrc_amd.hotdog_config(num_secondary_samples=K)
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(common.weights_material_np(smooth=True))
    return cfg, rc


def test_material_stage_k10_rounds_half_to_even_like_the_randoms():
    """K = 10 at diffuse_sample_fraction 0.5: Kd = 5 and Kc = round(2.5) = 2 with Python's round, which sizes cos_u1/u2
    [n, 2] and vmf_v [n, 3, 2] (oracle.material_ref.draw_randoms, prng.material_split).  material_check used lround
    (Kc = 3): cos_u1 read past its end, vmf_v / vmf_tmp at the wrong stride.  Picks handed over, smooth weights: every
    material key within the 1e-4 of test_material_stage_smooth_field_holds_1e4."""
    from oracle import material_ref
    cfg, rc = _smooth_rc_at(10)
    n = 5
    rays = nrc_amd.synthetic_rays(n, seed=77)
    rnd = material_ref.draw_randoms(cfg, n, seed=3)
    assert rnd["spec_u1"].shape == (n, 5) and rnd["cos_u1"].shape == (n, 2) and rnd["vmf_v"].shape == (n, 3, 2)
    ref = material_ref.material_forward(common.to_torch(common.weights_material_np(True)), cfg, common.rays_torch(rays), rnd)
    picks = dict(inds=ref["inds"][:, 0].numpy(), spec_inds=ref["debug"]["specular"]["inds"].numpy(),
                 diff_inds=ref["debug"]["diffuse"]["inds"].numpy())
    cres, mres = _material_with_picks(rc, rays, rnd, picks)
    assert np.array_equal(rc.workspace("inds", np.int32)[:n], picks["inds"])
    r = ref["render"]
    for k in MAT_ALL_KEYS:
        a = mres[k].cpu().numpy()
        d = np.abs(a - r[k].numpy().reshape(a.shape)).max()
        print(f"K=10 {k}: {d:.3e}")
        assert d <= RGB_TOL, (k, d)
    smp = rc.workspace("sec_samples")[:n * 10 * 5].reshape(n, 10, 5)
    for blk, name in ((slice(0, 5), "specular"), (slice(5, 10), "diffuse")):
        assert np.abs(smp[:, blk, :3] - ref["debug"][name]["local_lightdirs"].numpy()).max() <= RGB_TOL, name


def test_material_stage_k5_is_refused_with_the_outputs_untouched():
    """K = 5 at 0.5: round(2.5) + round(2.5) = 4, not 5 -- refused with RC_ERR_UNSUPPORTED as rc_material_randoms_plan
    refuses it, before anything is launched: every float of both output tables keeps the value it had."""
    import ctypes as C
    from nrc_amd import rc_ext
    from oracle import material_ref
    cfg, rc = _smooth_rc_at(5)
    n = 5
    rays = nrc_amd.synthetic_rays(n, seed=77)
    rnd = material_ref.draw_randoms(cfg, n, seed=3)
    r, held, n_ = rc._rays_struct(rays.hot_fields())
    crnd, mr = rc._material_randoms(rnd, n, 5, held)
    c_names = [nm for nm, _ in rc_ext.OUTPUTS if nm not in ("env_map_rgb", "rgb_no_env")]
    m_names = [nm for nm, _ in rc_ext.MAT_OUTPUTS]
    cshape = lambda nm: (n, 3) if rc_ext.OUTPUTS[rc_ext.OUTPUT_ID[nm]][1] == 3 else (n,)
    mshape = lambda nm: (n, 3) if rc_ext.MAT_OUTPUTS[rc_ext.MAT_OUTPUT_ID[nm]][1] == 3 else (n,)
    fill = lambda shape: torch.full(shape, 0.625, dtype=torch.float32, device="cuda:0")
    cres, cout = rc._outputs(rc_ext.OUTPUTS, c_names, cshape, {nm: fill(cshape(nm)) for nm in c_names})
    mres, mout = rc._outputs(rc_ext.MAT_OUTPUTS, m_names, mshape, {nm: fill(mshape(nm)) for nm in m_names})
    code = rc.lib.rc_render_material(rc._h, C.byref(r), n, C.byref(crnd), C.byref(mr), 5, C.byref(cout), C.byref(mout),
                                     rc._stream())
    torch.cuda.synchronize()
    assert code == -5, code                                             # RC_ERR_UNSUPPORTED
    assert b"Ks + Kd" in (rc.lib.rc_last_error(rc._h) or b"")
    for nm, t in list(cres.items()) + list(mres.items()):
        assert bool((t == 0.625).all()), nm
    with pytest.raises(rc_ext.RcError) as e:
        rc.render_material(rays.hot_fields(), rnd)
    assert e.value.code == -5


def test_material_stage_white_noise_with_picks(rc_smooth):
    """White-noise tables with the picks handed over: every ray is compared (no `same` mask).  One-ulp differences of the
    secondary sample positions are amplified by the 2048-cell random tables (the fp32 and fp64 oracles differ by 1e-3
    here), so the bound stays statistical for this weight set; the 1e-4 claim is the smooth-field test above."""
    from nrc_amd import rc_ext
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    wn = common.weights_material_np(False)
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(wn)
    n = 128
    rays = nrc_amd.synthetic_rays(n, seed=77)
    rnd = material_ref.draw_randoms(cfg, n, seed=3)
    ref = material_ref.material_forward(common.to_torch(wn), cfg, common.rays_torch(rays), rnd)
    picks = dict(inds=ref["inds"][:, 0].numpy(), spec_inds=ref["debug"]["specular"]["inds"].numpy(),
                 diff_inds=ref["debug"]["diffuse"]["inds"].numpy())
    cres, mres = _material_with_picks(rc, rays, rnd, picks)
    r = ref["render"]
    for k in MAT_ALL_KEYS:
        a = mres[k].cpu().numpy()
        d = np.abs(a - r[k].numpy().reshape(a.shape))
        assert np.percentile(d, 95) <= 1e-3, (k, np.percentile(d, 95))
        assert d.max() <= 2e-2, (k, d.max())


def test_material_stage_reports_missing_weights(rc):
    from nrc_amd import rc_ext
    from oracle import material_ref
    rays = nrc_amd.synthetic_rays(8)
    rnd = material_ref.draw_randoms(nrc_amd.hotdog_config(), 8)
    with pytest.raises(rc_ext.RcError, match="missing weight"):
        rc.render_material(rays.hot_fields(), rnd)      # `rc` carries the cache-only weight set


# ---------------------------------------------------------------------------------------------
# time-resolved cache (BASELINE configs[4])
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rc_transient():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    h.load_weights(common.weights_transient_np())
    return h


def _render_transient(h, n, jitter_seed=None, **kw):
    rays = nrc_amd.synthetic_transient_rays(n)
    rnd = None if jitter_seed is None else {"jitter": common.jitters(n, seed=jitter_seed)}
    out = h.render_transient(rays.hot_fields(), rnd, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


TRANSIENT_3 = ("integrated_rgb", "direct_rgb", "indirect_rgb", "diffuse_rgb", "specular_rgb", "albedo_rgb", "occ", "indirect_occ",
               "irradiance_rgb", "light_radiance_rgb", "n_dot_l_rgb", "direct_diffuse_rgb", "direct_specular_rgb",
               "indirect_diffuse_rgb", "indirect_specular_rgb")


@pytest.mark.parametrize("n,jitter_seed", [(48, None), (37, 9)])
def test_transient_render_vs_oracle_fp32(rc_transient, n, jitter_seed):
    """Every output of rc_render_transient against the fp32 oracle.  Per-bin radiance is O(1e-2) (the histogram
    spreads O(1) radiance over 700 bins): 1e-4 relative to the integrated radiance is the RGB budget."""
    out = _render_transient(rc_transient, n, jitter_seed)
    ref = {k: v.numpy() for k, v in common.oracle_transient(n, jitter_seed)["render"].items()}
    for k in ("rgb", "transient_direct_viz", "transient_indirect_viz", "transient_indirect_diffuse", "transient_indirect_specular"):
        assert out[k].shape == (n, 700, 3)
        assert np.abs(out[k] - ref[k]).max() <= 2e-5, k
    for k in TRANSIENT_3:
        assert np.abs(out[k] - ref[k]).max() <= RGB_TOL * max(1.0, np.abs(ref[k]).max()), k
    assert np.abs(out["direct_rgb_viz"] - ref["direct_rgb_viz"]).max() <= 2e-5 * np.abs(ref["direct_rgb_viz"]).max()
    assert np.abs(out["acc"] - ref["acc"]).max() <= RGB_TOL
    for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
        assert np.abs(out[k] - ref[k]).max() <= 1e-3, k
    for k in ("means", "normals_pred"):
        assert np.abs(out[k] - ref[k]).max() <= 5e-4, k
    for k in ("ray_dists", "light_dists"):
        assert np.abs(out[k] - ref[k][:, 0]).max() <= 5e-4, k


@pytest.mark.parametrize("name", ["transient_16_det.npz", "transient_16_jit.npz"])
def test_transient_render_vs_fp64_golden(rc_transient, name):
    g = dict(np.load(os.path.join(GOLD, name)))
    n, js = int(g["meta"][0]), int(g["meta"][1])
    out = _render_transient(rc_transient, n, None if js < 0 else js)
    assert np.abs(out["rgb"] - g["render_rgb"]).max() <= 5e-5
    assert np.abs(out["integrated_rgb"] - g["render_integrated_rgb"]).max() <= 2e-4 * np.abs(g["render_integrated_rgb"]).max()
    assert np.abs(out["acc"] - g["render_acc"]).max() <= RGB_TOL


def test_transient_far_samples_run_only_their_tile_range(rc_transient):
    """k_transient_bins runs the column tiles between the first and the last bin ANY sample of the workgroup's rays keeps
    (zero_invalid_bins, render_utils.py:1699-1767) and writes exact zeros elsewhere.  Rays whose samples all lie 2.6-3.9
    from camera and light keep bins ~[160, 440]: the range starts well inside the histogram on both sides."""
    from oracle import transient_ref
    n = 21
    rays = nrc_amd.synthetic_transient_rays(n, seed=77, near=2.6, far=3.9)
    cfg = nrc_amd.cornell_transient_config()
    ref = transient_ref.transient_forward(common.to_torch(common.weights_transient_np()), cfg, common.rays_torch(rays), None, None)["render"]
    ref = {k: v.numpy() for k, v in ref.items()}
    out = rc_transient.render_transient(rays.hot_fields(), None)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    live = np.abs(ref["transient_indirect_diffuse"]).sum((0, 2)) > 0
    assert live[:100].sum() == 0 and live[500:].sum() == 0 and live.sum() > 100          # the case is what it claims to be
    for k in ("rgb", "transient_direct_viz", "transient_indirect_viz", "transient_indirect_diffuse", "transient_indirect_specular"):
        assert np.abs(out[k] - ref[k]).max() <= 2e-5, k
    for k in ("transient_indirect_diffuse", "transient_indirect_specular"):
        assert not out[k][:, ~live].any(), k
    for k in TRANSIENT_3:
        assert np.abs(out[k] - ref[k]).max() <= RGB_TOL * max(1.0, np.abs(ref[k]).max()), k


def test_transient_properties_full_batch_1024(rc_transient):
    """BASELINE-size batch: size-independent properties of the per-bin composite instead of an oracle run."""
    n = 1024
    out = _render_transient(rc_transient, n, 3)
    rgb = out["rgb"]
    assert rgb.shape == (n, 700, 3) and np.all(np.isfinite(rgb)) and rgb.min() >= 0
    assert np.abs(rgb - (out["transient_direct_viz"] + out["transient_indirect_viz"])).max() <= 1e-7
    s = out["integrated_rgb"]
    assert np.abs(rgb.sum(1, dtype=np.float64) - s).max() <= 1e-4 * max(1.0, s.max())
    assert np.abs(out["direct_rgb"] + out["indirect_rgb"] - s).max() <= 2e-5 * max(1.0, s.max())
    # rgb composites: diffuse + specular = direct + indirect (per sample, before any time shift)
    lhs = out["diffuse_rgb"] + out["specular_rgb"]
    rhs = out["direct_diffuse_rgb"] + out["direct_specular_rgb"] + out["indirect_diffuse_rgb"] + out["indirect_specular_rgb"]
    assert np.abs(lhs - rhs).max() <= 2e-5 * max(1.0, lhs.max())
    # the unshifted per-bin composites add up to the per-sample bin sums
    ti = out["transient_indirect_diffuse"].sum(1, dtype=np.float64)
    assert np.abs(ti - out["indirect_diffuse_rgb"]).max() <= 1e-4 * max(1.0, ti.max())
    # time shift and temporal filter only move radiance (or drop it at the ends)
    unshifted = (out["transient_indirect_diffuse"] + out["transient_indirect_specular"]).sum(1, dtype=np.float64)
    assert np.all(out["indirect_rgb"] <= unshifted * (1 + 1e-4) + 1e-5)
    assert np.abs(out["indirect_occ"] - out["acc"][:, None]).max() <= 2e-6
    # determinism (the histogram accumulation order is fixed)
    again = _render_transient(rc_transient, n, 3, outputs=["rgb"])
    assert np.array_equal(again["rgb"], rgb)


def test_transient_dense_field_samples_share_bins():
    """+6 on the density bias: the weight sits on a few adjacent samples whose time shifts coincide, so both
    half-waves of k_transient_bins add into the same histogram entries."""
    from nrc_amd import rc_ext
    n = 24
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    h.load_weights(common.weights_transient_np(False, 6.0))
    rays = nrc_amd.synthetic_transient_rays(n)
    out = {k: v.cpu().numpy() for k, v in h.render_transient(rays.hot_fields(), {"jitter": common.jitters(n, seed=5)}).items()}
    r = {k: v.numpy() for k, v in common.oracle_transient(n, jitter_seed=5, density_shift=6.0)["render"].items()}
    assert r["acc"].min() > 0.99
    for k in ("rgb", "transient_direct_viz", "transient_indirect_viz"):
        assert np.abs(out[k] - r[k]).max() <= 1e-4 * max(1.0, np.abs(r[k]).max()), k
    for k in ("indirect_rgb", "direct_rgb", "integrated_rgb"):
        assert np.abs(out[k] - r[k]).max() <= 1e-4 * max(1.0, np.abs(r[k]).max()), k


def test_transient_direct_spill_into_next_ray(rc_transient):
    """The direct scatter indexes the flattened [rays * bins] histogram (render.py:447-475): path lengths beyond
    700 bins of ray r show up at the start of ray r + 1 -- and nowhere for the last ray of the batch."""
    n = 64
    rays = nrc_amd.synthetic_transient_rays(n)
    f = rays.hot_fields()
    full = rc_transient.render_transient(f, None, outputs=["transient_direct_viz"])["transient_direct_viz"].cpu().numpy()
    half = {k: np.asarray(v)[n // 2:] for k, v in f.items()}
    part = rc_transient.render_transient(half, None, outputs=["transient_direct_viz"])["transient_direct_viz"].cpu().numpy()
    # ray n/2 has a predecessor in the full batch and none in the half batch: only its early bins may differ
    d = np.abs(full[n // 2] - part[0])
    assert d[200:].max() == 0.0
    assert np.array_equal(full[n // 2 + 1:], part[1:])
    ref = common.oracle_transient(n)["render"]["transient_direct_viz"].numpy()
    assert np.abs(full - ref).max() <= 2e-5
    assert ref[1:, :100].max() > 0           # the spill is really there in this geometry (far = 4, light at the camera)


def test_transient_model_apply_and_errors():
    from nrc_amd import model as m, rc_ext
    mdl = m.Model(nrc_amd.cornell_transient_config(), 0)
    mdl.load_variables(common.weights_transient_np())
    rays = nrc_amd.synthetic_transient_rays(16)
    r = mdl.apply(None, None, rays, passes=("cache",))["render"]
    assert tuple(r["rgb"].shape) == (16, 700, 3) and tuple(r["integrated_rgb"].shape) == (16, 3)
    for k in ("transient_direct_viz", "transient_indirect_viz", "cache_rgb", "cache_diffuse_rgb", "acc", "distance_median",
              "normals_to_use", "lossmult", "vignette", "ambient_rgb"):
        assert k in r, k
    with pytest.raises(NotImplementedError):
        mdl.apply(None, None, rays, passes=("cache",), resample=True)
    with pytest.raises(rc_ext.RcError):        # steady-state entry point on a transient handle
        mdl.rc.render_rays(rays.hot_fields(), None)
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    w = dict(common.weights_transient_np())
    w.pop("params/Cache/Shader/light_power")
    h.load_weights(w)
    with pytest.raises(rc_ext.RcError, match="light_power"):
        h.render_transient(rays.hot_fields(), None)
    with pytest.raises(rc_ext.RcError):        # hotdog weights do not fit the transient inventory
        rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0).load_weights(common.weights_np())


def test_transient_occlusions_shadow_rays_vs_oracle():
    """use_occlusions (vis_only): one weights-only shadow ray per shaded sample through the secondary-ray sampler
    (analytic normals for the near offset, power-ladder distances, far = distance to the light - light_near).  Dense
    field (+6 on the density bias) so that a good part of the shadow rays saturates."""
    from nrc_amd import rc_ext
    n = 24
    cfg = nrc_amd.cornell_transient_config(use_occlusions=True)
    h = rc_ext.RadianceCache(cfg, 0)
    h.load_weights(common.weights_transient_np(False, 6.0))
    rays = nrc_amd.synthetic_transient_rays(n)
    rnd = {"jitter": common.jitters(n, seed=5), "shadow_jitter": common.shadow_jitters(n * 32, 13)}
    out = {k: v.cpu().numpy() for k, v in h.render_transient(rays.hot_fields(), rnd).items()}
    ref = common.oracle_transient(n, jitter_seed=5, occlusions=True, shadow_jitter_seed=13, density_shift=6.0)
    acc_ref = ref["shadow_acc"].numpy().reshape(-1)
    acc = h.workspace("sh_acc")[: n * 32]
    # shadow rays start ON the surface of a white-noise field: same amplification of position ulps as for the
    # primary rays, plus the discontinuous analytic normals that set their near plane
    d = np.abs(acc - acc_ref)
    assert np.median(d) <= 1e-5 and d.mean() <= 2e-3
    occ_ref = ref["shader"]["occ"].numpy()[..., 0].reshape(-1)
    lit = ref["shader"]["n_dot_l_rgb"].numpy()[..., 0].reshape(-1) > 0
    assert 0.02 < (occ_ref[lit] > 0).mean() < 0.98
    r = {k: v.numpy() for k, v in ref["render"].items()}
    # rays whose thresholded occlusion pattern agrees (a shadow acc next to 0.9 may flip): tight; all rays: loose
    same = np.all(((acc > 0.9) == (acc_ref > 0.9)).reshape(n, 32), axis=1)
    assert same.mean() >= 0.9
    same[1:] &= same[:-1].copy()          # the direct scatter of ray r - 1 spills into ray r (render.py:447-475)
    for k in ("rgb", "transient_direct_viz", "transient_indirect_viz"):
        assert np.abs(out[k][same] - r[k][same]).max() <= 5e-5, k
    for k in ("occ", "direct_rgb", "integrated_rgb", "diffuse_rgb", "specular_rgb"):
        assert np.abs(out[k][same] - r[k][same]).max() <= 2e-4 * max(1.0, np.abs(r[k]).max()), k
    assert np.abs(out["transient_indirect_viz"] - r["transient_indirect_viz"]).max() <= 5e-5     # not touched by the shadows


# ---------------------------------------------------------------------------------------------
# sizes beyond one workgroup per compute unit, empty / tiny transient batches
# ---------------------------------------------------------------------------------------------
def test_large_ragged_batch_fused_equals_staged(rc):
    """18 433 rays (4609 workgroups, the last one with a single live wave): every output of the fused kernel
    bitwise equal to the launch-per-stage plan, and the oracle on a strided subset of the rays."""
    n = 18433
    out = _render(rc, n, 4)
    st = _render(rc, n, 4, fused=False)
    for k, v in out.items():
        assert np.array_equal(st[k], v), k
    assert np.all(np.isfinite(out["rgb"])) and out["acc"].min() >= 0 and out["acc"].max() <= 1 + 1e-6
    sub = np.arange(0, n, 257)
    rays = nrc_amd.synthetic_rays(n)
    f = {k: np.asarray(v)[sub] for k, v in rays.hot_fields().items()}
    jit = [j[sub] for j in common.jitters(n, seed=4)]
    from oracle import cache_ref
    ref = cache_ref.cache_forward(common.weights_torch(), nrc_amd.hotdog_config(), common.rays_dict_torch(f),
                                  [torch.from_numpy(j) for j in jit], want_grad_normals=False)["render"]
    assert np.abs(out["rgb"][sub] - ref["rgb"].numpy()).max() <= RGB_TOL
    assert np.abs(out["acc"][sub] - ref["acc"].numpy()).max() <= RGB_TOL


def test_transient_empty_and_single_ray(rc_transient):
    rays = nrc_amd.synthetic_transient_rays(4)
    f0 = {k: np.asarray(v)[:0] for k, v in rays.hot_fields().items()}
    out = rc_transient.render_transient(f0, None, outputs=["rgb", "acc"])
    assert tuple(out["rgb"].shape) == (0, 700, 3) and tuple(out["acc"].shape) == (0,)
    one = _render_transient(rc_transient, 1)
    ref = common.oracle_transient(1)["render"]
    assert np.abs(one["rgb"] - ref["rgb"].numpy()).max() <= 2e-5
    assert np.abs(one["integrated_rgb"] - ref["integrated_rgb"].numpy()).max() <= RGB_TOL * max(1.0, float(ref["integrated_rgb"].abs().max()))


def test_transient_render_image_keys_and_shapes():
    """models.render_image with the time-resolved model: `rgb` is [H, W, 700, 3]; every `transient*` key except the two
    *_viz ones is dropped (internal/models.py:2403, 2459-2472); chunks are edge-padded."""
    from nrc_amd import model as M
    cfg = nrc_amd.cornell_transient_config(render_chunk_size=16)
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_transient_np())
    H, W = 5, 6
    flat = nrc_amd.synthetic_transient_rays(H * W)
    rays = flat.tree_map(lambda r: np.asarray(r).reshape((H, W) + np.asarray(r).shape[1:]))
    img, _ = M.render_image(M.bind_render_fn(M.create_render_fn(m)), None, rays, cfg, ("cache",), verbose=False)
    assert img["rgb"].shape == (H, W, 700, 3) and img["integrated_rgb"].shape == (H, W, 3) and img["acc"].shape == (H, W)
    assert "transient_direct_viz" in img and "transient_indirect_viz" in img
    assert not any(("transient" in k) and k not in ("transient_direct_viz", "transient_indirect_viz") for k in img)
    # chunk 0 (16 rays) of the image == the same 16 rays rendered directly
    direct = m.rc.render_transient({k: np.asarray(v)[:16] for k, v in flat.hot_fields().items()}, None, outputs=["rgb"])
    assert np.array_equal(img["rgb"].reshape(H * W, 700, 3)[:16], direct["rgb"].cpu().numpy())


@pytest.mark.parametrize("n,plan", [(4097, 1), (4097, 0), (25001, 1)])
def test_repeated_launches_are_bitwise_stable_with_workgroups_out_of_phase(rc, n, plan):
    """More rays than one round of workgroups: those sharing a CU then run DIFFERENT phases of the kernel at the same time.
    This is the screen that caught the instability of the two-wave kernel with every layer in the split-MFMA form
    (csrc/rc_dev_mlp.h INSTABILITY, tools/stress_repeat.py: one ray in a few hundred off by 1e-3 in most launches of a
    4097-ray batch); the plans
    the library runs must come out bit for bit the same every time."""
    from nrc_amd import rc_ext
    assert rc_ext.mlp_arithmetic() in ("f32-mfma", "bf16x3-split")
    rays = nrc_amd.synthetic_rays(n, seed=78)
    f = {k: torch.from_numpy(np.asarray(v)).cuda().contiguous() for k, v in rays.hot_fields().items()}
    rnd = {"jitter": [torch.from_numpy(j).cuda() for j in common.jitters(n, seed=6)]}
    rc.set_graph_mode(0)
    rc.set_fused(plan)
    try:
        first = {k: v.clone() for k, v in rc.render_rays(f, rnd).items()}
        for it in range(12 if n < 10000 else 4):
            out = rc.render_rays(f, rnd)
            torch.cuda.synchronize()
            for k, v in out.items():
                assert torch.equal(v, first[k]), (it, k, float((v - first[k]).abs().max()))
    finally:
        rc.set_fused(True)
        rc.set_graph_mode(1)


def test_repeated_launches_are_bitwise_stable(rc):
    """Race check of the weight-ring / LDS protocols: the same batch rendered many times (eager launches, two streams in
    flight) must come out bit for bit the same -- nothing in the cache pass depends on arrival order."""
    n = 1024
    rays = nrc_amd.synthetic_rays(n, seed=77)
    f = {k: torch.from_numpy(np.asarray(v)).cuda().contiguous() for k, v in rays.hot_fields().items()}
    rnd = {"jitter": [torch.from_numpy(j).cuda() for j in common.jitters(n, seed=5)]}
    rc.set_graph_mode(0)
    try:
        first = {k: v.clone() for k, v in rc.render_rays(f, rnd).items()}
        side = torch.cuda.Stream()
        for it in range(150):
            if it % 2:
                with torch.cuda.stream(side):
                    out = rc.render_rays(f, rnd)
                side.synchronize()
            else:
                out = rc.render_rays(f, rnd)
                torch.cuda.synchronize()
            for k, v in out.items():
                assert torch.equal(v, first[k]), (it, k)
    finally:
        rc.set_graph_mode(1)


def test_transient_repeated_launches_are_stable():
    """k_transient_bins adds into LDS histograms with plain read-add-writes; the lane / half-wave ownership makes that
    deterministic: repeated launches agree bit for bit."""
    from nrc_amd import rc_ext
    cfg = nrc_amd.cornell_transient_config()
    h = rc_ext.RadianceCache(cfg, 0)
    h.load_weights(common.weights_transient_np())
    rays = nrc_amd.synthetic_transient_rays(256)
    f = {k: torch.from_numpy(np.asarray(v)).cuda().contiguous() for k, v in rays.hot_fields().items()}
    keys = ["rgb", "integrated_rgb", "transient_indirect_viz", "transient_direct_viz"]
    first = {k: v.clone() for k, v in h.render_transient(f, None, outputs=keys).items()}
    for it in range(40):
        out = h.render_transient(f, None, outputs=keys)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(out[k], first[k]), (it, k)


def test_lean_resampling_pass_equals_the_full_one(rc):
    """A resampling pass that is not asked for normals recomputes the last level's hidden feature / predicted normals
    for the ONE picked sample per ray instead of storing them for all 32: same per-point arithmetic, same bits."""
    from nrc_amd import rc_ext
    n = 777
    rays, rnd = common.secondary_case(n, seed=13)
    mask = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY
    full = rc.render_rays(rays, rnd, mask)                                   # every output incl. normals: full pass
    keys = [k for k in full if "normals" not in k]
    lean = rc.render_rays(rays, rnd, mask, outputs=keys)                     # lean pass
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(lean[k], full[k]), k
    # primary rays with resample=True
    g = np.random.Generator(np.random.PCG64(3)).gumbel(size=(n, 32)).astype(np.float32)
    prays = nrc_amd.synthetic_rays(n, seed=14).hot_fields()
    prnd = {"jitter": common.jitters(n, seed=2), "gumbel": g}
    pmask = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE
    pfull = rc.render_rays(prays, prnd, pmask)
    plean = rc.render_rays(prays, prnd, pmask, outputs=["rgb", "acc", "diffuse_rgb", "specular_rgb"])
    torch.cuda.synchronize()
    for k in plean:
        assert torch.equal(plean[k], pfull[k]), k


@pytest.mark.parametrize("occ", [False, True])
def test_transient_fused_front_end_equals_the_staged_one(occ):
    """The proposal sampler of the time-resolved cache as ONE launch (FRONT variant of the fused kernel, power-ladder
    distances) hands the stages behind it bit for bit what the launch-per-stage front end does."""
    from nrc_amd import rc_ext
    cfg = nrc_amd.cornell_transient_config(use_occlusions=occ)
    h = rc_ext.RadianceCache(cfg, 0)
    h.load_weights(common.weights_transient_np())
    n = 203
    rays = nrc_amd.synthetic_transient_rays(n)
    rnd = {"jitter": common.jitters(n, seed=4)}
    if occ:
        rnd["shadow_jitter"] = common.shadow_jitters(n * 32, seed=6)      # one shadow ray per shaded sample
    a = h.render_transient(rays.hot_fields(), rnd)
    h.set_fused(False)
    b = h.render_transient(rays.hot_fields(), rnd)
    h.set_fused(True)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_nan_density_distance_mean_is_first_fence_post():
    """oracle/JAX_CALLS.md N1 + N3 on the device: a NaN `output_density_layer` bias on the last level makes every density
    of that level NaN (math.safe_exp's jnp.clip propagates it), hence the weights and the log-distance expectation;
    `jnp.nan_to_num(x, jnp.inf)` (render.py:233-237: jnp.inf binds to `copy`) turns that into 0.0 and the clip lifts it
    to tdist[..., 0] -- not to tdist[..., -1], which the `nan=inf` reading of rounds 1-3 produced.  All three launch
    plans (two-wave fused, launch-per-stage, one-wave fused) and the oracle."""
    from nrc_amd import rc_ext
    from oracle import cache_ref
    n = 70
    cfg = nrc_amd.hotdog_config()
    w = dict(common.weights_np())
    key = "params/Cache/Sampler/MLP_2/output_density_layer/bias"
    w[key] = np.full_like(w[key], np.nan)
    h = rc_ext.RadianceCache(cfg, 0)
    h.load_weights(w)
    rays = nrc_amd.synthetic_rays(n)
    ref = cache_ref.cache_forward(common.to_torch(w), cfg, common.rays_torch(rays), None, want_grad_normals=False)
    td_ref = ref["sampler"][-1]["tdist"].numpy()
    assert np.array_equal(ref["render"]["distance_mean"].numpy(), td_ref[:, 0])
    for plan in (1, 0, 3):
        h.set_fused(plan)
        out = h.render_rays(rays.hot_fields(), None, outputs=["distance_mean", "acc", "rgb"])
        torch.cuda.synchronize()
        dm = out["distance_mean"].cpu().numpy()
        assert np.isnan(out["acc"].cpu().numpy()).all(), plan           # the NaN really reached the integrator
        if plan == 0:
            td = h.workspace("tdist2").reshape(n, 33)
            assert np.array_equal(dm, td[:, 0]), plan
            assert np.abs(td - td_ref).max() <= 1e-4
        assert np.isfinite(dm).all() and np.abs(dm - td_ref[:, 0]).max() <= 1e-4, plan
        assert (dm < td_ref[:, -1] - 0.1).all(), plan                  # the old reading gave the last fence post
