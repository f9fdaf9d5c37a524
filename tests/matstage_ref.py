"""The material stage's forward kernels of csrc/rc_material.hip (k_material_head<4|16>, k_light_head, k_shading_heads,
k_brdf_sample, k_material_composite_all, k_material_integrate) on their own contracts, RcMatHeadArgs / RcLightHeadArgs /
RcBrdfSampleArgs / RcMatIntegrateArgs (csrc/rc_internal.h) and the reference lines cited in the header of rc_material.hip:
the cases, one reference of every kernel that runs in fp64 (`ft = np.float64`: the contract) and in float32 (`ft =
np.float32`: the kernels' arithmetic restated step by step, sequential sums, no contraction), the tolerances, mutated
references and the kernel table of the driver tests/matstage_check.hip.  numpy only.  Buffers, guards, canaries, the case
file and the result file are tests/sample_ref.py's (Cases, check, render, write_case_file, read_results) on this module's
kernel table; a later launch may read an earlier launch's output (heads -> sampler -> integrate) and is then held to its
own contract on the values that came back from the device (on the CPU: the producer's float32 restatement).

Tolerances (u = 2^-24, every bound is on |device - fp64 reference| unless it says otherwise):
  dense layers   a sum of K products + bias in any order: 2 (K + 2) u (sum |a| |b| + |bias|), the gemm test's bound; the
                 error of the inputs is carried through (ReLU is 1-Lipschitz): + sum err_a |b|
  sigmoid        s = 1 / (1 + exp(-x)): s' <= 1/4, exp, add, divide <= 4 u:  err_x / 4 + u |x| / 4 + 4 u; roughness
                 s (1 - r0) + r0: that (1 - r0) + 3 u
  kappa          softplus is 1-Lipschitz: err_q + u (|q| + 1) + 4 u (1 + kappa); the clamp at 50 is held exactly where
                 the fp64 softplus clears it by more than its bound
  logit          err_q + u (|q| + 1); the clamp at -50 held exactly likewise
  softmax weight relative: err_l[j] + max err_l + u (|l_j - m| + max |l - m|) + (128 + 8) u, + 2 tiny absolute
  lobe mean      m / |m|: (2 |err_m|_1) / |m| + 4 u with err_m = scale err_q + 4 u (|q scale| + |noise scale / 2| + |p|);
                 the cases hold |m| >= 0.1
  composite_all  (S + 2) u sum |w mat|
  integrate      per-sample term clip(L f, 0, rgb_max) w / max(pdf, 1e-5): the lobe f is a product of a fixed number of
                 factors -- GGX: D (3 u + 2 err_t / t, t = n_h^2 (a^2 - 1) + 1, err_t = 13 u n_h^2 |a^2 - 1| + u), Fresnel
                 (err_F / F from the 8 u of 1 - l.h through the fifth power), G 10 u, the quotient and L f 5 u; Lambert 6 u;
                 irradiance 4 u; the EnvMap's (1 - acc) 2 u -- the clip is 1-Lipschitz (and exact where L f clears
                 rgb_max), w / pdf 2 u.  A wave sum of K terms: (K + 2) u sum |terms| + sum err_term, / K; the sums of
                 passes 3 u; the output w (...) + bgw: 2 u + bg tol_acc; acc is an S-term sum: (S + 2) u sum |w|
  sampler        sampled local and global directions, pdf (scale 1 + |pdf|), MIS weight, and through them the mixture pdf
                 of 2 x 64 lobes: sin / cos / exp / sinh / log chains, 1 / (wo.h) and the vMF inverse CDF -- the floor is
                 MEASURED on the CPU, max |float32 restatement - fp64| over a family, and the device gets 4 x that
                 (MatCases.floors(); tests/test_matstage_ref.py holds 4 x floor <= 1e-4).  Measured: regular family
                 directions 9.2e-6 local, 9.1e-6 global, pdf 4.3e-6, weight 2.1e-5 (the worst lanes are vMF samples of a lobe
                 with kappa near 1e-2: w = 1 + log(arg) / kappa carries the ulp of arg a hundredfold); edge family 1.5e-6,
                 1.9e-6, 3.5e-6, 7.3e-6.  pdf and weight are exactly 0 where the contract says 0 (wn <= 0, z <= 0);
                 sec_origins, sec_near / far / lights and local_view equal the float32 restatement (IEEE operations only)
  kappa <= eps on a vMF-sampling lane (family "illcond"): w = 1 + log(arg) / max(kappa, eps) loses everything in float32
                 (arg = tmp + (1 - tmp) exp(-2 kappa) is 1 +- an ulp, times 2^23), so fp64 is not the contract there: the
                 reference runs in float32.  The device is held to the float32 restatement's own value within the regular
                 family's tolerance.  The cases take kappa = 0, eps / 2 and eps: exp(-2 kappa) = 1 - 2 kappa + 2 kappa^2 has
                 the float32 1 - 2 kappa as its nearest, arg is rounded to a multiple of 2^-24 and w comes out as a multiple
                 of 1 / 2, up to 0.5 away from fp64.  w hangs on the last bit of that exp, so the restatement's
                 transcendental functions are correctly rounded (_rounded): with numpy's own float32 exp, a neighbour of the
                 nearest float at both arguments, the restatement was 0.5 away from the device on 4 of 8 such lanes.
  the means, normals w p: one product, 2 u
No case and no element is excused."""
import sys

import numpy as np

import sample_ref as R
from sample_ref import CANARY, CSRC, EPS, FMAX, GUARD, ROOT, TINY, U, bf16, canary, is_canary  # noqa: F401

MAGIC_CASES, MAGIC_RESULTS = 0x4D41545343415345, 0x4D41545352534C54
N_INT, N_FLT, N_BUF = R.N_INT, R.N_FLT, R.N_BUF
RAYS = (1, 3, 4, 5, 9)
SPLITS = ((1, 2, 1), (2, 3, 1), (2, 3, 2), (4, 4, 2), (5, 5, 2), (5, 5, 3), (16, 16, 8), (32, 32, 16), (1, 63, 32), (61, 3, 1),
          (31, 33, 1), (31, 33, 32))
S_INTEGRATE = (1, 31, 32, 33, 63, 64)
S_COMPOSITE = S_INTEGRATE + (65,)
N_COMPOSITE = (1, 255, 256, 257)
MAT_CH = VMF_CH = SMP_CH = 5
MOUT = ("rgb", "acc", "direct_rgb", "indirect_rgb", "diffuse_rgb", "specular_rgb", "direct_diffuse_rgb", "direct_specular_rgb",
        "indirect_diffuse_rgb", "indirect_specular_rgb", "indirect_occ", "lighting_irradiance", "material_albedo",
        "material_roughness", "material_metalness", "material_F_0", "means", "normals_to_use", "ray_dists", "light_dists")
MOUT_SCALAR = ("acc", "indirect_occ", "material_roughness", "material_metalness", "material_F_0", "ray_dists", "light_dists")
MOUT_INTEGRATE = tuple(k for k in MOUT if not k.startswith("material_"))     # k_material_integrate writes these
KERNELS = ("mhead", "lhead", "heads", "sample", "composite", "integrate")
_MH = ("feat", "w0", "b0", "w1", "b1", "mat")
_LH = ("feat", "w0", "b0", "w1", "b1", "w2", "b2", "pts", "noise", "vmf", "vmf_logit")
_SEC = ("sec_origins", "sec_dirs", "sec_near", "sec_far", "sec_lights", "samples", "local_view")
SLOTS = {
    "mhead": (("n",), ("min_roughness",), _MH, ("mat",)),
    "lhead": (("n",), ("vmf_scale",), _LH, ("vmf", "vmf_logit")),
    "heads": (("n", "ln"), ("min_roughness", "vmf_scale"), _MH + tuple("l_" + s if s in _MH else s for s in _LH),
              ("mat", "vmf", "vmf_logit")),
    "sample": (("n", "Ks", "Kd", "Kc"), ("normal_eps", "near", "far"),
               ("pts", "nrm", "viewdirs", "lights", "mat", "vmf", "spec_u1", "spec_u2", "cos_u1", "cos_u2", "vmf_lobe", "vmf_v",
                "vmf_tmp", "vmf_lobe_gumbel", "vmf_logit") + _SEC, _SEC),
    "composite": (("n", "S"), ("f0",), ("weights", "mat", "out_albedo", "out_rough", "out_metal", "out_f0"),
                  ("out_albedo", "out_rough", "out_metal", "out_f0")),
    "integrate": (("n", "Ks", "Kd", "S"), ("f0", "rgb_max", "bg"),
                  ("mat", "samples", "local_view", "sec_rgb", "sec_acc", "sec_env", "weights", "filt_weight", "pts", "nrm",
                   "origins", "lights") + tuple("out_" + k for k in MOUT), tuple("out_" + k for k in MOUT)),
}
INT_SLOTS = ()                                       # no integer OUTPUT (vmf_lobe is an input: it travels as its bits)
FAMILIES = ("regular", "edges")
QUANTITIES = ("local", "global", "pdf", "weight", "mix")
MUTATIONS = ("kc_off_by_one", "diffuse_offset_rKs", "mis_no_2", "mis_light_pdf_local", "weight_not_zeroed", "wn_not_zeroing",
             "tie_high", "argmax_log_softmax", "mixture_upper_half_dropped", "sinh_neighbour", "softmax_max_not_subtracted",
             "rough_metal_swapped", "min_roughness_not_squared", "mean_over_K", "lane63_dropped", "bg_filtered_acc",
             "occ_scale_missing", "tail_wave_store")


def out_shape(kernel, slot, i):
    n = i.get("n", 0)
    K = i.get("Ks", 0) + i.get("Kd", 0)
    if kernel in ("mhead", "lhead", "heads"):
        m = i["ln"] if kernel == "heads" and slot != "mat" else n
        return {"mat": (m, MAT_CH), "vmf": (m, 128, VMF_CH), "vmf_logit": (m, 128)}[slot]
    if kernel == "sample":
        return {"sec_near": (n * K,), "sec_far": (n * K,), "samples": (n, K, SMP_CH), "local_view": (n, 3)}.get(slot, (n * K, 3))
    if kernel == "composite":
        return (n, 3) if slot == "out_albedo" else (n,)
    return (n,) if slot[4:] in MOUT_SCALAR else (n, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic, in `ft`


def _rounded(fn):
    """A transcendental function as the restatement takes it: correctly rounded in x's type (float32: evaluated in double and
    rounded once).  numpy's own float32 exp is a neighbour of the nearest float on some arguments (exp(-2^-22), exp(-2^-23)),
    and the ill-conditioned lanes hang on that bit."""
    def f(x):
        x = np.asarray(x)
        return fn(x.astype(np.float64)).astype(np.float32) if x.dtype == np.float32 else fn(x)
    return f


exp_, log_, log1p_, sin_, cos_, sinh_ = (_rounded(fn) for fn in (np.exp, np.log, np.log1p, np.sin, np.cos, np.sinh))


def _seqsum(x):
    """Sum over the last axis, sequential in x's type."""
    return np.cumsum(x, axis=-1, dtype=x.dtype)[..., -1] if x.shape[-1] else np.zeros(x.shape[:-1], x.dtype)


def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def make_frame(ft, n):
    """render_utils.get_rotation_matrix (render_utils.py:145-168) as make_frame(): (new_x, new_y, normal).  The switch of
    `up` compares the input with the float32 constant 0.9f in both precisions (the reference runs in float32)."""
    up = np.where((np.abs(n[..., 2]) < ft(np.float32(0.9)))[..., None], np.array([0, 0, 1], ft), np.array([0, 1, 0], ft))
    nx = cross3(up, n)
    nx = nx / (np.sqrt(dot3(nx, nx)) + ft(1e-10))[..., None]
    ny = cross3(n, nx)
    ny = ny / (np.sqrt(dot3(ny, ny)) + ft(1e-10))[..., None]
    return nx, ny, n


def to_local(d, f):
    return np.stack([dot3(d, f[0]), dot3(d, f[1]), dot3(d, f[2])], axis=-1)


def to_global(d, f):
    return d[..., 0:1] * f[0] + d[..., 1:2] * f[1] + d[..., 2:3] * f[2]


def l2n(ft, v):
    """ref_utils.l2_normalize (forward value)."""
    dsq = _seqsum(v * v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((dsq < ft(TINY))[..., None], ft(0.0), v / np.sqrt(np.maximum(ft(TINY), dsq))[..., None])


def ir_norm(ft, v):
    return v / np.sqrt(ft(1e-10) + dot3(v, v))[..., None]


def ggx_d(ft, c, a):
    t = c * c * (a * a - ft(1.0)) + ft(1.0)
    return (a * a) / np.maximum(ft(EPS), ft(np.pi) * (t * t))


def sigmoid(ft, x):
    return ft(1.0) / (ft(1.0) + exp_(-x))


def softplus(ft, x):
    return np.maximum(x, ft(0.0)) + log1p_(exp_(-np.abs(x)))


def dense(ft, x, w, b, cut=False):
    """x @ w + b, each output's products added in index order.  `cut`: both operands rounded to bfloat16."""
    if cut:
        x, w = bf16(x.astype(np.float32)), bf16(w.astype(np.float32))
    x, w = x.astype(ft), w.astype(ft)
    acc = np.zeros((x.shape[0], w.shape[1]), ft)
    for i in range(w.shape[0]):
        acc = acc + x[:, i, None] * w[i][None]
    return acc + b.astype(ft)[None]


def dense_bound(x, w, b, err_x=None):
    """The gemm test's bound on a float32 x @ w + b in any order, + the inputs' error carried through."""
    x, w = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64))
    t = 2.0 * (w.shape[0] + 2) * U * (x @ w + np.abs(b.astype(np.float64))[None])
    return t if err_x is None else t + err_x @ w


def material_head(ft, feat, w0, b0, w1, b1, min_roughness, mut=None, cut=False):
    """MaterialMLP._predict_material_and_feature / _get_microfacet_material (material.py:2073-2123, 1290-1322) from the grid
    features on: Dense 128 (no activation), Dense 10, albedo = sigmoid(o[0:3] - 1), roughness = sigmoid(o[6] - 1) (1 - r0) +
    r0 with r0 = min_roughness^2, metalness = sigmoid(o[8])."""
    h = dense(ft, feat, w0, b0, cut)
    o = dense(ft, h, w1, b1, cut)
    r0 = ft(min_roughness) if mut == "min_roughness_not_squared" else ft(min_roughness) * ft(min_roughness)
    cr, cm = (8, 6) if mut == "rough_metal_swapped" else (6, 8)
    mat = np.stack([sigmoid(ft, o[:, 0] - ft(1.0)), sigmoid(ft, o[:, 1] - ft(1.0)), sigmoid(ft, o[:, 2] - ft(1.0)),
                    sigmoid(ft, o[:, cr] - ft(1.0)) * (ft(1.0) - r0) + r0, sigmoid(ft, o[:, cm] + ft(0.0))], axis=-1)
    out = {"mat": mat, "_o": o}
    if ft is np.float64 and not cut and mut is None:
        eh = dense_bound(feat, w0, b0)
        eo = dense_bound(h, w1, b1, eh)[:, [0, 1, 2, 6, 8]]
        x = np.abs(o[:, [0, 1, 2, 6, 8]] - np.array([1, 1, 1, 1, 0.0]))
        t = 0.25 * (eo + U * x) + 4 * U
        t[:, 3] = t[:, 3] * (1.0 - float(r0)) + 3 * U
        out["_tol"] = {"mat": t}
    return out


def light_head(ft, feat, w0, b0, w1, b1, w2, b2, pts, noise, vmf_scale, mut=None, cut=False):
    """LightMLP.predict_lighting / get_vmfs (light_sampler.py:135-214): 32 -> 64 -> 64 -> 640 = 128 x (mean, kappa, logit),
    then LightSampler's l2_normalize and softmax."""
    n = feat.shape[0]
    h0 = np.maximum(dense(ft, feat, w0, b0, cut), ft(0.0))
    h1 = np.maximum(dense(ft, h0, w1, b1, cut), ft(0.0))
    q = dense(ft, h1, w2, b2, cut).reshape(n, 128, 5)
    sc, p, nz = ft(vmf_scale), pts.astype(ft)[:, None, :], noise.astype(ft).reshape(n, 128, 3)
    m = (q[..., 0:3] * sc + ft(0.0)) + nz * sc / ft(2.0) - p
    mean = l2n(ft, m)
    sp = softplus(ft, q[..., 3] + ft(1.0))
    kappa = np.minimum(sp, ft(50.0))
    lraw = q[..., 4] + ft(1.0)
    logit = np.maximum(lraw, ft(-50.0))
    mx = ft(0.0) if mut == "softmax_max_not_subtracted" else logit.max(axis=-1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = exp_(logit - mx)
        wgt = e / _seqsum(e)[..., None]
    out = {"vmf": np.concatenate([mean, kappa[..., None], wgt[..., None]], axis=-1), "vmf_logit": logit, "_m": m}
    if ft is np.float64 and not cut and mut is None:
        e0 = dense_bound(feat, w0, b0)
        e1 = dense_bound(h0, w1, b1, e0)
        eq = dense_bound(h1, w2, b2, e1).reshape(n, 128, 5)
        s = abs(float(vmf_scale))
        em = s * eq[..., 0:3] + 4 * U * (np.abs(q[..., 0:3]) * s + np.abs(nz) * s / 2 + np.abs(p))
        mn = np.sqrt((m * m).sum(-1))
        t_mean = (2.0 * em.sum(-1) / mn + 4 * U)[..., None] * np.ones(3)
        t_k = eq[..., 3] + U * (np.abs(q[..., 3]) + 1) + 4 * U * (1 + sp)
        t_k = np.where(sp - 50.0 > t_k, 0.0, t_k)
        t_l = eq[..., 4] + U * (np.abs(q[..., 4]) + 1)
        t_l = np.where(-50.0 - lraw > t_l, 0.0, t_l)
        d = np.abs(logit - mx)
        rel = t_l + t_l.max(-1, keepdims=True) + U * (d + d.max(-1, keepdims=True)) + (128 + 8) * U
        out["_tol"] = {"vmf": np.concatenate([t_mean, t_k[..., None], (rel * wgt + 2 * TINY)[..., None]], axis=-1), "vmf_logit": t_l}
        out["_mnorm"] = mn
    return out


def mixture(ft, gd, vmf, mut=None):
    """LightSampler.pdf (render_utils.py:1465-1490) with eval_vmf (:1335-1347, safe_exp = exp(min(x, 80))): the weighted vMF
    mixture of the 128 lobes at the global directions gd [n, Q, 3]."""
    m, kap, wgt = vmf[..., 0:3], vmf[..., 3], vmf[..., 4]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        den = ft(4.0) * ft(np.pi) * sinh_(kap)
        if mut == "sinh_neighbour":
            den = np.roll(den, -1, axis=-1)
        d = (gd[:, :, None, 0] * m[:, None, :, 0] + gd[:, :, None, 1] * m[:, None, :, 1]) + gd[:, :, None, 2] * m[:, None, :, 2]
        e = kap[:, None] * exp_(np.minimum(kap[:, None] * d, ft(80.0))) / den[:, None]
        e = np.where((kap <= ft(EPS))[:, None], ft(1.0) / (ft(4.0) * ft(np.pi)), e)
        t = wgt[:, None] * e
    if mut == "mixture_upper_half_dropped":
        t = t[..., :64]
    return np.maximum(_seqsum(t), ft(0.0))


def draw_lobe(ft, logit, gumbel, mut=None):
    """sample_vmf_vars (render_utils.py:1357-1372): jax.random.categorical = argmax(logits + gumbel), the first maximum."""
    lg = logit.astype(ft)
    if mut == "argmax_log_softmax":
        e = exp_(lg - lg.max(axis=-1, keepdims=True))
        lg = log_(np.maximum(e / _seqsum(e)[..., None], ft(TINY)))
    key = lg + gumbel.astype(ft)
    if mut == "tie_high":
        return 127 - np.argmax(key[:, ::-1], axis=-1), key
    return np.argmax(key, axis=-1), key


def brdf_sample(ft, Ks, Kd, Kc, a, f, mut=None):
    """get_secondary_rays / importance_sample_rays (render_utils.py:417-546, 722-1056, 1335-1490) as k_brdf_sample: lanes
    [0, Ks) GGX, [Ks, Ks + Kc) cosine, [Ks + Kc, Ks + Kd) the one drawn vMF lobe, power-heuristic MIS over (cosine, light).
    `a`: the arrays as stored (float32, vmf_lobe int32; optional ones None), `f`: normal_eps, near, far."""
    K, Kl = Ks + Kd, Kd - Kc
    n = a["pts"].size // 3
    g_ = lambda k, shape: a[k].astype(ft).reshape(shape)
    pts, nrm, mat, vmf = g_("pts", (n, 3)), g_("nrm", (n, 3)), g_("mat", (n, MAT_CH)), g_("vmf", (n, 128, VMF_CH))
    gview = -g_("viewdirs", (n, 3))
    key = None
    if a.get("vmf_lobe") is not None:
        lobe = a["vmf_lobe"].astype(np.int64).reshape(n)
    else:
        lobe, key = draw_lobe(ft, a["vmf_logit"].reshape(n, 128), a["vmf_lobe_gumbel"].reshape(n, 128), mut)
    lobe = np.clip(lobe, 0, 127)
    fr = make_frame(ft, nrm)
    lv = to_local(gview, fr)
    frk = tuple(x[:, None, :] for x in fr)
    alpha = mat[:, 3:4]
    pi = ft(np.pi)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        # GGX lanes: MicrofacetSampler.sample_directions (render_utils.py:501-531); single sampler -> weight 1
        u1, u2 = g_("spec_u1", (n, Ks)), g_("spec_u2", (n, Ks))
        tan2 = alpha * alpha * u1 / np.maximum(ft(1.0) - u1, ft(EPS))
        cost = ft(1.0) / np.sqrt(np.maximum(ft(1.0) + tan2, ft(EPS)))
        sint = np.sqrt(np.maximum(ft(1e-5), ft(1.0) - cost * cost))
        phi = u2 * ft(2.0) * pi - pi
        h = np.stack([sint * cos_(phi), sint * sin_(phi), cost], axis=-1)
        npdf = np.maximum(ggx_d(ft, cost, alpha) * np.abs(cost), ft(0.0))
        wn = dot3(lv[:, None, :], h)
        d = ft(2.0) * wn[..., None] * h - lv[:, None, :]
        s_pdf = npdf * (ft(1.0) / np.maximum(ft(4.0) * wn, ft(EPS)))
        if mut != "wn_not_zeroing":
            s_pdf = np.where(wn <= 0, ft(0.0), s_pdf)
        s_pdf = np.maximum(s_pdf, ft(0.0))
        s_ld = ir_norm(ft, d)
        # cosine lanes: CosineSampler (render_utils.py:425-433)
        c1, c2 = g_("cos_u1", (n, Kc)).copy(), g_("cos_u2", (n, Kc)).copy()
        vv, tmp = g_("vmf_v", (n, Kl, 2)), g_("vmf_tmp", (n, Kl))
        if mut == "kc_off_by_one":                                       # the last cosine lane loads the vMF lane's inputs
            c1[:, -1], c2[:, -1] = vv[:, 0, 0], vv[:, 0, 1]
        rr, ph = np.sqrt(c1), c2 * ft(2.0) * pi - pi
        x, y = rr * cos_(ph), rr * sin_(ph)
        z = np.sqrt(np.maximum(ft(1e-5), ft(1.0) - x * x - y * y))
        c_ld = np.stack([x, y, z], axis=-1)
        c_own = np.maximum(z / pi, ft(0.0))
        # vMF lanes: LightSampler -> sample_vmf (render_utils.py:1390-1428), every direction from ONE lobe per point
        q = vmf[np.arange(n), lobe]
        mean, kappa = q[:, 0:3], q[:, 3:4]
        tv = l2n(ft, np.stack([-mean[:, 1], mean[:, 0], np.zeros(n, ft)], axis=-1))
        bv = l2n(ft, cross3(mean, tv))
        v = l2n(ft, vv)
        arg = tmp + (ft(1.0) - tmp) * exp_(ft(-2.0) * kappa)
        w = ft(1.0) + (ft(1.0) / np.maximum(kappa, ft(EPS))) * log_(np.clip(arg, ft(TINY), ft(FMAX)))
        s = np.sqrt(np.clip(ft(1.0) - w * w, ft(0.0), ft(FMAX)))
        loc = np.stack([s * v[..., 0], s * v[..., 1], w], axis=-1)
        v_g = (tv[:, None, :] * loc[..., 0:1] + bv[:, None, :] * loc[..., 1:2]) + mean[:, None, :] * loc[..., 2:3]
        v_ld = to_local(v_g, frk)
        # the mixture pdf: queries [0, Kd) at every diffuse sample's global direction, [Kd, Kd + Kl) at the vMF samples'
        d_ld = np.concatenate([c_ld, v_ld], axis=1)
        d_gl = to_global(d_ld, frk)
        qdir = np.concatenate([d_ld if mut == "mis_light_pdf_local" else d_gl, v_g], axis=1)
        qpdf = mixture(ft, qdir, vmf, mut)
        own = np.concatenate([c_own, qpdf[:, Kd:]], axis=1)
        pc = np.maximum(np.where(d_ld[..., 2] < 0, ft(0.0), d_ld[..., 2] / pi), ft(0.0))
        pl = qpdf[:, :Kd]
        mden = pc * pc + pl * pl
        d_pdf = np.maximum(own, ft(0.0))
        d_w = (d_pdf * d_pdf) / np.maximum(mden, ft(1e-5))
        if mut != "mis_no_2":
            d_w = d_w * ft(2.0)
    ld = np.concatenate([s_ld, d_ld], axis=1)
    pdf = np.concatenate([s_pdf, d_pdf], axis=1)
    weight = np.concatenate([np.ones((n, Ks), ft), d_w], axis=1)
    if mut != "weight_not_zeroed":
        weight = np.where(ld[..., 2] > 0, weight, ft(0.0))
    gl = to_global(ld, frk)
    org = pts + nrm * ft(f["normal_eps"])
    lights = a["lights"].astype(ft).reshape(n, 3) if a.get("lights") is not None else np.zeros((n, 3), ft)

    def blocks(v):                                                      # [n, K, c] -> [specular block n Ks | diffuse block n Kd]
        c = v.shape[-1]
        if mut == "diffuse_offset_rKs":
            out = np.full((n * K, c), np.nan, ft)
            r = np.arange(n)[:, None]
            out[(r * Ks + np.arange(Ks)[None]).ravel()] = v[:, :Ks].reshape(-1, c)
            out[(r * Ks + r * Kd + np.arange(Kd)[None]).ravel()] = v[:, Ks:].reshape(-1, c)
            return out
        return np.concatenate([v[:, :Ks].reshape(-1, c), v[:, Ks:].reshape(-1, c)], axis=0)

    per = lambda v: np.broadcast_to(v[:, None, :], (n, K, v.shape[-1]))
    out = {"sec_origins": blocks(per(org)), "sec_dirs": blocks(gl), "sec_lights": blocks(per(lights)),
           "sec_near": blocks(np.full((n, K, 1), ft(f["near"])))[:, 0], "sec_far": blocks(np.full((n, K, 1), ft(f["far"])))[:, 0],
           "samples": np.concatenate([ld, pdf[..., None], weight[..., None]], axis=-1), "local_view": lv,
           "_lobe": lobe, "_key": key, "_qpdf": qpdf, "_wn": wn, "_gl": gl}
    if ft is np.float64:
        top = np.sort(key, axis=-1) if key is not None else None
        out["_margins"] = {
            "wo.n": np.abs(lv[:, 2]).min(), "wo.h": np.abs(wn).min(),
            "wi+wo": np.sqrt(((ld + lv[:, None, :]) ** 2).sum(-1)).min(), "z": np.abs(ld[..., 2]).min(), "mis": mden.min(),
            "u1": max(a["spec_u1"].max(), a["cos_u1"].max()), "kappa_lo": vmf[..., 3].min(), "kappa_hi": vmf[..., 3].max(),
            "nz": np.abs(np.abs(nrm[:, 2]) - float(np.float32(0.9))).min(), "mean_z": np.hypot(vmf[..., 0], vmf[..., 1]).min(),
            "lead": np.inf if top is None else (top[:, -1] - top[:, -2]).min()}
    return out


def material_composite_all(ft, w, mat, f0):
    """The material-only pass composited over all samples (models.py:1845-1912): sum_s w_s mat_s, sum_s w_s F_0."""
    w, mat = w.astype(ft), mat.astype(ft)
    t = w[..., None] * mat                                              # [n, S, 5]
    acc = _seqsum(np.moveaxis(t, 1, -1))                                # [n, 5]
    tf = w * ft(f0)
    out = {"out_albedo": acc[:, 0:3], "out_rough": acc[:, 3], "out_metal": acc[:, 4], "out_f0": _seqsum(tf)}
    if ft is np.float64:
        S = w.shape[1]
        b = (S + 2) * U * np.abs(t).sum(1)
        out["_tol"] = {"out_albedo": b[:, 0:3], "out_rough": b[:, 3], "out_metal": b[:, 4],
                       "out_f0": (S + 3) * U * np.abs(tf).sum(-1)}
    return out


def material_integrate(ft, Ks, Kd, S, a, f, mut=None):
    """get_lobe (Disney GGX, render_utils.py:566-695), integrate_reflect_rays (:1102-1193), the integration strategy
    (material.py:2705-2808) and MaterialIntegrator's composite of the one filtered sample (models.py:1531-1694) as
    k_material_integrate.  `a`: the arrays as stored; `f`: f0, rgb_max, bg."""
    K = Ks + Kd
    n = a["mat"].size // MAT_CH
    g_ = lambda k, shape: a[k].astype(ft).reshape(shape)
    mat, smp, wo = g_("mat", (n, MAT_CH)), g_("samples", (n, K, SMP_CH)), g_("local_view", (n, 3))[:, None, :]
    albedo, rough, metal = mat[:, None, 0:3], mat[:, None, 3:4], mat[:, None, 4:5]
    pi, f0, rgb_max = ft(np.pi), ft(f["f0"]), ft(f["rgb_max"])

    def lanes(k, c):                                                    # [n K, c] in blocks -> [n, K, c]
        v = g_(k, (n * K, c))
        if mut == "diffuse_offset_rKs":
            r = np.arange(n)[:, None]
            return np.concatenate([v[r * Ks + np.arange(Ks)[None]], v[(r * Ks + r * Kd + np.arange(Kd)[None]) % (n * K)]], axis=1)
        return np.concatenate([v[:n * Ks].reshape(n, Ks, c), v[n * Ks:].reshape(n, Kd, c)], axis=1)

    rgb_in, acc_in, env_in = lanes("sec_rgb", 3), lanes("sec_acc", 1), lanes("sec_env", 3)
    spec = (np.arange(K) < Ks)[None, :, None]
    wi, pdf = smp[..., 0:3], smp[..., 3:4]
    weight = np.where(wi[..., 2:3] > 0, np.maximum(smp[..., 4:5], ft(0.0)), ft(0.0))
    denom = np.maximum(pdf, ft(1e-5))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        h = ir_norm(ft, wi + wo)
        n_v, n_l, n_h = np.maximum(ft(0.0), wo[..., 2:3]), np.maximum(ft(0.0), wi[..., 2:3]), np.maximum(ft(0.0), h[..., 2:3])
        l_h = np.maximum(ft(0.0), dot3(wi, h))[..., None]
        D = ggx_d(ft, n_h, rough)
        k = rough / ft(2.0)
        G = (n_v / np.maximum(ft(EPS), n_v * (ft(1.0) - k) + k)) * (n_l / np.maximum(ft(EPS), n_l * (ft(1.0) - k) + k))
        c1 = np.clip(ft(1.0) - l_h, ft(0.0), ft(1.0))
        c2 = c1 * c1
        c5 = c1 * (c2 * c2)
        dl = np.maximum(ft(0.0), wi[..., 2:3]) / pi
        F0 = albedo * metal + f0 * (ft(1.0) - metal)
        Fr = F0 + (ft(1.0) - F0) * c5
        ggx = D * Fr * G / np.maximum(ft(EPS), ft(4.0) * n_v)
        lambert = n_l * albedo / pi
        lobe = np.where(spec, ggx * ft(1.0) * ft(1.0), lambert * ft(1.0) * (ft(1.0) - metal))
        rin = np.where(np.isnan(rgb_in), ft(0.0), rgb_in)
        rin = np.maximum(np.clip(rin, ft(-FMAX), ft(FMAX)), ft(0.0))
        ein = np.maximum(env_in, ft(0.0)) * (ft(1.0) - acc_in)
        ein = np.clip(np.where(np.isnan(ein), ft(0.0), ein), ft(-FMAX), ft(FMAX))
        est = lambda x: np.clip(x, ft(0.0), rgb_max) * weight / denom
        x_all = {"ind": rin * lobe, "dir": ein * lobe, "irr_i": rin * dl, "irr_d": ein * dl}
        terms = {k_: est(v) for k_, v in x_all.items()}
    kdiv = (ft(K), ft(K)) if mut == "mean_over_K" else (ft(Ks), ft(Kd))
    mean_s = lambda t: _seqsum(np.moveaxis(t[:, :Ks], 1, -1)) / kdiv[0]
    mean_d = lambda t: _seqsum(np.moveaxis(t[:, Ks:], 1, -1)) / kdiv[1]
    o_is, o_ds = mean_s(terms["ind"]), mean_s(terms["dir"])
    o_id, o_dd = mean_d(terms["ind"]), mean_d(terms["dir"])
    ii, id_ = mean_d(terms["irr_i"]), mean_d(terms["irr_d"])
    o_irr = (id_ + ii) * ft(0.5)
    occ_s = _seqsum(acc_in[:, :Ks, 0]) / kdiv[0]
    if mut != "occ_scale_missing":
        occ_s = occ_s * ft(0.5)
    wts = g_("weights", (n, S))
    acc_p = _seqsum(wts[:, :63] if (mut == "lane63_dropped" and S == 64) else wts)
    w1 = g_("filt_weight", (n,))
    w = w1[:, None]
    bgw = np.maximum(ft(0.0), ft(1.0) - (w1 if mut == "bg_filtered_acc" else acc_p)) * ft(f["bg"])
    rgb = ((o_dd + o_ds) + o_id) + o_is
    pts, nrm, org = g_("pts", (n, 3)), g_("nrm", (n, 3)), g_("origins", (n, 3))
    dist = lambda p: np.sqrt(((p[:, 0] - pts[:, 0]) * (p[:, 0] - pts[:, 0]) + (p[:, 1] - pts[:, 1]) * (p[:, 1] - pts[:, 1]))
                             + (p[:, 2] - pts[:, 2]) * (p[:, 2] - pts[:, 2]))
    out = {"rgb": w * rgb + bgw[:, None], "acc": acc_p, "direct_rgb": w * (o_dd + o_ds), "indirect_rgb": w * (o_id + o_is),
           "diffuse_rgb": w * (o_dd + o_id), "specular_rgb": w * (o_ds + o_is), "direct_diffuse_rgb": w * o_dd,
           "direct_specular_rgb": w * o_ds, "indirect_diffuse_rgb": w * o_id, "indirect_specular_rgb": w * o_is,
           "indirect_occ": w1 * occ_s, "lighting_irradiance": w * o_irr, "means": w * pts, "normals_to_use": w * nrm,
           "ray_dists": w1 * dist(org)}
    if a.get("lights") is not None:
        out["light_dists"] = w1 * dist(g_("lights", (n, 3)))
    out = {"out_" + k_: v for k_, v in out.items()}
    if ft is np.float64 and mut is None:
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            wh = np.abs(wi * h).sum(-1)[..., None]
            t = n_h * n_h * (rough * rough - 1.0) + 1.0
            et = 13 * U * n_h * n_h * np.abs(rough * rough - 1.0) + U
            rel_D = 4 * U + 2 * et / np.abs(t)
            ec1 = 8 * U * wh + U
            eF = 3 * U * (np.abs(albedo * metal) + np.abs(f0 * (1.0 - metal))) + (1.0 - F0) * (5 * c2 * c2 * ec1 + 3 * U * c5) + 3 * U * Fr
            rel_spec = rel_D + eF / np.maximum(Fr, TINY) + 15 * U
            rel_lobe = np.where(spec, rel_spec, 6 * U)
            rel = {"ind": rel_lobe, "dir": rel_lobe + 2 * U, "irr_i": 4 * U * np.ones_like(rel_lobe), "irr_d": 6 * U * np.ones_like(rel_lobe)}
            err = {}
            for k_, x in x_all.items():
                ax = np.abs(np.where(np.isnan(x), 0.0, x))
                r_ = np.broadcast_to(rel[k_], ax.shape)
                ex = np.where((x * (1.0 - r_) >= float(rgb_max)) | (x <= 0), 0.0, np.minimum(r_ * ax, float(rgb_max)))
                err[k_] = np.where(np.isfinite(ex), ex, 0.0) * weight / denom + 2 * U * np.abs(terms[k_])
        tm_s = lambda k_, o: (((Ks + 2) * U * np.abs(terms[k_][:, :Ks]).sum(1) + err[k_][:, :Ks].sum(1)) / Ks + U * np.abs(o))
        tm_d = lambda k_, o: (((Kd + 2) * U * np.abs(terms[k_][:, Ks:]).sum(1) + err[k_][:, Ks:].sum(1)) / Kd + U * np.abs(o))
        t_is, t_ds, t_id, t_dd = tm_s("ind", o_is), tm_s("dir", o_ds), tm_d("ind", o_id), tm_d("dir", o_dd)
        t_irr = 0.5 * (tm_d("irr_i", ii) + tm_d("irr_d", id_)) + 2 * U * np.abs(o_irr)
        t_acc = (S + 2) * U * np.abs(wts).sum(-1)
        aw = np.abs(w)
        fin = lambda name, t_x, val: aw * (t_x + 3 * U * np.abs(val)) + 2 * U * np.abs(out["out_" + name])
        tol = {"rgb": fin("rgb", t_dd + t_ds + t_id + t_is, rgb) + (abs(f["bg"]) * t_acc + 2 * U * np.abs(bgw))[:, None] + U * np.abs(out["out_rgb"]),
               "acc": t_acc, "direct_rgb": fin("direct_rgb", t_dd + t_ds, o_dd + o_ds),
               "indirect_rgb": fin("indirect_rgb", t_id + t_is, o_id + o_is), "diffuse_rgb": fin("diffuse_rgb", t_dd + t_id, o_dd + o_id),
               "specular_rgb": fin("specular_rgb", t_ds + t_is, o_ds + o_is), "direct_diffuse_rgb": fin("direct_diffuse_rgb", t_dd, o_dd),
               "direct_specular_rgb": fin("direct_specular_rgb", t_ds, o_ds), "indirect_diffuse_rgb": fin("indirect_diffuse_rgb", t_id, o_id),
               "indirect_specular_rgb": fin("indirect_specular_rgb", t_is, o_is), "lighting_irradiance": fin("lighting_irradiance", t_irr, o_irr),
               "indirect_occ": np.abs(w1) * ((Ks + 2) * U * np.abs(acc_in[:, :Ks, 0]).sum(-1) / Ks * 0.5 + 2 * U * np.abs(occ_s))
               + 2 * U * np.abs(out["out_indirect_occ"]),
               "means": 2 * U * np.abs(out["out_means"]), "normals_to_use": 2 * U * np.abs(out["out_normals_to_use"]),
               "ray_dists": 6 * U * np.abs(out["out_ray_dists"])}
        if "out_light_dists" in out:
            tol["light_dists"] = 6 * U * np.abs(out["out_light_dists"])
        out["_tol"] = {"out_" + k_: v for k_, v in tol.items()}
        out["_z"] = wi[..., 2]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# references per launch: {slot: values in ft, "_...": what the tolerances and the CPU test need}


def _arrays(cs, L, dev, names, ints=()):
    out = {}
    for s in names:
        idx = L["bufs"][s]
        out[s] = None if idx < 0 else (cs.value(idx, dev).view(np.int32) if s in ints else cs.value(idx, dev))
    return out


def ref_mhead(cs, L, ft, mut, dev, cut=False, prefix=""):
    a = _arrays(cs, L, dev, _MH[:5])
    n = L["ints"]["n"]
    return material_head(ft, a["feat"].reshape(n, 32), a["w0"].reshape(32, 128), a["b0"], a["w1"].reshape(128, 10), a["b1"],
                         L["flts"]["min_roughness"], mut, cut)


def ref_lhead(cs, L, ft, mut, dev, cut=False, prefix=""):
    a = _arrays(cs, L, dev, [prefix + s if s in _MH else s for s in _LH[:9]])
    a = {(k[len(prefix):] if prefix and k.startswith(prefix) else k): v for k, v in a.items()}
    n = L["ints"]["ln" if prefix else "n"]
    return light_head(ft, a["feat"].reshape(n, 32), a["w0"].reshape(32, 64), a["b0"], a["w1"].reshape(64, 64), a["b1"],
                      a["w2"].reshape(64, 640), a["b2"], a["pts"].reshape(n, 3), a["noise"], L["flts"]["vmf_scale"], mut, cut)


def ref_heads(cs, L, ft, mut, dev, cut=False):
    out, tol = {}, {}
    if L["ints"]["n"] > 0:
        m = ref_mhead(cs, L, ft, mut, dev, cut)
        out.update(m)
        tol.update(m.get("_tol", {}))
    if L["ints"]["ln"] > 0:
        l_ = ref_lhead(cs, L, ft, mut, dev, cut, prefix="l_")
        out.update(l_)
        tol.update(l_.get("_tol", {}))
    out["_tol"] = tol
    return out


def ref_sample(cs, L, ft, mut, dev):
    i = L["ints"]
    a = _arrays(cs, L, dev, SLOTS["sample"][2][:15], ints=("vmf_lobe",))
    return brdf_sample(ft, i["Ks"], i["Kd"], i["Kc"], a, L["flts"], mut)


def ref_composite(cs, L, ft, mut, dev):
    i = L["ints"]
    a = _arrays(cs, L, dev, ("weights", "mat"))
    out = material_composite_all(ft, a["weights"].reshape(i["n"], i["S"]), a["mat"].reshape(i["n"], i["S"], MAT_CH), L["flts"]["f0"])
    return {k: v for k, v in out.items() if k.startswith("_") or L["bufs"][k] >= 0}


def ref_integrate(cs, L, ft, mut, dev):
    i = L["ints"]
    a = _arrays(cs, L, dev, SLOTS["integrate"][2][:12])
    out = material_integrate(ft, i["Ks"], i["Kd"], i["S"], a, L["flts"], mut)
    return {k: v for k, v in out.items() if k.startswith("_") or L["bufs"][k] >= 0}


REFS = {"mhead": ref_mhead, "lhead": ref_lhead, "heads": ref_heads, "sample": ref_sample, "composite": ref_composite,
        "integrate": ref_integrate}


def reference(cs, li, ft=np.float64, mut=None, dev=None, **kw):
    L = cs.launches[li]
    with np.errstate(under="ignore"):
        return REFS[L["kernel"]](cs, L, ft, mut, dev, **kw)


def sample_errors(r32, r64):
    """max |float32 restatement - fp64| of a sampler launch per measured quantity (pdfs on the scale 1 + |fp64 value|)."""
    s32, s64 = r32["samples"].astype(np.float64), r64["samples"]
    return {"local": np.abs(s32[..., :3] - s64[..., :3]).max(), "global": np.abs(r32["_gl"].astype(np.float64) - r64["_gl"]).max(),
            "pdf": (np.abs(s32[..., 3] - s64[..., 3]) / (1.0 + np.abs(s64[..., 3]))).max(),
            "weight": np.abs(s32[..., 4] - s64[..., 4]).max(),
            "mix": (np.abs(r32["_qpdf"].astype(np.float64) - r64["_qpdf"]) / (1.0 + np.abs(r64["_qpdf"]))).max()}


class MatCases(R.Cases):
    def __init__(self):
        super().__init__(sys.modules[__name__])

    def floors(self):
        """{(family, quantity)}: max |float32 restatement - fp64| over the sampler launches of a family, measured once per
        case table on the CPU.  The device is held to 4 x these."""
        if self._floors is None:
            fl = {(fam, q): 0.0 for fam in FAMILIES for q in QUANTITIES}
            for li, L in enumerate(self.launches):
                if L["kernel"] == "sample" and L["family"] in FAMILIES:
                    e = sample_errors(reference(self, li, np.float32), reference(self, li, np.float64))
                    for q, v in e.items():
                        fl[(L["family"], q)] = max(fl[(L["family"], q)], float(v))
            self._floors = fl
        return self._floors


def expected(cs, li, dev=None):
    """(reference, tolerances) a device run of launch `li` is held to: the fp64 reference and its bounds; for the values the
    contract makes IEEE-exact, and for the whole of an "illcond" sampler launch, the float32 restatement."""
    L = cs.launches[li]
    ref = reference(cs, li, np.float64, dev=dev)
    if L["kernel"] != "sample":
        return ref, ref["_tol"]
    r32 = reference(cs, li, np.float32, dev=dev)
    fam = L["family"]
    fl = cs.floors()
    ffam = "regular" if fam == "illcond" else fam
    base = r32 if fam == "illcond" else ref
    smp = base["samples"].astype(np.float64)
    t = np.empty_like(smp)
    t[..., :3] = 4.0 * fl[(ffam, "local")]
    t[..., 3] = np.where(smp[..., 3] == 0, 0.0, 4.0 * fl[(ffam, "pdf")] * (1.0 + np.abs(smp[..., 3])))
    t[..., 4] = np.where(smp[..., 4] == 0, 0.0, 4.0 * fl[(ffam, "weight")])
    out = {k: r32[k] for k in ("sec_origins", "sec_near", "sec_far", "sec_lights", "local_view")}
    out.update(samples=smp, sec_dirs=base["sec_dirs"].astype(np.float64), _lobe=ref["_lobe"])
    tol = {k: 0.0 for k in ("sec_origins", "sec_near", "sec_far", "sec_lights", "local_view")}
    tol.update(samples=t, sec_dirs=4.0 * fl[(ffam, "global")])
    return out, tol


def render(cs, li, ref, mut=None):
    """The output buffers a device that computed `ref` in float32 would leave (sample_ref.render), and with "tail_wave_store"
    the rows the waves past n of the last block of four would store behind the last ray's."""
    out = R.render(cs, li, ref)
    L = cs.launches[li]
    n = L["ints"].get("n", 0)
    if mut == "tail_wave_store" and L["kernel"] in ("sample", "integrate") and n % 4:
        for slot in SLOTS[L["kernel"]][3]:
            idx = L["bufs"][slot]
            shape = out_shape(L["kernel"], slot, L["ints"])
            if idx < 0 or slot not in ref or shape[0] != n:
                continue
            row = np.asarray(ref[slot]).astype(np.float32).reshape(n, -1)[-1]
            at = GUARD + int(np.prod(shape))
            for extra in range(4 - n % 4):
                m = min(row.size, out[idx].size - at)
                out[idx][at:at + m] = row[:m]
                at += m
    return out


check = R.check
write_case_file = R.write_case_file
read_results = R.read_results


# ---------------------------------------------------------------------------------------------------------------------------
# cases


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _weights(rng):
    """One set of head weights (Flax kernels [in, out]) shared by every head launch.  The light head's last bias puts kappa
    = softplus(q3 + 1) in [0.05, 40] and leaves the means' |m| >= 0.1 (the cases assert it)."""
    u = lambda *s: rng.uniform(-1, 1, size=s).astype(np.float32)
    w = {"w0": u(32, 128) * 0.3, "b0": u(128) * 0.2, "w1": u(128, 10) * 0.15, "b1": u(10) * 0.5,
         "l_w0": u(32, 64) * 0.3, "l_b0": u(64) * 0.2, "l_w1": u(64, 64) * 0.2, "l_b1": u(64) * 0.2, "l_w2": u(64, 640) * 0.1,
         "l_b2": (u(640).reshape(128, 5) * np.array([1.5, 1.5, 1.5, 2.0, 2.0], np.float32)).reshape(-1)}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in w.items()}


def _lhead_inputs(rng, n, W):
    """Features, points and noise of n light-head points whose 128 unnormalised means all hold |m| >= 0.15 (a short mean's
    noise is pushed out along x until they do)."""
    ft_, pts, nz = (rng.uniform(-1, 1, size=(n, 32)).astype(np.float32), rng.uniform(-1, 1, size=(n, 3)).astype(np.float32),
                    rng.normal(size=(n, 128, 3)).astype(np.float32))
    for _ in range(8):
        m = light_head(np.float64, ft_, W["l_w0"], W["l_b0"], W["l_w1"], W["l_b1"], W["l_w2"], W["l_b2"], pts, nz, 2.0)["_m"]
        short = np.sqrt((m * m).sum(-1)) < 0.15
        if not short.any():
            return ft_, pts, nz
        nz[short, 0] += np.float32(1.0)
    raise AssertionError("short lobe means")


def _vmf_table(rng, n, kappa=None):
    """A stored lobe table [n, 128, 5] and its logits: unit means at least 1e-2 away from +-z, kappa log-uniform in
    [1e-2, 50), weights the float32 softmax of the logits."""
    m = _unit(rng.normal(size=(n, 128, 3)))
    flat = np.hypot(m[..., 0], m[..., 1]) < 0.02
    m[flat] = _unit(m[flat] + np.array([0.3, 0.2, 0.0]))
    kap = exp_(rng.uniform(log_(1e-2), log_(49.0), size=(n, 128))) if kappa is None else np.broadcast_to(kappa, (n, 128))
    lg = rng.uniform(-3, 3, size=(n, 128)).astype(np.float32)
    e = exp_(lg - lg.max(-1, keepdims=True))
    w = (e / np.cumsum(e, -1, dtype=np.float32)[..., -1:]).astype(np.float32)
    return np.concatenate([m, kap[..., None], w[..., None]], axis=-1).astype(np.float32), lg


def _gumbel_for(rng, logit, win, lead=2.5e-3):
    """Noise that makes `win` the argmax of logit + noise with the runner-up `lead` behind (fp64 keys)."""
    n = logit.shape[0]
    lg = logit.astype(np.float64)
    gap = rng.uniform(0.01, 3.0, size=(n, 128))
    gap[np.arange(n), (win + 1 + rng.integers(0, 127, size=n)) % 128] = lead
    g = (lg[np.arange(n), win][:, None] + 1.0) - lg - gap
    g[np.arange(n), win] = 1.0
    return g.astype(np.float32)


def _ray(rng):
    """One shading point of the regular family: normal, view, material."""
    while True:
        nrm = _unit(rng.normal(size=3))
        if abs(abs(nrm[2]) - 0.9) >= 2e-3:
            break
    while True:
        view = _unit(rng.normal(size=3))                                 # the kernel takes -viewdirs as the direction to the eye
        if 0.3 <= abs(float(-view @ nrm)):
            break
    mat = np.concatenate([rng.uniform(0.05, 0.95, size=3), rng.uniform(0.2, 0.8, size=1), rng.uniform(0.05, 0.95, size=1)])
    return nrm.astype(np.float32), view.astype(np.float32), mat.astype(np.float32)


SAMPLE_F = {"normal_eps": 1e-3, "near": 0.05, "far": 2.5}
MARGINS = {"wo.n": 0.05, "wo.h": 0.02, "wi+wo": 0.1, "z": 1e-3, "mis": 1e-3, "kappa_lo": 1e-2, "nz": 1e-3, "mean_z": 1e-2, "lead": 2e-3}


def margins_hold(m):
    return (all(m[k] >= v for k, v in MARGINS.items()) and m["u1"] <= 1 - 1e-3 and m["kappa_hi"] < 50.0)


def _regular_rays(rng, n, Ks, Kd, Kc, table=None):
    """The stored inputs of a regular sampler launch: every ray is redrawn until its fp64 reference holds the margins."""
    Kl = Kd - Kc
    rows = []
    for r in range(n):
        for _ in range(400):
            nrm, view, mat = _ray(rng)
            vmf, lg = table(r) if table else _vmf_table(rng, 1)
            a = {"pts": rng.uniform(-1, 1, size=(1, 3)).astype(np.float32), "nrm": nrm[None], "viewdirs": view[None], "mat": mat[None],
                 "vmf": vmf, "vmf_logit": lg, "spec_u1": rng.uniform(0.0, 0.9, size=(1, Ks)).astype(np.float32),
                 "spec_u2": rng.uniform(0, 1, size=(1, Ks)).astype(np.float32),
                 "cos_u1": rng.uniform(0.0, 0.98, size=(1, Kc)).astype(np.float32), "cos_u2": rng.uniform(0, 1, size=(1, Kc)).astype(np.float32),
                 "vmf_v": rng.normal(size=(1, Kl, 2)).astype(np.float32), "vmf_tmp": rng.uniform(0.02, 0.98, size=(1, Kl)).astype(np.float32),
                 "lights": rng.uniform(-2, 2, size=(1, 3)).astype(np.float32)}
            win = rng.integers(0, 128, size=1)
            a["vmf_lobe_gumbel"] = _gumbel_for(rng, lg, win)
            ref = brdf_sample(np.float64, Ks, Kd, Kc, a, SAMPLE_F)
            if margins_hold(ref["_margins"]) and ref["_lobe"][0] == win[0]:
                a["vmf_lobe"] = win.astype(np.int32)
                rows.append(a)
                break
        else:
            raise AssertionError("no regular ray found")
    return {k: np.concatenate([x[k] for x in rows], axis=0) for k in rows[0]}


def _sec_inputs(rng, n, K, S):
    return {"sec_rgb": rng.uniform(0, 2, size=(n * K, 3)).astype(np.float32), "sec_acc": rng.uniform(0, 1, size=n * K).astype(np.float32),
            "sec_env": rng.uniform(0, 1.5, size=(n * K, 3)).astype(np.float32),
            "weights": (rng.uniform(0, 1, size=(n, S)) / S).astype(np.float32), "filt_weight": rng.uniform(0.2, 1.5, size=n).astype(np.float32),
            "pts": rng.uniform(-1, 1, size=(n, 3)).astype(np.float32), "nrm": _unit(rng.normal(size=(n, 3))).astype(np.float32),
            "origins": rng.uniform(-2, 2, size=(n, 3)).astype(np.float32), "lights": rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)}


INTEGRATE_F = {"f0": 0.04, "rgb_max": 4.0, "bg": 0.75}


def build_cases(seed=20240911):
    rng = np.random.default_rng(seed)
    cs = MatCases()
    W = _weights(rng)
    WB = {k: cs.inp(v) for k, v in W.items()}
    mh_w = {k: WB[k] for k in ("w0", "b0", "w1", "b1")}
    lh_w = {k[2:]: WB[k] for k in ("l_w0", "l_b0", "l_w1", "l_b1", "l_w2", "l_b2")}
    lh_w_heads = {("l_" + k if k in _MH else k): v for k, v in lh_w.items()}
    feat = lambda n: rng.uniform(-1, 1, size=(n, 32)).astype(np.float32)
    # --- the heads: n = 1, 3, 4, 5, 9 alone, and (m.n, l.n) of k_shading_heads against the two separate launches
    for j, n in enumerate(RAYS):
        mr = (0.0, 0.25)[j % 2]
        cs.launch("mhead", f"mhead/n{n}", "heads", {"n": n}, {"min_roughness": mr}, outs=("mat",), feat=cs.inp(feat(n)), **mh_w)
        lf, lp, lz = (cs.inp(v) for v in _lhead_inputs(rng, n, W))
        cs.launch("lhead", f"lhead/n{n}", "heads", {"n": n}, {"vmf_scale": 2.0}, outs=("vmf", "vmf_logit"), feat=lf, pts=lp, noise=lz, **lh_w)
    for mn in (1, 3, 4, 5):
        for ln in (1, 2):
            mf = cs.inp(feat(mn))
            lf, lp, lz = (cs.inp(v) for v in _lhead_inputs(rng, ln, W))
            a = cs.launch("mhead", f"heads/m{mn}l{ln}/mhead", "heads", {"n": mn}, {"min_roughness": 0.25}, outs=("mat",), feat=mf, **mh_w)
            b = cs.launch("lhead", f"heads/m{mn}l{ln}/lhead", "heads", {"n": ln}, {"vmf_scale": 2.0}, outs=("vmf", "vmf_logit"), feat=lf,
                          pts=lp, noise=lz, **lh_w)
            c = cs.launch("heads", f"heads/m{mn}l{ln}", "heads", {"n": mn, "ln": ln}, {"min_roughness": 0.25, "vmf_scale": 2.0},
                          outs=("mat", "vmf", "vmf_logit"), feat=mf, l_feat=lf, pts=lp, noise=lz, **mh_w, **lh_w_heads)
            cs.launches[c]["twins"] = {"mat": (a, "mat"), "vmf": (b, "vmf"), "vmf_logit": (b, "vmf_logit")}
    # the two fallbacks of rc_launch_shading_heads: one count 0 (that head's pointers are null)
    mf = cs.inp(feat(3))
    a = cs.launch("mhead", "heads/m3l0/mhead", "heads", {"n": 3}, {"min_roughness": 0.25}, outs=("mat",), feat=mf, **mh_w)
    c = cs.launch("heads", "heads/m3l0", "heads", {"n": 3, "ln": 0}, {"min_roughness": 0.25, "vmf_scale": 2.0}, outs=("mat",), feat=mf, **mh_w)
    cs.launches[c]["twins"] = {"mat": (a, "mat")}
    lf, lp, lz = (cs.inp(v) for v in _lhead_inputs(rng, 2, W))
    b = cs.launch("lhead", "heads/m0l2/lhead", "heads", {"n": 2}, {"vmf_scale": 2.0}, outs=("vmf", "vmf_logit"), feat=lf, pts=lp, noise=lz, **lh_w)
    c = cs.launch("heads", "heads/m0l2", "heads", {"n": 0, "ln": 2}, {"min_roughness": 0.25, "vmf_scale": 2.0}, outs=("vmf", "vmf_logit"),
                  l_feat=lf, pts=lp, noise=lz, **lh_w_heads)
    cs.launches[c]["twins"] = {"vmf": (b, "vmf"), "vmf_logit": (b, "vmf_logit")}
    # 8211 points: k_material_head<16>, whose last block holds 3 points, against the same points in launches of <= 8192
    big = feat(8211)
    c = cs.launch("mhead", "mhead/n8211", "heads", {"n": 8211}, {"min_roughness": 0.25}, outs=("mat",), feat=cs.inp(big), **mh_w)
    parts = [cs.launch("mhead", f"mhead/n8211/part{k}", "heads", {"n": hi - lo}, {"min_roughness": 0.25}, outs=("mat",),
                       feat=cs.inp(big[lo:hi]), **mh_w) for k, (lo, hi) in enumerate(((0, 8192), (8192, 8211)))]
    cs.launches[c]["parts"] = parts
    # the light head's edges: kappa at the 50 clamp, the logit at the -50 clamp, all logits equal, large logits
    for name, q3, q4 in (("clamps", 60.0, -70.0), ("equal_logits", 0.5, 0.25), ("large_logits", 0.5, 94.0)):
        b2 = W["l_b2"].reshape(128, 5).copy()
        w2 = W["l_w2"].reshape(64, 128, 5).copy()
        if name == "clamps":                                             # half of the lobes clamp, the others stay free
            b2[::2, 3], b2[::2, 4] = q3, q4
        else:
            w2[..., 4], b2[:, 4] = 0.0, q4
            if name == "large_logits":
                b2[:, 4] += np.linspace(-1, 1, 128).astype(np.float32)
        lf, lp, lz = (cs.inp(v) for v in _lhead_inputs(rng, 3, W))
        li = cs.launch("lhead", f"lhead/{name}", "heads", {"n": 3}, {"vmf_scale": 2.0}, outs=("vmf", "vmf_logit"), feat=lf, pts=lp, noise=lz,
                       **dict(lh_w, w2=cs.inp(w2.reshape(64, 640)), b2=cs.inp(b2.reshape(-1))))
        cs.launches[li]["edge"] = name
    # --- the sampler and the integrator, regular family: every split, rays cycling through 1, 3, 4, 5, 9, S through its list
    for j, (Ks, Kd, Kc) in enumerate(SPLITS):
        n, S, K = RAYS[j % 5], S_INTEGRATE[j % 6], Ks + Kd
        tag = f"Ks{Ks}Kd{Kd}Kc{Kc}n{n}"
        a = _regular_rays(rng, n, Ks, Kd, Kc)
        B = {k: cs.inp(v) for k, v in a.items()}
        ints = {"n": n, "Ks": Ks, "Kd": Kd, "Kc": Kc}
        common = {k: B[k] for k in ("pts", "nrm", "viewdirs", "mat", "vmf", "spec_u1", "spec_u2", "cos_u1", "cos_u2", "vmf_v", "vmf_tmp")}
        if j % 2 == 0:
            common["lights"] = B["lights"]
        drawn = cs.launch("sample", f"sample/drawn/{tag}", "regular", ints, SAMPLE_F, outs=_SEC, vmf_lobe_gumbel=B["vmf_lobe_gumbel"],
                          vmf_logit=B["vmf_logit"], **common)
        given = cs.launch("sample", f"sample/given/{tag}", "regular", ints, SAMPLE_F, outs=_SEC, vmf_lobe=B["vmf_lobe"], **common)
        cs.launches[drawn]["winner"] = a["vmf_lobe"].astype(np.int64)
        cs.launches[drawn]["twin"] = given
        so = cs.launches[given]["bufs"]
        x = _sec_inputs(rng, n, K, S)
        X = {k: cs.inp(v) for k, v in x.items()}
        ins = dict(mat=B["mat"], samples=so["samples"], local_view=so["local_view"], **{k: X[k] for k in x if k != "lights"})
        iints = {"n": n, "Ks": Ks, "Kd": Kd, "S": S}
        full = cs.launch("integrate", f"integrate/all/{tag}S{S}", "regular", iints, INTEGRATE_F, outs=["out_" + k for k in MOUT],
                         lights=X["lights"], **ins)
        # every pointer allocated but no lights: light_dists keeps its canaries
        nl = cs.launch("integrate", f"integrate/nolights/{tag}S{S}", "regular", iints, INTEGRATE_F, outs=["out_" + k for k in MOUT], **ins)
        few = cs.launch("integrate", f"integrate/few/{tag}S{S}", "regular", iints, INTEGRATE_F,
                        outs=("out_rgb", "out_" + MOUT_INTEGRATE[1 + j % (len(MOUT_INTEGRATE) - 1)]), lights=X["lights"], **ins)
        for li in (nl, few):
            cs.launches[li]["twin"] = full
    # every S of the integrator at one split, and each output pointer alone once (the others null)
    a = _regular_rays(rng, 5, 4, 4, 2)
    B = {k: cs.inp(v) for k, v in a.items()}
    src = cs.launch("sample", "sample/given/forS", "regular", {"n": 5, "Ks": 4, "Kd": 4, "Kc": 2}, SAMPLE_F, outs=_SEC,
                    **{k: B[k] for k in a if k not in ("vmf_lobe_gumbel", "vmf_logit")})
    so = cs.launches[src]["bufs"]
    for j, S in enumerate(S_INTEGRATE):
        x = _sec_inputs(rng, 5, 8, S)
        X = {k: cs.inp(v) for k, v in x.items()}
        ins = dict(mat=B["mat"], samples=so["samples"], local_view=so["local_view"], **X)
        iints = {"n": 5, "Ks": 4, "Kd": 4, "S": S}
        full = cs.launch("integrate", f"integrate/S{S}", "regular", iints, INTEGRATE_F, outs=["out_" + k for k in MOUT_INTEGRATE], **ins)
        for k in MOUT_INTEGRATE[j::len(S_INTEGRATE)]:
            li = cs.launch("integrate", f"integrate/S{S}/only_{k}", "regular", iints, INTEGRATE_F, outs=("out_" + k,), **ins)
            cs.launches[li]["twin"] = full
    # --- the same point as the last ray of n = 1, 5 and 9 (the tail waves of a partial block, the per-wave LDS slices)
    Ks, Kd, Kc = 5, 5, 2
    a9 = _regular_rays(rng, 9, Ks, Kd, Kc)
    x9 = _sec_inputs(rng, 9, Ks + Kd, 33)
    group = []
    for n in (1, 5, 9):
        rows = np.r_[np.arange(n - 1), 8]
        a = {k: np.ascontiguousarray(v[rows]) for k, v in a9.items()}
        B = {k: cs.inp(v) for k, v in a.items()}
        li = cs.launch("sample", f"sample/lastray/n{n}", "regular", {"n": n, "Ks": Ks, "Kd": Kd, "Kc": Kc}, SAMPLE_F, outs=_SEC,
                       **{k: B[k] for k in a if k != "vmf_lobe"})
        cs.launches[li]["winner"] = a["vmf_lobe"].astype(np.int64)
        so = cs.launches[li]["bufs"]
        lanes = np.concatenate([(rows[:, None] * Ks + np.arange(Ks)).ravel(), (9 * Ks + rows[:, None] * Kd + np.arange(Kd)).ravel()])
        x = {k: np.ascontiguousarray(v[lanes] if k.startswith("sec_") else v[rows]) for k, v in x9.items()}
        ii = cs.launch("integrate", f"integrate/lastray/n{n}", "regular", {"n": n, "Ks": Ks, "Kd": Kd, "S": 33}, INTEGRATE_F,
                       outs=["out_" + k for k in MOUT_INTEGRATE], mat=B["mat"], samples=so["samples"], local_view=so["local_view"],
                       **{k: cs.inp(v) for k, v in x.items()})
        group.append((li, ii))
    cs.lastray = group
    # --- the chain heads -> sampler -> integrate: the sampler reads the device's own mat / vmf / vmf_logit
    for n, (Ks, Kd, Kc) in ((5, (4, 4, 2)), (9, (16, 16, 8))):
        fm = feat(4 * n)
        fl_, pp, nz = _lhead_inputs(rng, 4 * n, W)
        m32 = material_head(np.float32, fm, W["w0"], W["b0"], W["w1"], W["b1"], 0.25)["mat"]
        l32 = light_head(np.float32, fl_, W["l_w0"], W["l_b0"], W["l_w1"], W["l_b1"], W["l_w2"], W["l_b2"], pp, nz, 2.0)
        # candidate points: the first n whose ray holds the margins on the heads' float32 restatement
        keep, rows = [], []
        for c_ in range(4 * n):
            if len(keep) == n:
                break
            try:
                a = _regular_rays(rng, 1, Ks, Kd, Kc, table=lambda r: (l32["vmf"][c_:c_ + 1], l32["vmf_logit"][c_:c_ + 1]))
            except AssertionError:
                continue
            a["mat"], a["pts"] = m32[c_:c_ + 1], pp[c_:c_ + 1]
            if margins_hold(brdf_sample(np.float64, Ks, Kd, Kc, a, SAMPLE_F)["_margins"]):
                keep.append(c_)
                rows.append(a)
        assert len(keep) == n, (n, len(keep))
        a = {k: np.concatenate([x[k] for x in rows], axis=0) for k in rows[0]}
        B = {k: cs.inp(v) for k, v in a.items() if k not in ("mat", "vmf", "vmf_logit", "pts")}
        P = cs.inp(pp[keep])
        hd = cs.launch("heads", f"chain/heads/n{n}", "heads", {"n": n, "ln": n}, {"min_roughness": 0.25, "vmf_scale": 2.0},
                       outs=("mat", "vmf", "vmf_logit"), feat=cs.inp(fm[keep]), l_feat=cs.inp(fl_[keep]), pts=P, noise=cs.inp(nz[keep]),
                       **mh_w, **lh_w_heads)
        ho = cs.launches[hd]["bufs"]
        sm = cs.launch("sample", f"chain/sample/n{n}", "regular", {"n": n, "Ks": Ks, "Kd": Kd, "Kc": Kc}, SAMPLE_F, outs=_SEC, pts=P,
                       mat=ho["mat"], vmf=ho["vmf"], vmf_logit=ho["vmf_logit"], **{k: v for k, v in B.items() if k != "vmf_lobe"})
        cs.launches[sm]["winner"] = a["vmf_lobe"].astype(np.int64)
        so = cs.launches[sm]["bufs"]
        x = _sec_inputs(rng, n, Ks + Kd, 32)
        x["pts"], x["nrm"] = pp[keep], a["nrm"]
        cs.launch("integrate", f"chain/integrate/n{n}", "regular", {"n": n, "Ks": Ks, "Kd": Kd, "S": 32}, INTEGRATE_F,
                  outs=["out_" + k for k in MOUT_INTEGRATE], mat=ho["mat"], samples=so["samples"], local_view=so["local_view"],
                  **{k: cs.inp(v) for k, v in x.items()})
    _edge_cases(cs, rng)
    # --- k_material_composite_all
    for j, S in enumerate(S_COMPOSITE):
        for n in (N_COMPOSITE if S in (1, 65) else (N_COMPOSITE[j % 4],)):
            w = (rng.uniform(0, 1, size=(n, S)) * (rng.uniform(size=(n, S)) > 0.3) / S).astype(np.float32)
            mat = rng.uniform(0, 1, size=(n, S, MAT_CH)).astype(np.float32)
            Wb, Mb = cs.inp(w), cs.inp(mat)
            full = cs.launch("composite", f"composite/all/S{S}n{n}", "composite", {"n": n, "S": S}, {"f0": 0.04},
                             outs=SLOTS["composite"][3], weights=Wb, mat=Mb)
            one = cs.launch("composite", f"composite/one/S{S}n{n}", "composite", {"n": n, "S": S}, {"f0": 0.04},
                            outs=(SLOTS["composite"][3][j % 4],), weights=Wb, mat=Mb)
            cs.launches[one]["twin"] = full
    return cs


def _edge_cases(cs, rng):
    """The edge family: exactly representable inputs on the clamps and branches, so both precisions take the same side."""
    Ks, Kd, Kc = 4, 4, 2
    n = 9
    K = Ks + Kd
    a = _regular_rays(rng, n, Ks, Kd, Kc)
    # u1 = 0 and 1, u2 = 0 and 1 on the GGX and the cosine lanes of every ray
    a["spec_u1"][:, :4] = np.array([0.0, 1.0, 0.5, 0.25], np.float32)
    a["spec_u2"][:, :4] = np.array([0.0, 1.0, 0.5, 0.125], np.float32)
    a["cos_u1"][:, :2] = np.array([1.0, 0.0], np.float32)
    a["cos_u2"][:, :2] = np.array([0.25, 1.0], np.float32)
    z = np.array([0.0, 0.0, 1.0], np.float32)
    f9 = np.float32(0.9)
    side = np.sqrt(np.float32(1.0) - f9 * f9)
    # ray 0: view exactly along -n (viewdirs = n); ray 1: view in the tangent plane of n = +z; rays 2-4: n.z = 0.9f and its
    # float neighbours; ray 5: n = -z; ray 6: n = +z with every lobe pointing into the surface (z <= 0 on the vMF lanes);
    # ray 7: the drawn lobe's mean exactly (0, 0, 1); ray 8: (0, 0, -1)
    a["nrm"][0], a["viewdirs"][0] = z, z
    a["nrm"][1], a["viewdirs"][1] = z, np.array([-1.0, 0.0, 0.0], np.float32)
    for r, nz in zip((2, 3, 4), (f9, np.nextafter(f9, np.float32(0)), np.nextafter(f9, np.float32(1)))):
        a["nrm"][r] = np.array([side, 0.0, nz], np.float32)
        a["viewdirs"][r] = -_unit(np.array([0.3, 0.2, 0.9])).astype(np.float32)
    a["nrm"][5], a["viewdirs"][5] = -z, np.array([0.0, 0.6, 0.8], np.float32)
    a["nrm"][6], a["viewdirs"][6] = z, np.array([0.0, -0.6, -0.8], np.float32)
    a["vmf"][6, :, 0:3] = _unit(a["vmf"][6, :, 0:3] * np.array([1, 1, 0]) + np.array([0, 0, -3.0])).astype(np.float32)
    a["vmf"][6, :, 3] = 40.0
    for r in range(n):
        if a["vmf_lobe"][r] in (5, 70):
            a["vmf_lobe"][r] = 6
    for r, s in ((7, 1.0), (8, -1.0)):
        a["nrm"][r], a["viewdirs"][r] = z, np.array([0.0, -0.6, -0.8], np.float32)
        a["vmf"][r, a["vmf_lobe"][r], 0:3] = np.array([0.0, 0.0, s], np.float32)
    # kappa <= eps on lobes that are NOT sampled (the uniform branch of the mixture), kappa at the 50 clamp
    a["vmf"][:, 5, 3], a["vmf"][:, 70, 3], a["vmf"][:, 9, 3], a["vmf"][:, 100, 3] = 0.0, EPS, 50.0, 50.0
    B = {k: cs.inp(v) for k, v in a.items()}
    li = cs.launch("sample", "edges/sample", "edges", {"n": n, "Ks": Ks, "Kd": Kd, "Kc": Kc}, SAMPLE_F, outs=_SEC,
                   **{k: B[k] for k in a if k not in ("vmf_lobe_gumbel", "vmf_logit", "lights")})
    cs.launches[li]["edge"] = "sample"
    # the lobe draw: equal keys at (17, 81) -> 17, at (3, 40) -> 3, all keys equal -> 0, a winner in the upper 64, the clamp
    # of log(softmax) (logit 60 against -50 with noise 105: the raw keys say lobe 20, 60 > 55); vmf_lobe out of range
    lg = np.zeros((n, 128), np.float32)
    g = np.zeros((n, 128), np.float32)
    lg[0] = np.linspace(-2, -1, 128).astype(np.float32)
    lg[0, 17], g[0, 17], lg[0, 81], g[0, 81] = 0.5, 1.0, 1.0, 0.5
    lg[1] = np.linspace(-2, -1, 128).astype(np.float32)
    lg[1, 3], g[1, 3], lg[1, 40], g[1, 40] = 0.25, 2.0, 1.25, 1.0
    lg[2], g[2] = 0.75, 0.5
    lg[3] = np.linspace(-2, -1, 128).astype(np.float32)
    g[3, 101] = 4.0
    lg[4], lg[4, 20], g[4, 90] = -50.0, 60.0, 105.0
    lg[5:], g[5:] = lg[3], g[3]
    win = np.array([17, 3, 0, 101, 20, 101, 101, 101, 101])
    a2 = dict(a, vmf_logit=lg, vmf_lobe_gumbel=g)
    a2["vmf"] = a["vmf"].copy()
    for r, s in ((7, 1.0), (8, -1.0)):
        a2["vmf"][r, 101, 0:3] = np.array([0.0, 0.0, s], np.float32)
    B2 = dict(B, vmf_logit=cs.inp(lg), vmf_lobe_gumbel=cs.inp(g), vmf=cs.inp(a2["vmf"]))
    rest = {k: B2[k] for k in a if k not in ("vmf_lobe_gumbel", "vmf_logit", "vmf_lobe")}
    ints = {"n": n, "Ks": Ks, "Kd": Kd, "Kc": Kc}
    drawn = cs.launch("sample", "edges/lobe/drawn", "edges", ints, SAMPLE_F, outs=_SEC, vmf_lobe_gumbel=B2["vmf_lobe_gumbel"],
                      vmf_logit=B2["vmf_logit"], **rest)
    given = cs.launch("sample", "edges/lobe/given", "edges", ints, SAMPLE_F, outs=_SEC, vmf_lobe=cs.inp(win.astype(np.int32)), **rest)
    cs.launches[drawn].update(winner=win, twin=given, edge="lobe")
    lo = np.array([-1, 128, 1000, 0, 127, -2 ** 31, 2 ** 31 - 1, 127, 0], np.int32)
    oob = cs.launch("sample", "edges/lobe/out_of_range", "edges", ints, SAMPLE_F, outs=_SEC, vmf_lobe=cs.inp(lo), **rest)
    inr = cs.launch("sample", "edges/lobe/in_range", "edges", ints, SAMPLE_F, outs=_SEC,
                    vmf_lobe=cs.inp(np.clip(lo, 0, 127).astype(np.int32)), **rest)
    cs.launches[oob]["twin"] = inr
    # kappa <= eps on the SAMPLED lobe: the float32 restatement is the contract (module docstring)
    a3 = {k: v.copy() for k, v in _regular_rays(rng, 5, Ks, Kd, Kc).items()}
    a3["vmf"][np.arange(5), a3["vmf_lobe"], 3] = np.array([0.0, EPS, EPS / 2, EPS, EPS / 2], np.float32)
    li = cs.launch("sample", "illcond/sample", "illcond", {"n": 5, "Ks": Ks, "Kd": Kd, "Kc": Kc}, SAMPLE_F, outs=_SEC,
                   **{k: cs.inp(v) for k, v in a3.items() if k not in ("vmf_lobe_gumbel", "vmf_logit")})
    cs.launches[li]["edge"] = "illcond"
    # the integrator's edges on stored samples: NaN / inf / negative radiance, a negative EnvMap, acc 0, 1 and 1.5, pdf below
    # 1e-5, a negative MIS weight, z <= 0, rgb_max small enough to clip, filt_weight 0; ray 3: every diffuse sample below
    n = 5
    smp = np.zeros((n, K, SMP_CH), np.float32)
    smp[..., 0:3] = _unit(rng.normal(size=(n, K, 3)) + np.array([0, 0, 1.5])).astype(np.float32)
    smp[..., 3] = rng.uniform(0.1, 2.0, size=(n, K))
    smp[..., 4] = rng.uniform(0.2, 2.0, size=(n, K))
    smp[0, 0, 3], smp[0, 5, 3], smp[1, 1, 4], smp[1, 6, 4] = 1e-7, 0.0, -0.5, -2.0
    smp[2, 2, 2], smp[2, 7, 2], smp[3, Ks:, 2] = 0.0, -0.25, -np.abs(smp[3, Ks:, 2])
    lv = _unit(rng.normal(size=(n, 3)) + np.array([0, 0, 2.0])).astype(np.float32)
    x = _sec_inputs(rng, n, K, 32)
    x["sec_rgb"][0:6, 0] = np.array([np.nan, np.inf, -np.inf, -1.0, 3e38, 50.0], np.float32)
    x["sec_rgb"][n * Ks:n * Ks + 4, 1] = np.array([np.nan, np.inf, -2.0, 100.0], np.float32)
    x["sec_env"][1:5, 2] = np.array([-1.0, np.inf, np.nan, 80.0], np.float32)
    x["sec_acc"][0:4] = np.array([0.0, 1.0, 1.5, 1.0], np.float32)
    x["sec_env"][3] = np.inf                                              # inf (1 - 1) = NaN -> 0
    x["filt_weight"][4] = 0.0
    mat = np.stack([_ray(rng)[2] for _ in range(n)])
    for name, fl in (("clip", dict(INTEGRATE_F, rgb_max=0.125)), ("noclip", INTEGRATE_F)):
        X = {k: cs.inp(v) for k, v in x.items()}
        li = cs.launch("integrate", f"edges/integrate/{name}", "edges", {"n": n, "Ks": Ks, "Kd": Kd, "S": 32}, fl,
                       outs=["out_" + k for k in MOUT_INTEGRATE], mat=cs.inp(mat), samples=cs.inp(smp), local_view=cs.inp(lv), **X)
        cs.launches[li]["edge"] = "integrate"
    # a launch whose diffuse samples ALL lie below the surface: exactly zero diffuse terms
    below = smp[:3].copy()
    below[:, Ks:, 2] = -np.abs(below[:, Ks:, 2])
    below[0, Ks, 2] = 0.0
    y = _sec_inputs(rng, 3, K, 31)
    li = cs.launch("integrate", "edges/integrate/below", "edges", {"n": 3, "Ks": Ks, "Kd": Kd, "S": 31}, INTEGRATE_F,
                   outs=["out_" + k for k in MOUT_INTEGRATE], mat=cs.inp(mat[:3]), samples=cs.inp(below), local_view=cs.inp(lv[:3]),
                   **{k: cs.inp(v) for k, v in y.items()})
    cs.launches[li]["edge"] = "integrate"
    for mr in (0.0, 0.25):
        cs.launch("mhead", f"edges/mhead/min_roughness{mr}", "heads", {"n": 3}, {"min_roughness": mr}, outs=("mat",),
                  feat=cs.inp(rng.uniform(-1, 1, size=(3, 32)).astype(np.float32)),
                  **{k: cs.launches[0]["bufs"][k] for k in ("w0", "b0", "w1", "b1")})
