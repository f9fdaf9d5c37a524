"""The per-ray kernels of csrc/rc_sample.hip (k_sample_intervals, k_sample_level, k_resample, k_composite, k_composite_pick,
k_ladder_bounds) on their own contracts, RcSampleArgs / RcResampleArgs / RcCompositeArgs (csrc/rc_internal.h): the cases, one
reference of every kernel that runs in fp64 (`ft = np.float64`: the contract) and in float32 (`ft = np.float32`: the kernels'
arithmetic restated step by step, sequential sums, no contraction), the tolerances, mutated references and the file format
of the driver tests/sample_check.hip.  numpy only.

Buffers.  Every array a launch reads or writes is a numbered backing buffer with GUARD floats in front and behind; every
float that is not a logical element is a canary NaN (CANARY).  int32 arrays travel as their bits.  An output buffer holds
canaries alone until its launch; a later launch may read it (the ladder bounds feed k_sample_level's s_bounds, k_resample's
filt_weight / acc feed k_composite and k_composite_pick): the reference of the reader then takes the producer's values as
they came back from the device (on the CPU: the producer's float32 restatement), so every launch is held to its own contract
on its own inputs.

Case file (little endian): int64 [magic, n_buf, n_launch, 1 + N_INT + N_FLT + N_BUF], int64 [n_buf][2] (first float of the
stored data or -1 for an output buffer, floats with guards), int64 [n_launch][..] (kernel, ints, float32 bits, buffer
numbers or -1 for a null pointer, in the order of SLOTS), then the float32 data of the stored buffers.
Result file: int64 [magic, n_out, n_launch, driver wall time in us], then every output buffer whole, in buffer order.

Tolerances (u = 2^-24, every bound is on |device - fp64 reference|; S samples, all sums of S terms in any order):
  alpha weights  dd = density |(t1 - t0) |d|| carries <= 6 u relative (one subtraction, |d| = sqrt of a 3-term sum, two
                 products).  alpha = 1 - exp(-dd) carries an ABSOLUTE error: exp <= 2 u of a value <= 1, the argument's
                 6 u dd exp(-dd) <= 2.3 u, the subtraction u/2 -- 5 u in all, and exactly 0 for dd = 0.  The exclusive sum E
                 of the scan is off by (S + 5) u E, which enters the transmittance T = exp(-E) as a RELATIVE error, + 2 u for
                 exp.  w = alpha T +- u w:   tol_w = u (5 T + w (3 + (S + 5) E)) + 2 tiny (results below the normal range)
  acc, composite sums of products   (S + 2) u sum |terms| + sum tol_w |value|  (the gemm test's bound + the weights' error);
                 a product of two shade channels' sum (diffuse, indirect) and the distances |o - m| add 4 u per term
  filt_weight    w_k / (p_k + 1e-8), p = softmax(log w): relative  r_k + (r_k + r_m + u (|l_k| + |m| + |l_k - m| + 4))
                 + sum_j p_j (r_j + r_m + u (|l_j| + |m| + |l_j - m| + 4)) + (S + 4) u  with r = tol_w / w, l = log w, m = max l
  distance_mean  exp(N / max(eps, acc)), N = sum w log(mid):  dN = sum (tol_w |log mid| + w u (2 + 3 |log mid|)) + (S + 2) u
                 sum |w log mid|, de = dN / acc + |N| tol_acc / acc^2 + u |e|, tolerance exp(e) (de + 3 u) (the clip to
                 [t_0, t_S] is 1-Lipschitz)
  ladder         y = |p - 1| / p ((x premult / |p - 1| + 1)^p - 1): the power's argument carries 3 u, the power |p| times
                 that + 2 u of powf on a value P <= 1:  tol = |p - 1| / |p| (P (3 |p| + 2) + 2) u + u |y| (+ premult 6 u x when
                 x is the replaced near)
  resampled posts, percentiles   the inverse CDF amplifies the few ulps between a wave scan and a sequential sum, so the
                 floor is MEASURED on the CPU, max |float32 restatement - fp64| over the family, and the device gets 4 x
                 that (Cases.floors(), measured once per case table; tests/test_sample_ref.py holds them below 2.5e-5).  k_sample_level's tdist: the post's tolerance times
                 the slope of s -> t (|far - near|, or that of the inverse ladder at the post) + the map's own rounding;
                 its means: |d| (5 tol_t + 8 u |t_mean|) + 2 u |mean| + u |o|  (|d t_mean / d t0| + |d t_mean / d t1| <= 5)
  exact family   P a power of two, equal logits, t multiples of 2^-10: weights 1 / P and every partial sum are exact in any
                 order, so the device has to equal the float32 restatement bit for bit
No case and no element is excused."""
import os
import sys

import numpy as np

GUARD = 256                                  # floats; > 3 rows of 65 posts: a store by a clamped wave lands in a guard
CANARY = 0x7FC0BEEF
MAGIC_CASES, MAGIC_RESULTS = 0x53414D5043415345, 0x53414D5052534C54
U = 2.0 ** -24
EPS, TINY, FMAX = (float(v) for v in (np.finfo(np.float32).eps, np.finfo(np.float32).tiny, np.finfo(np.float32).max))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")

RAYS = (1, 3, 4, 5, 9)
BINS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
SAMPLES = (2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64)
PRODUCTION = ((1, 64), (64, 64), (64, 32))

OUT_NAMES = ("rgb", "acc", "distance_mean", "distance_percentile_5", "distance_median", "distance_percentile_95",
             "diffuse_rgb", "specular_rgb", "direct_rgb", "indirect_rgb", "albedo_rgb", "indirect_diffuse_rgb",
             "indirect_specular_rgb", "indirect_occ", "means", "normals", "normals_pred", "ray_dists", "light_dists",
             "env_map_rgb", "rgb_no_env")                             # rc_abi.h's RC_OUT_* in order
OUT_SCALAR = ("acc", "distance_mean", "distance_percentile_5", "distance_median", "distance_percentile_95", "ray_dists",
              "light_dists")
SH_RGB, SH_AD, SH_ID, SH_IS, SH_TINT, SHADE_CH = 0, 3, 6, 9, 12, 15
KERNELS = ("intervals", "level", "resample", "composite", "pick", "ladder")
N_INT, N_FLT, N_BUF = 8, 8, 40
# kernel -> (ints, floats, buffers, the buffers it writes); the driver reads the slots in this order
SLOTS = {
    "intervals": (("n", "P", "S"), (), ("t", "logits", "jitter", "out"), ("out",)),
    "level": (("n", "P", "S", "secondary", "use_raydist"),
              ("anneal", "padding", "raydist_p", "raydist_premult", "eps_dot_min", "far_clamp"),
              ("origins", "directions", "viewdirs", "near", "far", "normals", "prev_sdist", "prev_tdist", "prev_density",
               "prev_weights", "jitter", "sdist", "tdist", "means", "s_bounds"), ("prev_weights", "sdist", "tdist", "means")),
    "resample": (("n", "S"), (), ("tdist", "density", "directions", "gumbel", "inds_in", "inds_out", "filt_weight", "weights",
                                  "acc_out", "src_out", "means", "normals", "pts_out", "nrm_out"),
                 ("inds_out", "filt_weight", "weights", "acc_out", "src_out", "pts_out", "nrm_out")),
    "composite": (("n", "S", "Sf"), ("bg", "pct0", "pct1", "pct2"),
                  ("directions", "origins", "lights", "tdist", "density", "means", "normals_pred", "normals_grad", "shade",
                   "inds", "filt_weight", "weights") + tuple("out_" + k for k in OUT_NAMES),
                  ("weights",) + tuple("out_" + k for k in OUT_NAMES)),
    "pick": (("n",), ("bg",), ("shade_rgb", "filt_weight", "acc", "out_rgb", "out_acc"), ("out_rgb", "out_acc")),
    "ladder": ((), ("near", "far", "far_clamp", "p", "premult"), ("out",), ("out",)),
}
INT_SLOTS = ("inds_in", "inds_out", "src_out", "inds")
PCT_SLOTS = ("out_distance_percentile_5", "out_distance_median", "out_distance_percentile_95")
POST_FAMILIES = ("round", "flat", "level", "pct")
MUTATIONS = ("side_left", "last_post_not_reflected", "no_sort", "cdf_end_not_one", "scan_restart_16", "scan_restart_32",
             "scan_restart_48", "lane63_dropped", "no_excl_shift", "tie_high", "inds_unclamped", "pct_filtered",
             "bg_filtered_acc", "clamped_wave_store", "inversion_check_misses_last", "inversion_check_misses_first")


def canary(n):
    return np.full(n, CANARY, np.uint32).view(np.float32)


def is_canary(x):
    return x.view(np.uint32) == CANARY


def bf16(x):
    """float32 rounded to bfloat16 (nearest even), as float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def out_shape(kernel, slot, i):
    n, P, S = i.get("n", 0), i.get("P", 0), i.get("S", 0)
    if kernel == "intervals":
        return (n, S + 1)
    if kernel == "level":
        return {"prev_weights": (n, P), "sdist": (n, S + 1), "tdist": (n, S + 1), "means": (3, n * S)}[slot]
    if kernel == "resample":
        return {"weights": (n, S), "pts_out": (n, 3), "nrm_out": (n, 3)}.get(slot, (n,))
    if kernel == "composite":
        return (n, S) if slot == "weights" else ((n,) if slot[4:] in OUT_SCALAR else (n, 3))
    if kernel == "pick":
        return (n, 3) if slot == "out_rgb" else (n,)
    return (2,)


class Cases:
    """`spec`: the module that describes the kernels of a case table -- KERNELS, SLOTS, INT_SLOTS, out_shape, reference, the
    two file magics -- this one unless another driver's table (tests/matstage_ref.py) brings its own."""

    def __init__(self, spec=None):
        self.spec = spec or sys.modules[__name__]
        self.bufs, self.stored, self.launches, self.producer = [], [], [], {}
        self._chain, self._floors = {}, None

    def inp(self, a):
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.int32), a.dtype
        self.bufs.append(np.concatenate([canary(GUARD), a.ravel().view(np.float32), canary(GUARD)]))
        self.stored.append(True)
        return len(self.bufs) - 1

    def out(self, shape):
        self.bufs.append(canary(int(np.prod(shape)) + 2 * GUARD))
        self.stored.append(False)
        return len(self.bufs) - 1

    def launch(self, kernel, name, family, ints=None, flts=None, outs=(), **bufs):
        """`bufs`: slot -> buffer number (inputs); `outs`: the output slots to allocate.  Every other slot is a null pointer."""
        ints, flts = dict(ints or {}), {k: float(np.float32(v)) for k, v in (flts or {}).items()}
        si, sf, sb, so = self.spec.SLOTS[kernel]
        assert set(ints) == set(si) and set(flts) == set(sf) and set(bufs) <= set(sb) and set(outs) <= set(so), (kernel, name)
        b = {s: -1 for s in sb}
        b.update(bufs)
        li = len(self.launches)
        for s in outs:
            b[s] = self.out(self.spec.out_shape(kernel, s, ints))
            self.producer[b[s]] = (li, s)
        self.launches.append({"kernel": kernel, "name": name, "family": family, "ints": ints, "flts": flts, "bufs": b})
        return li

    def floors(self):
        """The measured floors of the resampled posts and percentiles: max |float32 restatement - fp64| over the launches of
        a family (k_sample_intervals' rounding and flat families, k_sample_level's sdist, k_composite's percentiles), measured
        once per case table on the CPU.  The device is held to 4 x these."""
        if self._floors is None:
            fl = dict.fromkeys(POST_FAMILIES, 0.0)
            for li, L in enumerate(self.launches):
                slots = {"intervals": ("out",), "level": ("sdist",), "composite": PCT_SLOTS}.get(L["kernel"], ())
                slots = [x for x in slots if L["bufs"][x] >= 0]
                if not slots or L["family"] == "exact":
                    continue
                r64, r32 = reference(self, li, np.float64), reference(self, li, np.float32)
                fam = "pct" if L["kernel"] == "composite" else L["family"]
                for x in slots:
                    fl[fam] = max(fl[fam], float(np.abs(r32[x].astype(np.float64) - r64[x]).max()))
            self._floors = fl
        return self._floors

    def value(self, idx, dev=None):
        """The logical floats of buffer `idx` as a launch reads them: stored data, or what its producer left there."""
        if self.stored[idx]:
            return self.bufs[idx][GUARD:-GUARD]
        if dev is not None:
            return dev[idx][GUARD:-GUARD]
        if idx not in self._chain:
            li, slot = self.producer[idx]
            v = self.spec.reference(self, li, np.float32)[slot]
            self._chain[idx] = (v.astype(np.int32).view(np.float32) if slot in self.spec.INT_SLOTS else v.astype(np.float32)).ravel()
        return self._chain[idx]


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic, in `ft`


def _cumsum(x):
    return np.cumsum(x, axis=-1, dtype=x.dtype)


def _sum(x, mut=None):
    """Sum over the lanes (last axis), sequential in x's type."""
    if mut == "lane63_dropped" and x.shape[-1] == 64:
        x = x[..., :63]
    return _cumsum(x)[..., -1] if x.shape[-1] else np.zeros(x.shape[:-1], x.dtype)


def _scan(x, mut=None):
    incl = _cumsum(x)
    if mut and mut.startswith("scan_restart_"):
        k = int(mut[13:])
        if x.shape[-1] > k:
            incl = np.concatenate([incl[..., :k], _cumsum(x[..., k:])], axis=-1)
    return incl


def uspec(S, has_jitter, ft):
    """stepfun.py:186-202 (make_uspec): double arithmetic, rounded to `ft` on use."""
    if not has_jitter:
        pad = 1.0 / (2.0 * S)
        return ft(pad), ft(1.0 - pad - EPS), ft(0.0)
    u_max = EPS + (1.0 - EPS) / S
    return ft(0.0), ft(1.0 - u_max), ft((1.0 - u_max) / (S - 1) - EPS)


def alpha_weights(ft, density, tdist, dirs, mut=None, cut=False):
    """render.py:143-168 as alpha_weight().  Returns (w, dd, exclusive sum).  `cut`: dd rounded to bfloat16."""
    d = dirs.astype(ft)
    dn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    t = tdist.astype(ft)
    dd = density.astype(ft) * np.abs((t[:, 1:] - t[:, :-1]) * dn[:, None])
    if cut:
        dd = bf16(dd).astype(ft)
    incl = _scan(dd, mut)
    excl = incl if mut == "no_excl_shift" else np.concatenate([np.zeros_like(dd[:, :1]), incl[:, :-1]], axis=-1)
    w = (ft(1.0) - np.exp(-dd)) * np.exp(-excl)
    return w, dd, excl


def safe_log(x):
    return np.log(np.clip(x, x.dtype.type(TINY), x.dtype.type(FMAX)))


def sample_intervals(ft, t, logits, S, jitter=None, mut=None):
    """stepfun.sample_intervals (stepfun.py:125-250, math.py:412-457) as sample_intervals_wave(): [n, S + 1] posts."""
    n, P = logits.shape
    t, lg = t.astype(ft), logits.astype(ft)
    if P > 1:
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.exp(lg - lg.max(axis=-1, keepdims=True))
            wn = e / _sum(e, mut)[:, None]
        incl = _scan(wn, mut)
        last = np.minimum(ft(1.0), incl[:, P - 1:]) if mut == "cdf_end_not_one" else np.ones((n, 1), ft)
        cw = np.concatenate([np.zeros((n, 1), ft), np.minimum(ft(1.0), incl[:, :P - 1]), last], axis=-1)
    else:
        cw = np.tile(np.array([[0.0, 1.0]], ft), (n, 1))
    start, stop, mj = uspec(S, jitter is not None, ft)
    step = np.arange(S).astype(ft) / ft(S - 1)
    u = start * (ft(1.0) - step) + stop * step
    u[S - 1] = stop
    u = np.tile(u, (n, 1))
    if jitter is not None:
        u = u + jitter.astype(ft)[:, None] * mj
    out = np.empty((n, S + 1), ft)
    eps2 = ft(EPS) * ft(EPS)
    for r in range(n):
        idx = np.searchsorted(cw[r], u[r], side="left" if mut == "side_left" else "right")
        i1, i0 = np.minimum(idx, P), np.maximum(idx - 1, 0)
        c0, c1, t0, t1 = cw[r][i0], cw[r][i1], t[r][i0], t[r][i1]
        off = np.clip((u[r] - c0) / np.maximum(eps2, c1 - c0), ft(0.0), ft(1.0))
        c = t0 + off * (t1 - t0)
        mid = (c[1:] + c[:-1]) / ft(2.0)
        first = ft(2.0) * c[0] - mid[0]
        last = c[-1] if mut == "last_post_not_reflected" else ft(2.0) * c[-1] - mid[-1]
        v = np.clip(np.concatenate([[first], mid, [last]]).astype(ft), ft(0.0), ft(1.0))
        if mut in ("inversion_check_misses_last", "inversion_check_misses_first"):      # the ballot over the pairs, one short
            inv = v[:-1] > v[1:]
            need = (inv[:-1] if mut.endswith("last") else inv[1:]).any()
            out[r] = np.sort(v, kind="stable") if need else v
        else:
            out[r] = v if mut == "no_sort" else np.sort(v, kind="stable")
    return out


def power_ladder(ft, x, p, premult):
    x = x.astype(ft) * ft(premult)
    pm1 = np.abs(ft(p) - ft(1.0))
    xs = np.abs(x) / np.maximum(ft(TINY), pm1)
    y = pm1 / ft(p) * (np.power(xs + ft(1.0), ft(p)) - ft(1.0))
    y = np.clip(y, ft(-FMAX), ft(FMAX))
    return np.where(x < 0, -y, y)


def ladder_y_max(p):
    return float(np.nextafter(np.float32((np.float32(p) - np.float32(1.0)) / np.float32(p)), np.float32(-np.inf)))


def inv_power_ladder(ft, y, p, premult):
    yp = np.abs(y)
    if p < 0:
        ym = ft(ladder_y_max(p))
        yp = np.clip(yp, -ym, ym)
    pm1 = np.abs(ft(p) - ft(1.0))
    x = pm1 * (np.power((ft(p) / pm1) * yp + ft(1.0), ft(1.0) / ft(p)) - ft(1.0))
    return np.where(y < 0, -x, x) / ft(premult)


def interp1(ft, x, xp, fp):
    """jnp.interp as interp1() of rc_dev_sample.h, one x."""
    m = len(xp)
    i = int(np.clip(np.searchsorted(xp, x, side="right"), 1, m - 1))
    df, dxx, delta = fp[i] - fp[i - 1], xp[i] - xp[i - 1], x - xp[i - 1]
    f = fp[i - 1] if abs(dxx) <= ft(1.4210855e-14) else fp[i - 1] + (delta / dxx) * df
    if x < xp[0]:
        f = fp[0]
    if x > xp[m - 1]:
        f = fp[m - 1]
    return f


# ---------------------------------------------------------------------------------------------------------------------------
# references per kernel: {slot: values in ft (ints as int64), "_...": what the tolerances need}


def _args(cs, L, dev):
    i, f, b = L["ints"], L["flts"], L["bufs"]

    def get(slot, shape, dtype=np.float32):
        if b[slot] < 0:
            return None
        v = cs.value(b[slot], dev)
        assert v.size == int(np.prod(shape)), (L["name"], slot, v.size, shape)
        return v.view(dtype).reshape(shape)
    return i, f, b, get


def ref_intervals(cs, L, ft, mut, dev):
    i, f, b, get = _args(cs, L, dev)
    n, P, S = i["n"], i["P"], i["S"]
    return {"out": sample_intervals(ft, get("t", (n, P + 1)), get("logits", (n, P)), S, get("jitter", (n,)), mut)}


def ref_ladder(cs, L, ft, mut, dev):
    f = L["flts"]
    x = np.array([f["near"], min(np.float32(f["far"]), np.float32(f["far_clamp"]))], np.float32)
    return {"out": power_ladder(ft, x, f["p"], f["premult"])}


def ref_level(cs, L, ft, mut, dev):
    i, f, b, get = _args(cs, L, dev)
    n, P, S = i["n"], i["P"], i["S"]
    o, d = get("origins", (n, 3)).astype(ft), get("directions", (n, 3)).astype(ft)
    near, far = get("near", (n,)).astype(ft), get("far", (n,)).astype(ft)
    out = {"_near_replaced": np.zeros(n, bool)}
    if i["secondary"]:
        far = np.minimum(far, ft(f["far_clamp"]))
        nrm = get("normals", (n, 3))
        if nrm is not None:
            v, nrm = get("viewdirs", (n, 3)).astype(ft), nrm.astype(ft)
            dp = v[:, 0] * nrm[:, 0] + v[:, 1] * nrm[:, 1] + v[:, 2] * nrm[:, 2]
            off = np.clip(ft(f["eps_dot_min"]) / np.maximum(dp, ft(1e-5)), near, far)
            off = np.where(dp > 0, off, near)
            near = np.maximum(near, off)
            near = np.minimum(np.maximum(near, ft(1e-5)), far - ft(1e-5))
            out["_near_replaced"][:] = True
    if b["prev_sdist"] < 0:
        assert P == 1
        w = np.ones((n, 1), ft)
        st = np.tile(np.array([[0.0, 1.0]], ft), (n, 1))
    else:
        w, dd, excl = alpha_weights(ft, get("prev_density", (n, P)), get("prev_tdist", (n, P + 1)), d, mut)
        st = get("prev_sdist", (n, P + 1))
        out.update(_pw=w, _dd=dd, _excl=excl)
        if b["prev_weights"] >= 0:
            out["prev_weights"] = w
    logit = ft(f["anneal"]) * safe_log(w + ft(f["padding"]))
    s = sample_intervals(ft, st, logit, S, get("jitter", (n,)), mut)
    if i["use_raydist"]:
        sb = get("s_bounds", (2,))
        if sb is not None:
            s_near, s_far = np.full(n, sb[0], ft), np.full(n, sb[1], ft)
        else:
            s_near, s_far = (power_ladder(ft, x, f["raydist_p"], f["raydist_premult"]) for x in (near, far))
        y = s * s_far[:, None] + (ft(1.0) - s) * s_near[:, None]
        t = inv_power_ladder(ft, y, f["raydist_p"], f["raydist_premult"])
        out.update(_y=y, _s_near=s_near, _s_far=s_far)
    else:
        t = s * far[:, None] + (ft(1.0) - s) * near[:, None]
    out.update(sdist=s, tdist=t, _near=near, _far=far)
    if b["means"] >= 0:
        t0, t1 = t[:, :-1], t[:, 1:]
        sm, df = t0 + t1, t1 - t0
        tm = sm * (ft(0.5) + (df * df) / np.maximum(ft(EPS) * ft(EPS), ft(3.0) * (sm * sm) + df * df))
        out["means"] = np.stack([(d[:, c, None] * tm + o[:, c, None]).ravel() for c in range(3)])
        out["_tm"] = tm
    return out


def ref_resample(cs, L, ft, mut, dev, cut=False):
    i, f, b, get = _args(cs, L, dev)
    n, S = i["n"], i["S"]
    w, dd, excl = alpha_weights(ft, get("density", (n, S)), get("tdist", (n, S + 1)), get("directions", (n, 3)), mut, cut)
    logit = safe_log(w)
    m = logit.max(axis=-1, keepdims=True)
    e = np.exp(logit - m)
    p = e / _sum(e, mut)[:, None]
    if b["inds_in"] >= 0:
        raw = get("inds_in", (n,), np.int32).astype(np.int64)
        ind = raw if mut == "inds_unclamped" else np.clip(raw, 0, S - 1)
    else:
        key = logit + get("gumbel", (n, S)).astype(ft)
        ind = np.argmax(key, axis=-1)
        if mut == "tie_high":
            ind = S - 1 - np.argmax(key[:, ::-1], axis=-1)
    rows, sel = np.arange(n), np.clip(ind, 0, S - 1)
    out = {"weights": w, "inds_out": ind, "filt_weight": w[rows, sel] / (ft(1.0) * p[rows, sel] + ft(1e-8)),
           "_dd": dd, "_excl": excl, "_p": p, "_logit": logit, "_sel": sel}
    if b["acc_out"] >= 0:
        out["acc_out"] = _sum(w, mut)
    if b["src_out"] >= 0:
        out["src_out"] = rows * S + ind
    if b["pts_out"] >= 0:
        q = rows * S + sel
        out["pts_out"] = get("means", (3, n * S)).astype(ft)[:, q].T
        out["nrm_out"] = get("normals", (3, n * S)).astype(ft)[:, q].T
    return out


def ref_composite(cs, L, ft, mut, dev, cut=False):
    i, f, b, get = _args(cs, L, dev)
    n, S, Sf = i["n"], i["S"], i["Sf"]
    d = get("directions", (n, 3))
    t = get("tdist", (n, S + 1)).astype(ft)
    wnf, dd, excl = alpha_weights(ft, get("density", (n, S)), t, d, mut, cut)
    acc = _sum(wnf, mut)
    out = {"_wnf": wnf, "_dd": dd, "_excl": excl, "_acc": acc, "_terms": {}, "_val": {}}
    resampled = Sf == 1 and b["inds"] >= 0
    rows = np.arange(n)
    if resampled:
        sel = get("inds", (n,), np.int32).astype(np.int64)
        hit = (sel >= 0) & (sel < S)                                   # no lane equals a pick outside [0, S): all zero
        w = np.zeros((n, S), ft)
        w[rows[hit], sel[hit]] = get("filt_weight", (n,)).astype(ft)[hit]
        sh = np.zeros((SHADE_CH, n, S), ft)
        sh[:, rows[hit], sel[hit]] = get("shade", (SHADE_CH, n)).astype(ft)[:, hit]
    else:
        assert Sf == S
        w = wnf
        sh = get("shade", (SHADE_CH, n, S)).astype(ft)
    out["_w"] = w

    def put(name, terms, shape3=True, extra=None, per_term=0.0):
        if b["out_" + name] < 0:
            return
        v = _sum(terms, mut if not resampled else None)                # [c, n] or [n]
        if extra is not None:
            v = v + extra
        out["out_" + name] = v.T if shape3 else v
        out["_terms"]["out_" + name] = (terms, per_term)

    bgw = np.maximum(ft(0.0), ft(1.0) - (_sum(w) if mut == "bg_filtered_acc" else acc)) * ft(f["bg"])
    put("rgb", w[None] * sh[SH_RGB:SH_RGB + 3], extra=bgw[None])
    put("direct_rgb", w[None] * sh[SH_AD:SH_AD + 3])
    put("indirect_diffuse_rgb", w[None] * sh[SH_ID:SH_ID + 3])
    put("indirect_specular_rgb", w[None] * sh[SH_IS:SH_IS + 3])
    put("specular_rgb", w[None] * sh[SH_IS:SH_IS + 3])
    put("albedo_rgb", w[None] * sh[SH_TINT:SH_TINT + 3])
    put("diffuse_rgb", w[None] * (sh[SH_AD:SH_AD + 3] + sh[SH_ID:SH_ID + 3]), per_term=1.0)
    put("indirect_rgb", w[None] * (sh[SH_ID:SH_ID + 3] + sh[SH_IS:SH_IS + 3]), per_term=1.0)
    put("indirect_occ", np.broadcast_to(w[None], (3, n, S)).copy())
    mean = get("means", (3, n, S))
    if mean is not None:
        mean = mean.astype(ft)
        put("means", w[None] * mean)
        for name, src in (("ray_dists", "origins"), ("light_dists", "lights")):
            p0 = get(src, (n, 3))
            if p0 is not None:
                p0 = p0.astype(ft)
                dx, dy, dz = (p0[:, c, None] - mean[c] for c in range(3))
                put(name, w * np.sqrt(dx * dx + dy * dy + dz * dz), shape3=False, per_term=4.0)
    for name, src in (("normals_pred", "normals_pred"), ("normals", "normals_grad")):
        v = get(src, (3, n, S))
        if v is not None:
            put(name, w[None] * v.astype(ft))
    if b["weights"] >= 0:
        out["weights"] = wnf
    if b["out_acc"] >= 0:
        out["out_acc"] = acc
    if any(b["out_" + k] >= 0 for k in OUT_NAMES[2:6]):
        wd = w if mut == "pct_filtered" else wnf
        tmid = ft(0.5) * (t[:, :-1] + t[:, 1:])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            lt = np.log(tmid)
            den = np.maximum(ft(EPS), acc)
            e = _sum(wnf * lt, mut) / den
            dm = np.exp(e)
        dm = np.where(np.isnan(dm), ft(0.0), dm)
        dm = np.minimum(dm, ft(FMAX))
        dm = np.minimum(np.maximum(dm, t[:, 0]), t[:, S])
        out.update(_lt=lt, _e=e)
        if b["out_distance_mean"] >= 0:
            out["out_distance_mean"] = dm
        incl = _scan(wd / den[:, None], mut)
        last = np.minimum(ft(1.0), incl[:, S - 1:]) if mut == "cdf_end_not_one" else np.ones((n, 1), ft)
        cw = np.concatenate([np.zeros((n, 1), ft), np.minimum(ft(1.0), incl[:, :S - 1]), last], axis=-1)
        for k, name in enumerate(("distance_percentile_5", "distance_median", "distance_percentile_95")):
            if b["out_" + name] >= 0:
                ps = ft(f["pct%d" % k]) / ft(100.0)
                out["out_" + name] = np.array([interp1(ft, ps, cw[r], t[r]) for r in range(n)], ft)
    return out


def ref_pick(cs, L, ft, mut, dev):
    i, f, b, get = _args(cs, L, dev)
    n = i["n"]
    acc = get("acc", (n,)).astype(ft)
    out = {}
    if b["out_rgb"] >= 0:
        bgw = np.maximum(ft(0.0), ft(1.0) - acc) * ft(f["bg"])
        out["out_rgb"] = (get("filt_weight", (n,)).astype(ft)[None] * get("shade_rgb", (3, n)).astype(ft) + bgw[None]).T
    if b["out_acc"] >= 0:
        out["out_acc"] = acc
    return out


REFS = {"intervals": ref_intervals, "level": ref_level, "resample": ref_resample, "composite": ref_composite, "pick": ref_pick,
        "ladder": ref_ladder}


def reference(cs, li, ft=np.float64, mut=None, dev=None, **kw):
    L = cs.launches[li]
    with np.errstate(under="ignore", over="ignore"):
        return REFS[L["kernel"]](cs, L, ft, mut, dev, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# tolerances, from the fp64 reference


def tol_alpha(S, w, dd, excl):
    T = np.exp(-excl)
    return np.where(dd == 0, 0.0, U * (5.0 * T + w * (3.0 + (S + 5) * excl)) + 2 * TINY)


def tol_ladder(x, p, premult, replaced=False):
    pm1 = abs(p - 1.0)
    pw = (np.abs(x * premult) / pm1 + 1.0) ** p
    y = pm1 / abs(p) * np.abs(pw - 1.0)
    return pm1 / abs(p) * (pw * (3 * abs(p) + 2) + 2) * U + U * y + (premult * 6 * U * np.abs(x) if replaced else 0.0)


def tolerances(cs, li, ref):
    """{output slot: bound on |device - ref| (0: the same bits / the same integer)} for the fp64 reference `ref`."""
    L = cs.launches[li]
    k, i, f, fam = L["kernel"], L["ints"], L["flts"], L["family"]
    S = i.get("S", 0)
    if k == "intervals":
        return {"out": 0.0 if fam == "exact" else 4.0 * cs.floors()[fam]}
    if k == "ladder":
        x = np.array([f["near"], min(f["far"], f["far_clamp"])])
        return {"out": tol_ladder(x, f["p"], f["premult"])}
    if k == "pick":
        return {"out_acc": 0.0, "out_rgb": 3 * U * np.abs(ref["out_rgb"]) + 2 * U * abs(f["bg"])} if "out_rgb" in ref else {"out_acc": 0.0}
    if k == "level":
        tol = {}
        if "prev_weights" in ref:
            tol["prev_weights"] = tol_alpha(i["P"], ref["_pw"], ref["_dd"], ref["_excl"])
        ts = 4.0 * cs.floors()["level"]
        tol["sdist"] = ts
        near, far = ref["_near"], ref["_far"]
        if i["use_raydist"]:
            p, pm = f["raydist_p"], f["raydist_premult"]
            pm1 = abs(p - 1.0)
            sn, sf = ref["_s_near"], ref["_s_far"]
            if L["bufs"]["s_bounds"] >= 0:
                dl = 0.0                                                  # an input of this launch
            else:
                dl = tol_ladder(near, p, pm, ref["_near_replaced"].any()) + tol_ladder(far, p, pm)
            dy = (np.abs(sf - sn) * ts + dl + 3 * U * np.maximum(np.abs(sn), np.abs(sf)))[:, None]
            ym = ladder_y_max(p)
            base = lambda y: (p / pm1) * np.clip(np.abs(y), 0, ym) + 1.0
            slope = np.maximum(base(ref["_y"]) ** (1.0 / p - 1.0), base(np.abs(ref["_y"]) + dy) ** (1.0 / p - 1.0)) / pm
            pw = base(ref["_y"]) ** (1.0 / p)
            tol["tdist"] = slope * dy + (pm1 * pw * 4 * U + 2 * U * np.abs(ref["tdist"]) * pm) / pm
        else:
            tol["tdist"] = (np.abs(far - near) * ts + 4 * U * np.maximum(np.abs(near), np.abs(far)))[:, None] * np.ones_like(ref["tdist"])
        if "means" in ref:
            n = i["n"]
            tt = np.maximum(tol["tdist"][:, :-1], tol["tdist"][:, 1:])
            d, o = (cs.value(L["bufs"][s]).reshape(n, 3).astype(np.float64) for s in ("directions", "origins"))
            tol["means"] = np.stack([(np.abs(d[:, c, None]) * (5 * tt + 8 * U * np.abs(ref["_tm"])) + U * np.abs(o[:, c, None])).ravel()
                                     for c in range(3)]) + 2 * U * np.abs(ref["means"])
        return tol
    tw = tol_alpha(S, ref["weights"] if k == "resample" else ref["_wnf"], ref["_dd"], ref["_excl"])
    if k == "resample":
        w, p, lg, sel = ref["weights"], ref["_p"], ref["_logit"], ref["_sel"]
        rows = np.arange(i["n"])
        r = tw / np.maximum(w, TINY)
        m = lg.max(axis=-1, keepdims=True)
        rm = r[rows, lg.argmax(axis=-1)][:, None]
        re = r + rm + U * (np.abs(lg) + np.abs(m) + np.abs(lg - m) + 4)
        rel = r[rows, sel] + re[rows, sel] + (p * re).sum(axis=-1) + (S + 4) * U
        tol = {"weights": tw, "inds_out": 0.0, "src_out": 0.0, "pts_out": 0.0, "nrm_out": 0.0,
               "filt_weight": rel * np.abs(ref["filt_weight"]) + 2 * TINY}
        if "acc_out" in ref:
            tol["acc_out"] = (S + 2) * U * w.sum(axis=-1) + tw.sum(axis=-1)
        return {s: t for s, t in tol.items() if s in ref}
    assert k == "composite"
    resampled = i["Sf"] == 1 and L["bufs"]["inds"] >= 0
    acc = ref["_acc"]
    tacc = (S + 2) * U * acc + tw.sum(axis=-1)
    tol = {"weights": tw, "out_acc": tacc}
    for slot, (terms, per_term) in ref["_terms"].items():
        wt = np.zeros_like(tw) if resampled else tw                       # the filtered weight is an input
        with np.errstate(invalid="ignore", divide="ignore"):
            val = np.where(ref["_w"] > 0, np.abs(terms) / ref["_w"], 0.0)
        t = ((S + 2) + per_term) * U * np.abs(terms).sum(axis=-1) + (wt * val).sum(axis=-1)
        if slot == "out_rgb":
            t = t + (tacc * abs(f["bg"]) + 2 * U * abs(f["bg"]))[None]
        tol[slot] = t.T if t.ndim == 2 else t
    if "_e" in ref:
        with np.errstate(invalid="ignore", divide="ignore"):
            lt, e, w = np.abs(ref["_lt"]), ref["_e"], ref["_wnf"]
            dn = (np.where(w > 0, tw * lt + w * U * (2 + 3 * lt), 0.0)).sum(axis=-1) + (S + 2) * U * np.where(w > 0, w * lt, 0.0).sum(axis=-1)
            den = np.maximum(EPS, acc)
            de = dn / den + np.abs(e) * tacc / den + U * np.abs(e)
            t = np.exp(e) * (de + 3 * U)
        tol["out_distance_mean"] = np.where(np.isfinite(t), t, 0.0)      # acc == 0 (every weight exactly 0): e is 0 or NaN exactly
        for name in ("distance_percentile_5", "distance_median", "distance_percentile_95"):
            tol["out_" + name] = 4.0 * cs.floors()["pct"]
    return {s: t for s, t in tol.items() if s in ref}


def expected(cs, li, dev=None):
    """(reference, tolerances) a device run of launch `li` is held to: the fp64 reference and its bounds, or for the exact
    family the float32 restatement and the same bits."""
    ref = reference(cs, li, np.float64, dev=dev)
    if cs.launches[li]["family"] == "exact":
        return reference(cs, li, np.float32, dev=dev), {"out": 0.0}
    return ref, tolerances(cs, li, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# checking a set of output buffers against a reference (the GPU test on the device's buffers, the CPU test on mutated ones)


def render(cs, li, ref, mut=None):
    """The output buffers a device that computed `ref` in float32 would leave: {buffer: floats with guards}."""
    L = cs.launches[li]
    out = {}
    for slot in cs.spec.SLOTS[L["kernel"]][3]:
        idx = L["bufs"][slot]
        if idx < 0:
            continue
        if slot not in ref:                                               # allocated, not to be written
            out[idx] = cs.bufs[idx].copy()
            continue
        v = ref[slot]
        v = v.astype(np.int32).view(np.float32) if slot in cs.spec.INT_SLOTS else v.astype(np.float32)
        buf = cs.bufs[idx].copy()
        buf[GUARD:GUARD + v.size] = v.ravel()
        n = L["ints"].get("n", 0)
        if mut == "clamped_wave_store" and L["kernel"] in ("intervals", "level", "composite") and n % 4 and v.ndim == 2 and v.shape[0] == n:
            for extra in range(4 - n % 4):                               # the waves past n store their (clamped) ray's row
                at = GUARD + v.size + extra * v.shape[1]
                buf[at:at + v.shape[1]] = v[-1]
        out[idx] = buf
    return out


def check(cs, li, got, ref, tol):
    """`got`: {buffer: floats with guards}.  Returns (failures [(slot, what, figure)], {slot: max error / tolerance})."""
    L = cs.launches[li]
    bad, ratio = [], {}
    for slot in cs.spec.SLOTS[L["kernel"]][3]:
        idx = L["bufs"][slot]
        if idx < 0:
            continue
        shape = cs.spec.out_shape(L["kernel"], slot, L["ints"])
        size = int(np.prod(shape))
        buf = got[idx]
        if not (is_canary(buf[:GUARD]).all() and is_canary(buf[GUARD + size:]).all()):
            bad.append((slot, "canary", int((~is_canary(np.concatenate([buf[:GUARD], buf[GUARD + size:]]))).sum())))
        g = buf[GUARD:GUARD + size]
        if slot not in ref:                                               # allocated but not to be written
            if not is_canary(g).all():
                bad.append((slot, "written", int((~is_canary(g)).sum())))
            continue
        want = np.asarray(ref[slot])
        if slot in cs.spec.INT_SLOTS:
            if not np.array_equal(g.view(np.int32).astype(np.int64), want.ravel()):
                bad.append((slot, "index", g.view(np.int32).tolist()))
            continue
        g64 = g.astype(np.float64).reshape(shape)
        t = np.broadcast_to(np.asarray(tol[slot], np.float64), shape)
        if np.isnan(g64).any() or np.isnan(t).any():
            bad.append((slot, "nan", int(np.isnan(g64).sum())))
            continue
        exact = t == 0
        if exact.any():
            a, b = g.reshape(shape)[exact], want.astype(np.float32)[exact]
            # a bound of 0 asks for the same value; the exact family for the same bits.  (A sum of products that are all
            # zero is +0 or -0 with the order of the additions: both are the value the contract names.)
            if not (np.array_equal(a.view(np.uint32), b.view(np.uint32)) if L["family"] == "exact" else np.array_equal(a, b)):
                bad.append((slot, "bits" if L["family"] == "exact" else "value", float(np.abs(g64 - want)[exact].max())))
        err = np.abs(g64 - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(exact, 0.0, err / t).max(initial=0.0))
        ratio[slot] = r
        if r > 1.0:
            bad.append((slot, "tolerance", r))
        if L["kernel"] in ("intervals", "level") and slot in ("out", "sdist"):
            if not ((np.diff(g64, axis=-1) >= 0).all() and g64.min() >= 0 and g64.max() <= 1):
                bad.append((slot, "sorted in [0, 1]", float(np.diff(g64, axis=-1).min())))
    return bad, ratio


# ---------------------------------------------------------------------------------------------------------------------------
# file formats


def write_case_file(path, cs):
    nf = 1 + N_INT + N_FLT + N_BUF
    table, at = [], 0
    for buf, stored in zip(cs.bufs, cs.stored):
        table.append((at if stored else -1, buf.size))
        at += buf.size if stored else 0
    rec = np.full((len(cs.launches), nf), -1, np.int64)
    for n, L in enumerate(cs.launches):
        si, sf, sb, _ = cs.spec.SLOTS[L["kernel"]]
        rec[n, 0] = cs.spec.KERNELS.index(L["kernel"])
        rec[n, 1:1 + N_INT] = 0
        rec[n, 1 + N_INT:1 + N_INT + N_FLT] = 0
        for j, s in enumerate(si):
            rec[n, 1 + j] = L["ints"][s]
        for j, s in enumerate(sf):
            rec[n, 1 + N_INT + j] = int(np.float32(L["flts"][s]).view(np.uint32))
        for j, s in enumerate(sb):
            rec[n, 1 + N_INT + N_FLT + j] = L["bufs"][s]
    with open(path, "wb") as fh:
        np.array([cs.spec.MAGIC_CASES, len(cs.bufs), len(cs.launches), nf], np.int64).tofile(fh)
        np.array(table, np.int64).reshape(-1, 2).tofile(fh)
        rec.tofile(fh)
        for buf, stored in zip(cs.bufs, cs.stored):
            if stored:
                buf.tofile(fh)


def read_results(path, cs):
    """{buffer: floats with guards} of every output buffer, and the driver's wall time in seconds."""
    head = np.fromfile(path, np.int64, 4)
    outs = [n for n, s in enumerate(cs.stored) if not s]
    assert head[0] == cs.spec.MAGIC_RESULTS and head[1] == len(outs) and head[2] == len(cs.launches), head
    data = np.fromfile(path, np.float32, offset=32)
    assert data.size == sum(cs.bufs[n].size for n in outs), data.size
    got, at = {}, 0
    for n in outs:
        got[n] = data[at:at + cs.bufs[n].size]
        at += cs.bufs[n].size
    return got, head[3] * 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# cases


def pairs():
    """(P, S): every S with P = 1 and P = 64, every P with S = 32 and S = 64, the diagonal, the production pairs."""
    ps = [(P, S) for P in (1, 64) for S in SAMPLES] + [(P, S) for S in (32, 64) for P in BINS]
    ps += [(S, S) for S in SAMPLES] + list(PRODUCTION)
    return sorted(set(ps))


def _rays(rng, n):
    d = rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, size=(n, 1))
    return (rng.uniform(-1, 1, size=(n, 3)).astype(np.float32), d.astype(np.float32))


def _sorted_posts(rng, n, P, lo=0.0, hi=1.0):
    t = np.sort(rng.uniform(lo, hi, size=(n, P + 1)), axis=-1)
    t[:, 0], t[:, -1] = lo, hi
    return t.astype(np.float32)


def _jitter(rng, n):
    j = rng.uniform(0, 1, size=n).astype(np.float32)
    j[0] = 0.0
    j[-1] = np.nextafter(np.float32(1.0), np.float32(0.0))             # n == 1: the largest float below 1
    return j


def _density(rng, n, S, kinds, t=None, d=None):
    """kinds per ray: 'o' ordinary (a third of the samples empty), 'z' zero everywhere, 's' saturating in its first intervals,
    'l' late (only the last two samples have density: the last lane carries the weight),
    'm' moderate (every dd in [0.02, 0.5] for unit-length intervals: well-conditioned weights).  With the posts `t` and the
    directions `d` an ordinary sample's dd = density |dt| |d| is 0 or in [0.05, 0.05 + 6 / S]: alpha = 1 - exp(-dd) then
    carries its absolute error of an ulp of 1 as a relative error <= 6e-6, which the proposal sampler's padding of 1e-5
    inside the logarithm would otherwise blow up to a per cent of a bin's weight."""
    dens = np.exp(rng.uniform(-1.0, 3.5, size=(n, S)))
    if t is not None:
        dt = np.abs(np.diff(t.astype(np.float64), axis=-1)) * np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)
        dens = rng.uniform(0.05, 0.05 + 6.0 / S, size=(n, S)) / np.maximum(dt, 1e-6)
    keep = rng.uniform(size=(n, S)) > 0.33
    keep[:, -2:] |= np.array([k == "l" for k in kinds])[:, None]
    dens = dens * keep
    for r, k in enumerate(kinds):
        if k == "z":
            dens[r] = 0.0
        elif k == "s":
            dens[r, :2] = 3e4 if t is None else 300.0 / np.maximum(dt[r, :2], 1e-6)
        elif k == "m":
            dens[r] = rng.uniform(0.02, 0.5, size=S)
        elif k == "l":
            dens[r, :max(S - 2, 0)] = 0.0
    return dens.astype(np.float32)


def _kinds(n, j, moderate=False):
    if moderate:
        return ["m"] * n
    return [("o", "z", "s", "l", "z")[(r + j) % 5] for r in range(n)]


def _tdist(rng, n, S, kinds, unit=False):
    """Sorted t posts per ray; a 'z' ray starts at -0.25, 0.25: the first midpoint is 0, log 0 = -inf, 0 * -inf = NaN."""
    if unit:                                                            # |d| = 1 and every interval 1 long: dd = density
        return np.tile(np.arange(1, S + 2, dtype=np.float32), (n, 1))
    t = np.sort(rng.uniform(0.3, 5.0, size=(n, S + 1)), axis=-1).astype(np.float32)
    for r, k in enumerate(kinds):
        if k == "z" and r % 2 == 1:
            t[r, 0], t[r, 1] = -0.25, 0.25
    return t


def build_cases(seed=20240607):
    rng = np.random.default_rng(seed)
    cs = Cases()
    P_S = pairs()
    pct = {"pct0": 5.0, "pct1": 50.0, "pct2": 95.0}
    # --- k_sample_intervals
    for j, (P, S) in enumerate(P_S):
        n = RAYS[j % 5]
        tag = f"P{P}S{S}n{n}"
        for jit in (False, True):
            t, lg = _sorted_posts(rng, n, P), rng.uniform(-2, 2, size=(n, P)).astype(np.float32)
            kw = {"jitter": cs.inp(_jitter(rng, n))} if jit else {}
            cs.launch("intervals", f"si/round/{tag}/j{int(jit)}", "round", {"n": n, "P": P, "S": S}, outs=("out",), t=cs.inp(t),
                      logits=cs.inp(lg), **kw)
            if P & (P - 1) == 0:
                t = np.sort(rng.integers(0, 1025, size=(n, P + 1)), axis=-1).astype(np.float32) / 1024
                lg = np.full((n, P), rng.integers(-3, 4), np.float32)
                kw = {"jitter": cs.inp(_jitter(rng, n))} if jit else {}
                cs.launch("intervals", f"si/exact/{tag}/j{int(jit)}", "exact", {"n": n, "P": P, "S": S}, outs=("out",),
                          t=cs.inp(t), logits=cs.inp(lg), **kw)
        if P >= 3:
            t, lg = _sorted_posts(rng, n, P), rng.uniform(-2, 2, size=(n, P)).astype(np.float32)
            lg[rng.uniform(size=(n, P)) < 0.4] = -100.0
            lg[:, 0] = np.where(lg[:, 0] == -100.0, 0.5, lg[:, 0])       # u = 0 (jitter 0) stays off a repeated post at 0
            lg[:, -1] = np.where(lg[:, -1] == -100.0, -0.5, lg[:, -1])   # and u = 1 - 2 eps (the largest jitter) off one at 1
            cs.launch("intervals", f"si/flat/{tag}", "flat", {"n": n, "P": P, "S": S}, outs=("out",), t=cs.inp(t),
                      logits=cs.inp(lg), jitter=cs.inp(_jitter(rng, n)))
            cs.launch("intervals", f"si/flat/{tag}/j0", "flat", {"n": n, "P": P, "S": S}, outs=("out",), t=cs.inp(t),
                      logits=cs.inp(lg))
    for P, S, n in ((64, 64, 5), (33, 17, 3), (17, 33, 9), (3, 64, 1), (64, 32, 4)):
        tag = f"P{P}S{S}n{n}"
        first = np.full((n, P), -np.inf, np.float32)
        first[:, 0] = 1.0
        lastb = np.full((n, P), -np.inf, np.float32)                     # exp(-inf) = 0 in every precision: P - 1 posts
        lastb[:, -1] = -1.0                                              # exactly 0, and u = 0 (jitter 0) ties with them
        rep = _sorted_posts(rng, n, P)
        rep[:, 1:P:2] = rep[:, 0:P - 1:2][:, :rep[:, 1:P:2].shape[1]]    # every other bin has zero width
        desc = np.ascontiguousarray(_sorted_posts(rng, n, P)[:, ::-1])   # t not ascending: the sort has work to do
        for name, t, lg in (("first", _sorted_posts(rng, n, P), first), ("last", _sorted_posts(rng, n, P), lastb),
                            ("repeated_t", rep, rng.uniform(-2, 2, size=(n, P)).astype(np.float32)),
                            ("descending_t", desc, rng.uniform(-2, 2, size=(n, P)).astype(np.float32))):
            for jit in (False, True):
                kw = {"jitter": cs.inp(_jitter(rng, n))} if jit else {}
                cs.launch("intervals", f"si/flat/{name}/{tag}/j{int(jit)}", "flat", {"n": n, "P": P, "S": S}, outs=("out",),
                          t=cs.inp(t), logits=cs.inp(lg), **kw)
    # --- k_ladder_bounds and k_sample_level
    # eps_dot_min 0.08: with near in [0.02, 0.3] and far in [1, 1.9] the replaced near eps / dp lies inside (near, far) for
    # dp = 0.6 and 0.9 on most rays, at far for the tiny dp, and stays the ray's own for dp <= 0
    lad = {"raydist_p": -1.5, "raydist_premult": 2.0, "eps_dot_min": 0.08, "far_clamp": 2.0}
    for near, far, clamp in ((0.05, 1.0, 2.0), (1e-3, 6.0, 2.0), (0.3, 1.7, 1e6), (0.0, 0.5, 2.0)):
        cs.launch("ladder", f"ladder/{near}/{far}/{clamp}", "ladder",
                  flts={"near": near, "far": far, "far_clamp": clamp, "p": -1.5, "premult": 2.0}, outs=("out",))
    cs.launch("ladder", "ladder/p-0.5", "ladder", flts={"near": 0.2, "far": 3.0, "far_clamp": 2.5, "p": -0.5, "premult": 1.0},
              outs=("out",))
    for j, (P, S) in enumerate(P_S):
        n = RAYS[(j + 2) % 5]
        variant = j % 6
        o, d = _rays(rng, n)
        ints = {"n": n, "P": P, "S": S, "secondary": int(variant in (2, 3, 5)), "use_raydist": int(variant in (2, 3, 5))}
        flts = dict(lad, anneal=0.4, padding=1e-5)
        near = rng.uniform(0.02, 0.3, size=n).astype(np.float32)
        far = rng.uniform(1.0, 1.9, size=n).astype(np.float32)
        if variant == 5:
            far[::2] = 6.0                                               # beyond far_clamp
        if variant == 3:
            near[:], far[:] = 0.05, 6.0
        kw = {"origins": cs.inp(o), "directions": cs.inp(d), "near": cs.inp(near), "far": cs.inp(far)}
        outs = ["sdist", "tdist"] + ([] if variant == 4 else ["means"])
        if variant in (1, 2, 4, 5):
            kw["jitter"] = cs.inp(_jitter(rng, n))
        if variant == 2:
            v = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n, 1))
            nz = np.array([0.6, -0.3, 1e-7, 0.0, 2e-5, 0.9, 5e-3, -1.0, 0.05], np.float32)[:n]
            nrm = np.concatenate([rng.uniform(-0.5, 0.5, size=(n, 2)).astype(np.float32), nz[:, None]], axis=-1)
            kw.update(viewdirs=cs.inp(v), normals=cs.inp(nrm))
        if P > 1:                                                        # P == 1: level 0 (no previous level)
            # posts of even width +- 30 %: a wide bin of little weight is a steep stretch of the inverse CDF, and the level
            # family's floor has to stay below 2.5e-5 (4 x floor <= 1e-4)
            ps = ((np.arange(P + 1) + rng.uniform(-0.3, 0.3, size=(n, P + 1))) / P).astype(np.float32)
            ps[:, 0], ps[:, -1] = 0.0, 1.0
            pt = (near[:, None] + ps * (far - near)[:, None]).astype(np.float32)
            kw.update(prev_sdist=cs.inp(ps), prev_tdist=cs.inp(pt), prev_density=cs.inp(_density(rng, n, P, _kinds(n, j), pt, d)))
            if variant in (0, 2, 5):
                outs.append("prev_weights")
        name = f"level/v{variant}/P{P}S{S}n{n}"
        li = cs.launch("level", name, "level", ints, flts, outs=outs, **kw)
        if variant == 3:                                                 # the same batch on the bounds of k_ladder_bounds
            lb = cs.launch("ladder", name + "/bounds", "ladder", flts={"near": 0.05, "far": 6.0, "far_clamp": 2.0, "p": -1.5,
                                                                       "premult": 2.0}, outs=("out",))
            tw = cs.launch("level", name + "/s_bounds", "level", ints, flts, outs=outs,
                           s_bounds=cs.launches[lb]["bufs"]["out"], **kw)
            cs.launches[tw]["twin"] = li
    # posts out of order in front of the inversion check that replaces k_sample_level's rank sort.  "inv": a previous level
    # without density (equal logits: one u per bin for P == S) whose sdist has only its last post lowered below post P - 2
    # (ray % 3 == 0: the pair (S - 1, S) alone is inverted), only its first post raised above post 2 (ray % 3 == 1: the pair
    # (0, 1) alone), or descends throughout (ray % 3 == 2).  "desc": a descending sdist on ordinary densities.
    for P, S, n in ((64, 64, 9), (33, 33, 5), (17, 17, 3), (3, 3, 4)):
        for jit in (False, True):
            o, d = _rays(rng, n)
            near, far = rng.uniform(0.02, 0.3, size=n).astype(np.float32), rng.uniform(1.0, 1.9, size=n).astype(np.float32)
            ps = ((np.arange(P + 1) + rng.uniform(-0.3, 0.3, size=(n, P + 1))) / P).astype(np.float32)
            for r in range(n):
                if r % 3 == 0:
                    ps[r, P] = ps[r, P - 2] - np.float32(0.25 / P)
                elif r % 3 == 1:
                    ps[r, 0] = ps[r, 2] + np.float32(0.25 / P)
                else:
                    ps[r] = ps[r, ::-1]
            pt = (near[:, None] + np.linspace(0, 1, P + 1)[None] * (far - near)[:, None]).astype(np.float32)
            kw = {"jitter": cs.inp(np.full(n, 0.5, np.float32))} if jit else {}
            li = cs.launch("level", f"level/inv/P{P}S{S}n{n}/j{int(jit)}", "level",
                           {"n": n, "P": P, "S": S, "secondary": 0, "use_raydist": 0}, dict(lad, anneal=0.4, padding=1e-5),
                           outs=("sdist", "tdist", "means"), origins=cs.inp(o), directions=cs.inp(d), near=cs.inp(near), far=cs.inp(far),
                           prev_sdist=cs.inp(ps), prev_tdist=cs.inp(pt), prev_density=cs.inp(np.zeros((n, P), np.float32)), **kw)
            cs.launches[li]["inversions"] = "single"
    for P, S, n in ((64, 64, 4), (33, 17, 5), (17, 33, 3), (63, 64, 1)):
        for jit in (False, True):
            o, d = _rays(rng, n)
            near, far = rng.uniform(0.02, 0.3, size=n).astype(np.float32), rng.uniform(1.0, 1.9, size=n).astype(np.float32)
            ps = ((np.arange(P + 1) + rng.uniform(-0.3, 0.3, size=(n, P + 1))) / P).astype(np.float32)
            ps[:, 0], ps[:, -1] = 0.0, 1.0
            ps = np.ascontiguousarray(ps[:, ::-1])
            pt = (near[:, None] + np.linspace(0, 1, P + 1)[None] * (far - near)[:, None]).astype(np.float32)
            kw = {"jitter": cs.inp(_jitter(rng, n))} if jit else {}
            li = cs.launch("level", f"level/desc/P{P}S{S}n{n}/j{int(jit)}", "level",
                           {"n": n, "P": P, "S": S, "secondary": 1, "use_raydist": 1}, dict(lad, anneal=0.4, padding=1e-5),
                           outs=("sdist", "tdist", "means", "prev_weights"), origins=cs.inp(o), directions=cs.inp(d), near=cs.inp(near),
                           far=cs.inp(far), prev_sdist=cs.inp(ps), prev_tdist=cs.inp(pt),
                           prev_density=cs.inp(_density(rng, n, P, _kinds(n, P), pt, d)), **kw)
            cs.launches[li]["inversions"] = "all"
    # a u on a CDF post in k_sample_level: anneal 1e30 without padding makes the softmax one-hot in every precision (the other
    # bins' exp underflows to exactly 0), so the CDF is 0 up to the one bin with density (bin 2 + ray) and 1 after it, and
    # u = 0 (jitter 0) ties with the leading posts: searchsorted's side decides between post 0 and that bin
    for P, S, n in ((64, 32, 4), (17, 33, 3)):
        o, d = _rays(rng, n)
        near, far = rng.uniform(0.02, 0.3, size=n).astype(np.float32), rng.uniform(1.0, 1.9, size=n).astype(np.float32)
        ps = _sorted_posts(rng, n, P)
        pt = (near[:, None] + ps * (far - near)[:, None]).astype(np.float32)
        dens = np.zeros((n, P), np.float32)
        dens[np.arange(n), 2 + np.arange(n)] = 50.0
        cs.launch("level", f"level/onehot/P{P}S{S}n{n}", "level", {"n": n, "P": P, "S": S, "secondary": 0, "use_raydist": 0},
                  dict(lad, anneal=1e30, padding=0.0), outs=("sdist", "tdist", "means", "prev_weights"), origins=cs.inp(o),
                  directions=cs.inp(d), near=cs.inp(near), far=cs.inp(far), prev_sdist=cs.inp(ps), prev_tdist=cs.inp(pt),
                  prev_density=cs.inp(dens), jitter=cs.inp(_jitter(rng, n)))
    # --- k_resample, k_composite, k_composite_pick
    for j, S in enumerate(SAMPLES):
        n = RAYS[(j + 1) % 5]
        tag = f"S{S}n{n}"
        o, d = _rays(rng, n)
        kinds = _kinds(n, j)
        dens, td = _density(rng, n, S, kinds), _tdist(rng, n, S, kinds)
        means = rng.uniform(-1, 1, size=(3, n * S)).astype(np.float32)
        nrm = rng.normal(size=(3, n * S)).astype(np.float32)
        ngr = rng.normal(size=(3, n * S)).astype(np.float32)
        lights = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
        shade = rng.uniform(0, 1, size=(SHADE_CH, n * S)).astype(np.float32)
        B = {"directions": cs.inp(d), "origins": cs.inp(o), "tdist": cs.inp(td), "density": cs.inp(dens), "means": cs.inp(means),
             "normals_pred": cs.inp(nrm), "shade": cs.inp(shade)}
        ints = {"n": n, "S": S, "Sf": S}
        flts = dict(pct, bg=0.75)
        every = ["weights"] + ["out_" + k for k in OUT_NAMES[:19]]
        extras = ("means", "ray_dists", "light_dists", "normals_pred", "normals", "indirect_occ")
        group = []
        group.append(cs.launch("composite", f"comp/all/{tag}", "composite", ints, flts, outs=every, lights=cs.inp(lights),
                               normals_grad=cs.inp(ngr), **B))
        group.append(cs.launch("composite", f"comp/rgbacc/{tag}", "composite", ints, flts, outs=("out_rgb", "out_acc"), **B))
        group.append(cs.launch("composite", f"comp/one/{tag}", "composite", ints, flts,
                               outs=("out_rgb", "out_acc", "out_" + extras[j % 6]), lights=cs.inp(lights), normals_grad=cs.inp(ngr), **B))
        group.append(cs.launch("composite", f"comp/geom/{tag}", "composite", ints, flts,
                               outs=("out_rgb", "out_acc", "out_distance_mean", "out_distance_median") + tuple("out_" + k for k in extras),
                               lights=cs.inp(lights), normals_grad=cs.inp(ngr), **B))
        # every pointer allocated, but no lights and no gradient normals: those three outputs keep their canaries
        group.append(cs.launch("composite", f"comp/nolights/{tag}", "composite", ints, flts, outs=every, **B))
        for li in group[1:]:
            cs.launches[li]["twin"] = group[0]
        # k_resample: the pick given (out-of-range values are clamped), every optional output
        R = {"tdist": B["tdist"], "density": B["density"], "directions": B["directions"]}
        raw = np.array([-5, S, S + 100, 2 ** 31 - 1, 0, S - 1, S // 2, -(2 ** 31), 1], np.int32)[np.arange(n) + (j % 4)
                                                                                                 if n <= 5 else np.arange(n)]
        rs = cs.launch("resample", f"resample/inds/{tag}", "resample", {"n": n, "S": S}, inds_in=cs.inp(raw), means=B["means"],
                       normals=B["normals_pred"], outs=("inds_out", "filt_weight", "weights", "acc_out", "src_out", "pts_out", "nrm_out"), **R)
        cs.launch("resample", f"resample/inds/bare/{tag}", "resample", {"n": n, "S": S}, inds_in=cs.inp(raw),
                  outs=("inds_out", "filt_weight", "weights"), **R)
        ro = cs.launches[rs]["bufs"]
        sel = np.clip(raw.astype(np.int64), 0, S - 1).astype(np.int32)
        shade1 = rng.uniform(0, 1, size=(SHADE_CH, n)).astype(np.float32)
        B1 = dict(B, shade=cs.inp(shade1), inds=cs.inp(sel), filt_weight=ro["filt_weight"])
        ints1 = {"n": n, "S": S, "Sf": 1}
        cs.launch("composite", f"comp1/all/{tag}", "composite", ints1, flts, outs=every, lights=cs.inp(lights),
                  normals_grad=cs.inp(ngr), **B1)
        c1 = cs.launch("composite", f"comp1/rgbacc/{tag}", "composite", ints1, flts, outs=("out_rgb", "out_acc"), **B1)
        cs.launches[c1]["twin"] = c1 - 1                                  # comp1/all: the batched butterfly
        pk = cs.launch("pick", f"pick/{tag}", "pick", {"n": n}, {"bg": 0.75}, outs=("out_rgb", "out_acc"),
                       shade_rgb=cs.inp(shade1[:3]), filt_weight=ro["filt_weight"], acc=ro["acc_out"])
        cs.launches[pk]["twin"] = c1
        if S in (2, 64):
            for keep in ("out_rgb", "out_acc"):
                cs.launch("pick", f"pick/{keep}/{tag}", "pick", {"n": n}, {"bg": 0.75}, outs=(keep,), shade_rgb=cs.inp(shade1[:3]),
                          filt_weight=ro["filt_weight"], acc=ro["acc_out"])
        # the Gumbel pick: the winner leads the runner-up by >= 2e-3 in fp64 on well-conditioned weights
        kinds = _kinds(n, j, moderate=True)
        dens, td = _density(rng, n, S, kinds), _tdist(rng, n, S, kinds, unit=True)
        unit = np.zeros((n, 3), np.float32)
        unit[np.arange(n), np.arange(n) % 3] = 1.0
        w64 = alpha_weights(np.float64, dens, td, unit)[0]
        lg = np.log(np.clip(w64, TINY, FMAX))
        win = rng.integers(0, S, size=n)
        win[0], win[-1] = S - 1, 0
        lead = rng.uniform(0.01, 3.0, size=(n, S))
        lead[np.arange(n), (win + 1 + rng.integers(0, S - 1, size=n)) % S] = 2e-3      # the runner-up, 2e-3 behind
        gum = (lg[np.arange(n), win][:, None] + 1.0) - lg - lead
        gum[np.arange(n), win] = 1.0
        G = {"tdist": cs.inp(td), "density": cs.inp(dens), "directions": cs.inp(unit), "gumbel": cs.inp(gum.astype(np.float32))}
        li = cs.launch("resample", f"resample/gumbel/{tag}", "resample", {"n": n, "S": S}, means=B["means"], normals=B["normals_pred"],
                       outs=("inds_out", "filt_weight", "weights", "acc_out", "src_out", "pts_out", "nrm_out"), **G)
        cs.launches[li]["winner"] = win
        li = cs.launch("resample", f"resample/gumbel/bare/{tag}", "resample", {"n": n, "S": S},
                       outs=("inds_out", "filt_weight", "weights"), **G)
        cs.launches[li]["winner"] = win
        # exact ties on a ray without density (every logit is log(tiny), the same bits)
        a, b2 = ((17, 49) if S >= 50 else (17, 33) if S >= 34 else (1, 17) if S >= 18 else (max(S - 2, 0) - (S > 2), S - 1))
        gum = np.zeros((n, S), np.float32)
        for r in range(n):
            if r % 2 == 1 or n == 1:
                gum[r, a] = gum[r, b2] = 1.0                               # two equal maxima: the lower index wins
            else:
                gum[r] = 0.25 * (r + 1)                                    # equal noise everywhere: index 0 wins
        win = np.array([a if (r % 2 == 1 or n == 1) else 0 for r in range(n)])
        li = cs.launch("resample", f"resample/ties/{tag}", "resample", {"n": n, "S": S},
                       outs=("inds_out", "filt_weight", "weights", "acc_out", "src_out"), tdist=cs.inp(td),
                       density=cs.inp(np.zeros((n, S), np.float32)), directions=cs.inp(unit), gumbel=cs.inp(gum))
        cs.launches[li]["winner"] = win
    return cs
