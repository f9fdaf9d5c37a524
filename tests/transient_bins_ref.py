"""The time-resolved cache's per-bin kernels (k_shadow_rays, k_transient_bins of csrc/rc_transient.hip, k_transient_slice of
csrc/rc_transient_slice.hip, k_transient_bins_bwd of csrc/rc_transient_bwd.hip) on their own contracts, RcShadowRayArgs /
RcTransBinsArgs / RcTransSliceArgs / RcTransBinsBwdArgs (csrc/rc_internal.h): the cases, one reference of every kernel in
fp64 (the contract) and in float32 (the same operations in float32, the per-bin heads' softplus in the kernels' exp2 / log2
form), the tolerances, mutated references and the kernel table of the driver tests/transient_check.hip.  Buffers, guards,
canaries, the case file and the result file are tests/sample_ref.py's (Cases, write_case_file, read_results) on this
module's kernel table.

The contracts are restated from the reference's functions, not from the kernels:
  zero_invalid_bins        render_utils.py:1699-1767: a bin b of a sample is zeroed when (b + threshold) * exposure <
                           light_dist, when b * exposure + cam_dist > max_dists, and (light_zero) when light_dist < light_near
  the two heads            nerf.py:1712-1758: softplus(x_irr W_irr + b + irradiance_bias) * indirect_scale and tint_ibrdf *
                           max(softplus(x_slf W_slf + b + rgb_bias), 0) * indirect_scale, zeroed, then clipped to [0, rgb_max]
  shift_map_coordinates    render.py:480-507: out[y] = in(y - d), d = (ray_dist + shift) / exposure, linear, zero outside
  shift_direct             render.py:436-477: w (direct) at max(floor(d), 0) and ceil(d) with weights 1 - (d - low) and d -
                           low, d = (light_dist + ray_dist) / exposure + shift / exposure, on the flattened [rays * bins] axis
  temporal filter          render.py:406-417: scipy.signal.convolve(direct, taps, mode="same")
  shadow rays              nerf.py:1233-1288
A whole `forward` is a few lines of gathers, scatters and sums on [n, 32, 700, 3] arrays: no tiles, no windows, no lanes.
Where the kernels' contract is narrower than render.py's flattened scatter it is the kernels' that is stated: a direct target
below bin 0 is dropped (render.py's index arithmetic would put it into the previous ray of the batch, or wrap to the end of
the batch for ray 0), and a target at or beyond bin 1400 is dropped (render.py: two rays further on).  Neither happens at
transient_shift = 0 with distances inside the histogram.

Decisions that the reference takes in float32 are taken in float32 in BOTH forms (`decisions`): the two travel-time
comparisons, light_dist < light_near, floor of the shifted coordinate y - d, floor / ceil of the direct coordinate.  The
values (weights of the shift, of the scatter, everything else) are fp64 in the fp64 form.  The cases keep every such
decision 16 float32 ulp away from flipping, except exact ties placed where float32 and fp64 agree exactly (dyadic
exposure and distances); `near_ties` measures it and tests/test_transient_bins_ref.py asserts it for every case.  No
element is excluded from any comparison.

Tolerances (u = 2^-24; every bound is on |device - fp64 reference|):
  head pre-activation   z = x W + b, K products and the bias in any order: c(K) (sum |x w| + |b|) from the fp64 reference's
                        own sum of absolute products, c(K) = 2 (K + 2) u for the split-form build (gemm_ref / matstage_ref's
                        constant) and (K + 2) u for the fp32 build, k_transient_slice (fp32 FMA chains in both builds) and
                        k_transient_bins_bwd (fp32 MFMA in both builds)
  softplus_bins         max(x, 0) + log2(1 + exp2(-|x| log2 e)) ln 2 on the hardware transcendentals, without the series for
                        small exp: its error is MEASURED on the CPU, max |float32 restatement in that form - fp64| / (1 +
                        fp64) over the pre-activations of all cases (Cases.softplus_allowance), and the device gets 4 x that,
                        as matstage_ref does for its sampler floors; slope <= 1 carries the pre-activation's bound through
  diff, spec            x indirect_scale (2 u), x tint_ibrdf (u); the clip is 1-Lipschitz; a bin outside the sample's window
                        is an exact zero with tolerance 0
  val = w (diff + spec) |w| (t_diff + t_spec) + 2 u |val|
  shifted sum           out[y] = sum_s a_s (1 - f_s) + b_s f_s: f = y - d - floor carries t_f = u (2 |d| + |y - d| + 2) (the
                        sum, the quotient, the difference, 1 - f); per term t_a (1 - f) + t_b f + t_f (|a| + |b|) + 2 u |term|,
                        and (64 + 2) u sum |terms| for the 64 additions in any order
  direct scatter        term = w (dd + ds) weight: |w (dd + ds)| t_d + 4 u |term|, t_d = u (3 |l + r| / e + 2 |shift / e| + |d|);
                        m terms landing in one bin in any order: (m + 2) u sum |terms|
  temporal filter       sum |tap| t_in + (n_taps + 2) u sum |tap in|
  sums over bins        (700 + 2) u sum |.| + the entries' bounds; sums over the 32 samples (32 + 2) u sum |.|, + 2 u per product
  slices                w v[ceil t] + (1 - w) v[floor t]: the histograms' bounds with the same weights + 3 u |.|
  backward              sigmoid' <= 1 / 4: t_sig = t_z / 4 + 4 u; gsum = wa G[y0] + wb G[y0 + 1]: t_f (|G0| + |G1|) + 3 u |.|;
                        products carry their factors' bounds; sums as above.  The clamp's derivative is a step: the backward
                        cases keep every pre-clamp value further from rgb_max than its own bound (asserted on the CPU)
  shadow rays           origins, normals, lights, near: the float32 restatement's bits (IEEE operations, no contraction);
                        dirs 8 u; far 4 u (dist + |far|), exactly shadow_near / shadow_far where the fp64 value clears the
                        clamp by more than that
Exact-zero claims are a tolerance of 0: equality is asserted.  No case and no element is excused."""
import sys

import numpy as np
import torch

import sample_ref as R
from sample_ref import CANARY, CSRC, GUARD, ROOT, U, canary, is_canary  # noqa: F401

MAGIC_CASES, MAGIC_RESULTS = 0x54524E5343415345, 0x54524E5352534C54
N_INT, N_FLT, N_BUF = R.N_INT, R.N_FLT, R.N_BUF
BINS, HIST, LD_SLF, TSLICE_MAX, S = 700, 2100, 2104, 8, 32
TS_DD, TS_DS, TS_ALBEDO, TS_TIB, TS_ROUGH, TS_NDOTL, TS_IRRAD, TS_OCC, TS_LDIST, TS_RDIST, TS_CAMDIST, TS_COUNT = \
    0, 3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19
KERNELS = ("shadow", "bins", "slice", "bins_bwd")
_IN = ("w_slf", "b_slf", "w_irr", "b_irr", "slf_feat", "irr_feat", "tshade", "weights")
_FLT = ("exposure", "shift", "max_dists", "irradiance_bias", "slf_rgb_bias", "indirect_scale", "rgb_max", "light_near")
HIST_OUT = ("out_rgb", "out_direct", "out_indirect", "out_ti_diffuse", "out_ti_specular")
RAY_OUT = ("out_direct_rgb", "out_indirect_rgb", "out_integrated_rgb", "out_diffuse_rgb", "out_specular_rgb", "out_albedo_rgb",
           "out_occ", "out_indirect_occ", "out_irradiance_rgb", "out_light_radiance_rgb", "out_n_dot_l_rgb",
           "out_direct_diffuse_rgb", "out_direct_specular_rgb", "out_indirect_diffuse_rgb", "out_indirect_specular_rgb",
           "out_direct_rgb_viz")
SLICE_OUT = ("out_rgb", "out_direct", "out_indirect")
BWD_OUT = ("dz_irr", "dz_slf", "x_irr", "x_slf", "d_tib", "d_direct", "d_weights")
_SHADOW_OUT = ("origins", "dirs", "near", "far", "out_normals", "out_lights")
# kernel -> (ints, floats, buffers, the buffers it writes); the driver reads the slots in this order
SLOTS = {
    "shadow": (("n", "samples_per_ray"), ("normal_eps", "shadow_near", "shadow_far", "light_near"),
               ("means", "normals", "lights") + _SHADOW_OUT, _SHADOW_OUT),
    "bins": (("n_rays", "bin_zero_threshold_light", "light_zero", "n_taps"), _FLT, _IN + ("taps",) + HIST_OUT + RAY_OUT,
             HIST_OUT + RAY_OUT),
    "slice": (("n_rays", "bin_zero_threshold_light", "light_zero", "n_taps", "count"), _FLT, _IN + ("taps", "t") + SLICE_OUT,
              SLICE_OUT),
    "bins_bwd": (("n_rays", "r0", "C", "bin_zero_threshold_light", "light_zero"), _FLT, _IN + ("G", "Gt") + BWD_OUT, BWD_OUT),
}
INT_SLOTS = ()
FAMILIES = ("window", "compare", "shift", "direct", "taps", "flags", "rays", "pointers")
MUTATIONS = {                                 # mutated reference -> the family meant to catch it
    "win_lo_off": "window", "win_hi_off": "window", "thr_ignored": "compare", "light_zero_ignored": "flags",
    "trunc_not_floor": "shift", "at_b_swapped": "shift", "seam_carry_dropped": "window", "tile_behind_not_run": "window",
    "spill_dropped": "direct", "taps_reversed": "taps", "filter_centre_off": "taps", "clamp_omitted": "flags",
    "zero_weight_contributes": "flags",
}
CORNELL = {"exposure": 0.01, "shift": 0.0, "irradiance_bias": -2.0, "slf_rgb_bias": -2.0, "indirect_scale": 0.05,
           "rgb_max": 100.0, "light_near": 0.7, "thr": 100, "light_zero": 1, "max_bin": 699}
K_SLF, K_IRR = 129, 65                        # products of a head pre-activation, the bias step included


def c_split(K):
    return 2.0 * (K + 2) * U


def c_f32(K):
    return (K + 2) * U


def out_shape(kernel, slot, i):
    n = i.get("n_rays", i.get("n", 0))
    if kernel == "shadow":
        return (n,) if slot in ("near", "far") else (n, 3)
    if kernel == "bins":
        return (n, BINS, 3) if slot in HIST_OUT else (n, 3)
    if kernel == "slice":
        return (n, i["count"], 3)
    C = i["C"]
    return {"dz_irr": (C * S, HIST), "dz_slf": (C * S, LD_SLF), "x_irr": (C * S, 64), "x_slf": (C * S, 128),
            "d_tib": (n * S, 3), "d_direct": (n * S, 3), "d_weights": (n * S,)}[slot]


def acc_feat(t, r, h):
    """Feature that accumulator register r of tile t holds on half-wave h (v_mfma_f32_32x32x2_f32 D layout)."""
    return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h


def layout_feat(x):
    """Plain activations [n, 32 samples, 32 T features] -> the [n][16 T steps][64 lanes] layout k_transient_shader stores
    (slf_feat: T = 4, irr_feat: T = 2): step 16 t + r, lane 32 h + j holds feature acc_feat(t, r, h) of sample j -- the
    steps_acc order of rc_pack_host.h."""
    n, s, F = x.shape
    assert s == S and F % 32 == 0
    out = np.empty((n, F // 2, 64), np.float32)
    for t in range(F // 32):
        for r in range(16):
            for h in range(2):
                out[:, 16 * t + r, 32 * h:32 * h + 32] = x[:, :, acc_feat(t, r, h)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of a bins / slice / bins_bwd launch


class WSet:
    """The two head layers, plain: output_rgba_layer [128][2101] + bias, transient_indirect_layer [64][2100] + bias."""

    def __init__(self, rng, scale):
        self.w_slf = (rng.normal(size=(128, HIST + 1)) * scale).astype(np.float32)
        self.b_slf = (rng.normal(size=HIST + 1) * scale).astype(np.float32)
        self.w_irr = (rng.normal(size=(64, HIST)) * scale * 1.4).astype(np.float32)
        self.b_irr = (rng.normal(size=HIST) * scale).astype(np.float32)
        self.bufs = None


class Scene:
    """One set of inputs of the per-bin kernels.  x_slf [n, 32, 128], x_irr [n, 32, 64] plain activations, tshade
    [TS_COUNT, n * 32], weights [n, 32], P the settings (CORNELL's keys + max_dists), taps float32 [n_taps] or None."""

    def __init__(self, wset, x_slf, x_irr, tshade, weights, P, taps=None):
        self.wset, self.x_slf, self.x_irr, self.tshade, self.weights = wset, x_slf, x_irr, tshade, weights
        self.n = weights.shape[0]
        self.P = dict(P)
        self.taps = None if taps is None or len(taps) == 0 else np.asarray(taps, np.float32)
        self.bufs, self._fw = None, {}

    def ts(self, ch, k=1):
        v = self.tshade[ch:ch + k].reshape(k, self.n, S)
        return v[0] if k == 1 else np.moveaxis(v, 0, -1)

    def flts(self):
        return {k: self.P[k] for k in _FLT}


def f32(x):
    return np.asarray(x, np.float32)


def decisions(sc, mut=None):
    """Everything discontinuous, in float32 as the reference computes it.  keep [n, 32, 700]; i0 [n, 32, 700] = floor(y -
    d_ind); low, high [n, 32] (int64) of the direct scatter; d_ind, d_dir [n, 32] float32."""
    P = sc.P
    e, sh = np.float32(P["exposure"]), np.float32(P["shift"])
    ld, rd, cam = sc.ts(TS_LDIST), sc.ts(TS_RDIST), sc.ts(TS_CAMDIST)
    b = np.arange(BINS)
    thr = 0 if mut == "thr_ignored" else P["thr"]
    bl = (b + thr + (1 if mut == "win_lo_off" else 0)).astype(np.float32)
    bh = (b - (1 if mut == "win_hi_off" else 0)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        close = (bl * e)[None, None] < ld[..., None]
        far = (bh * e)[None, None] + cam[..., None] > np.float32(P["max_dists"])
        kill = (ld < np.float32(P["light_near"])) if (P["light_zero"] and mut != "light_zero_ignored") else np.zeros_like(ld, bool)
        keep = ~(close | far | kill[..., None])
        d_ind = (rd + sh) / e
        y = b.astype(np.float32)[None, None] - d_ind[..., None]
        i0 = np.clip(np.floor(y), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
        d_dir = (ld + rd) / e + sh / e
        low = np.clip(np.maximum(np.floor(d_dir), np.float32(0.0)), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
        high = np.clip(np.ceil(d_dir), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    return {"keep": keep, "i0": i0, "y32": y, "low": low, "high": high, "d_ind": d_ind, "d_dir": d_dir}


def windows(keep):
    """(lo, hi) [n, 32] of the kept bins (lo = 700, hi = -1 when none); the kept bins of a sample are contiguous."""
    any_ = keep.any(-1)
    lo = np.where(any_, keep.argmax(-1), BINS)
    hi = np.where(any_, BINS - 1 - keep[..., ::-1].argmax(-1), -1)
    assert np.array_equal(keep.sum(-1), np.where(any_, hi - lo + 1, 0))
    return lo, hi


def _ulp32(x):
    return np.spacing(np.abs(f32(x))).astype(np.float64)


def near_ties(sc, margin=16.0):
    """Number of float32 decisions of `decisions` within `margin` float32 ulp of flipping that are no exact tie on which
    float32 and fp64 agree.  Products and sums of a few float32 values are exact in fp64."""
    P = sc.P
    e, sh = float(np.float32(P["exposure"])), float(np.float32(P["shift"]))
    ld, rd, cam = (sc.ts(c).astype(np.float64) for c in (TS_LDIST, TS_RDIST, TS_CAMDIST))
    b = np.arange(BINS, dtype=np.float64)
    bad = 0
    with np.errstate(over="ignore", invalid="ignore"):
        def count(a64, a32, rhs):                  # a < rhs or a > rhs, a computed in fp64 and in float32
            scale = margin * np.maximum(_ulp32(a64), _ulp32(rhs))
            close_ = np.abs(a64 - rhs) <= scale
            exact = (a64 == rhs) & (a32.astype(np.float64) == a64)
            return int((close_ & ~exact).sum())
        e32 = np.float32(e)
        a64 = ((b + P["thr"]) * e)[None, None] + 0.0 * ld[..., None]
        a32 = (f32(b + P["thr"]) * e32)[None, None] + np.float32(0.0) * f32(ld)[..., None]
        bad += count(a64, a32, ld[..., None] + 0.0 * a64)
        c64 = (b * e)[None, None] + cam[..., None]
        c32 = (f32(b) * e32)[None, None] + f32(cam)[..., None]
        bad += count(c64, c32, np.full_like(c64, float(np.float32(P["max_dists"]))))
        if P["light_zero"]:
            bad += count(ld, f32(ld), np.full_like(ld, float(np.float32(P["light_near"]))))
        # floor(y - d) over y = 0 .. 699 and floor / ceil of the direct coordinate: distance of the coordinate from an integer
        d64 = (rd + sh) / e
        d32 = (f32(rd) + np.float32(sh)) / e32
        far_out = np.abs(d64) > 4.0 * BINS            # every bin maps outside the histogram either way
        frac = np.abs(d64 - np.round(d64))
        exact = (d64 == np.round(d64)) & (d32.astype(np.float64) == d64)
        bad += int(((frac <= margin * _ulp32(np.abs(d64) + BINS)) & ~exact & ~far_out).sum())
        q64 = (ld + rd) / e + sh / e
        q32 = (f32(ld) + f32(rd)) / e32 + np.float32(sh) / e32
        frac = np.abs(q64 - np.round(q64))
        exact = (q64 == np.round(q64)) & (q32.astype(np.float64) == q64)
        far_out = (np.abs(q64) > 4.0 * BINS)
        bad += int(((frac <= margin * _ulp32(q64)) & ~exact & ~far_out).sum())
    return bad


def T(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def softplus(x, hw=False):
    if hw:
        assert x.dtype == torch.float32
        e = torch.exp2(-x.abs() * float(np.float32(1.44269504088896341)))
        return torch.clamp(x, min=0.0) + torch.log2(1.0 + e) * float(np.float32(0.693147180559945309))
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))


def _take(v, idx):
    """v [n, 32, 700, 3] at bins idx [n, 32, 700], zero outside [0, 700)."""
    ok = (idx >= 0) & (idx < BINS)
    g = torch.gather(v, 2, torch.clamp(idx, 0, BINS - 1)[..., None].expand(-1, -1, -1, 3))
    return torch.where(ok[..., None], g, torch.zeros_like(g))


def conv_same(x, taps, mut=None):
    """scipy.signal.convolve(x, taps[None, :, None], mode="same") along the bin axis of [n, 700, 3], as explicit shifts:
    out[b] = sum_k taps[k] x[b + (K - 1) // 2 - k]."""
    if taps is None:
        return x
    K = len(taps)
    half = (K - 1) // 2 + (1 if mut == "filter_centre_off" else 0)
    tp = taps[::-1] if mut == "taps_reversed" else taps
    out = torch.zeros_like(x)
    for k in range(K):
        sft = k - half                               # out[b] += tp[k] x[b - sft]
        lo, hi = max(0, sft), min(BINS, BINS + sft)
        if lo < hi:
            out[:, lo:hi] = out[:, lo:hi] + float(tp[k]) * x[:, lo - sft:hi - sft]
    return out


def forward(sc, dt=torch.float64, mut=None, hw=False, leaves=None):
    """Everything k_transient_bins writes, from the contracts in the module docstring.  -> dict of tensors; the keys starting
    with "_" are intermediates the tolerances use.  `leaves`: a dict that receives the tensors the backward differentiates
    with respect to (z_irr, z_slf, tib, w, direct as leaves of the graph)."""
    n, P = sc.n, sc.P
    D = decisions(sc, mut)
    sca = lambda k: float(np.float32(P[k]))
    e, sh = sca("exposure"), sca("shift")
    W = sc.wset
    z_slf = T(sc.x_slf, dt).reshape(-1, 128) @ T(W.w_slf[:, :HIST], dt) + T(W.b_slf[:HIST], dt)
    z_irr = T(sc.x_irr, dt).reshape(-1, 64) @ T(W.w_irr, dt) + T(W.b_irr, dt)
    z_slf, z_irr = z_slf.reshape(n, S, BINS, 3), z_irr.reshape(n, S, BINS, 3)
    w, tib = T(sc.weights, dt), T(sc.ts(TS_TIB, 3), dt)
    dd, ds = T(sc.ts(TS_DD, 3), dt), T(sc.ts(TS_DS, 3), dt)
    direct = dd + ds
    if leaves is not None:
        z_slf, z_irr, w, tib, direct = (v.detach().requires_grad_(True) for v in (z_slf, z_irr, w, tib, direct))
        leaves.update(z_slf=z_slf, z_irr=z_irr, w=w, tib=tib, direct=direct)
    sp_i, sp_s = softplus(z_irr + sca("irradiance_bias"), hw), softplus(z_slf + sca("slf_rgb_bias"), hw)
    diff_pre = sp_i * sca("indirect_scale")
    spec_pre = (tib[:, :, None, :] * torch.clamp(sp_s, min=0.0)) * sca("indirect_scale")
    hi = float("inf") if mut == "clamp_omitted" else sca("rgb_max")
    keep = torch.from_numpy(D["keep"])[..., None]
    zero = torch.zeros_like(diff_pre)
    diff = torch.where(keep, torch.clamp(diff_pre, 0.0, hi), zero)
    spec = torch.where(keep, torch.clamp(spec_pre, 0.0, hi), zero)
    w_ind = torch.where(w == 0, torch.full_like(w, 0.5), w) if mut == "zero_weight_contributes" else w
    val = w_ind[:, :, None, None] * (diff + spec)
    # shift_map_coordinates: out[y] = val(y - d), linear, zero outside
    d_ind = (T(sc.ts(TS_RDIST), dt) + sh) / e
    bins = torch.arange(BINS, dtype=dt)
    i0 = torch.from_numpy(D["i0"])
    fw = (bins[None, None] - d_ind[..., None]) - i0.to(dt)
    if mut in ("trunc_not_floor", "at_b_swapped", "seam_carry_dropped", "tile_behind_not_run"):
        indirect = _shift_scatter_mutated(sc, D, val.detach().to(torch.float64).numpy(), mut)
        indirect = T(indirect, dt)
        a = b = None
    else:
        a, b = _take(val, i0), _take(val, i0 + 1)
        indirect = (a * (1.0 - fw)[..., None] + b * fw[..., None]).sum(1)
    # shift_direct: two scatter-adds on the flattened [n * 700] axis; a bin in [700, 1400) is the next ray's
    d_dir = (T(sc.ts(TS_LDIST), dt) + T(sc.ts(TS_RDIST), dt)) / e + sh / e
    low, high = torch.from_numpy(D["low"]), torch.from_numpy(D["high"])
    w_high = d_dir - low.to(dt)
    w_low = 1.0 - w_high
    vald = w[..., None] * direct
    base = (torch.arange(n) * BINS)[:, None]
    dh = torch.zeros(n * BINS, 3, dtype=dt)
    terms = []
    for idx, wt in ((low, w_low), (high, w_high)):
        ok = (idx >= 0) & (idx < (BINS if mut == "spill_dropped" else 2 * BINS)) & (base + idx < n * BINS)
        term = vald * wt[..., None]
        dh = dh.index_add(0, (base + idx)[ok], term[ok])
        terms.append((idx, ok, term))
    dh = dh.reshape(n, BINS, 3)
    taps = None if sc.taps is None else sc.taps.astype(np.float64 if dt == torch.float64 else np.float32)
    df = conv_same(dh, taps, mut)
    r = {"out_rgb": df + indirect, "out_direct": df, "out_indirect": indirect,
         "out_ti_diffuse": (w[:, :, None, None] * diff).sum(1), "out_ti_specular": (w[:, :, None, None] * spec).sum(1)}
    bs_d, bs_s = diff.sum(2), spec.sum(2)                                  # [n, 32, 3] per-sample sums over the bins
    ws = lambda x: (w[..., None] * x).sum(1)
    one3 = torch.ones(3, dtype=dt)
    r.update(out_direct_rgb=df.sum(1), out_indirect_rgb=indirect.sum(1), out_integrated_rgb=df.sum(1) + indirect.sum(1),
             out_diffuse_rgb=ws(dd + bs_d), out_specular_rgb=ws(ds + bs_s), out_albedo_rgb=ws(T(sc.ts(TS_ALBEDO, 3), dt)),
             out_occ=ws(T(sc.ts(TS_OCC), dt)[..., None] * one3), out_indirect_occ=ws(torch.ones(n, S, 3, dtype=dt)),
             out_irradiance_rgb=ws(T(sc.ts(TS_IRRAD), dt)[..., None] * one3),
             out_light_radiance_rgb=ws(torch.ones(n, S, 3, dtype=dt)),
             out_n_dot_l_rgb=ws(T(sc.ts(TS_NDOTL), dt)[..., None] * one3), out_direct_diffuse_rgb=ws(dd),
             out_direct_specular_rgb=ws(ds), out_indirect_diffuse_rgb=ws(bs_d), out_indirect_specular_rgb=ws(bs_s),
             out_direct_rgb_viz=(dd + ds).sum(1))
    r.update(_D=D, _diff=diff, _spec=spec, _diff_pre=diff_pre, _spec_pre=spec_pre, _sp_i=sp_i, _sp_s=sp_s, _z_irr=z_irr,
             _z_slf=z_slf, _val=val, _fw=fw, _a=a, _b=b, _d_ind=d_ind, _d_dir=d_dir, _dh=dh, _terms=terms, _vald=vald,
             _bs_d=bs_d, _bs_s=bs_s, _w=w, _tib=tib, _dd=dd, _ds=ds, _w_low=w_low, _w_high=w_high, _direct=direct)
    return r


def _shift_scatter_mutated(sc, D, val, mut):
    """The time shift as a scatter from the source bins (numpy, fp64), with one thing wrong.  Unmutated it equals the
    gather of `forward` (tests/test_transient_bins_ref.py asserts that): source bin b of a sample reaches y0 = b + floor(d)
    with weight 1 - g and y0 + 1 with g, g = d - floor(d)."""
    n = sc.n
    d = D["d_ind"].astype(np.float64)
    fd = np.trunc(d) if mut == "trunc_not_floor" else np.floor(d)
    g = d - fd
    wa, wb = 1.0 - g, g
    if mut == "at_b_swapped":
        tie = g == 0
        wa, wb = np.where(tie, 0.0, wa), np.where(tie, 1.0, wb)
    out = np.zeros((n, BINS + 2, 3))                                 # bin 700, 701: the dummy targets
    b = np.arange(BINS)
    ent = 3 * b[:, None] + np.arange(3)[None]                        # entry of (bin, channel)
    fdi = np.clip(fd, -2 * BINS, 2 * BINS).astype(np.int64)
    lo, hi = windows(D["keep"])
    for r in range(n):
        carry_ok = np.ones((BINS, 3), bool)
        if mut == "seam_carry_dropped":                              # the target's lane is one of the first three of a tile
            carry_ok = (ent + 3) % 32 >= 3
        if mut == "tile_behind_not_run":                             # the tile range of the workgroup (4 rays) ends a group early
            g0 = 4 * (r // 4)
            bhi = int(hi[g0:g0 + 4].max())
            f_end = 96 * (((3 * bhi + 2) // 32) // 3 + 1) if bhi >= 0 else 0
            carry_ok = ent + 3 < f_end
        for s in range(S):
            y0 = b + fdi[r, s]
            v = val[r, s]
            for tgt, wt, okm in ((y0, wa[r, s], None), (y0 + 1, wb[r, s], carry_ok)):
                ok = (tgt >= 0) & (tgt < BINS)
                t = np.where(ok, tgt, BINS)
                contrib = v * wt
                if okm is not None:
                    contrib = np.where(okm, contrib, 0.0)
                np.add.at(out[r], t, contrib)
    return out[:, :BINS]


def shift_scatter(sc, val):
    """The unmutated scatter form (see _shift_scatter_mutated), for the CPU test's cross-check of the gather."""
    return _shift_scatter_mutated(sc, decisions(sc), val, None)


def np64(t):
    return t.detach().to(torch.float64).numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def _take_np(v, idx):
    ok = (idx >= 0) & (idx < BINS)
    g = np.take_along_axis(v, np.clip(idx, 0, BINS - 1)[..., None], axis=2)
    return np.where(ok[..., None], g, 0.0)


def head_abs_sums(sc):
    """sum_k |x_k w_k| + |b| of both head pre-activations, fp64, [n, 32, 700, 3] each."""
    W = sc.wset
    a_s = np.abs(sc.x_slf.astype(np.float64)).reshape(-1, 128) @ np.abs(W.w_slf[:, :HIST].astype(np.float64)) + np.abs(W.b_slf[:HIST].astype(np.float64))
    a_i = np.abs(sc.x_irr.astype(np.float64)).reshape(-1, 64) @ np.abs(W.w_irr.astype(np.float64)) + np.abs(W.b_irr.astype(np.float64))
    return a_s.reshape(sc.n, S, BINS, 3), a_i.reshape(sc.n, S, BINS, 3)


def _elem_bounds(sc, r, c, allow):
    """Bounds of diff, spec, val [n, 32, 700, 3] and of the softplus values from the fp64 forward `r`."""
    P = sc.P
    isc = abs(float(np.float32(P["indirect_scale"])))
    a_s, a_i = head_abs_sums(sc)
    keep = r["_D"]["keep"][..., None]
    sp_i, sp_s = np64(r["_sp_i"]), np64(r["_sp_s"])
    tsp_i = c(K_IRR) * a_i + U * np.abs(np64(r["_z_irr"]) + P["irradiance_bias"]) + allow * (1.0 + sp_i)
    tsp_s = c(K_SLF) * a_s + U * np.abs(np64(r["_z_slf"]) + P["slf_rgb_bias"]) + allow * (1.0 + sp_s)
    tib = np.abs(np64(r["_tib"]))[:, :, None, :]
    t_diff = np.where(keep, tsp_i * isc + 2 * U * np.abs(np64(r["_diff_pre"])), 0.0)
    t_spec = np.where(keep, tib * tsp_s * isc + 3 * U * np.abs(np64(r["_spec_pre"])), 0.0)
    w = np.abs(np64(r["_w"]))[:, :, None, None]
    t_val = w * (t_diff + t_spec) + 2 * U * np.abs(np64(r["_val"]))
    return {"t_diff": t_diff, "t_spec": t_spec, "t_val": t_val, "tsp_i": tsp_i, "tsp_s": tsp_s}


def _t_frac(r):
    """Bound of the shift's fractional weight f = (y - d) - floor: [n, 32, 700]."""
    d = np.abs(np64(r["_d_ind"]))[..., None]
    y = np.arange(BINS, dtype=np.float64)[None, None]
    return U * (2.0 * d + np.abs(y - np64(r["_d_ind"])[..., None]) + 2.0)


def _t_dir(sc, r):
    """Bound of the direct coordinate d = (l + r) / e + shift / e: [n, 32]."""
    e, sh = float(np.float32(sc.P["exposure"])), float(np.float32(sc.P["shift"]))
    lr = np.abs(sc.ts(TS_LDIST).astype(np.float64) + sc.ts(TS_RDIST).astype(np.float64)) / e
    return U * (3.0 * lr + 2.0 * abs(sh / e) + np.abs(np64(r["_d_dir"])))


def tol_bins(sc, r, c, allow):
    """Tolerances of every output of k_transient_bins from the fp64 forward `r` (module docstring)."""
    n = sc.n
    E = _elem_bounds(sc, r, c, allow)
    D = r["_D"]
    fw = np64(r["_fw"])
    a, b = np64(r["_a"]), np64(r["_b"])
    ta, tb = _take_np(E["t_val"], D["i0"]), _take_np(E["t_val"], D["i0"] + 1)
    tf = _t_frac(r)
    with np.errstate(over="ignore", invalid="ignore"):
        wa, wb = np.abs(1.0 - fw)[..., None], np.abs(fw)[..., None]
        mag = np.where(a != 0, np.abs(a) * wa, 0.0) + np.where(b != 0, np.abs(b) * wb, 0.0)
        t_term = np.where(ta != 0, ta * wa, 0.0) + np.where(tb != 0, tb * wb, 0.0) + tf[..., None] * (np.abs(a) + np.abs(b)) + 2 * U * mag
    t_ind = t_term.sum(1) + 66 * U * mag.sum(1)
    # direct scatter
    td = _t_dir(sc, r)
    vald = np.abs(np64(r["_vald"]))
    T_, A_, cnt = np.zeros((n * BINS, 3)), np.zeros((n * BINS, 3)), np.zeros((n * BINS, 1))
    base = (np.arange(n) * BINS)[:, None]
    for idx, ok, term in r["_terms"]:
        idx, ok, term = idx.numpy(), ok.numpy(), np.abs(np64(term))
        flat = (base + idx)[ok]
        np.add.at(T_, flat, (vald * td[..., None] + 4 * U * term)[ok])
        np.add.at(A_, flat, term[ok])
        np.add.at(cnt, flat, 1.0)
    t_dh = (T_ + (cnt + 2) * U * A_).reshape(n, BINS, 3)
    dh = np.abs(np64(r["_dh"]))
    if sc.taps is None:
        t_df = t_dh
    else:
        at = np.abs(sc.taps.astype(np.float64))
        t_df = np64(conv_same(T(t_dh, torch.float64), at)) + (len(at) + 2) * U * np64(conv_same(T(dh, torch.float64), at))
    df, ind = np64(r["out_direct"]), np64(r["out_indirect"])
    tol = {"out_direct": t_df, "out_indirect": t_ind, "out_rgb": t_df + t_ind + U * np.abs(df + ind)}
    w = np.abs(np64(r["_w"]))
    w4 = w[:, :, None, None]
    diff, spec = np64(r["_diff"]), np64(r["_spec"])
    tol["out_ti_diffuse"] = (w4 * E["t_diff"]).sum(1) + 36 * U * (w4 * diff).sum(1)
    tol["out_ti_specular"] = (w4 * E["t_spec"]).sum(1) + 36 * U * (w4 * spec).sum(1)
    t_bs_d = E["t_diff"].sum(2) + (BINS + 2) * U * diff.sum(2)
    t_bs_s = E["t_spec"].sum(2) + (BINS + 2) * U * spec.sum(2)
    tol["out_direct_rgb"] = t_df.sum(1) + (BINS + 2) * U * np.abs(df).sum(1)
    tol["out_indirect_rgb"] = t_ind.sum(1) + (BINS + 2) * U * np.abs(ind).sum(1)
    tol["out_integrated_rgb"] = tol["out_direct_rgb"] + tol["out_indirect_rgb"] + U * np.abs(df.sum(1) + ind.sum(1))
    w3 = w[..., None]
    dd, ds = np.abs(np64(r["_dd"])), np.abs(np64(r["_ds"]))
    bs_d, bs_s = np64(r["_bs_d"]), np64(r["_bs_s"])
    wsum = lambda x: 37 * U * (w3 * np.abs(x)).sum(1)
    tol["out_diffuse_rgb"] = (w3 * t_bs_d).sum(1) + wsum(dd + bs_d)
    tol["out_specular_rgb"] = (w3 * t_bs_s).sum(1) + wsum(ds + bs_s)
    tol["out_indirect_diffuse_rgb"] = (w3 * t_bs_d).sum(1) + wsum(bs_d)
    tol["out_indirect_specular_rgb"] = (w3 * t_bs_s).sum(1) + wsum(bs_s)
    one = np.ones((n, S, 3))
    for k, x in (("albedo_rgb", sc.ts(TS_ALBEDO, 3)), ("occ", sc.ts(TS_OCC)[..., None] * one), ("indirect_occ", one),
                 ("irradiance_rgb", sc.ts(TS_IRRAD)[..., None] * one), ("light_radiance_rgb", one),
                 ("n_dot_l_rgb", sc.ts(TS_NDOTL)[..., None] * one), ("direct_diffuse_rgb", dd), ("direct_specular_rgb", ds)):
        tol["out_" + k] = wsum(x.astype(np.float64))
    tol["out_direct_rgb_viz"] = 36 * U * (dd + ds).sum(1)
    return tol


def slice_of(hist, t):
    """engine/trainer.py:1693-1726: w v[ceil t] + (1 - w) v[floor t], w = t - floor t, of [n, 700, 3] -> [n, count, 3]."""
    t = np.asarray(t, np.float32).astype(np.float64)
    lo, hi = np.floor(t).astype(int), np.ceil(t).astype(int)
    w = (t - lo)[None, :, None]
    return w * hist[:, hi] + (1.0 - w) * hist[:, lo]


# ---------------------------------------------------------------------------------------------------------------------------
# backward


def backward(sc, G, Gt, dt=torch.float64):
    """d (sum G . indirect + sum Gt . direct before the filter) / d (z_irr, z_slf, tib, direct, w) by autograd through
    `forward` (k_transient_loss hands the kernel G and Gt = the filter's transpose of G)."""
    leaves = {}
    r = forward(sc, dt, leaves=leaves)
    loss = (T(G, dt).reshape(sc.n, BINS, 3) * r["out_indirect"]).sum() + (T(Gt, dt).reshape(sc.n, BINS, 3) * r["_dh"]).sum()
    loss.backward()
    g = {k: v.grad for k, v in leaves.items()}
    return r, g


def ref_bwd(sc, G, Gt, r0, C, dt=torch.float64):
    r, g = backward(sc, G, Gt, dt)
    n = sc.n
    rows = slice(r0, r0 + C)
    dz_slf = torch.zeros(C * S, LD_SLF, dtype=dt)
    dz_slf[:, :HIST] = g["z_slf"][rows].reshape(C * S, HIST)
    out = {"dz_irr": g["z_irr"][rows].reshape(C * S, HIST), "dz_slf": dz_slf,
           "x_irr": T(sc.x_irr[rows], dt).reshape(C * S, 64), "x_slf": T(sc.x_slf[rows], dt).reshape(C * S, 128)}
    mask = np.zeros(n, bool)
    mask[rows] = True
    for k, key, shape in (("d_tib", "tib", (n * S, 3)), ("d_direct", "direct", (n * S, 3)), ("d_weights", "w", (n * S,))):
        out[k] = g[key].reshape(shape)
        out["_written_" + k] = np.broadcast_to(np.repeat(mask, S).reshape((n * S,) + (1,) * (len(shape) - 1)), shape)
    out["_fwd"] = r
    return out


def tol_bwd(sc, G, Gt, r0, C, ref):
    r = ref["_fwd"]
    n, P = sc.n, sc.P
    c = c_f32
    E = _elem_bounds(sc, r, c, 4 * U)
    isc = abs(float(np.float32(P["indirect_scale"])))
    D = r["_D"]
    keep = D["keep"][..., None]
    G3, Gt3 = np.abs(np.asarray(G, np.float64)).reshape(n, BINS, 3), np.abs(np.asarray(Gt, np.float64)).reshape(n, BINS, 3)
    d = np64(r["_d_ind"])
    fd = np.floor(D["d_ind"]).astype(np.float64)                          # the float32 decision
    g = np.abs(d - fd)[..., None, None]
    y0 = (np.arange(BINS)[None, None] + np.clip(fd, -2 * BINS, 2 * BINS).astype(np.int64)[..., None])
    Gs = np.broadcast_to(G3[:, None], (n, S, BINS, 3))
    g0, g1 = _take_np(Gs, y0), _take_np(Gs, y0 + 1)
    gsum = np.abs(1.0 - g) * g0 + g * g1
    tf = (U * (2.0 * np.abs(d) + np.abs(fd) + BINS + 2.0))[..., None, None]
    t_gsum = tf * (g0 + g1) + 3 * U * gsum
    w = np.abs(np64(r["_w"]))[:, :, None, None]
    tib = np.abs(np64(r["_tib"]))[:, :, None, :]
    rgb_max = float(np.float32(P["rgb_max"]))
    cg_d, cg_s = np64(r["_diff_pre"]) < rgb_max, np64(r["_spec_pre"]) < rgb_max
    sig_i = 1.0 / (1.0 + np.exp(-(np64(r["_z_irr"]) + P["irradiance_bias"])))
    sig_s = 1.0 / (1.0 + np.exp(-(np64(r["_z_slf"]) + P["slf_rgb_bias"])))
    a_s, a_i = head_abs_sums(sc)
    tsig_i, tsig_s = c(K_IRR) * a_i / 4 + 4 * U, c(K_SLF) * a_s / 4 + 4 * U
    gd = np.where(keep & cg_d, w * gsum * isc, 0.0)
    gs = np.where(keep & cg_s, w * gsum * isc, 0.0)
    t_gd = np.where(keep & cg_d, w * isc * t_gsum, 0.0) + 4 * U * gd
    t_gs = np.where(keep & cg_s, w * isc * t_gsum, 0.0) + 4 * U * gs
    rows = slice(r0, r0 + C)
    tol = {"x_irr": 0.0, "x_slf": 0.0}
    tol["dz_irr"] = (gd * tsig_i + t_gd * sig_i + U * gd * sig_i)[rows].reshape(C * S, HIST)
    t = np.zeros((C * S, LD_SLF))
    t[:, :HIST] = (gs * tib * tsig_s + tib * sig_s * t_gs + 5 * U * gs * tib * sig_s)[rows].reshape(C * S, HIST)
    tol["dz_slf"] = t
    sp_s = np64(r["_sp_s"])
    term = gs * sp_s
    tol["d_tib"] = ((t_gs * sp_s + gs * E["tsp_s"] + 2 * U * term).sum(2) + (BINS + 2) * U * term.sum(2)).reshape(n * S, 3)
    # direct: gat = w_low Gt[low] + w_high Gt[high] on the flattened axis
    td = _t_dir(sc, r)
    flat = Gt3.reshape(n * BINS, 3)
    base = (np.arange(n) * BINS)[:, None]
    gat, t_gat = np.zeros((n, S, 3)), np.zeros((n, S, 3))
    for (idx, ok, _), wt in zip(r["_terms"], (r["_w_low"], r["_w_high"])):
        idx, ok = idx.numpy(), ok.numpy()
        gv = np.where(ok[..., None], flat[np.clip(base + idx, 0, n * BINS - 1)], 0.0)
        wv = np.where(ok, np.abs(np64(wt)), 0.0)[..., None]
        gat += wv * gv
        t_gat += td[..., None] * gv + 3 * U * wv * gv
    w3 = np.abs(np64(r["_w"]))[..., None]
    tol["d_direct"] = (w3 * t_gat + U * w3 * gat).reshape(n * S, 3)
    direct = np.abs(np64(r["_direct"]))
    ds_ = np64(r["_diff"]) + np64(r["_spec"])
    tw = (t_gsum * ds_ + gsum * (E["t_diff"] + E["t_spec"]) + 2 * U * gsum * ds_).sum((2, 3)) + (HIST + 2) * U * (gsum * ds_).sum((2, 3))
    tw = tw + (direct * t_gat + 2 * U * direct * gat).sum(-1) + 6 * U * (direct * gat).sum(-1)
    tol["d_weights"] = tw.reshape(n * S) + U * np.abs(np64(ref["d_weights"]))
    return tol


def clamp_margin(sc, c=c_f32):
    """min over the kept elements of (|pre-clamp value - rgb_max| - its own bound): positive when no derivative of the
    clamp can flip between the device and the fp64 reference."""
    with torch.no_grad():
        r = forward(sc)
    E = _elem_bounds(sc, r, c, 4 * U)
    keep = r["_D"]["keep"][..., None]
    rgb_max = float(np.float32(sc.P["rgb_max"]))
    m = np.inf
    for pre, t in ((r["_diff_pre"], E["t_diff"]), (r["_spec_pre"], E["t_spec"])):
        v = np.where(keep, np.abs(np64(pre) - rgb_max) - t, np.inf)
        m = min(m, float(v.min()))
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# shadow rays


def shadow(ft, a, mut=None):
    """_compute_occlusions' rays (nerf.py:1233-1288): origin = mean + normal eps, direction = (light - mean) / max(dist,
    1e-5), near = shadow_near, far = clip(dist - light_near, shadow_near, shadow_far); normals and lights copied per sample."""
    n, spr = a["n"], a["samples_per_ray"]
    m, nr = a["means"].reshape(3, n).T.astype(ft), a["normals"].reshape(3, n).T.astype(ft)
    l = a["lights"].reshape(-1, 3)[np.arange(n) // spr].astype(ft)
    o = l - m
    dist = np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2])
    dn = np.maximum(dist, ft(1e-5))
    eps, near, far_, ln = (ft(np.float32(a[k])) for k in ("normal_eps", "shadow_near", "shadow_far", "light_near"))
    return {"origins": m + nr * eps, "dirs": o / dn[:, None], "near": np.full(n, near, ft),
            "far": np.minimum(np.maximum(dist - ln, near), far_), "out_normals": nr, "out_lights": l, "_dist": dist}


def expected_shadow(a):
    r64, r32 = shadow(np.float64, a), shadow(np.float32, a)
    ref = {k: r32[k] for k in ("origins", "near", "out_normals", "out_lights")}
    tol = {k: 0.0 for k in ref}
    ref["dirs"], tol["dirs"] = r64["dirs"], np.where(r64["dirs"] == 0, 0.0, 8 * U)
    near, far_ = float(np.float32(a["shadow_near"])), float(np.float32(a["shadow_far"]))
    raw = r64["_dist"] - float(np.float32(a["light_near"]))
    t = 4 * U * (r64["_dist"] + np.abs(r64["far"]))
    t = np.where((raw < near - t) | (raw > far_ + t), 0.0, t)
    ref["far"], tol["far"] = r64["far"], t
    return ref, tol


# ---------------------------------------------------------------------------------------------------------------------------
# the case table


def sc_forward(sc, dt=torch.float64, mut=None, hw=False):
    """The outputs of `forward` as fp64 numpy arrays (and "_D", the decisions), cached per scene."""
    key = (dt, mut, hw)
    if key not in sc._fw:
        with torch.no_grad():
            r = forward(sc, dt, mut, hw)
        sc._fw[key] = dict({k: np64(v) for k, v in r.items() if not k.startswith("_")}, _D=r["_D"])
    return sc._fw[key]


def scene_ref(sc):
    """The fp64 outputs of a scene with the parts of their tolerances, cached: every bound is linear in the head constant
    and in the softplus allowance, tol = T00 + m dC + allow dA with c(K) = m (K + 2) u.  "sp_err": the scene's share of
    Cases.softplus_allowance."""
    if "ref" not in sc._fw:
        with torch.no_grad():
            r = forward(sc)
        zero = lambda K: 0.0
        T00, T10, T01 = tol_bins(sc, r, zero, 0.0), tol_bins(sc, r, c_f32, 0.0), tol_bins(sc, r, zero, 1.0)
        worst = 0.0
        for z, bias in ((r["_z_irr"], "irradiance_bias"), (r["_z_slf"], "slf_rgb_bias")):
            x64 = z + float(np.float32(sc.P[bias]))
            s64 = softplus(x64)
            s32 = softplus(x64.to(torch.float32), hw=True).to(torch.float64)
            worst = max(worst, float(((s32 - s64).abs() / (1.0 + s64)).max()))
        sc._fw["ref"] = {"outs": {k: np64(r[k]) for k in HIST_OUT + RAY_OUT}, "D": r["_D"], "T00": T00,
                         "dC": {k: T10[k] - T00[k] for k in T00}, "dA": {k: T01[k] - T00[k] for k in T00}, "sp_err": worst}
        sc._fw[(torch.float64, None, False)] = dict(sc._fw["ref"]["outs"], _D=r["_D"])
    return sc._fw["ref"]


def scene_tol(sc, c, allow):
    R_ = scene_ref(sc)
    m = c(K_SLF) / c_f32(K_SLF)
    return {k: R_["T00"][k] + m * R_["dC"][k] + allow * R_["dA"][k] for k in R_["T00"]}


class TransCases(R.Cases):
    def __init__(self):
        super().__init__(sys.modules[__name__])
        self.scenes, self._allow = [], None

    def softplus_allowance(self):
        """max |softplus_bins in float32 - fp64 softplus| / (1 + fp64 softplus) over the head pre-activations of every
        scene, on the CPU.  The device is held to 4 x this."""
        if self._allow is None:
            self._allow = max(scene_ref(sc)["sp_err"] for sc in self.scenes)
        return self._allow


def reference(cs, li, ft=np.float64, mut=None, dev=None, hw=None):
    """The outputs of launch li: fp64 (the contract) or float32 (the restatement, softplus in the kernels' form)."""
    L = cs.launches[li]
    k = L["kernel"]
    dt = torch.float64 if ft == np.float64 else torch.float32
    hw = (ft == np.float32) if hw is None else hw
    if k == "shadow":
        return shadow(ft, L["args"], mut)
    sc = L["scene"]
    if k == "bins_bwd":
        out = ref_bwd(sc, L["G"], L["Gt"], L["ints"]["r0"], L["ints"]["C"], dt)
        return {s: (np64(v) if torch.is_tensor(v) else v) for s, v in out.items()}
    r = sc_forward(sc, dt, mut, hw)
    if k == "bins":
        return {s: v for s, v in r.items() if not s.startswith("_")}
    return {s: slice_of(r[s], L["t"]) for s in SLICE_OUT}


def expected(cs, li, dev=None, c=c_split):
    """(reference, tolerances) a device run of launch `li` is held to.  `c`: the head constant of the build under test."""
    L = cs.launches[li]
    k = L["kernel"]
    if k == "shadow":
        return expected_shadow(L["args"])
    sc = L["scene"]
    if k == "bins_bwd":
        ref = ref_bwd(sc, L["G"], L["Gt"], L["ints"]["r0"], L["ints"]["C"])
        ref = {s: (np64(v) if torch.is_tensor(v) else v) for s, v in ref.items()}
        return ref, tol_bwd(sc, L["G"], L["Gt"], L["ints"]["r0"], L["ints"]["C"], ref)
    tol, r = scene_tol(sc, c, 4.0 * cs.softplus_allowance()), scene_ref(sc)["outs"]
    if k == "bins":
        return r, tol
    t = np.asarray(L["t"], np.float32)
    ref = {s: slice_of(r[s], t) for s in SLICE_OUT}
    # the slice kernel's heads are fp32 FMA chains in both builds: c_f32 <= c, the histograms' bounds hold for it
    return ref, {s: slice_of(tol[s], t) + 3 * U * np.abs(ref[s]) for s in SLICE_OUT}


def render(cs, li, ref, mut=None):
    """The output buffers a device that computed `ref` in float32 would leave: {buffer: floats with guards}; elements a
    launch does not write ("_written_<slot>" False) stay canaries."""
    L = cs.launches[li]
    out = {}
    for slot in SLOTS[L["kernel"]][3]:
        idx = L["bufs"][slot]
        if idx < 0:
            continue
        buf = cs.bufs[idx].copy()
        v = np.asarray(ref[slot]).astype(np.float32).ravel()
        m = np.asarray(ref.get("_written_" + slot, True))
        m = np.broadcast_to(m, np.asarray(ref[slot]).shape).ravel()
        seg = buf[GUARD:GUARD + v.size]
        seg[m] = v[m]
        out[idx] = buf
    return out


def check(cs, li, got, ref, tol):
    """`got`: {buffer: floats with guards}.  Returns (failures [(slot, what, figure)], {slot: max error / tolerance}).
    A tolerance of 0 asks for the same value; an element the launch does not write has to be a canary still."""
    L = cs.launches[li]
    bad, ratio = [], {}
    for slot in SLOTS[L["kernel"]][3]:
        idx = L["bufs"][slot]
        if idx < 0:
            continue
        shape = out_shape(L["kernel"], slot, L["ints"])
        size = int(np.prod(shape))
        buf = got[idx]
        assert buf.size == size + 2 * GUARD
        if not (is_canary(buf[:GUARD]).all() and is_canary(buf[GUARD + size:]).all()):
            bad.append((slot, "canary", int((~is_canary(np.concatenate([buf[:GUARD], buf[GUARD + size:]]))).sum())))
        g = buf[GUARD:GUARD + size].reshape(shape)
        want = np.asarray(ref[slot], np.float64).reshape(shape)
        written = np.broadcast_to(np.asarray(ref.get("_written_" + slot, True)), shape)
        if not is_canary(g[~written]).all():
            bad.append((slot, "written outside the chunk", int((~is_canary(g[~written])).sum())))
        g64 = g.astype(np.float64)
        t = np.broadcast_to(np.asarray(tol[slot], np.float64), shape)
        if np.isnan(g64[written]).any() or np.isnan(t[written]).any():
            bad.append((slot, "nan", int(np.isnan(g64[written]).sum())))
            continue
        exact = (t == 0) & written
        if exact.any() and not np.array_equal(g[exact], want.astype(np.float32)[exact]):
            bad.append((slot, "value", float(np.abs(g64 - want)[exact].max())))
        err = np.abs(g64 - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            rr = float(np.where(exact | ~written, 0.0, err / t).max(initial=0.0))
        ratio[slot] = rr
        if not rr <= 1.0:
            bad.append((slot, "tolerance", rr))
    return bad, ratio


write_case_file = R.write_case_file
read_results = R.read_results


# ---------------------------------------------------------------------------------------------------------------------------
# cases

MAXD_TOP = 740                                   # max_dists = 740 exposures where a window has to reach bin 699


def _ramp25():
    t = np.arange(1, 26, dtype=np.float64)
    return (t / t.sum()).astype(np.float32)


def _gauss(sigma):
    half = int(np.floor(4.0 * sigma + 0.5))
    k = np.arange(-half, half + 1, dtype=np.float32)
    v = np.exp(-(k * k) / np.float32(2.0 * sigma * sigma)).astype(np.float32) - np.float32(np.exp(-8.0))
    return (v / v.sum(dtype=np.float32)).astype(np.float32)


def _asym(K, rng):
    v = rng.uniform(0.2, 1.0, K) * np.linspace(1.0, 0.25, K)
    return (v / v.sum()).astype(np.float32)


def make_scene(rng, wset, n, P, lo, hi, d_ind, taps=None, zero_w=None, ld_override=None, act=1.0, alpha=None):
    """A scene whose samples keep exactly the bins [lo, hi] ([n, 32] int; lo > hi: none) and whose time shift (ray_dist +
    shift) / exposure is d_ind ([n, 32]; integral values are met exactly when exposure, shift are dyadic).  light_dist sits
    `alpha` of a bin below (lo + threshold) exposures, cam_dist half a bin below the last kept bin's limit; both are
    re-drawn until no decision of `decisions` is a near tie."""
    P = dict(P)
    e = float(np.float32(P["exposure"]))
    P.setdefault("max_dists", float(np.float32(np.float64(P.pop("max_bin", 699)) * np.float64(np.float32(P["exposure"])))))
    P.pop("max_bin", None)
    maxd = float(np.float32(P["max_dists"]))
    lo, hi, d_ind = (np.broadcast_to(np.asarray(v), (n, S)).copy() for v in (lo, hi, d_ind))
    empty = lo > hi
    x_slf = np.maximum(rng.normal(0.3, 0.5, (n, S, 128)), 0.0).astype(np.float32) * np.float32(act)
    x_irr = np.maximum(rng.normal(0.3, 0.5, (n, S, 64)), 0.0).astype(np.float32) * np.float32(act)
    ts = np.zeros((TS_COUNT, n * S), np.float32)
    ts[TS_DD:TS_DD + 6] = rng.uniform(0.0, 0.6, (6, n * S))
    ts[TS_ALBEDO:TS_ALBEDO + 3] = rng.uniform(0.05, 0.9, (3, n * S))
    ts[TS_TIB:TS_TIB + 3] = rng.uniform(0.05, 0.95, (3, n * S))
    ts[TS_ROUGH] = rng.uniform(0.1, 1.0, n * S)
    ts[TS_NDOTL] = rng.uniform(0.0, 1.0, n * S)
    ts[TS_IRRAD] = rng.uniform(0.0, 2.0, n * S)
    ts[TS_OCC] = rng.uniform(0.0, 1.0, n * S) * (rng.uniform(size=n * S) < 0.5)
    w = rng.uniform(0.05, 1.0, (n, S))
    w = (w / w.sum(-1, keepdims=True) * rng.uniform(0.5, 1.0, (n, 1))).astype(np.float32)
    if zero_w is not None:
        w[np.broadcast_to(zero_w, (n, S))] = 0.0
    integral = d_ind == np.round(d_ind)
    sc = None
    for attempt in range(40):
        a = rng.uniform(0.2, 0.8, (n, S)) if alpha is None else np.broadcast_to(alpha, (n, S))
        ld = np.where(empty, (BINS + P["thr"] + 7.5) * e, (lo + P["thr"] - a) * e)
        if P["thr"] == 0:
            ld = np.where((lo == 0) & ~empty, 0.0, ld)
        cam = np.where(empty, maxd * 0.25, maxd - (hi + rng.uniform(0.3, 0.7, (n, S))) * e)
        dj = np.where(integral, d_ind, d_ind + rng.uniform(-0.02, 0.02, (n, S)) * (attempt > 0))
        rd = dj * e - float(np.float32(P["shift"]))
        if ld_override is not None:
            ld = np.where(np.isnan(ld_override), ld, ld_override)
        ts[TS_LDIST], ts[TS_RDIST], ts[TS_CAMDIST] = (f32(v).ravel() for v in (ld, rd, cam))
        sc = Scene(wset, x_slf, x_irr, ts.copy(), w, P, taps)
        if near_ties(sc) == 0:
            break
    else:
        raise AssertionError("no tie-free inputs found")
    if ld_override is None:
        glo, ghi = windows(decisions(sc)["keep"])
        assert np.array_equal(glo[~empty], lo[~empty]) and np.array_equal(ghi[~empty], hi[~empty]) and (glo[empty] > ghi[empty]).all(), \
            "the inputs do not give the windows asked for"
    return sc


def _sub_windows(rng, n, lo, hi, full_every=2):
    """Per-sample windows inside [lo, hi]: every `full_every`-th sample the whole of it, the others a random part."""
    L = rng.integers(lo, hi + 1, (n, S))
    H = np.array([[rng.integers(L[r, s], hi + 1) for s in range(S)] for r in range(n)])
    full = (np.arange(S) % full_every == 0)[None]
    return np.where(full, lo, L), np.where(full, hi, H)


def _slice_times(sc, count):
    """`count` times at and between the bins of interest: 0, 699, the largest entries of the direct and of the indirect
    histogram (integral), a quarter behind the one, half in front of the other, and the edges of the kept bins."""
    r = sc_forward(sc)
    dmax = int(r["out_direct"].max((0, 2)).argmax())
    imax = int(r["out_indirect"].max((0, 2)).argmax())
    lo, hi = windows(r["_D"]["keep"])
    wl = int(lo[lo <= hi].min()) if (lo <= hi).any() else 350
    t = [float(dmax), 0.0, 699.0, float(imax), dmax + 0.25, imax - 0.5, wl + 0.75, 698.5]
    t = [min(max(x, 0.0), 699.0) for x in t]
    return np.asarray(t[:count], np.float32)


def build_cases(seed=20241020):
    """The case table.  Every scene gives one k_transient_bins launch and one k_transient_slice launch with RC_TSLICE_MAX
    times on the same buffers (some a second with one time); the backward cases reuse scenes of the forward families."""
    rng = np.random.default_rng(seed)
    cs = TransCases()
    wsets = [WSet(rng, 0.18), WSet(rng, 1.4)]

    def wbufs(ws):
        if ws.bufs is None:
            ws.bufs = {k: cs.inp(getattr(ws, k)) for k in ("w_slf", "b_slf", "w_irr", "b_irr")}
        return ws.bufs

    def sbufs(sc):
        if sc.bufs is None:
            sc.bufs = dict(wbufs(sc.wset), slf_feat=cs.inp(layout_feat(sc.x_slf)), irr_feat=cs.inp(layout_feat(sc.x_irr)),
                           tshade=cs.inp(sc.tshade), weights=cs.inp(sc.weights))
            if sc.taps is not None:
                sc.bufs["taps"] = cs.inp(sc.taps)
            cs.scenes.append(sc)
        return sc.bufs

    def add(name, family, sc, outs=HIST_OUT + RAY_OUT, slice_outs=SLICE_OUT, counts=(TSLICE_MAX,), bins=True):
        ints = {"n_rays": sc.n, "bin_zero_threshold_light": sc.P["thr"], "light_zero": sc.P["light_zero"],
                "n_taps": 0 if sc.taps is None else len(sc.taps)}
        made = []
        if bins:
            li = cs.launch("bins", name, family, ints, sc.flts(), outs=outs, **sbufs(sc))
            cs.launches[li]["scene"] = sc
            made.append(li)
        for count in counts:
            t = _slice_times(sc, count)
            li = cs.launch("slice", f"{name}/slice{count}", family, dict(ints, count=count), sc.flts(), outs=slice_outs,
                           t=cs.inp(t), **sbufs(sc))
            cs.launches[li].update(scene=sc, t=t, twin=made[0] if bins else None)
            made.append(li)
        return made

    def add_bwd(name, family, sc, r0=0, C=None):
        C = sc.n if C is None else C
        G = rng.normal(size=(sc.n, HIST)).astype(np.float32)
        Gt = rng.normal(size=(sc.n, HIST)).astype(np.float32)
        ints = {"n_rays": sc.n, "r0": r0, "C": C, "bin_zero_threshold_light": sc.P["thr"], "light_zero": sc.P["light_zero"]}
        b = {k: v for k, v in sbufs(sc).items() if k != "taps"}
        li = cs.launch("bins_bwd", name, family, ints, sc.flts(), outs=BWD_OUT, G=cs.inp(G), Gt=cs.inp(Gt), **b)
        cs.launches[li].update(scene=sc, G=G, Gt=Gt)
        return li

    A, B = wsets
    taps25 = _gauss(3.0)
    base = dict(CORNELL)
    top = dict(CORNELL, max_bin=MAXD_TOP)
    dspread = lambda n, lo=3.0, hi=60.0: rng.uniform(lo, hi, (n, S))
    cs.window_specs = {}

    # ---- window placement: the union of a workgroup's windows is exactly [lo, hi]
    for lo, hi in ((0, 0), (0, 31), (31, 32), (32, 63), (33, 671), (640, 698), (699, 699), (0, 699)):
        P = top if hi == 699 else base
        L, H = _sub_windows(rng, 3, lo, hi)
        sc = make_scene(rng, A, 3, P, L, H, dspread(3, 0.5, 12.0), taps25)
        made = add(f"window[{lo},{hi}]", "window", sc, counts=(TSLICE_MAX, 1) if (lo, hi) == (33, 671) else (TSLICE_MAX,))
        cs.window_specs[made[0]] = (lo, hi)
        if (lo, hi) in ((0, 31), (32, 63), (33, 671)):
            add_bwd(f"bwd/window[{lo},{hi}]", "window", sc, 0, 3)
    n = 5                                         # rays 0-3 (one workgroup): no sample keeps a bin; ray 4 does
    L, H = _sub_windows(rng, n, 100, 180)
    L[:4], H[:4] = 1, 0
    sc = make_scene(rng, A, n, base, L, H, dspread(n), taps25)
    add("window/empty_workgroup", "window", sc)
    add_bwd("bwd/window/empty_workgroup", "window", sc, 0, 5)
    n = 4                                         # ray 2 of four keeps nothing
    L, H = _sub_windows(rng, n, 200, 320)
    L[2], H[2] = 1, 0
    add("window/empty_ray", "window", make_scene(rng, A, n, base, L, H, dspread(n), taps25))
    L, H = _sub_windows(rng, n, 5, 20)            # disjoint windows in one workgroup
    L2, H2 = _sub_windows(rng, n, 600, 690)
    L[1], H[1] = L2[1], H2[1]
    L[2:], H[2:] = 1, 0
    add("window/disjoint", "window", make_scene(rng, A, n, base, L, H, dspread(n, 0.5, 8.0), taps25))

    # ---- window comparisons: exposures and thresholds; exact ties at a dyadic exposure
    for e in (2.0 ** -7, 0.01, 0.037):
        for thr in (0, 1, 100, 699):
            lo_ = 40 if thr < 699 else 0
            P = dict(base, exposure=e, thr=thr, light_near=0.0 if thr < 100 else base["light_near"] * e / 0.01)
            L, H = _sub_windows(rng, 2, lo_, 400)
            tie = None
            if e == 2.0 ** -7:                    # half of the samples: light_dist exactly (lo + thr) exposures, a kept tie
                tie = np.where(np.arange(S)[None] % 2 == 1, 0.0, np.nan) + np.zeros((2, 1))
            sc = make_scene(rng, A, 2, P, L, H, np.round(dspread(2)) if tie is not None else dspread(2), None,
                            alpha=None if tie is None else np.where(np.isnan(tie), 0.5, 0.0))
            add(f"compare/e={e:.4g}/thr={thr}", "compare", sc)
    sc = make_scene(rng, A, 2, dict(base, thr=0, light_near=0.0), *_sub_windows(rng, 2, 0, 300), dspread(2))
    add("compare/thr=0/lo=0", "compare", sc)

    # ---- shift
    dy = dict(top, exposure=2.0 ** -7, light_near=0.7 * 2.0 ** -7 / 0.01)
    for name, P, d in (
            ("zero", dict(dy, shift=0.0), np.round(dspread(3, 2.0, 40.0)) + 0.0),
            ("int+", dict(dy, shift=17 * 2.0 ** -7), np.round(dspread(3, 20.0, 60.0))),
            ("int-", dict(dy, shift=-9 * 2.0 ** -7), np.round(dspread(3, -8.0, 30.0))),
            ("frac+", dict(top, shift=12.37 * 0.01), dspread(3, 13.0, 60.0)),
            ("frac-", dict(top, shift=-12.37 * 0.01), dspread(3, -12.0, 30.0)),
            ("below", dict(top, shift=-3.0), dspread(3, -290.0, -200.0)),          # larger than every ray_dist
            ("past", dict(top, shift=9.0), dspread(3, 900.0, 960.0)),              # every target past bin 699
            ("mixed_ties", dict(dy, shift=3 * 2.0 ** -7), np.where(rng.uniform(size=(3, S)) < 0.5, np.round(dspread(3)), dspread(3)))):
        L, H = _sub_windows(rng, 3, 600 if name == "below" else 20, 699)
        sc = make_scene(rng, A, 3, P, L, H, d, taps25)
        add(f"shift/{name}", "shift", sc)
        if name in ("int-", "frac-", "below", "mixed_ties"):
            add_bwd(f"bwd/shift/{name}", "shift", sc, 0, 3)
    d = np.repeat(rng.uniform(5.0, 40.0, (3, 1)), S, 1)                            # the samples of a ray share one shift
    d[1] = np.round(d[1])
    add("shift/coincide", "shift", make_scene(rng, A, 3, dict(dy, shift=0.0), *_sub_windows(rng, 3, 50, 400), d, taps25))

    # ---- direct part: d_dir = light_dist / e + d_ind
    n = 3
    L, H = _sub_windows(rng, n, 300, 500)         # (lo + 100) + d_ind in [695, 712]: spill into the next ray's bins 0..k
    d = 600.0 - (L + 100.0) + rng.uniform(95.0, 112.0, (n, S))
    add("direct/spill", "direct", make_scene(rng, A, n, base, L, H, d, taps25))
    add("direct/spill/one_ray", "direct", make_scene(rng, A, 1, base, L[:1], H[:1], d[:1], taps25))   # no predecessor, no successor
    P = dict(dy, shift=0.0)
    L, H = _sub_windows(rng, n, 60, 300)
    sc = make_scene(rng, A, n, P, L, H, np.round(dspread(n)), taps25, alpha=0.0)   # light_dist, ray_dist whole exposures
    D = decisions(sc)
    assert (D["low"] == D["high"]).all()
    add("direct/integral", "direct", sc)
    add_bwd("bwd/direct/integral", "direct", sc, 1, 2)
    L, H = _sub_windows(rng, n, 10, 200)          # ceil(d) <= 0: shift below -(light_dist + ray_dist)
    d = -(L + 100.0) - rng.uniform(1.0, 30.0, (n, S))
    sc = make_scene(rng, A, n, dict(base, shift=-6.0), L, H, d, taps25)
    assert (decisions(sc)["high"] <= 0).all()
    add("direct/negative", "direct", sc)
    add_bwd("bwd/direct/negative", "direct", sc, 0, 3)
    L, H = _sub_windows(rng, n, 100, 300)         # one sample 3e9 bins away in each direction
    far = np.full((n, S), np.nan)
    far[0, 5], far[1, 20] = 3e9 * 0.01, -3e9 * 0.01
    sc = make_scene(rng, A, n, base, L, H, dspread(n), taps25, ld_override=far)
    add("direct/far", "direct", sc)

    # ---- taps: orientation, count, the zero padding at both ends of the histogram
    n = 2
    L, H = _sub_windows(rng, n, 0, 40)
    d = np.where(np.arange(S)[None] % 2 == 0, rng.uniform(0.0, 15.0, (n, S)) - (L + 100.0),       # direct energy in bins 0..15
                 rng.uniform(684.0, 699.0, (n, S)) - (L + 100.0))                                 # and in 684..699
    for name, taps in (("0", None), ("3", np.array([0.5, 0.3, 0.2], np.float32)), ("25", _ramp25()), ("31", _asym(31, rng)),
                       ("32", _asym(32, rng)), ("33", _gauss(4.0) * np.linspace(1.3, 0.7, 33).astype(np.float32)),
                       ("49", _asym(49, rng)), ("25gauss", taps25)):
        sc = make_scene(rng, A, n, dict(base, shift=-2.0), L, H, d, taps)
        add(f"taps/{name}", "taps", sc)

    # ---- flags and clamps
    n = 3
    L, H = _sub_windows(rng, n, 30, 90)
    near_mix = np.where(rng.uniform(size=(n, S)) < 0.4, rng.uniform(0.05, 0.65, (n, S)), np.nan)   # light_dist < light_near
    for lz in (0, 1):
        sc = make_scene(rng, A, n, dict(base, light_zero=lz, thr=699), 0, H, dspread(n), taps25, ld_override=near_mix)
        add(f"flags/light_zero={lz}", "flags", sc)
        add_bwd(f"bwd/flags/light_zero={lz}", "flags", sc, 0, 3)
    sc = make_scene(rng, B, n, dict(base, rgb_max=0.1), L, H, dspread(n), taps25)
    add("flags/rgb_max/wide", "flags", make_scene(rng, B, n, dict(base, rgb_max=0.1), *_sub_windows(rng, n, 0, 698), dspread(n), taps25))
    add("flags/rgb_max", "flags", sc)
    # the backward's clamp: rgb_max in the widest gap between the pre-clamp values around their median
    with torch.no_grad():
        r = forward(sc)
    keep = r["_D"]["keep"][..., None] & np.ones(3, bool)
    v = np.sort(np.concatenate([np64(r["_diff_pre"])[keep], np64(r["_spec_pre"])[keep]]))
    v = v[int(0.35 * v.size):int(0.65 * v.size)]
    g = int(np.diff(v).argmax())
    scb = Scene(sc.wset, sc.x_slf, sc.x_irr, sc.tshade, sc.weights, dict(sc.P, rgb_max=float(np.float32(0.5 * (v[g] + v[g + 1])))), sc.taps)
    add("flags/rgb_max/gap", "flags", scb)
    add_bwd("bwd/flags/rgb_max", "flags", scb, 0, 3)
    sc = make_scene(rng, A, n, dict(base, indirect_scale=1.0, irradiance_bias=3.0, slf_rgb_bias=-8.0), L, H, dspread(n), taps25)
    add("flags/scale=1,bias=+3,-8", "flags", sc)
    add_bwd("bwd/flags/scale=1,bias=+3,-8", "flags", sc, 0, 3)
    sc = make_scene(rng, A, n, dict(base, irradiance_bias=-8.0, slf_rgb_bias=3.0), L, H, dspread(n), taps25)
    add("flags/bias=-8,+3", "flags", sc)
    zw = rng.uniform(size=(n, S)) < 0.3
    zw[1] = True                                  # a whole ray of weight 0
    sc = make_scene(rng, A, n, base, L, H, dspread(n), taps25, zero_w=zw)
    add("flags/zero_weights", "flags", sc)
    add_bwd("bwd/flags/zero_weights", "flags", sc, 0, 3)

    # ---- ray counts against 4 rays per workgroup; a chunk of the backward that is not the whole batch
    cs.lastray = []
    L9, H9 = _sub_windows(rng, 9, 120, 260)
    d9 = dspread(9)
    one = make_scene(rng, A, 9, base, L9, H9, d9, taps25)
    for n in (1, 3, 4, 5, 9):
        sc = Scene(A, one.x_slf[:n], one.x_irr[:n], one.tshade.reshape(TS_COUNT, 9, S)[:, :n].reshape(TS_COUNT, n * S).copy(),
                   one.weights[:n], one.P, one.taps)
        made = add(f"rays/{n}", "rays", sc)
        cs.lastray.append((n, made[0]))
        if n in (1, 5, 9):
            add_bwd(f"bwd/rays/{n}", "rays", sc, 0, n)
        if n == 9:
            add_bwd("bwd/rays/9/chunk[3,8)", "rays", sc, 3, 5)
            add_bwd("bwd/rays/9/chunk[8,9)", "rays", sc, 8, 1)

    # ---- output pointers: every optional output null; out_rgb alone; the slices' outputs one at a time
    sc = Scene(A, one.x_slf[:5], one.x_irr[:5], one.tshade.reshape(TS_COUNT, 9, S)[:, :5].reshape(TS_COUNT, 5 * S).copy(),
               one.weights[:5], one.P, one.taps)
    add("pointers/none", "pointers", sc, outs=(), slice_outs=())
    add("pointers/rgb", "pointers", sc, outs=("out_rgb",), slice_outs=("out_rgb",))
    add("pointers/direct", "pointers", sc, outs=("out_direct", "out_direct_rgb"), slice_outs=("out_direct",))
    add("pointers/indirect", "pointers", sc, outs=("out_indirect", "out_ti_specular"), slice_outs=("out_indirect",))

    # ---- shadow rays
    for n in (1, 255, 256, 257):
        for spr in (1, 5, 32):
            nr = -(-n // spr)
            means = rng.uniform(-1.0, 1.0, (3, n)).astype(np.float32)
            lights = rng.uniform(-1.5, 1.5, (nr, 3)).astype(np.float32)
            nrm = rng.normal(size=(3, n)).astype(np.float32)
            li_ = lights[np.arange(n) // spr].T
            k = np.arange(n)
            means[:, k % 7 == 0] = li_[:, k % 7 == 0]                                              # dist = 0
            sel = k % 7 == 1
            means[:, sel] = li_[:, sel] + np.float32(3e-6) * np.sign(nrm[:, sel])                   # dist < 1e-5
            sel = k % 7 == 2
            means[:, sel] = li_[:, sel] + np.float32(0.2) * nrm[:, sel] / np.linalg.norm(nrm[:, sel], axis=0)   # below light_near + near
            sel = k % 7 == 3
            means[:, sel] = li_[:, sel] + np.float32(9.0) * nrm[:, sel] / np.linalg.norm(nrm[:, sel], axis=0)   # beyond shadow_far
            args = dict(n=n, samples_per_ray=spr, normal_eps=1e-3, shadow_near=0.05, shadow_far=4.0, light_near=0.7,
                        means=means, normals=nrm, lights=lights)
            li = cs.launch("shadow", f"shadow/n={n}/spr={spr}", "shadow", {"n": n, "samples_per_ray": spr},
                           {k_: args[k_] for k_ in SLOTS["shadow"][1]}, outs=_SHADOW_OUT, means=cs.inp(means),
                           normals=cs.inp(nrm), lights=cs.inp(lights))
            cs.launches[li]["args"] = args
    return cs
