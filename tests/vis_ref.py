"""numpy restatement of the reference's visualisation arithmetic (internal/vis.py:50-137, 319-743, internal/image.py:192-200,
internal/utils.py:394-400) as this package defines it, with the working precision as an argument.

The weighted percentile is given twice: literally (a STABLE argsort, a cumulative sum, np.interp) and as the closed form the
device evaluates without a sort.  The pictures follow rc_vis_images' item operations one by one."""
import numpy as np

EPS = np.finfo(np.float32).eps
F32_MAX = np.finfo(np.float32).max
OPS = ("srgb", "binsum_srgb", "binsum_clip_srgb", "matte", "abs", "turbo")


def _weights(x, w, dtype):
    x = np.asarray(x).reshape(-1)
    return x, (np.ones(x.shape, dtype) if w is None else np.asarray(w).reshape(-1).astype(dtype))


def weighted_percentile(x, w, ps, dtype=np.float64):
    """vis.weighted_percentile read literally, with a stable sort and the cumulative sum in `dtype`; NaN where a weight is
    negative, NaN or infinite (the device's refusal)."""
    x, w = _weights(x, w, dtype)
    if not np.all(np.isfinite(w) & (w >= 0)):
        return np.full(len(ps), np.nan)
    idx = np.argsort(x, kind="stable")
    x, w = x[idx].astype(np.float64), w[idx]
    acc_w = np.cumsum(w, dtype=dtype)
    t = np.asarray(ps, dtype) * (acc_w[-1] / dtype(100))
    return np.interp(t.astype(np.float64), acc_w.astype(np.float64), x)


def weighted_percentile_closed(x, w, ps, dtype=np.float64):
    """The same quantity without a sort: C(v) = the weight of the elements <= v, v1 the smallest value with C(v1) > t, ...
    (include/rc_abi.h).  NaN values form the largest key, -0 and +0 one key."""
    x, w = _weights(x, w, dtype)
    if not np.all(np.isfinite(w) & (w >= 0)):
        return np.full(len(ps), np.nan)
    key = np.where(np.isnan(x), np.inf, x.astype(np.float64) + 0.0)          # order only; inf itself ties with NaN below
    rank = np.where(np.isnan(x), 2, np.where(np.isposinf(x), 1, 0))
    levels = sorted(set(zip(rank.tolist(), key.tolist())))
    level_of = {lv: i for i, lv in enumerate(levels)}
    lv = np.array([level_of[(r, k)] for r, k in zip(rank.tolist(), key.tolist())])
    value_of = [np.nan if r == 2 else k for r, k in levels]
    per_level = np.zeros(len(levels), dtype)
    for i in range(len(levels)):
        per_level[i] = np.sum(w[lv == i], dtype=dtype)
    C = np.cumsum(per_level, dtype=dtype)
    W = C[-1]
    out = []
    for p in ps:
        t = dtype(p) * (W / dtype(100))
        above = np.flatnonzero(C > t)
        if above.size == 0:
            out.append(value_of[-1])
            continue
        i1 = int(above[0])
        v1 = value_of[i1]
        B = C[i1 - 1] if i1 > 0 else dtype(0)
        w_f = w[np.flatnonzero(lv == i1)[0]]
        top = B + w_f
        if top <= t or i1 == 0:
            out.append(v1)
            continue
        v0 = value_of[i1 - 1]
        B, top, t = np.float64(B), np.float64(top), np.float64(t)
        out.append((v1 - v0) / (top - B) * (t - B) + v0)
    return np.asarray(out, np.float64)


def linear_to_srgb(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    with np.errstate(all="ignore"):
        srgb0 = dtype(323 / 25) * x
        srgb1 = (dtype(211) * np.maximum(dtype(EPS), x) ** dtype(5 / 12) - dtype(11)) / dtype(200)
        return np.where(x <= dtype(0.0031308), srgb0, srgb1)


def to_u8(x):
    """utils.save_img_u8's 8-bit form; np.round rounds half to even."""
    return np.round(np.clip(np.nan_to_num(x), 0.0, 1.0) * 255).astype(np.uint8)


def turbo_index(v):
    """matplotlib's lookup of a 256-entry ListedColormap at v in [0, 1]."""
    return np.minimum(np.trunc(np.asarray(v) * 256), 255).astype(np.int64)


def depth_curve(x, dtype):
    with np.errstate(all="ignore"):
        return -np.log(np.asarray(x, dtype) + dtype(EPS))


def cmap_value(value, bounds, auto_bounds=None, dtype=np.float64):
    """visualize_cmap's normalised value in [0, 1] (NaN -> 0) with the depth curve.  bounds: (lo, hi) float64; a bound of
    exactly 0 is falsy and replaced by the image's own percentile -/+ eps when auto_bounds is given."""
    lo, hi = float(bounds[0]), float(bounds[1])
    if auto_bounds is not None:
        lo = lo or (float(auto_bounds[0]) - float(EPS))
        hi = hi or (float(auto_bounds[1]) + float(EPS))
    lo, hi = dtype(np.float32(lo)) if dtype is np.float32 else dtype(lo), dtype(np.float32(hi)) if dtype is np.float32 else dtype(hi)
    c_lo, c_hi, c_x = depth_curve(lo, dtype), depth_curve(hi, dtype), depth_curve(value, dtype)
    with np.errstate(all="ignore"):
        v = np.clip((c_x - np.minimum(c_lo, c_hi)) / np.abs(c_hi - c_lo), dtype(0), dtype(1))
    return np.nan_to_num(v)


def item(op, src, lut=None, n_bins=0, scale=1.0, divide=1.0, divisor=None, offset=0.0, exponent=1.0, acc=None, mask=None,
         bounds=None, auto_bounds=None, nan_to_num=False, dtype=np.float64):
    """One item of rc_vis_images -> the float picture [H, W, 3] in `dtype` and, for "turbo", the normalised value besides
    (else None).  src: [H, W, c] or [H, W, n_bins, c]; divisor: the array whose np.max divides."""
    src = np.asarray(src, dtype)
    with np.errstate(all="ignore"):
        if op == "turbo":
            v = cmap_value(src.reshape(src.shape[:2]), bounds, auto_bounds, dtype)
            y = np.asarray(lut, dtype)[turbo_index(v)]
        else:
            v = None
            if n_bins:
                src = src.sum(-2, dtype=dtype)
            x = np.abs(src) if op == "abs" else src
            x = (x * dtype(scale)) / dtype(divide)
            if divisor is not None:
                x = x / np.max(np.asarray(divisor, dtype))
            if op in ("srgb", "binsum_srgb"):
                y = linear_to_srgb(x, dtype)
            elif op == "binsum_clip_srgb":
                y = linear_to_srgb(np.clip(x, dtype(0), dtype(1)), dtype)
            elif op == "matte":
                y = x ** dtype(exponent) if exponent != 1.0 else x
                if offset != 0.0:
                    y = y + dtype(offset)
                if acc is not None:
                    y = y + (dtype(1) - np.asarray(acc, dtype))[..., None]
            else:
                y = x
            y = y * np.ones(src.shape[:2] + (3,), dtype)
        if nan_to_num:                                       # the reference's pictures are float32: its largest finite value
            y = np.nan_to_num(y, posinf=float(F32_MAX), neginf=-float(F32_MAX))
        if mask is not None:
            y = np.where((np.asarray(mask) > 0)[..., None], y, dtype(1))
    return y, v


def suite(r, lut, img_scale=1.0, var_scale=1.0, vis_material=False, masks=None, transient=False, dtype=np.float64):
    """vis.visualize_suite / visualize_transient_suite (vis.py:319-743) followed by the trainer's masking of the depth
    pictures (trainer.py:1949-1953), entry by entry in the reference's order, for the source keys that `r` holds (an entry
    whose source is missing is left out).  r: [H, W, ...] arrays.  Returns ({vis key: picture [H, W, 3] in `dtype`},
    {depth key: normalised value [H, W]}); the percentiles are the float64 reading in both precisions."""
    out, values = {}, {}
    ntn = not transient

    def put(key, src, op, **kw):
        if src in r and kw.get("divisor", "") is not None:
            out[key], v = item(op, r[src], lut=lut, nan_to_num=ntn, dtype=dtype, **kw)
            if v is not None:
                values[key] = v

    def have(k):
        return r[k] if k in r else None

    H, W = r["acc"].shape[:2]
    acc = np.asarray(r["acc"]).reshape(H, W)
    if "distance_mean" in r:
        acc = np.where(np.isnan(np.asarray(r["distance_mean"]).reshape(H, W)), np.float32(0), acc)
    r = dict(r, acc=acc[..., None])
    put("acc", "acc", "matte")
    if "distance_median" in r:
        ps = [0.5, 99.5]
        bounds = weighted_percentile(r["distance_median"], acc, ps)
        for key, src in (("depth_mean", "distance_mean"), ("depth_median", "distance_median"), ("depth_gt", "depth_gt")):
            if src in r and (src != "depth_gt" or transient):
                put(key, src, "turbo", bounds=bounds, auto_bounds=weighted_percentile(r[src], acc, ps), mask=masks)
    put("lossmult", "lossmult", "matte")
    if transient:
        put("vignette", "vignette", "matte", divisor=have("vignette"))
        n_bins = r["rgb"].shape[2]
        put("color", "rgb", "binsum_clip_srgb", n_bins=n_bins, divide=img_scale)
        put("color_cache", "cache_rgb", "binsum_srgb", n_bins=n_bins)
        put("color_cache0", "cache_rgb", "binsum_clip_srgb", n_bins=n_bins, divide=img_scale)
    else:
        put("color", "rgb", "srgb")
        put("color_var", "rgb_variance", "abs", scale=var_scale / img_scale)
        put("color_cache", "cache_rgb", "srgb")
        put("color_cache0", "cache_rgb", "srgb", divisor=have("cache_rgb"))
    scaled = img_scale if transient else 1.0
    for name in ("diffuse", "specular", "direct", "indirect", "direct_diffuse", "direct_specular", "indirect_diffuse",
                 "indirect_specular"):
        put(f"cache_{name}_color", f"cache_{name}_rgb", "srgb", divide=scaled)
    for name in ("ambient", "albedo", "ambient_diffuse", "ambient_specular"):
        put(f"cache_{name}_color", f"cache_{name}_rgb", "srgb")
    put("cache_occ", "cache_occ", "matte")
    put("cache_indirect_occ", "cache_indirect_occ", "matte")
    if transient:
        put("cache_irradiance_color", "cache_irradiance_rgb", "srgb", divisor=have("cache_irradiance_rgb"))
        put("cache_light_radiance_color", "cache_light_radiance_rgb", "matte", divisor=have("cache_light_radiance_rgb"))
        put("cache_n_dot_l_color", "cache_n_dot_l_rgb", "srgb", divisor=have("cache_n_dot_l_rgb"))
    else:
        put("cache_irradiance_color", "cache_irradiance_rgb", "srgb")
        put("slf_rgb", "cache_incoming_rgb", "srgb")
        put("slf_rgb0", "cache_incoming_rgb", "srgb", divisor=have("cache_rgb"))
        put("env_map_rgb", "cache_env_map_rgb", "srgb")
        put("env_map_rgb0", "cache_env_map_rgb", "srgb", divisor=have("cache_rgb"))
        put("slf_depth", "cache_incoming_s_dist", "matte")
        put("slf_acc", "cache_incoming_acc", "matte")
    if vis_material:
        put("color_irradiance_cache", "irradiance_cache", "srgb")
        put("material_albedo", "material_albedo", "matte", exponent=1.0 / 2.2, acc=acc)
        for key in ("material_roughness", "material_F_0", "material_metalness", "material_diffuseness", "material_mirrorness"):
            put(key, key, "matte", acc=acc)
        if "material_rgb" in r:
            for name in ("diffuse", "specular", "direct", "indirect", "direct_diffuse", "direct_specular", "indirect_diffuse",
                         "indirect_specular"):
                put(f"material_{name}_color", f"{name}_rgb", "srgb", divide=scaled)
            put("material_occ", "occ", "matte")
            put("material_indirect_occ", "indirect_occ", "matte")
        if transient:
            put("material_lighting_irradiance", "lighting_irradiance", "srgb", divisor=have("cache_irradiance_rgb"))
            put("direct_rgb_no_integration", "direct_rgb_viz", "srgb", divisor=have("direct_rgb_viz"))
        else:
            put("material_lighting_irradiance", "lighting_irradiance", "srgb")
    for key in r:
        if key.startswith("normals"):
            put(key, key, "matte", divide=2.0, offset=0.5, acc=acc)
    return out, values
