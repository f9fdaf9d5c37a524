"""numpy restatement of the shift-invariant metrics (internal/image_utils.py:74-189), for the CPU and
GPU tests of rc_eval_shift_invariant.  Test helper, not a test module.  Every function takes a `dtype` (np.float64: the
reference value; np.float32: the same arithmetic at the kernels' precision).

  shifted copy  jnp.pad(im0, (ri, rj), "reflect"), rolled by (-di, -dj) and cropped, in index form:
                shifted[y, x] = im0[R_H(y + di), R_W(x + dj)], R_n numpy's "reflect" (no edge repeat).
  mse map       mean over the channels of (shifted - im1)^2: the channels added in order, then divided by 3.
  ssim map      both images reflect-padded by 5, dm_pix.ssim's map (eval_metrics_ref.ssim) of the [H + 10, W + 10] pair,
                the channels added in order, then divided by 3.
  pooling       flax.linen.avg_pool(metric, (2 hw + 1,) * 2, padding="same"), read as: the sum over the window with zeros
                outside the image, divided by (2 hw + 1)^2.  flax is not part of the reference tree, so this reading is
                not pinned against a run of it; the pooled value only ranks the shifts of one pixel, and any per-pixel
                positive normalisation gives the same picks.  Order: along H, then along W, taps in increasing order, one
                division.
  search        di outer, dj inner; the first shift is taken, a later one replaces the best where pooled >= best (ssim) or
                pooled <= best (mse): an exact tie goes to the later shift.
  scores        mse: mean of the chosen shifts' unpooled map; ssim: mean of it over [5:-5, 5:-5].
"""
from __future__ import annotations

import numpy as np

import eval_metrics_ref as ref

PAD = 5


def reflect(i, n):
    """numpy's "reflect" of indices at most n - 1 outside [0, n)."""
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i > n - 1, 2 * (n - 1) - i, i))


def shifted(im0, di, dj):
    H, W = im0.shape[:2]
    return im0[reflect(np.arange(H) + di, H)][:, reflect(np.arange(W) + dj, W)]


def mse_map(a, b, dtype=np.float64):
    d = np.asarray(a, dtype) - np.asarray(b, dtype)
    d = d * d
    return ((d[..., 0] + d[..., 1]) + d[..., 2]) / dtype(3)


def pad_reflect(z):
    H, W = z.shape[:2]
    return z[reflect(np.arange(-PAD, H + PAD), H)][:, reflect(np.arange(-PAD, W + PAD), W)]


def ssim_map(a, b, dtype=np.float64):
    m = ref.ssim(pad_reflect(np.asarray(a, dtype)), pad_reflect(np.asarray(b, dtype)), dtype)[1]
    return ((m[..., 0] + m[..., 1]) + m[..., 2]) / dtype(3)


def pool(metric, hw, dtype=np.float64):
    """Box sum with zeros outside, along H then W, taps in increasing order, then one division."""
    m = np.asarray(metric, dtype)
    H, W = m.shape
    taps = 2 * hw + 1
    p = np.zeros((H + 2 * hw, W), dtype)
    p[hw: hw + H] = m
    cols = np.zeros((H, W), dtype)
    for k in range(taps):
        cols = cols + p[k: k + H]
    p = np.zeros((H, W + 2 * hw), dtype)
    p[:, hw: hw + W] = cols
    out = np.zeros((H, W), dtype)
    for k in range(taps):
        out = out + p[:, k: k + W]
    return out / dtype(taps * taps)


def search(im0, im1, kind, search_radii, hw, dtype=np.float64):
    """compute_shift_invariant_metric -> dict: opt_metric, opt_di, opt_dj [H, W]; "pooled" [(2 ri + 1)(2 rj + 1), H, W],
    the pooled map of every shift in the search's order; "shifts", their (di, dj); "score"."""
    im0, im1 = np.asarray(im0, dtype), np.asarray(im1, dtype)
    ri, rj = search_radii
    fn = ssim_map if kind == "ssim" else mse_map
    stack, shifts = [], []
    best = None
    for di in range(-ri, ri + 1):
        for dj in range(-rj, rj + 1):
            metric = fn(shifted(im0, di, dj), im1, dtype)
            pooled = pool(metric, hw, dtype)
            stack.append(pooled)
            shifts.append((di, dj))
            if best is None:
                best, opt = pooled, metric
                odi, odj = np.full(metric.shape, di, np.int32), np.full(metric.shape, dj, np.int32)
                continue
            take = pooled >= best if kind == "ssim" else pooled <= best
            best = np.where(take, pooled, best)
            opt = np.where(take, metric, opt)
            odi, odj = np.where(take, np.int32(di), odi), np.where(take, np.int32(dj), odj)
    score = opt[PAD:-PAD, PAD:-PAD].mean(dtype=np.float64) if kind == "ssim" else opt.mean(dtype=np.float64)
    return dict(opt_metric=opt, opt_di=odi, opt_dj=odj, pooled=np.stack(stack), shifts=shifts, score=float(score))


def margins(pooled, kind):
    """Per pixel, the gap between the best pooled value and the runner-up over the shifts ([H, W]; 0: an exact tie)."""
    s = np.sort(pooled, axis=0)
    if s.shape[0] == 1:
        return np.full(s.shape[1:], np.inf)
    return s[-1] - s[-2] if kind == "ssim" else s[1] - s[0]


def evaluate(pred, gt, search_radii=(4, 4), hw=8, want_ssim=True, dtype=np.float64):
    """rc_eval_shift_invariant: {"mse", "psnr", "ssim" (NaN without want_ssim), "mse_search", "ssim_search"}."""
    out = {"ssim": float("nan"), "ssim_search": None}
    out["mse_search"] = search(pred, gt, "mse", search_radii, hw, dtype)
    out["mse"] = out["mse_search"]["score"]
    out["psnr"] = float(ref.mse_to_psnr(np.float64(out["mse"])))
    if want_ssim:
        out["ssim_search"] = search(pred, gt, "ssim", search_radii, hw, dtype)
        out["ssim"] = out["ssim_search"]["score"]
    return out


def planted(h, w, seed, shift=(1, -2), noise=0.02):
    """(pred, gt) float32 [h, w, 3]: gt a window of a smooth random field, pred the window displaced by `shift` plus
    `noise` of Gaussian noise.  shifted(pred, -shift) then lines up with gt: the search picks (-shift[0], -shift[1])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = 12
    f = rng.uniform(0.0, 1.0, size=(h + 2 * m, w + 2 * m, 3))
    k = np.array([1.0, 2.0, 3.0, 2.0, 1.0]) / 9.0
    for axis in (0, 1):                              # smooth along both axes; the borders of the field are not used
        f = sum(kk * np.roll(f, s, axis=axis) for kk, s in zip(k, range(-2, 3)))
    gt = f[m: m + h, m: m + w]
    pred = f[m + shift[0]: m + shift[0] + h, m + shift[1]: m + shift[1] + w] + noise * rng.standard_normal((h, w, 3))
    return pred.astype(np.float32), gt.astype(np.float32)


def independent(h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(0.0, 1.0, size=(h, w, 3)).astype(np.float32), rng.uniform(0.0, 1.0, size=(h, w, 3)).astype(np.float32)
