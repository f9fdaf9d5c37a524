"""The numpy restatement of the per-view evaluation (tests/eval_metrics_ref.py) pinned independently of itself: against
scipy's correlation, a literal four-loop SSIM, closed forms and hand-made cases; and MetricHarness' refusals.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage

import eval_metrics_ref as ref

EPS = float(np.finfo(np.float32).eps)
C1, C2 = 1e-4, 9e-4


def _images(h, w, seed=0, hi=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(0.0, hi, size=(h, w, 3)), rng.uniform(0.0, hi, size=(h, w, 3))


def test_window_is_dm_pix_gaussian():
    w = ref.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15
    assert np.allclose(w, w[::-1], rtol=0, atol=1e-17)
    assert np.allclose(w / w[5], np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2), rtol=1e-14, atol=0)


def test_moments_against_scipy_correlate1d():
    a, b = _images(17, 23, seed=1)
    w = ref.window()

    def scipy_valid(z):
        z = ndimage.correlate1d(z, w, axis=0, mode="constant")
        z = ndimage.correlate1d(z, w, axis=1, mode="constant")
        return z[5:-5, 5:-5]

    got = ref.moments(a, b)
    for g, z in zip(got, (a, b, a * a, b * b, a * b)):
        assert g.shape == (7, 13, 3)
        assert np.abs(g - scipy_valid(z)).max() < 1e-14


def _ssim_loops(a, b):
    """dm_pix.ssim written out: for every valid window position and channel, the 11 x 11 weighted sums."""
    w = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
    w = w / w.sum()
    H, W, C = a.shape
    out = np.zeros((H - 10, W - 10, C))
    for y in range(H - 10):
        for x in range(W - 10):
            for c in range(C):
                m = np.zeros(5)
                for i in range(11):
                    for j in range(11):
                        u, v, k = a[y + i, x + j, c], b[y + i, x + j, c], w[i] * w[j]
                        m += k * np.array([u, v, u * u, v * v, u * v])
                s00, s11 = max(EPS ** 2, m[2] - m[0] ** 2), max(EPS ** 2, m[3] - m[1] ** 2)
                s01 = m[4] - m[0] * m[1]
                s01 = np.sign(s01) * min(np.sqrt(s00 * s11), abs(s01))
                out[y, x, c] = ((2 * m[0] * m[1] + C1) * (2 * s01 + C2)) / ((m[0] ** 2 + m[1] ** 2 + C1) * (s00 + s11 + C2))
    return out.mean(), out


def test_ssim_against_four_loops():
    a, b = _images(11, 12, seed=2)
    b = 0.5 * a + 0.5 * b                        # correlated: sigma01 is neither zero nor at its bound
    val, smap = ref.ssim(a, b)
    lval, lmap = _ssim_loops(a, b)
    assert smap.shape == (1, 2, 3)
    assert np.abs(smap - lmap).max() < 1e-13 and abs(val - lval) < 1e-13


@pytest.mark.parametrize("a,b", [(0.5, 0.25), (0.3, 0.9), (0.0, 1.0)])
def test_ssim_of_constant_images_closed_form(a, b):
    A, B = np.full((12, 13, 3), a), np.full((12, 13, 3), b)
    val, _ = ref.ssim(A, B)
    want = (2 * a * b + C1) / (a * a + b * b + C1) * C2 / (C2 + 2 * EPS ** 2)
    assert abs(val - want) < 1e-12


def test_ssim_of_identical_images_is_one():
    a, _ = _images(14, 15, seed=3, hi=1.2)
    val, smap = ref.ssim(a, a.copy())
    assert abs(val - 1.0) < 1e-12 and np.abs(smap - 1.0).max() < 1e-12


def test_ssim_of_shifted_image_is_below_one():
    g, _ = _images(12, 46, seed=4)
    val, _ = ref.ssim(g[:, 1:], g[:, :-1])        # 12 x 45: the prediction is the ground truth moved by one pixel
    assert val < 0.9


def test_ssim_refuses_small_images():
    with pytest.raises(ValueError):
        ref.ssim(np.zeros((10, 20, 3)), np.zeros((10, 20, 3)))


def test_linear_to_srgb_branches():
    knee = 0.0031308
    x = np.array([0.0, EPS / 4, knee, np.nextafter(knee, 1.0), 0.5, 1.0, 1.2])
    y = ref.linear_to_srgb(x)
    assert y[0] == 0.0
    assert y[1] == 12.92 * EPS / 4                                          # linear branch: the eps floor is not reached
    assert y[2] == 12.92 * knee                                             # <= : the knee itself is linear
    assert abs(y[3] - (1.055 * knee ** (5 / 12) - 0.055)) < 1e-12           # (211 x^(5/12) - 11) / 200
    assert abs(y[2] - y[3]) < 1e-6                                          # the two branches meet at the knee
    assert abs(y[5] - 1.0) < 1e-15 and y[6] > 1.0                           # no clip without clip_eval
    assert ref.linear_to_srgb(np.array([-1.0]))[0] == -12.92
    assert ref.linear_to_srgb(np.array([0.5], np.float32), np.float32).dtype == np.float32


def test_postprocess_clip_eval_and_exposure():
    x = np.array([[[0.1, 0.5, 1.5]]])
    assert np.array_equal(ref.postprocess(x, exposure=0.7), ref.linear_to_srgb(x * 0.7))
    y = ref.postprocess(x, clip_eval=True)
    assert y.max() == 1.0 and np.array_equal(y[..., :2], ref.linear_to_srgb(x[..., :2]))
    with pytest.raises(ValueError):
        ref.postprocess(np.zeros((2, 2, 4, 3)), clip_eval=True)


def test_postprocess_bin_sum_clip():
    x = np.zeros((1, 2, 4, 3))
    x[0, 0, :, 0] = [0.25, 0.5, 0.25, 0.5]        # sum 1.5: / 3 = 0.5
    x[0, 0, :, 1] = 2.0                           # sum 8: / 3 clipped to 1
    x[0, 1, :, 2] = -1.0                          # negative: clipped to 0
    y = ref.postprocess(x, img_scale=3.0)
    assert y.shape == (1, 2, 3)
    assert y[0, 0, 0] == ref.linear_to_srgb(np.array(0.5)) and abs(y[0, 0, 1] - 1.0) < 1e-15 and y[0, 1, 2] == 0.0
    assert np.array_equal(ref.bin_sums(x)[0, 0], [1.5, 8.0, 0.0])


def test_mse_with_mask_keeps_full_denominator():
    pred, gt = np.full((11, 11, 3), 0.5), np.zeros((11, 11, 3))
    mask = np.zeros((11, 11))
    mask[:, :5] = 1.0
    r = ref.evaluate(pred, gt, mask=mask, skip_postprocess=True)
    assert abs(r["mse"] - 0.25 * 55 / 121) < 1e-15                 # 55 unmasked pixels of 121, / (121 x 3) values
    assert np.array_equal(r["post_pred"][:, 5:], np.zeros((11, 6, 3)))


def test_mse_zero_gives_infinite_psnr():
    a, _ = _images(11, 11, seed=5)
    r = ref.evaluate(a, a.copy())
    assert r["mse"] == 0.0 and r["psnr"] == np.inf
    assert abs(ref.mse_to_psnr(0.01) - 20.0) < 1e-12


def test_iou_disjoint_equal_nested():
    a, b = np.zeros((1, 1, 4, 3)), np.zeros((1, 1, 4, 3))
    a[0, 0, 0], b[0, 0, 1] = 1.0, 1.0
    assert ref.transient_iou(a, b) == 0.0                          # disjoint
    assert ref.transient_iou(a, a) == 1.0                          # equal
    c = a.copy()
    c[0, 0, 1:3] = 1.0                                             # a inside c: 3 of 9
    assert abs(ref.transient_iou(a, c) - 3.0 / 9.0) < 1e-15


def test_normal_mae_zero_norm_branch_and_mean_over_all_pixels():
    z, x = [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]
    normals = np.array([z, x, z, [0.0, 0.0, 0.0]])
    normals_gt = np.array([z, z, [0.0, 0.0, 0.0], z])
    acc = np.ones(4)
    mask = np.array([1.0, 1.0, 1.0, 0.0])
    ang = ref.normal_angles(normals, acc, normals_gt, mask)
    # pixel 2: a zero ground-truth normal stays zero -> dot 0 -> 90 degrees; pixel 3 is masked out (its gt normal is
    # shifted by 1 - mask = 1 first, and the angle is multiplied by the mask)
    assert np.allclose(ang, [0.0, 90.0, 90.0, 0.0], atol=1e-12)
    assert abs(ref.normal_mae(normals, acc, normals_gt, mask) - 180.0 / 4.0) < 1e-12     # / 4 pixels, not / sum(mask) = 3
    # acc = 0 shifts the prediction by one: (1, 1, 2) / sqrt 6 against z
    ang0 = ref.normal_angles(np.array([z]), np.zeros(1), np.array([z]))
    assert abs(ang0[0] - np.degrees(np.arccos(2.0 / np.sqrt(6.0)))) < 1e-12
    # below the 1e-5 threshold the vector is zeroed, above it is normalised
    tiny = ref.normal_angles(np.array([[0.0, 0.0, 5e-6], [0.0, 0.0, 2e-5]]), np.ones(2), np.array([z, z]))
    assert np.allclose(tiny, [90.0, 0.0], atol=1e-12)


def test_depth_l1_divides_by_mask_sum():
    d, gt = np.array([[1.0, 2.0], [3.0, 4.0]]), np.zeros((2, 2))
    mask = np.array([[1.0, 0.0], [1.0, 0.0]])
    assert ref.depth_l1(d, gt, mask) == (1.0 + 3.0) / 2.0
    assert ref.depth_l1(d, gt) == 2.5


def test_evaluate_fills_slots_by_inputs():
    a, b = _images(11, 12, seed=6)
    r = ref.evaluate(a, b)
    assert all(np.isnan(r[k]) for k in ("transient_iou", "l1_mean", "l1_median", "mae"))
    assert all(np.isfinite(r[k]) for k in ("mse", "psnr", "ssim"))
    r32 = ref.evaluate(a, b, dtype=np.float32)
    assert r32["post_pred"].dtype == np.float32 and r32["ssim_map"].dtype == np.float32
    assert abs(float(r32["ssim"]) - r["ssim"]) < 1e-4


def test_metric_harness_refusals():
    import nrc_amd
    from nrc_amd import metrics

    assert nrc_amd.MetricHarness is metrics.MetricHarness and nrc_amd.evaluate_view is metrics.evaluate_view
    with pytest.raises(NotImplementedError, match="LPIPS"):
        metrics.MetricHarness(None, disable_lpips=False)
    with pytest.raises(NotImplementedError, match="shift-invariant"):
        metrics.MetricHarness(None, disable_search_invariant=False)
    h = metrics.MetricHarness(None)                                # the defaults construct
    assert h.disable_ssim is False
    with pytest.raises(ValueError, match="RadianceCache"):
        h(np.zeros((11, 11, 3), np.float32), np.zeros((11, 11, 3), np.float32))


def test_binding_lists_the_result_slots_in_header_order():
    import os
    import re

    from nrc_amd import rc_ext

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "rc_abi.h")).read()
    body = src[src.index("RC_EVAL_MSE = 0"):src.index("} rc_eval_slot;")]
    enum = [e.lower() for e in re.findall(r"RC_EVAL_([A-Z_0-9]+)", body) if e != "COUNT"]
    assert enum == list(rc_ext.EVAL_SLOTS) == list(ref.SLOTS) and rc_ext.RC_EVAL_COUNT == len(enum)
