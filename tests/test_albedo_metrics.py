"""The albedo evaluation without a GPU: the numpy restatement is pinned where the kernels rely on it (the
float32 median is the mean of the two middle order statistics, the lstsq system solves to a closed form), and the code of
rc_eval_albedo / rc_albedo_ratio is read from the gfx950 code objects: the exports are there and bound, the kernels
exist, none of them uses scratch or an MFMA."""
import ctypes

import numpy as np
import pytest

import albedo_metrics_ref as ref
import loss_cases as lc
from test_code_objects import product  # noqa: F401  (fixture)

KERNELS = {"k_albedo_count", "k_albedo_scan", "k_albedo_write", "k_albedo_begin", "k_albedo_hist", "k_albedo_narrow",
           "k_albedo_lstsq", "k_albedo_lstsq_finish", "k_albedo_score", "k_albedo_finish"}


def _rows(m, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    pred = r.uniform(0.02, 1.3, size=(m, 3)).astype(np.float32)
    gt = (pred * r.uniform(0.5, 1.5, size=(m, 3))).astype(np.float32)
    gt[::3] = np.minimum(pred[::3], 1.0)            # ratios of exactly 1: ties across the median position
    if m > 1:
        gt[1] = -gt[1]                              # a negative ratio
    return gt, pred


@pytest.mark.parametrize("m", [1, 2, 7, 64, 257, 1000])
def test_float32_median_is_the_mean_of_the_middle_order_statistics(m):
    gt, pred = _rows(m, seed=m)
    got = ref.ratio([gt], [pred], use_median=True, dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == (1, 3)
    ratios = gt / np.clip(pred, np.float32(1e-6), np.float32(1.0))
    assert ratios.dtype == np.float32
    s = np.sort(ratios, axis=0)
    lo, hi = s[(m - 1) // 2], s[m // 2]
    want = (lo + hi) / np.float32(2)
    assert want.dtype == np.float32
    assert np.array_equal(got[0], want), (got, want)
    # a view's own median is the same statistic
    view = ref.evaluate(pred.reshape(1, m, 3), np.ones((1, m), np.float32), gt.reshape(1, m, 3), dtype=np.float32)
    assert view["valid"] == m and np.array_equal(view["ratio"], want)


def test_median_of_no_rows_and_of_a_nan():
    empty = np.zeros((0, 3), np.float32)
    assert np.isnan(ref.ratio([empty], [empty], use_median=True, dtype=np.float32)).all()
    gt, pred = _rows(9, seed=1)
    gt[4, 1] = np.nan
    got = ref.ratio([gt], [pred], use_median=True, dtype=np.float32)[0]
    assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all()


@pytest.mark.parametrize("gamma", [True, False])
def test_closed_form_equals_the_literal_lstsq(gamma):
    views = [_rows(m, seed=10 + m) for m in (50, 301, 128)]
    gts, preds = [np.abs(g) for g, _ in views], [p for _, p in views]
    r64 = ref.ratio(gts, preds, use_median=False, gamma=gamma, dtype=np.float64)
    r32 = ref.ratio(gts, preds, use_median=False, gamma=gamma, dtype=np.float32)
    closed = ref.closed_form(gts, preds, gamma)
    print(f"gamma={gamma}: lstsq fp64 {r64} closed form {closed} |closed - fp64| {np.abs(closed - r64).max():.3e} "
          f"|fp32 - fp64| {np.abs(r32 - r64).max():.3e}")
    assert r64.shape == closed.shape == (1, 3) and r32.dtype == np.float32
    lc.check(closed, r64, r32.astype(np.float64), f"closed form gamma={gamma}")


def test_albedo_exports_are_present_and_bound():
    from nrc_amd import rc_ext

    lib = ctypes.CDLL(rc_ext.library_path())
    for name in ("rc_eval_albedo", "rc_albedo_ratio"):
        assert hasattr(lib, name) and name in rc_ext.EXPORTS, name
    assert len(rc_ext.ALBEDO_SLOTS) == rc_ext.RC_ALBEDO_COUNT == 6


def test_albedo_kernels_use_no_scratch_and_no_mfma(product):  # noqa: F811
    ks = {v["base"]: v for v in product.values() if v["base"] in KERNELS}
    assert set(ks) == KERNELS, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, (name, v["scratch"])
        assert not v["mfma"], (name, v["mfma"])
