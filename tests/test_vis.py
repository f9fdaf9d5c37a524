"""The visualisation arithmetic on the CPU: the closed form of the weighted percentile against its literal
reading, the colour table against matplotlib's, and the two integer rules (8-bit rounding, colormap index)."""
import os

import numpy as np
import pytest

import vis_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turbo_lut.npy")
PS = [0.0, 0.5, 5.0, 50.0, 99.5, 100.0]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _random_case(r, n):
    levels = np.concatenate([r.normal(size=6), [0.0, -0.0, 1.5, -2.0]]).astype(np.float32)
    x = r.choice(levels, size=n) if r.random() < 0.7 else r.normal(size=n).astype(np.float32)
    w = (r.integers(0, 9, size=n) / 8.0).astype(np.float32)
    w[r.random(n) < 0.3] = 0.0
    if r.random() < 0.3 and n > 3:
        at = r.integers(0, n, size=2)
        x[at] = np.nan
        w[at] = 0.0 if r.random() < 0.5 else w[at]
    return x.astype(np.float32), w


def test_closed_form_equals_the_literal_reading():
    r = np.random.default_rng(7)
    for case in range(300):
        n = int(r.integers(1, 60))
        x, w = _random_case(r, n)
        lit, closed = ref.weighted_percentile(x, w, PS), ref.weighted_percentile_closed(x, w, PS)
        assert _same(lit, closed), (case, x, w, lit, closed)


@pytest.mark.parametrize("what", ["all_zero", "single", "single_zero", "two_equal", "unweighted"])
def test_closed_form_edge_cases(what):
    x, w = {"all_zero": ([3.0, 1.0, 2.0, 1.0], [0, 0, 0, 0]), "single": ([4.5], [0.25]), "single_zero": ([4.5], [0.0]),
            "two_equal": ([2.0, 2.0], [0.0, 1.0]), "unweighted": ([5.0, -1.0, 3.0, 3.0, 0.0], None)}[what]
    x = np.asarray(x, np.float32)
    w = None if w is None else np.asarray(w, np.float32)
    lit, closed = ref.weighted_percentile(x, w, PS), ref.weighted_percentile_closed(x, w, PS)
    assert _same(lit, closed), (lit, closed)
    if what == "all_zero":
        assert np.all(lit == 3.0)                       # no value has C(v) > t: the largest value


def test_refused_weights_give_nan():
    x = np.arange(4, dtype=np.float32)
    for bad in (-1.0, np.nan, np.inf):
        w = np.array([1.0, bad, 1.0, 1.0], np.float32)
        assert np.isnan(ref.weighted_percentile(x, w, [50.0])).all() and np.isnan(ref.weighted_percentile_closed(x, w, [50.0])).all()


def test_turbo_lut_equals_golden_and_matplotlib():
    from nrc_amd import rc_ext

    lut = rc_ext.vis_turbo_lut()
    golden = np.load(GOLDEN)
    assert lut.dtype == np.float32 and lut.shape == (256, 3) and np.array_equal(lut, golden)
    try:
        from matplotlib import colormaps
    except ImportError:
        return
    assert np.array_equal(golden, np.asarray(colormaps["turbo"](np.arange(256))[:, :3], np.float32))
    v = np.array([0.0, 0.3, 255 / 256, 1.0])           # the float lookup goes through the same index rule
    assert np.array_equal(np.asarray(colormaps["turbo"](v)[:, :3], np.float32), golden[ref.turbo_index(v)])


def test_u8_rounds_half_to_even():
    x = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 127.5 / 255, -0.2, 1.7, np.nan, np.inf, -np.inf, 1.0, 0.0])
    exact = np.array([0.5, 1.5, 2.5, 127.5]) / 255 * 255
    assert np.array_equal(exact, [0.5, 1.5, 2.5, 127.5])       # the halves are hit exactly in float64
    assert ref.to_u8(x).tolist() == [0, 2, 2, 128, 0, 255, 0, 255, 0, 255, 0]


def test_colormap_index_rule():
    v = np.array([0.0, 1.0, 255 / 256, 254.999 / 256, 1 / 256, np.nan_to_num(np.nan)])
    assert ref.turbo_index(v).tolist() == [0, 255, 255, 254, 1, 0]
    # a NaN depth, a depth of 0 and a negative depth through visualize_cmap: NaN -> 0, the others inside [0, 1]
    got = ref.cmap_value(np.array([[np.nan, 0.0, -1.0, 2.0, 50.0]]), (2.0, 6.0), dtype=np.float32)
    assert got.dtype == np.float32 and got[0, 0] == 0.0 and got[0, 2] == 0.0 and got[0, 1] == 1.0 and got[0, 3] == 1.0 and got[0, 4] == 0.0


def test_zero_bound_takes_the_automatic_one():
    x = np.array([[1.0, 2.0, 4.0]])
    kept = ref.cmap_value(x, (1.0, 4.0), auto_bounds=(2.0, 3.0))
    auto = ref.cmap_value(x, (0.0, 4.0), auto_bounds=(2.0, 3.0))
    want = ref.cmap_value(x, (2.0 - float(ref.EPS), 4.0))
    assert np.array_equal(auto, want) and not np.array_equal(auto, kept)
