"""rc_weighted_percentile, rc_image_max and rc_vis_images on the GPU against the numpy restatement of
tests/vis_ref.py.

The percentiles of quantised weights (multiples of 2^-12: every double sum is exact in any order) must EQUAL the float64
restatement; those of raw float32 weights lie within 3 x the distance between the float64 restatement and the same with
its sums in np.longdouble, plus 1e-12 of the value range.  Float pictures go through loss_cases.check: 3 x the float32
restatement's own distance from float64 plus 1e-6 of the scale.  The two integer forms (the colormap index, the 8-bit
value) may be off by one only where the float64 value lies within that bound of a step, and such pixels are at most 1 %
of a case.  The shapes are the smallest that cross each boundary of the 64-lane, 256-thread kernels."""
import os

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import nrc_amd
import vis_ref as ref
from nrc_amd import metrics, prng, rc_ext, vis
from nrc_amd import model as M
from test_gpu_eval_metrics import _mask, _two_cameras, _ws_ptr

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
PS = [0.5, 50.0, 99.5]
LUT = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turbo_lut.npy"))
LUT_U8 = ref.to_u8(LUT.astype(np.float64))
ROW_OF = {tuple(row): k for k, row in enumerate(LUT.tolist())}
HUGE = 1e30                                   # from here on a float picture has to equal the float32 restatement


@pytest.fixture(scope="module")
def rc():
    return rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)          # the visualisation calls need no weights


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---- weighted percentile ---------------------------------------------------------------------------------------------------

LEVELS = np.array([-3.5, -1.25, -0.5, 0.0, 0.125, 0.75, 1.0, 1.5, 2.25, 4.0, 17.0, 1.0e3], np.float32)     # 12 distinct levels


def _quantised(n, seed, all_zero=False):
    """Values from 12 levels (many ties), -0 beside +0, NaN values of weight zero; weights k / 4096 with a third of them 0.
    Reseeds until every t is at least 1e-9 W away from every cumulative sum, where the function jumps."""
    for attempt in range(50):
        r = _rng(seed + 1000 * attempt)
        x = r.choice(LEVELS, size=n)
        w = (r.integers(1, 4097, size=n) / 4096.0).astype(np.float32)
        w[r.random(n) < 1.0 / 3.0] = 0.0
        if n >= 2:
            x[n // 2 - 1], x[n // 2] = -0.0, 0.0
        if n >= 4:
            at = r.choice(n, size=max(1, n // 16), replace=False)
            at = at[(at != n // 2 - 1) & (at != n // 2)]
            x[at], w[at] = np.nan, 0.0
        if all_zero:
            w[:] = 0.0
        W = float(np.sum(w, dtype=np.float64))
        if W == 0.0:
            return x, w
        acc_w = np.cumsum(w[np.argsort(x, kind="stable")], dtype=np.float64)
        t = np.asarray(PS) * (W / 100.0)
        if np.abs(acc_w[None, :] - t[:, None]).min() >= 1e-9 * W:
            return x, w
    raise AssertionError("no seed keeps t away from the cumulative sums")


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_percentile_quantised_weights_equal_fp64(rc, n):
    for seed in (3, 4):
        x, w = _quantised(n, seed + n)
        want = ref.weighted_percentile(x, w, PS)
        assert _same(want, ref.weighted_percentile_closed(x, w, PS))
        got = rc.weighted_percentile(x, w, PS).cpu().numpy()
        print(f"n {n} seed {seed}: got {got} want {want}")
        assert _same(got, want), (n, seed, got, want)
    x, w = _quantised(n, 9)
    assert _same(rc.weighted_percentile(x, None, PS).cpu().numpy(), ref.weighted_percentile(x, None, PS))     # all ones


def test_percentile_all_weights_zero(rc):
    x, w = _quantised(257, 5, all_zero=True)
    want = ref.weighted_percentile(x, w, PS)
    got = rc.weighted_percentile(x, w, PS).cpu().numpy()
    assert _same(got, want) and np.isnan(want).all()                  # the largest value: a NaN sorts last
    x = np.where(np.isnan(x), np.float32(2.0), x)
    got = rc.weighted_percentile(x, w, PS).cpu().numpy()
    assert _same(got, ref.weighted_percentile(x, w, PS)) and np.all(got == 1.0e3)


def test_percentile_raw_float32_weights(rc):
    r = _rng(11)
    x = r.uniform(0.5, 6.0, size=(33, 31)).astype(np.float32)
    w = r.uniform(size=(33, 31)).astype(np.float32)
    ps = [0.5, 5.0, 50.0, 95.0, 99.5]
    r64 = ref.weighted_percentile(x, w, ps)
    rld = ref.weighted_percentile(x, w, ps, dtype=np.longdouble)
    got = rc.weighted_percentile(x, w, ps).cpu().numpy()
    own = np.abs(r64 - rld)
    tol = 3.0 * own + 1e-12 * float(x.max() - x.min())
    print(f"raw weights: |got - fp64| {np.abs(got - r64)} |fp64 - longdouble| {own} granted {tol}")
    assert np.all(np.abs(got - r64) <= tol), (got, r64, tol)


def test_percentile_refusals_and_repeats(rc):
    x, w = _quantised(4097, 21)
    want = rc.weighted_percentile(x, w, PS)
    for bad in (-0.25, np.nan, np.inf):
        wb = w.copy()
        wb[1234] = bad
        assert np.isnan(rc.weighted_percentile(x, wb, PS).cpu().numpy()).all(), bad
        assert torch.equal(rc.weighted_percentile(x, w, PS).view(torch.int64), want.view(torch.int64))   # twice: bitwise
    ptrs = [_ws_ptr(rc, "vz:" + k) for k in ("state", "part")]
    s = torch.cuda.Stream()
    dx, dw = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    s.wait_stream(torch.cuda.current_stream())
    got = rc.weighted_percentile(dx, dw, PS, stream_handle=s.cuda_stream)
    s.synchronize()
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    small = rc.weighted_percentile(x[:65], w[:65], PS).cpu().numpy()
    assert _same(small, ref.weighted_percentile(x[:65], w[:65], PS))
    assert ptrs == [_ws_ptr(rc, "vz:" + k) for k in ("state", "part")]                # the smaller call reallocated nothing
    out = torch.zeros(9, dtype=torch.float64, device="cuda")
    arr = (rc_ext.C.c_double * 9)(*([50.0] * 9))
    call = lambda v, o, n, k: rc.lib.rc_weighted_percentile(rc._h, v, None, n, arr, k, o, rc._stream())
    for what, args in (("value", (None, out.data_ptr(), 10, 1)), ("out", (dx.data_ptr(), None, 10, 1)),
                       ("n_ps", (dx.data_ptr(), out.data_ptr(), 10, 9)), ("n_ps", (dx.data_ptr(), out.data_ptr(), 10, 0)),
                       ("n", (dx.data_ptr(), out.data_ptr(), 0, 1)), ("n", (dx.data_ptr(), out.data_ptr(), 2 ** 31, 1))):
        code = call(*args)
        msg = (rc.lib.rc_last_error(rc._h) or b"").decode()
        assert code == INVALID_ARG and "rc_weighted_percentile" in msg and what in msg, (what, code, msg)
    assert torch.equal(rc.weighted_percentile(x, w, PS).view(torch.int64), want.view(torch.int64))


# ---- np.max ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_image_max_equals_numpy(rc, n, with_nan):
    x = _rng(n).normal(size=n + 1).astype(np.float32)
    x[n // 3] = 7.5 if n > 1 else x[0]
    if with_nan:
        x[(2 * n) // 3] = np.nan
    with np.errstate(invalid="ignore"):
        assert _same(rc.image_max(x[:n]).cpu().numpy(), [np.max(x[:n])])
        d = torch.from_numpy(x).cuda()
        assert _same(rc.image_max(d[1:]).cpu().numpy(), [np.max(x[1:])])           # not 16-byte aligned: the scalar path
    with pytest.raises(rc_ext.RcError):
        rc.image_max(np.zeros(0, np.float32))


# ---- pictures --------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (3, 5), (8, 8), (16, 16), (1, 257), (33, 31), (64, 96)]


def _plant(a, r, values):
    """values at random places of a (as many as fit)."""
    flat = a.reshape(-1)
    at = r.choice(flat.size, size=min(len(values), flat.size // 2), replace=False)
    flat[at] = values[: at.size]


def _items(h, w, seed):
    """Every operation of rc_vis_images once or more on an [h, w] view: (name, item).  A "divisor" is the ARRAY whose maximum divides: the device item takes rc.image_max of it."""
    r = _rng(seed)
    f32 = lambda *shape, lo=0.0, hi=1.0: r.uniform(lo, hi, size=shape).astype(np.float32)
    colour, grey, other = f32(h, w, 3, hi=1.6), f32(h, w, 1, hi=1.2), f32(h, w, 3, lo=0.2, hi=2.5)
    _plant(colour, r, [np.nan, np.inf, -np.inf, -0.3, 3.5, 0.001, 0.0031308, 0.0])
    _plant(grey, r, [-0.2, 40.0, 0.0])
    acc = f32(h, w)
    normals = r.normal(size=(h, w, 3)).astype(np.float32)
    albedo = f32(h, w, 1)
    _plant(albedo, r, [-0.1, np.nan, np.inf])
    mask = (r.random((h, w)) > 0.25).astype(np.float32)
    _plant(mask, r, [-1.0, 0.5])
    depth = f32(h, w, lo=1.5, hi=6.0)
    _plant(depth, r, [0.0, np.nan, -1.0, 1.0e-9, 50.0])
    bounds = ref.weighted_percentile(depth, acc, [0.5, 99.5])
    if not np.all(np.isfinite(bounds)) or bounds[0] == bounds[1]:
        bounds = np.array([1.6, 5.5])
    k = lambda **kw: kw
    return [
        ("srgb3", k(src=colour, op="srgb")),
        ("srgb1 / max", k(src=grey, op="srgb", divide=1.3, divisor=other)),
        ("srgb3 nan_to_num", k(src=colour, op="srgb", nan_to_num=True, mask=mask)),
        ("normals matte", k(src=normals, op="matte", divide=2.0, offset=0.5, acc=acc)),
        ("albedo matte", k(src=albedo, op="matte", exponent=1.0 / 2.2, acc=acc, nan_to_num=True)),
        ("plain 1 channel", k(src=grey, op="matte", mask=mask)),
        ("plain / max", k(src=other, op="matte", divisor=other)),
        ("abs", k(src=normals, op="abs", scale=0.7 / 1.3)),
        ("turbo masked", k(src=depth, op="turbo", channels=1, bounds=bounds, mask=mask)),
        ("turbo", k(src=depth, op="turbo", channels=1, bounds=bounds[::-1].copy(), nan_to_num=True)),
    ]


def _bin_items(h, w, seed):
    r = _rng(seed)
    few = r.uniform(0.0, 0.4, size=(h, w, 5, 3)).astype(np.float32)
    many = (r.uniform(size=(h, w, 700, 3)) * r.uniform(0.0, 0.004, size=(h, w, 1, 1))).astype(np.float32)
    one = r.uniform(0.0, 0.3, size=(h, w, 5, 1)).astype(np.float32)
    few[0, 0, 2, 1], few[1, 1, 0, 0], few[2, 2, 4, 2] = np.nan, -3.0, 9.0
    k = lambda **kw: kw
    return [
        ("5 bins", k(src=few, op="binsum_srgb", n_bins=5)),
        ("5 bins clip", k(src=few, op="binsum_clip_srgb", n_bins=5, divide=0.8)),
        ("700 bins clip", k(src=many, op="binsum_clip_srgb", n_bins=700, divide=0.9)),
        ("700 bins", k(src=many, op="binsum_srgb", n_bins=700, divisor=few[..., 0, :].copy())),
        ("5 bins 1 channel", k(src=one, op="binsum_srgb", n_bins=5, nan_to_num=True)),
    ]


def _device_items(rc, items, **outputs):
    """The items as rc.vis_images takes them: the divisor arrays reduced on the device."""
    return [dict(it, **outputs, **({"divisor": rc.image_max(it["divisor"])} if "divisor" in it else {})) for it in items]


def _restate(it, dtype):
    kw = {k: v for k, v in it.items() if k not in ("src", "op", "channels")}
    return ref.item(it["op"], it["src"] if it["src"].ndim > 2 else it["src"][..., None], lut=LUT, dtype=dtype, **kw)


def _check_float(got, y64, y32, what):
    """loss_cases.check where the float64 picture is finite and below HUGE; elsewhere (NaN, inf, nan_to_num's largest
    float) the picture has to be the float32 restatement's."""
    special = ~np.isfinite(y64) | (np.abs(y64) >= HUGE)
    assert _same(got[special], y32[special]) and np.isfinite(got[~special]).all(), (what, "NaN / inf pattern")
    z = lambda x: np.where(special, 0.0, np.asarray(x, np.float64))
    if not special.all():
        print(f"{what}: max|got - fp64| {np.abs(z(got) - z(y64)).max():.3e} max|fp32 - fp64| {np.abs(z(y32) - z(y64)).max():.3e}")
        lc.check(z(got), z(y64), z(y32), what)
    return special, lc.granted(z(y64), z(y32))


def _check_u8(got, y64, bound, what, budget):
    """|got - ref| <= 1, equal where the float64 x 255 is further than bound x 255 from a half-integer."""
    x = np.clip(np.nan_to_num(y64), 0.0, 1.0) * 255
    want = np.round(x).astype(np.int64)
    close = np.abs(np.abs(x - np.floor(x)) - 0.5) <= bound * 255
    budget[0] += int(close.sum())
    diff = np.abs(got.astype(np.int64) - want)
    assert diff.max() <= 1 and np.all(diff[~close] == 0), (what, int(diff.max()), int((diff[~close] != 0).sum()))


def _check_turbo(got_f32, got_u8, v64, v32, mask, what, budget):
    """Every pixel is a row of the table, at an index within 1 of the float64 one and equal to it where 256 v is further
    from a step than the bound on v allows; the 8-bit picture is the same row's; 1 where the mask is not > 0."""
    bound = lc.granted(v64, v32)
    k_ref = ref.turbo_index(v64)
    x = v64 * 256
    step = np.clip(np.round(x), 1, 255)                               # 0 and 256 are no steps: trunc stays inside the end bins
    close = np.abs(x - step) <= bound * 256
    out = np.zeros(v64.shape, bool) if mask is None else ~(mask > 0)
    budget[0] += int((close & ~out).sum())
    print(f"{what}: bound on v {bound:.3e}, {int((close & ~out).sum())} of {close.size} pixels next to a step")
    for (i, j), kr in np.ndenumerate(k_ref):
        if out[i, j]:
            assert np.all(got_f32[i, j] == 1.0) and np.all(got_u8[i, j] == 255), (what, i, j)
            continue
        k = ROW_OF.get(tuple(got_f32[i, j].tolist()))
        assert k is not None and abs(k - kr) <= 1 and (k == kr or close[i, j]), (what, i, j, k, int(kr), float(x[i, j]))
        assert np.array_equal(got_u8[i, j], LUT_U8[k]), (what, i, j)


def _run_items(rc, h, w, items, what):
    """One rc_vis_images call with both outputs of every item, checked item by item; the close pixels of the case."""
    both = _device_items(rc, [it for _, it in items], f32=True, u8=True)
    got = rc.vis_images(both, h, w)
    again = rc.vis_images(both, h, w)
    budget, total = [0], 0
    for (name, it), g, g2 in zip(items, got, again):
        label = f"{what} {name}"
        f, u = g["f32"].cpu().numpy(), g["u8"].cpu().numpy()
        assert f.shape == (h, w, 3) and u.shape == (h, w, 3) and u.dtype == np.uint8
        assert torch.equal(g["f32"].view(torch.int32), g2["f32"].view(torch.int32)) and torch.equal(g["u8"], g2["u8"]), label
        (y64, v64), (y32, v32) = _restate(it, np.float64), _restate(it, np.float32)
        total += f.size if it["op"] != "turbo" else v64.size
        if it["op"] == "turbo":
            _check_turbo(f, u, v64, v32, it.get("mask"), label, budget)
            continue
        special, bound = _check_float(f, y64, y32, label)
        y = np.where(special, y32.astype(np.float64), y64)             # the 8-bit form of what the float picture has to be
        _check_u8(u, y, bound, label, budget)
    print(f"{what}: {budget[0]} of {total} values may differ by one step")
    assert budget[0] <= 0.01 * total, (what, budget[0], total)


@pytest.mark.parametrize("h,w", SHAPES)
def test_vis_images_every_operation(rc, h, w):
    _run_items(rc, h, w, _items(h, w, seed=100 * h + w), f"{h}x{w}")


def test_vis_images_bins(rc):
    _run_items(rc, 11, 12, _bin_items(11, 12, seed=77), "11x12 bins")


def test_vis_images_more_items_than_one_launch(rc):
    h, w = 3, 5
    items = (_items(h, w, seed=1) + _items(h, w, seed=2) + _items(h, w, seed=3))[:27]
    _run_items(rc, h, w, items, "27 items")


def test_u8_only_and_f32_only_equal_both(rc):
    h, w = 33, 31
    items = [it for _, it in _items(h, w, seed=5)]
    both = rc.vis_images(_device_items(rc, items, f32=True, u8=True), h, w)
    only_u8 = rc.vis_images(_device_items(rc, items), h, w)
    only_f32 = rc.vis_images(_device_items(rc, items, f32=True), h, w)
    for b, u, f in zip(both, only_u8, only_f32):
        assert set(u) == {"u8"} and set(f) == {"f32"}
        assert torch.equal(b["u8"], u["u8"]) and torch.equal(b["f32"].view(torch.int32), f["f32"].view(torch.int32))


def test_depth_bound_of_exactly_zero_takes_the_automatic_bound(rc):
    h, w = 16, 16
    r = _rng(8)
    depth = r.uniform(1.0, 5.0, size=(h, w)).astype(np.float32)
    acc = r.uniform(size=(h, w)).astype(np.float32)
    auto = rc.weighted_percentile(depth, acc, [0.5, 99.5])
    a = auto.cpu().numpy()
    assert _same(a, ref.weighted_percentile(depth, acc, [0.5, 99.5]))
    run = lambda bounds, auto_bounds: rc.vis_images([dict(src=depth, op="turbo", channels=1, bounds=np.asarray(bounds, np.float64),
                                                          auto_bounds=auto_bounds, f32=True)], h, w)[0]["f32"].cpu().numpy()
    zero_lo = run([0.0, 4.0], auto)
    assert np.array_equal(zero_lo, run([a[0] - float(ref.EPS), 4.0], None))
    assert not np.array_equal(zero_lo, run([1.0, 4.0], auto))           # a bound that is not 0 is kept
    zero_hi = run([1.5, 0.0], auto)
    assert np.array_equal(zero_hi, run([1.5, a[1] + float(ref.EPS)], None))
    v64 = ref.cmap_value(depth, (0.0, 4.0), auto_bounds=a)
    v32 = ref.cmap_value(depth, (0.0, 4.0), auto_bounds=a, dtype=np.float32)
    _check_turbo(zero_lo, ref.to_u8(zero_lo.astype(np.float64)), v64, v32, None, "zero lo", [0])
    # vis.visualize_cmap: no bounds at all are the image's own percentiles -/+ eps
    own = vis.visualize_cmap(rc, torch.from_numpy(depth).cuda(), torch.from_numpy(acc).cuda()).cpu().numpy()
    assert np.array_equal(own, run([a[0] - float(ref.EPS), a[1] + float(ref.EPS)], None))


def test_vis_images_refusals_leave_the_handle_usable(rc):
    h, w = 8, 8
    items = _device_items(rc, [it for _, it in _items(h, w, seed=6)])
    want = rc.vis_images(items, h, w)
    src = torch.zeros((h, w, 3), device="cuda")
    hist = torch.zeros((h, w, 4, 3), device="cuda")
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    b = torch.ones(2, dtype=torch.float64, device="cuda")

    def call(n_items=1, height=h, width=w, null=False, **kw):
        it = rc_ext.rc_vis_item(src=src.data_ptr(), channels=3, n_bins=0, op=0, scale=1.0, divide=1.0, exponent=1.0,
                                out_u8=out.data_ptr())
        for k, v in kw.items():
            setattr(it, k, v)
        return rc.lib.rc_vis_images(rc._h, None if null else rc_ext.C.byref(it), n_items, height, width, rc._stream())

    turbo = rc_ext.VIS_OP_ID["turbo"]
    cases = [
        ("null items", call(null=True)), ("n_items", call(n_items=0)), ("height", call(height=0)), ("width", call(width=-2)),
        ("2^31", call(height=2 ** 16, width=2 ** 15)), ("null src", call(src=None)), ("no output", call(out_u8=None)),
        ("channels", call(channels=2)), ("unknown operation", call(op=17)), ("n_bins", call(n_bins=4)),
        ("n_bins", call(src=hist.data_ptr(), op=rc_ext.VIS_OP_ID["binsum_srgb"], n_bins=0)),
        ("RC_VIS_TURBO", call(op=turbo, channels=1)), ("RC_VIS_TURBO", call(op=turbo, bounds=b.data_ptr())),
    ]
    for what, code in cases:
        assert code == INVALID_ARG, (what, code)
    assert call() == 0                                                   # the same item without a fault is taken
    for a, g in zip(want, rc.vis_images(items, h, w)):
        assert torch.equal(a["u8"], g["u8"])
    with pytest.raises(ValueError):
        rc.vis_images([dict(src=np.zeros((h, w + 1, 3), np.float32), op="srgb")], h, w)
    with pytest.raises(ValueError):
        rc.vis_images([dict(src=np.zeros((h, w, 3), np.float32), op="srgb", gamma=2.2)], h, w)


def test_refusal_messages_name_the_fault(rc):
    src = torch.zeros((4, 4, 3), device="cuda")
    it = rc_ext.rc_vis_item(src=src.data_ptr(), channels=3, op=0, scale=1.0, divide=1.0, exponent=1.0)
    assert rc.lib.rc_vis_images(rc._h, rc_ext.C.byref(it), 1, 4, 4, rc._stream()) == INVALID_ARG
    msg = (rc.lib.rc_last_error(rc._h) or b"").decode()
    assert "rc_vis_images" in msg and "no output" in msg, msg


# ---- end to end: render a camera of a DeviceDataset, score it, draw it -----------------------------------------------------

H, W = 24, 20


def _scene(weights):
    cfg = nrc_amd.hotdog_config(render_chunk_size=128)               # 480 rays: three whole chunks and a padded one of 96
    m = M.Model(cfg, 0)
    m.load_variables(weights)
    p2c, c2w = _two_cameras(H, W, 4.0)
    ds = nrc_amd.DeviceDataset(m.rc, p2c, c2w, np.zeros((2, H, W, 3), np.float32), near=2.0, far=6.0)
    fn = M.bind_render_fn(M.create_render_fn(m))
    rays = ds.generate_ray_batch(1).rays.tree_map(lambda t: t.cpu().numpy())
    return cfg, m, ds, fn, rays


def _image_keys(img, h, w):
    """The per-pixel float arrays of a render_image result, as [h, w, ...]."""
    return {k: np.asarray(v) for k, v in img.items()
            if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.shape[:2] == (h, w)}


def _compare_suite(got, r, mask, what, h, w, must_have, **kw):
    s64, v64 = ref.suite(r, LUT, masks=mask, dtype=np.float64, **kw)
    s32, v32 = ref.suite(r, LUT, masks=mask, dtype=np.float32, **kw)
    assert set(got) == set(s64), (what, sorted(set(got) ^ set(s64)))
    assert must_have <= set(got), (what, sorted(must_have - set(got)))
    budget, total = [0], 0
    for key, pic in got.items():
        u = pic.cpu().numpy()
        assert u.shape == (h, w, 3) and u.dtype == np.uint8, (what, key)
        if key in v64:
            out = ~(mask > 0)
            k_ref = ref.turbo_index(v64[key])
            bound = lc.granted(v64[key], v32[key])
            x = v64[key] * 256
            close = np.abs(x - np.clip(np.round(x), 1, 255)) <= bound * 256
            budget[0] += int((close & ~out).sum())
            total += k_ref.size
            assert np.all(u[out] == 255), (what, key)
            ok = np.zeros(k_ref.shape, bool)
            for d in (-1, 0, 1):
                hit = np.all(u == LUT_U8[np.clip(k_ref + d, 0, 255)], axis=-1)
                ok |= hit & ((d == 0) | close)
            assert np.all(ok | out), (what, key, int((~(ok | out)).sum()))
            continue
        special = ~np.isfinite(s64[key]) | (np.abs(s64[key]) >= HUGE)
        z = lambda a: np.where(special, 0.0, np.asarray(a, np.float64))
        y = np.where(special, s32[key].astype(np.float64), s64[key])
        total += u.size
        _check_u8(u, y, lc.granted(z(s64[key]), z(s32[key])), f"{what} {key}", budget)
    print(f"{what}: {len(got)} pictures, {budget[0]} of {total} values may differ by one step: {sorted(got)}")
    assert budget[0] <= 0.01 * total, (what, budget[0], total)


def _scores(res):
    return {k: v for k, v in res.items() if k not in ("rays_per_sec", "vis")}


def test_evaluate_view_visualize_cache_pass(tmp_path):
    cfg, m, ds, fn, rays = _scene(common.weights_np())
    img = M.render_image(fn, None, rays, cfg, ("cache",), verbose=False)[0]
    mask = _mask(H, W)
    plain = metrics.evaluate_view(m, ds, 1, masks=mask)
    got = metrics.evaluate_view(m, ds, 1, masks=mask, visualize=True)
    assert "vis" not in plain and set(got) == set(plain) | {"vis"}
    assert _scores(got) == pytest.approx(_scores(plain), rel=0, abs=0, nan_ok=True)
    _compare_suite(got["vis"], _image_keys(img, H, W), mask, "cache pass", H, W,
                   {"acc", "depth_mean", "depth_median", "color", "color_cache", "color_cache0", "cache_albedo_color", "normals"})
    try:
        from PIL import Image
    except ImportError:
        return
    paths = vis.save_suite(got["vis"], str(tmp_path), 7)
    assert set(paths) == set(got["vis"]) and paths["color"].endswith(os.path.join("color", "0007.png"))
    assert np.array_equal(np.asarray(Image.open(paths["depth_median"])), got["vis"]["depth_median"].cpu().numpy())
    with pytest.raises(ValueError):
        vis.save_suite({"color": got["vis"]["color"].float()}, str(tmp_path), 8)


def test_evaluate_view_visualize_material_pass():
    passes = ("cache", "light", "material")
    cfg, m, ds, fn, rays = _scene(common.weights_material_np())
    key = prng.PRNGKey(5)
    img = M.render_image(fn, key, rays, cfg, passes, verbose=False)[0]
    mask = _mask(H, W)
    plain = metrics.evaluate_view(m, ds, 1, passes=passes, masks=mask, rng=key)
    got = metrics.evaluate_view(m, ds, 1, passes=passes, masks=mask, rng=key, visualize=True)
    assert _scores(got) == pytest.approx(_scores(plain), rel=0, abs=0, nan_ok=True)
    _compare_suite(got["vis"], _image_keys(img, H, W), mask, "material pass", H, W,
                   {"acc", "depth_median", "color", "color_cache0", "material_albedo", "material_roughness", "material_F_0",
                    "material_diffuse_color", "normals"}, vis_material=True)


def test_evaluate_view_visualize_transient():
    h = w = 11
    cfg = nrc_amd.cornell_transient_config(render_chunk_size=64)     # 121 rays: one whole chunk and one of 57
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_transient_np())
    p2c, c2w = _two_cameras(h, w, 2.5)
    ds = nrc_amd.DeviceDataset(m.rc, p2c, c2w, np.zeros((2, h, w, 3), np.float32), near=0.7, far=4.0)
    fields = {k: v.reshape(h * w, -1) for k, v in ds.generate_ray_batch(0).rays.hot_fields().items() if k != "lossmult"}
    # Not models.render_image here: it edge-pads the last chunk to a full one, and on a time-resolved handle a ray's direct
    # light past the last bin lands in the next ray of its batch, so the batch boundaries are part of the result.  The
    # restatement is fed the chunks evaluate_view renders, read back (as tests/test_gpu_eval_metrics.py does for the scores).
    names = list(metrics._TRANSIENT_VIS_KEYS)
    parts = [m.rc.render_transient({k: v[i: i + 64] for k, v in fields.items()}, None, outputs=names) for i in range(0, h * w, 64)]
    r = {k: np.concatenate([p[k].cpu().numpy() for p in parts]) for k in names}
    r = {k: v.reshape((h, w) + v.shape[1:]) for k, v in r.items()}
    r.update({"cache_" + k: r[k] for k in M._FINAL_INTEGRATOR_KEYS if k in r})
    r["vignette"], r["lossmult"] = np.ones((h, w, 1), np.float32), np.ones((h, w, 3), np.float32)
    gt = r["rgb"].copy()
    mask = _mask(h, w)
    scale = float(r["rgb"].sum(-2).max()) / 1.5                        # some bin sums above img_scale: the clip is taken
    plain = metrics.evaluate_view(m, ds, 0, gt=gt, masks=mask, img_scale=scale)
    got = metrics.evaluate_view(m, ds, 0, gt=gt, masks=mask, img_scale=scale, visualize=True)
    assert _scores(got) == pytest.approx(_scores(plain), rel=0, abs=0, nan_ok=True)
    _compare_suite(got["vis"], r, mask, "transient view", h, w,
                   {"acc", "depth_median", "color", "color_cache", "color_cache0", "vignette", "cache_n_dot_l_color", "normals"},
                   transient=True, img_scale=scale)
    # with a ground-truth depth: drawn by the transient suite, with distance_median's bounds; not by visualize_suite
    r["depth_gt"] = (r["distance_mean"] * _rng(43).uniform(0.8, 1.25, size=(h, w))).astype(np.float32)
    dev = {k: torch.from_numpy(v).cuda() for k, v in r.items()}
    unscaled = vis.visualize_transient_suite(dev, cfg, masks=mask, rc=m.rc)    # the config has no img_scale: 1
    _compare_suite(unscaled, r, mask, "transient view, img_scale 1, depth_gt", h, w, {"color", "cache_diffuse_color", "depth_gt"},
                   transient=True)
    plain_keys = {k: v for k, v in dev.items() if v.dim() < 4 or k not in ("rgb", "cache_rgb")}
    assert "depth_gt" not in vis.visualize_suite(plain_keys, cfg, masks=mask, rc=m.rc)
