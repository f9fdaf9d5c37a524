"""rc_eval_albedo and rc_albedo_ratio on the GPU against the numpy restatement of
tests/albedo_metrics_ref.py.  The pair rows, the valid count, the advanced device count and the median ratios are compared
EXACTLY with the fp32 restatement (every operation involved is one correctly rounded fp32 operation); the images, mse,
psnr and the least-squares ratio through loss_cases.check: 3 x the fp32 restatement's own distance from fp64 plus 1e-6 of
the quantity's scale.  The shapes are the smallest that cross each boundary of the 256-thread, 64-lane kernels."""
import ctypes

import numpy as np
import pytest
import torch

import albedo_metrics_ref as ref
import common
import loss_cases as lc
import nrc_amd
from nrc_amd import metrics, prng, rc_ext
from nrc_amd import model as M
from test_gpu_eval_metrics import _mask, _two_cameras, _ws_ptr

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
GUARD = -777.25
WS = ("pairs", "wg", "state", "part")


@pytest.fixture(scope="module")
def rc():
    return rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)          # the albedo calls need no weights


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _same(a, b):
    """Equal as floats, NaN in the same places, +0 == -0."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _check(got, r64, r32, what):
    """loss_cases.check on the finite values of the fp64 restatement; where that is NaN or infinite (the psnr of an
    exact match) the result has to be the same."""
    got, r64, r32 = (np.asarray(x, np.float64) for x in (got, r64, r32))
    special = ~np.isfinite(r64)
    assert _same(got[special], r64[special]) and np.isfinite(got[~special]).all(), (what, "NaN / inf pattern")
    if special.all():
        return
    z = lambda x: np.where(special, 0.0, x)
    print(f"{what}: max|got - fp64| {np.abs(z(got) - z(r64)).max():.3e} max|fp32 - fp64| {np.abs(z(r32) - z(r64)).max():.3e}")
    lc.check(z(got), z(r64), z(r32), what)


def _equal(a, b):
    """Two results of eval_albedo: every score and the ratio equal as floats."""
    return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)


def _valid(c):
    m = np.ones(c["acc"].shape, bool) if c["mask"] is None else c["mask"] > 0
    return m & (c["acc"] > 0.5)


def _case(h, w, masked, seed, parity=None, negative=True):
    """A view with the planted inputs: a third of the pixels with gt == p (ratio exactly 1, ties across the median, whose
    other ratios spread around, below or above 1 by channel); p below 1e-6 and albedo + (1 - acc) above 1 (both clips); gt = 0; acc == 0.5
    (excluded); a mask value of 0.5 (in, weighting the mse); a masked-out run (longer than a workgroup where the image
    allows); one negative gt on a valid pixel.  parity: the parity of the valid count, reached by dropping one valid pixel."""
    r, n = _rng(seed), h * w
    albedo = r.uniform(0.05, 0.9, size=(n, 3)).astype(np.float32)
    acc = r.uniform(0.55, 1.0, size=n).astype(np.float32)
    factor = r.uniform([0.5, 0.2, 0.9], [1.5, 1.0, 1.6], size=(n, 3))     # the median lies inside the ties, below them, mostly above
    gt = np.clip((albedo + (np.float32(1) - acc)[:, None]) * factor, 0.0, 1.0).astype(np.float32)
    acc[::3] = 1.0
    gt[::3] = albedo[::3]                               # p = albedo + 0 = gt
    mask = None
    if masked:
        mask = np.ones(n, np.float32)
        run = min(n // 3, 300)
        mask[n // 2: n // 2 + run] = 0.0
        mask[n - 1] = 0.0
        if n > 40:
            mask[5] = 0.5
            mask[7] = -1.0                              # not in
    if n > 40:
        albedo[10], acc[10], gt[10] = 0.0, 1.0, 0.3     # p = 0: below 1e-6
        albedo[11], acc[11] = 0.9, 0.6                  # p = 1.3: above 1
        gt[13] = 0.0
        acc[14] = 0.5                                   # excluded: the comparison is strict
        acc[16] = 0.2
        if negative:
            gt[17, 2] = -0.2
    c = dict(albedo=albedo.reshape(h, w, 3), acc=acc.reshape(h, w), albedo_gt=gt.reshape(h, w, 3),
             mask=None if mask is None else mask.reshape(h, w))
    if parity is not None:
        v = np.flatnonzero(_valid(c).reshape(-1))
        if v.size % 2 != parity:
            c["acc"].reshape(-1)[v[-1]] = 0.3
        assert int(_valid(c).sum()) % 2 == parity
    return c


def _compare(rc, c, what, base=0, **kw):
    """One call with every optional output and an AlbedoPairs whose count starts at `base`, against both restatements."""
    n = c["acc"].size
    pairs = rc_ext.AlbedoPairs(rc, base + n, fill=GUARD)
    pairs.count.fill_(base)
    got = rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"], pairs=pairs, keep_images=True, **kw)
    r64, r32 = ref.both(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"], **kw)
    m = r32["valid"]
    want_rows = np.concatenate([r32["pairs_gt"], r32["pairs_pred"]], axis=1)
    rows, count = pairs.rows()
    print(f"{what}: valid {got['valid']} (restatement {m}) count {count} ratio {got['ratio']} restatement {r32['ratio']}")
    assert got["valid"] == m == int(_valid(c).sum()) and count == base + m, (what, got["valid"], m, count)
    assert _same(rows[base:], want_rows), (what, "pair rows")
    assert np.all(rows[:base] == GUARD) and np.all(pairs.buffer[count:].cpu().numpy() == GUARD), (what, "rows outside")
    if "ratio" not in kw:
        own = rc.workspace("ea:pairs")[: 6 * m].reshape(m, 6)
        assert _same(own, want_rows), (what, "the workspace's rows")
    assert _same(np.asarray(got["ratio"], np.float32), r32["ratio"]), (what, got["ratio"], r32["ratio"])
    for k in ("post_pred", "post_gt", "ratio_im"):
        _check(got[k].cpu().numpy(), r64[k], r32[k], f"{what} {k}")
    for k in ("mse", "psnr"):
        _check(got[k], r64[k], r32[k], f"{what} {k}")
    return got, r64, r32


# 16 x 16 is one workgroup of 256 threads, 1 x 257 one more pixel; 8 x 8 one wave, 5 x 13 one more
SIZES = [(1, 1), (3, 5), (8, 8), (5, 13), (16, 16), (1, 257), (33, 31), (64, 96)]


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("h,w", SIZES)
def test_view_vs_restatement(rc, h, w, masked, parity):
    if h * w == 1 and masked:
        c = _case(h, w, False, seed=1)
        c["mask"] = np.full((1, 1), 0.5 if parity else 0.0, np.float32)
    else:
        c = _case(h, w, masked, seed=h * 100 + w, parity=parity)
    what = f"{h}x{w} masked={masked} parity={parity}"
    got, _, r32 = _compare(rc, c, what, base=parity * 3)
    assert got["valid"] % 2 == parity
    if h * w > 40:
        assert np.isnan(got["mse"])                     # the negative gt: NaN ** (1 / 2.2), as numpy
        ties = (r32["pairs_gt"] / np.clip(r32["pairs_pred"], np.float32(1e-6), np.float32(1)) == 1).mean()
        assert ties > 0.25, ties
        # the same view without the negative value: finite scores
        c = _case(h, w, masked, seed=h * 100 + w, parity=parity, negative=False)
        got, _, _ = _compare(rc, c, what + " no negative")
        assert np.isfinite(got["mse"]) and np.isfinite(got["psnr"])


def test_nan_in_one_channel(rc):
    c = _case(33, 31, True, seed=5, negative=False)
    v = np.flatnonzero(_valid(c).reshape(-1))
    c["albedo_gt"].reshape(-1, 3)[v[v.size // 2], 1] = np.nan
    got, _, r32 = _compare(rc, c, "NaN in channel 1")
    assert np.isnan(got["ratio"][1]) and np.isfinite(got["ratio"][0]) and np.isfinite(got["ratio"][2])
    assert np.isnan(got["mse"])


def test_no_valid_pixel(rc):
    c = _case(5, 13, True, seed=6, negative=False)
    c["acc"][:] = 0.4
    got, _, _ = _compare(rc, c, "no valid pixel", base=7)
    assert got["valid"] == 0 and np.isnan(got["ratio"]).all() and np.isfinite(got["mse"])


def test_ratio_handed_in(rc):
    c = _case(33, 31, True, seed=7, negative=False)
    ratio = np.array([0.8, 1.2, 1.5], np.float32)
    got, r64, _ = _compare(rc, c, "ratio handed in", ratio=ratio, albedo_clip=0.9)
    assert np.isclose(r64["post_pred"], 0.9 ** (1 / 2.2), rtol=1e-12, atol=0).any()      # the clip at albedo_clip is taken
    dev = rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"], ratio=torch.from_numpy(ratio).cuda()[None],
                         albedo_clip=0.9)
    assert _equal(dev, {k: got[k] for k in dev})


def _three_views():
    return [_case(5, 13, False, seed=11, negative=False), _case(16, 16, True, seed=12, negative=False),
            _case(33, 31, True, seed=13, negative=False)]


def test_three_views_appended(rc):
    views = _three_views()
    pairs = rc_ext.AlbedoPairs(rc, sum(c["acc"].size for c in views), fill=GUARD)
    r32s, r64s = [], []
    for c in views:
        rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"], pairs=pairs, sync=False)
        r64, r32 = ref.both(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"])
        r32s.append(r32)
        r64s.append(r64)
    want = np.concatenate([np.concatenate([r["pairs_gt"], r["pairs_pred"]], axis=1) for r in r32s])
    med = rc.albedo_ratio(pairs, use_median=True).cpu().numpy()
    rows, count = pairs.rows()
    assert count == want.shape[0] and _same(rows, want)
    m32 = ref.ratio([r["pairs_gt"] for r in r32s], [r["pairs_pred"] for r in r32s], use_median=True, dtype=np.float32)
    print(f"median over {count} rows: got {med} restatement {m32}")
    assert med.shape == (1, 3) and _same(med, m32)
    assert _same(metrics.pairs_ratio(rc, pairs, correct_median=True).cpu().numpy(), m32)
    for gamma in (True, False):
        got = rc.albedo_ratio(pairs, use_median=False, gamma=gamma).cpu().numpy()
        l64 = ref.ratio([r["pairs_gt"] for r in r64s], [r["pairs_pred"] for r in r64s], False, gamma, np.float64)
        l32 = ref.ratio([r["pairs_gt"] for r in r32s], [r["pairs_pred"] for r in r32s], False, gamma, np.float32)
        _check(got, l64, l32, f"least squares gamma={gamma}")
    assert np.all(pairs.buffer[count:].cpu().numpy() == GUARD)
    empty = rc_ext.AlbedoPairs(rc, 16)
    for kw in (dict(use_median=True), dict(use_median=False), dict(use_median=False, gamma=False)):
        assert np.isnan(rc.albedo_ratio(empty, **kw).cpu().numpy()).all(), kw


def test_overflow(rc):
    views = _three_views()
    total = sum(int(_valid(c).sum()) for c in views)
    pairs = rc_ext.AlbedoPairs(rc, total, fill=GUARD)
    cap = total - 100
    pairs.capacity = cap                               # the floats behind row `cap` are the guard
    for c in views:
        rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"], pairs=pairs, sync=False)
    count = int(pairs.count.item())
    assert count == total > cap
    assert np.all(pairs.buffer[cap:].cpu().numpy() == GUARD)
    assert not np.any(pairs.buffer[:cap].cpu().numpy() == GUARD)
    for kw in (dict(use_median=True), dict(use_median=False)):
        assert np.isnan(rc.albedo_ratio(pairs, **kw).cpu().numpy()).all(), kw
    with pytest.raises(RuntimeError, match="rows"):
        metrics.pairs_ratio(rc, pairs)
    # the view itself is scored from its own rows whatever became of the caller's buffer
    c = views[2]
    want = rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"])
    assert _equal(rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"], pairs=pairs), want)


def test_two_calls_are_bitwise_equal(rc):
    c = _case(64, 96, True, seed=14, negative=False)
    runs = []
    for _ in range(2):
        pairs = rc_ext.AlbedoPairs(rc, c["acc"].size, fill=GUARD)
        r = rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"], mask=c["mask"], pairs=pairs, keep_images=True, sync=False)
        runs.append((r, pairs, rc.albedo_ratio(pairs, use_median=False), rc.albedo_ratio(pairs, use_median=True)))
    (a, pa, la, ma), (b, pb, lb, mb) = runs
    assert torch.equal(a["result"].view(torch.int64), b["result"].view(torch.int64))
    for k in ("post_pred", "post_gt", "ratio_im"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(pa.buffer.view(torch.int32), pb.buffer.view(torch.int32)) and torch.equal(pa.count, pb.count)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(ma.view(torch.int32), mb.view(torch.int32))


def test_stream_and_workspace_reuse(rc):
    big, small = _case(64, 96, True, seed=15, negative=False), _case(5, 13, False, seed=16, negative=False)
    args = lambda c: (c["albedo"], c["acc"], c["albedo_gt"])
    want_big, want_small = rc.eval_albedo(*args(big), mask=big["mask"]), rc.eval_albedo(*args(small))
    lsq = rc.albedo_ratio(rc_ext.AlbedoPairs(rc, 64 * 96))             # the least squares' partial sums
    ptrs = [_ws_ptr(rc, "ea:" + k) for k in WS]
    s = torch.cuda.Stream()
    dev = [torch.from_numpy(x).cuda() for x in args(small)]
    s.wait_stream(torch.cuda.current_stream())
    assert _equal(rc.eval_albedo(*dev, stream_handle=s.cuda_stream), want_small)
    with torch.cuda.stream(s):
        assert _equal(rc.eval_albedo(*dev), want_small)
        pairs = rc_ext.AlbedoPairs(rc, 65)
        rc.eval_albedo(*dev, pairs=pairs, sync=False)
        med = rc.albedo_ratio(pairs, use_median=True)
    torch.cuda.current_stream().wait_stream(s)
    assert med.cpu().numpy().reshape(-1).tolist() == want_small["ratio"]
    assert _equal(rc.eval_albedo(*args(big), mask=big["mask"]), want_big)
    assert ptrs == [_ws_ptr(rc, "ea:" + k) for k in WS]                 # the smaller image reallocated nothing
    del lsq


def test_refusals_leave_the_handle_usable(rc):
    c = _case(5, 13, False, seed=17, negative=False)
    dev = {k: torch.from_numpy(c[k]).cuda() for k in ("albedo", "acc", "albedo_gt")}
    out = torch.empty(rc_ext.RC_ALBEDO_COUNT, dtype=torch.float64, device="cuda:0")
    pairs = rc_ext.AlbedoPairs(rc, 65)
    ratio = torch.empty(3, dtype=torch.float32, device="cuda:0")
    want = rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"])

    def view(out_ptr=out.data_ptr(), **kw):
        im = rc_ext.rc_albedo_images(height=5, width=13, albedo_clip=1.0, **{k: v.data_ptr() for k, v in dev.items()})
        for k, v in kw.items():
            setattr(im, k, v)
        return rc.lib.rc_eval_albedo(rc._h, ctypes.byref(im), out_ptr, rc._stream())

    def ratio_call(p=pairs.buffer.data_ptr(), cap=65, cnt=pairs.count.data_ptr(), r=ratio.data_ptr()):
        return rc.lib.rc_albedo_ratio(rc._h, p, cap, cnt, 1, 1, r, rc._stream())

    cases = [
        ("albedo", lambda: view(albedo=None), "rc_eval_albedo"), ("acc", lambda: view(acc=None), "rc_eval_albedo"),
        ("albedo_gt", lambda: view(albedo_gt=None), "rc_eval_albedo"), ("out", lambda: view(out_ptr=None), "rc_eval_albedo"),
        ("images", lambda: rc.lib.rc_eval_albedo(rc._h, None, out.data_ptr(), rc._stream()), "rc_eval_albedo"),
        ("height", lambda: view(height=0), "height"), ("width", lambda: view(width=-3), "width"),
        ("clip inf", lambda: view(albedo_clip=float("inf")), "albedo_clip"),
        ("clip nan", lambda: view(albedo_clip=float("nan")), "albedo_clip"),
        ("pairs without count", lambda: view(pairs=pairs.buffer.data_ptr(), pairs_capacity=65), "pairs_count"),
        ("negative capacity", lambda: view(pairs=pairs.buffer.data_ptr(), pairs_capacity=-1, pairs_count=pairs.count.data_ptr()), "pairs_capacity"),
        ("capacity 2^31", lambda: view(pairs=pairs.buffer.data_ptr(), pairs_capacity=2 ** 31, pairs_count=pairs.count.data_ptr()), "pairs_capacity"),
        ("ratio: pairs", lambda: ratio_call(p=None), "rc_albedo_ratio"), ("ratio: count", lambda: ratio_call(cnt=None), "rc_albedo_ratio"),
        ("ratio: ratio", lambda: ratio_call(r=None), "rc_albedo_ratio"),
        ("ratio: negative capacity", lambda: ratio_call(cap=-1), "pairs_capacity"),
        ("ratio: capacity 2^31", lambda: ratio_call(cap=2 ** 31), "pairs_capacity"),
    ]
    for what, call, text in cases:
        code = call()
        msg = (rc.lib.rc_last_error(rc._h) or b"").decode()
        assert code == INVALID_ARG and text in msg and ("rc_eval_albedo" in msg or "rc_albedo_ratio" in msg), (what, code, msg)
        assert _equal(rc.eval_albedo(c["albedo"], c["acc"], c["albedo_gt"]), want), what
    assert int(pairs.count.item()) == 0                                # nothing was launched
    with pytest.raises(ValueError):
        rc.eval_albedo(c["albedo"], c["acc"][:, :12].copy(), c["albedo_gt"])     # the binding: acc of another size


# ---- end to end: render a camera of a DeviceDataset and score its albedo -------------------------------------------------

H, W = 24, 20
SCALE = np.array([0.8, 1.1, 0.6])


def _albedo_gt(rendered):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    delta = (0.02 * np.sin(0.7 * xx + 0.4 * yy))[..., None] * np.array([1.0, -1.0, 0.5])
    return np.clip(rendered * SCALE + delta, 0.0, 1.0).astype(np.float32)


def _scene(weights):
    cfg = nrc_amd.hotdog_config(render_chunk_size=128)               # 480 rays: three whole chunks and a padded one of 96
    m = M.Model(cfg, 0)
    m.load_variables(weights)
    p2c, c2w = _two_cameras(H, W, 4.0)
    ds = nrc_amd.DeviceDataset(m.rc, p2c, c2w, np.zeros((2, H, W, 3), np.float32), near=2.0, far=6.0)
    fn = M.bind_render_fn(M.create_render_fn(m))
    rays = [ds.generate_ray_batch(c).rays.tree_map(lambda t: t.cpu().numpy()) for c in range(2)]
    return cfg, m, ds, fn, rays


def _albedo_scores(got, r64, r32, what):
    print(f"{what}: albedo_psnr {got['albedo_psnr']!r} fp64 {float(r64['psnr'])!r} ratio {got['albedo_ratio']} fp32 {r32['ratio']}")
    _check(got["albedo_mse"], r64["mse"], r32["mse"], what + " albedo_mse")
    _check(got["albedo_psnr"], r64["psnr"], r32["psnr"], what + " albedo_psnr")
    assert np.isfinite(got["albedo_psnr"])


def test_evaluate_view_albedo_cache_pass():
    cfg, m, ds, fn, rays = _scene(common.weights_np())
    img = M.render_image(fn, None, rays[1], cfg, ("cache",), verbose=False)[0]
    gt = _albedo_gt(img["albedo_rgb"])
    mask = _mask(H, W)
    plain = metrics.evaluate_view(m, ds, 1, masks=mask)
    got = metrics.evaluate_view(m, ds, 1, masks=mask, albedo=gt)
    assert set(got) == set(plain) | {"albedo_mse", "albedo_psnr", "albedo_ratio"}
    assert {k: got[k] for k in plain if k != "rays_per_sec"} == pytest.approx(
        {k: v for k, v in plain.items() if k != "rays_per_sec"}, rel=0, abs=0, nan_ok=True)
    r64, r32 = ref.both(img["albedo_rgb"], img["acc"], gt, mask=mask)
    assert r32["valid"] > 50
    _albedo_scores(got, r64, r32, "cache pass")
    assert _same(np.asarray(got["albedo_ratio"], np.float32), r32["ratio"])
    assert 10.0 < got["albedo_psnr"] < 80.0
    with pytest.raises(NotImplementedError):
        metrics.evaluate_view(m, ds, 1, passes=("cache", "is_secondary"))


def test_evaluate_view_material_pass():
    passes = ("cache", "light", "material")
    cfg, m, ds, fn, rays = _scene(common.weights_material_np())
    key = prng.PRNGKey(5)
    with pytest.raises(ValueError, match="randoms"):
        metrics.evaluate_view(m, ds, 1, passes=passes)
    img = M.render_image(fn, key, rays[1], cfg, passes, verbose=False)[0]
    gt = _albedo_gt(img["material_albedo"])
    mask = _mask(H, W)
    got = metrics.evaluate_view(m, ds, 1, passes=passes, masks=mask, rng=key, albedo=gt)
    r64, r32 = ref.both(img["material_albedo"], img["acc"], gt, mask=mask)
    assert r32["valid"] > 50
    _albedo_scores(got, r64, r32, "material pass")
    assert _same(np.asarray(got["albedo_ratio"], np.float32), r32["ratio"])      # exact: the images are render_image's
    # psnr from the material rgb (the data set's images are zeros: the exact mse of the masked post-processed render)
    import eval_metrics_ref as eref
    e64, e32 = eref.both(img["rgb"], np.zeros((H, W, 3), np.float32), mask=mask)
    for k in ("mse", "psnr"):
        _check(got[k], e64[k], e32[k], "material rgb " + k)
    # the test-set ratio over both cameras, fed back
    imgs = [M.render_image(fn, k, rays[c], cfg, passes, verbose=False)[0] for c, k in enumerate(_camera_keys(key, 2))]
    gts = np.stack([_albedo_gt(i["material_albedo"]) for i in imgs])
    masks = np.stack([np.ones((H, W), np.float32), mask])
    per = [ref.both(i["material_albedo"], i["acc"], gts[c], mask=masks[c]) for c, i in enumerate(imgs)]
    for use_median in (True, False):
        ratio = metrics.albedo_ratio(m, ds, gts, cams=[0, 1], passes=passes, masks=masks, rng=key, correct_median=use_median)
        assert ratio.shape == (1, 3) and ratio.is_cuda
        t64 = ref.ratio([p[0]["pairs_gt"] for p in per], [p[0]["pairs_pred"] for p in per], use_median, True, np.float64)
        t32 = ref.ratio([p[1]["pairs_gt"] for p in per], [p[1]["pairs_pred"] for p in per], use_median, True, np.float32)
        if use_median:
            assert _same(ratio.cpu().numpy(), t32), (ratio, t32)
        else:
            _check(ratio.cpu().numpy(), t64, t32, "test-set least squares")
        k1 = _camera_keys(key, 2)[1]
        fed = metrics.evaluate_view(m, ds, 1, passes=passes, masks=mask, rng=k1, albedo=gts[1], albedo_ratio=ratio, albedo_clip=0.95)
        a64, a32 = (ref.evaluate(imgs[1]["material_albedo"], imgs[1]["acc"], gts[1], mask=mask, ratio=t, albedo_clip=0.95, dtype=d)
                    for t, d in ((t64, np.float64), (t32, np.float32)))
        _albedo_scores(fed, a64, a32, f"ratio fed back (median={use_median})")
        assert np.asarray(fed["albedo_ratio"], np.float32).tolist() == ratio.cpu().numpy().reshape(-1).tolist()


def _camera_keys(key, n):
    """The keys metrics.albedo_ratio hands to its cameras: prng.chunk_keys, camera by camera."""
    keys = []
    for _ in range(n):
        k, key = prng.chunk_keys(key)
        keys.append(k)
    return keys
