"""rc_eval_image on the GPU against the fp64 restatement of tests/eval_metrics_ref.py.  Every comparison
is loss_cases.check: 3 x the fp32 restatement's own distance from fp64 plus 1e-6 of the quantity's scale.  The shapes are
the smallest at which each kernel can still go wrong: one window, partial 32 x 32 tiles with the seam crossed along either
axis, whole tiles; pixel rows of 15 and 2100 floats, 16-byte aligned or not."""
import ctypes

import numpy as np
import pytest
import torch

import common
import eval_metrics_ref as ref
import loss_cases as lc
import nrc_amd
from nrc_amd import metrics, rc_ext
from nrc_amd import model as M

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5
SCALARS = ref.SLOTS
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def rc():
    return rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)          # rc_eval_image needs no weights


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _images(h, w, seed):
    """Uniform in [0, 1.2] -- both branches of linear_to_srgb and values above 1 -- with a few values planted at and
    around the knee, at 0 and below float32's eps."""
    r = _rng(seed)
    a = r.uniform(0.0, 1.2, size=(h, w, 3)).astype(np.float32)
    b = np.clip(a + r.normal(scale=0.1, size=a.shape), 0.0, 1.2).astype(np.float32)
    plant = np.array([0.0, 1e-9, 0.0031308, 0.0031309, 0.002, 0.004], np.float32)
    a.reshape(-1)[: plant.size] = plant
    b.reshape(-1)[3: 3 + plant.size] = plant
    return a, b


def _mask(h, w):
    m = np.ones((h, w), np.float32)
    m[h // 4: h // 4 + max(2, h // 3), w // 5: w // 5 + max(3, w // 2)] = 0.0
    return m


def _scalars(got, r64, r32, what, keys=SCALARS):
    for k in keys:
        print(f"{what} {k}: got {got[k]!r} fp64 {float(r64[k])!r} |got - fp64| {abs(got[k] - float(r64[k])):.3e} "
              f"|fp32 - fp64| {abs(float(r32[k]) - float(r64[k])):.3e}")
        if np.isnan(r64[k]):
            assert np.isnan(got[k]), (what, k, got[k])
        else:
            lc.check(np.float64(got[k]), np.float64(r64[k]), np.float64(r32[k]), f"{what} {k}")


def _compare(rc, pred, gt, what, **kw):
    """One call with every optional output against both restatements: images and the SSIM map element-wise, then the
    scalars.  Returns (got, fp64 restatement)."""
    got = rc.eval_image(pred, gt, keep_images=True, ssim_map=True, **kw)
    r64, r32 = ref.both(pred, gt, **kw)
    for k in ("post_pred", "post_gt", "ssim_map"):
        g = got[k].cpu().numpy()
        assert g.shape == r64[k].shape, (what, k, g.shape)
        print(f"{what} {k}: max|got - fp64| {np.abs(g - r64[k]).max():.3e} max|fp32 - fp64| {np.abs(r32[k] - r64[k]).max():.3e}")
        lc.check(g, r64[k], r32[k], f"{what} {k}")
    _scalars(got, r64, r32, what)
    return got, r64


SIZES = [(11, 11), (12, 45), (43, 33), (64, 96)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("h,w", SIZES)
def test_psnr_ssim_vs_fp64(rc, h, w, masked):
    pred, gt = _images(h, w, seed=h * 100 + w)
    got, _ = _compare(rc, pred, gt, f"{h}x{w} masked={masked}", mask=_mask(h, w) if masked else None, exposure=0.7)
    assert all(np.isnan(got[k]) for k in ("transient_iou", "l1_mean", "l1_median", "mae"))


def test_clip_eval_and_plain_images(rc):
    pred, gt = _images(12, 45, seed=7)
    _compare(rc, pred, gt, "clip_eval", clip_eval=True, exposure=1.3)
    _compare(rc, pred, gt, "as they are", skip_postprocess=True)


@pytest.mark.parametrize("h,w", SIZES)
def test_identical_images(rc, h, w):
    pred, _ = _images(h, w, seed=3)
    got = rc.eval_image(pred, pred.copy(), exposure=0.7)
    assert got["mse"] == 0.0 and got["psnr"] == np.inf and abs(got["ssim"] - 1.0) <= 1e-6, got


@pytest.mark.parametrize("a,b", [(0.5, 0.25), (0.3, 0.9)])
def test_constant_images_closed_form(rc, a, b):
    A, B = np.full((12, 45, 3), a, np.float32), np.full((12, 45, 3), b, np.float32)
    got = rc.eval_image(A, B, skip_postprocess=True)
    a, b = float(np.float32(a)), float(np.float32(b))
    want = (2 * a * b + 1e-4) / (a * a + b * b + 1e-4) * 9e-4 / (9e-4 + 2 * EPS ** 2)
    s32 = float(ref.ssim(A, B, np.float32)[0])
    print(f"constant {a} {b}: got {got['ssim']!r} closed form {want!r} fp32 restatement {s32!r}")
    lc.check(np.float64(got["ssim"]), np.float64(want), np.float64(s32), "constant images")
    lc.check(np.float64(got["mse"]), np.float64((a - b) ** 2), np.float64(ref.evaluate(A, B, skip_postprocess=True, dtype=np.float32)["mse"]), "constant mse")


def _histograms(h, w, nb, seed):
    """Per-pixel brightness spread over [0, 1.5 img_scale] of bin sums, so the clip at 1 is taken by some pixels."""
    r = _rng(seed)
    level = r.uniform(0.0, 1.5 * 3.0 / nb * 2.0, size=(h, w, 1, 1))
    pred = (r.uniform(0.0, 1.0, size=(h, w, nb, 3)) * level).astype(np.float32)
    gt = (pred * r.uniform(0.5, 1.5, size=pred.shape)).astype(np.float32)
    return pred, gt


def _offset(x, floats):
    """x on the device, `floats` floats behind a 256-byte boundary."""
    flat = torch.empty(x.size + 64, dtype=torch.float32, device="cuda:0")
    v = flat[floats: floats + x.size]
    v.copy_(torch.from_numpy(x.reshape(-1)))
    return v.view(x.shape)


@pytest.mark.parametrize("nb,offsets", [(5, (0, 0)), (5, (1, 1)), (5, (3, 3)), (5, (1, 0)), (7, (2, 2)), (700, (0, 0)), (700, (1, 1))])
def test_bins_vs_fp64(rc, nb, offsets):
    """11 x 12 pixels; n_bins = 5: rows of 15 floats (no multiple of four: head and tail on most pixels); the arrays
    start 0, 1 or 3 floats behind a 16-byte boundary, or differently (the scalar path)."""
    h, w = 11, 12
    pred, gt = _histograms(h, w, nb, seed=nb)
    dp, dg = _offset(pred, offsets[0]), _offset(gt, offsets[1])
    what = f"bins={nb} offsets={offsets}"
    got = rc.eval_image(dp, dg, img_scale=3.0, keep_images=True, ssim_map=True)
    r64, r32 = ref.both(pred, gt, img_scale=3.0)
    for k in ("binsum_pred", "binsum_gt"):
        g = rc.workspace("ev:" + k)[: h * w * 3].reshape(h, w, 3)
        print(f"{what} {k}: max|got - fp64| {np.abs(g - r64[k]).max():.3e} max|fp32 - fp64| {np.abs(r32[k] - r64[k]).max():.3e}")
        lc.check(g, r64[k], r32[k], f"{what} {k}")
    assert (r64["binsum_pred"] / 3.0 > 1.0).any() and (r64["binsum_pred"] / 3.0 < 1.0).any()
    for k in ("post_pred", "post_gt", "ssim_map"):
        lc.check(got[k].cpu().numpy(), r64[k], r32[k], f"{what} {k}")
    _scalars(got, r64, r32, what)
    same = rc.eval_image(dp, dp.clone(), img_scale=3.0)
    assert same["transient_iou"] == 1.0 and same["mse"] == 0.0, same


@pytest.mark.parametrize("masked", [False, True])
def test_depth_and_normals_vs_fp64(rc, masked):
    h, w = 13, 17
    r = _rng(21)
    pred, gt = _images(h, w, seed=22)
    mask = _mask(h, w) if masked else None
    unit = lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    normals_gt = unit(r.normal(size=(h, w, 3)))
    normals = (unit(normals_gt + 0.3 * r.normal(size=(h, w, 3))) * r.uniform(0.5, 1.0, size=(h, w, 1))).astype(np.float32)
    acc = r.uniform(0.6, 1.0, size=(h, w)).astype(np.float32)
    acc[2, 3:6] = 0.0                                   # the prediction is shifted by one
    normals[5, 5] = 0.0
    acc[5, 5] = 1.0                                     # a zero prediction, not shifted: the zero-norm branch
    normals_gt[7, 1:4] = 0.0                            # zero ground-truth normals (inside the mask: stay zero)
    depth = r.uniform(2.0, 6.0, size=(h, w)).astype(np.float32)
    dmean = (depth + r.normal(scale=0.2, size=(h, w))).astype(np.float32)
    dmed = (depth + r.normal(scale=0.1, size=(h, w))).astype(np.float32)
    kw = dict(mask=mask, acc=acc, normals=normals, normals_gt=normals_gt, distance_mean=dmean, distance_median=dmed, depth_gt=depth)
    got, r64 = _compare(rc, pred, gt, f"depth+normals masked={masked}", **kw)
    assert all(np.isfinite(got[k]) for k in ("l1_mean", "l1_median", "mae"))
    # only one of the two distances
    one = rc.eval_image(pred, gt, mask=mask, distance_median=dmed, depth_gt=depth)
    assert np.isnan(one["l1_mean"]) and one["l1_median"] == got["l1_median"] and np.isnan(one["mae"])


def test_two_calls_are_bitwise_equal(rc):
    pred, gt = _images(12, 45, seed=5)
    a = rc.eval_image(pred, gt, mask=_mask(12, 45), ssim_map=True, sync=False)
    b = rc.eval_image(pred, gt, mask=_mask(12, 45), ssim_map=True, sync=False)
    assert torch.equal(a["result"].view(torch.int64), b["result"].view(torch.int64))
    assert torch.equal(a["ssim_map"].view(torch.int32), b["ssim_map"].view(torch.int32))


def _ws_ptr(rc, name):
    ptr, cnt = ctypes.c_void_p(), ctypes.c_int64()
    rc._check(rc.lib.rc_workspace_ptr(rc._h, name.encode(), ctypes.byref(ptr), ctypes.byref(cnt)))
    return ptr.value


def test_stream_and_workspace_reuse(rc):
    big, small = _images(64, 96, seed=8), _images(12, 45, seed=9)
    want_big, want_small = rc.eval_image(*big), rc.eval_image(*small)
    ptrs = [_ws_ptr(rc, "ev:" + k) for k in ("post_pred", "post_gt", "part")]
    s = torch.cuda.Stream()
    dev = [torch.from_numpy(x).cuda() for x in small]
    s.wait_stream(torch.cuda.current_stream())
    got = rc.eval_image(*dev, stream_handle=s.cuda_stream)
    assert got == pytest.approx(want_small, rel=0, abs=0, nan_ok=True)
    with torch.cuda.stream(s):
        got = rc.eval_image(*dev)
    assert got == pytest.approx(want_small, rel=0, abs=0, nan_ok=True)
    torch.cuda.current_stream().wait_stream(s)
    assert rc.eval_image(*big) == pytest.approx(want_big, rel=0, abs=0, nan_ok=True)
    assert ptrs == [_ws_ptr(rc, "ev:" + k) for k in ("post_pred", "post_gt", "part")]       # the smaller images reallocated nothing


def test_refusals_leave_the_handle_usable(rc):
    pred, gt = _images(12, 13, seed=10)
    hist = np.zeros((12, 13, 4, 3), np.float32)
    n3 = np.ones((12, 13, 3), np.float32)
    cases = [
        ("pred", lambda: rc.eval_image(None, gt), INVALID_ARG, "pred and gt"),
        ("gt", lambda: rc.eval_image(pred, None), INVALID_ARG, "pred and gt"),
        ("height", lambda: rc.eval_image(pred[:10], gt[:10]), INVALID_ARG, "window"),
        ("width", lambda: rc.eval_image(pred[:, :10].copy(), gt[:, :10].copy()), INVALID_ARG, "window"),
        ("clip_eval with bins", lambda: rc.eval_image(hist, hist, clip_eval=True), UNSUPPORTED, "clip_eval"),
        ("normals without normals_gt", lambda: rc.eval_image(pred, gt, normals=n3, acc=n3[..., 0].copy()), INVALID_ARG, "normals"),
        ("normals without acc", lambda: rc.eval_image(pred, gt, normals=n3, normals_gt=n3), INVALID_ARG, "normals"),
    ]
    want = rc.eval_image(pred, gt)
    for what, call, code, text in cases:
        with pytest.raises(rc_ext.RcError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (what, str(e.value))
        assert rc.eval_image(pred, gt) == pytest.approx(want, rel=0, abs=0, nan_ok=True), what
    with pytest.raises(ValueError):
        rc.eval_image(pred, gt[:, :12].copy())                       # the binding: gt of another size


# ---- end to end: render a camera of a DeviceDataset and score it ---------------------------------------------------------

def _lookat(origin):
    o = np.asarray(origin, np.float64)
    look = -o / np.linalg.norm(o)
    right = np.cross(look, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
    up = np.cross(right, look)
    return np.concatenate([np.stack([right, up, -look], axis=1), o[:, None]], axis=1)


def _two_cameras(H, W, radius):
    c2w = np.stack([_lookat(o) for o in radius * np.array([[0.0, -0.87, 0.5], [0.6, -0.6, 0.53]])])
    p2c = np.stack([nrc_amd.get_pixtocam(f, W, H) for f in (1.2 * W, 1.4 * W)])
    return p2c.astype(np.float32), c2w.astype(np.float32)


def test_evaluate_view_end_to_end():
    H, W = 24, 20
    cfg = nrc_amd.hotdog_config(render_chunk_size=128)               # 480 rays: three whole chunks and one of 96
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_np())
    p2c, c2w = _two_cameras(H, W, 4.0)
    blank = nrc_amd.DeviceDataset(m.rc, p2c, c2w, np.zeros((2, H, W, 3), np.float32), near=2.0, far=6.0)
    fn = M.bind_render_fn(M.create_render_fn(m))
    renders = []
    for c in range(2):
        rays = blank.generate_ray_batch(c).rays.tree_map(lambda t: t.cpu().numpy())
        renders.append(M.render_image(fn, None, rays, cfg, ("cache",), verbose=False)[0])
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    delta = (0.05 * np.sin(0.7 * xx + 0.4 * yy))[..., None] * np.array([1.0, -1.0, 0.5])     # a perturbation of amplitude 0.05
    images = np.stack([np.clip(r["rgb"] + delta, 0.0, None) for r in renders]).astype(np.float32)
    ds = nrc_amd.DeviceDataset(m.rc, p2c, c2w, images, near=2.0, far=6.0)
    img = renders[1]
    mask = _mask(H, W)
    r = _rng(31)
    depth = (img["distance_mean"] + r.normal(scale=0.1, size=(H, W))).astype(np.float32)
    ngt = r.normal(size=(H, W, 3))
    ngt = (ngt / np.linalg.norm(ngt, axis=-1, keepdims=True)).astype(np.float32)
    got = metrics.evaluate_view(m, ds, 1, masks=mask, depth=depth, normals=ngt, exposure=0.9)
    kw = dict(mask=mask, acc=img["acc"], normals=img["normals"], normals_gt=ngt, distance_mean=img["distance_mean"],
              distance_median=img["distance_median"], depth_gt=depth, exposure=0.9)
    r64, r32 = ref.both(img["rgb"], images[1], **kw)
    _scalars(got, r64, r32, "evaluate_view", keys=("mse", "psnr", "ssim", "l1_mean", "l1_median", "mae"))
    assert np.isnan(got["transient_iou"]) and got["rays_per_sec"] > 0
    assert 5.0 < got["psnr"] < 60.0                     # the perturbation is there, and it is small
    plain = metrics.evaluate_view(m, ds, 1)
    assert all(np.isnan(plain[k]) for k in ("transient_iou", "l1_mean", "l1_median", "mae")) and plain["mse"] > 0
    # MetricHarness on the post-processed tensors of the same view
    on_dev = m.rc.eval_image(img["rgb"], images[1], mask=mask, exposure=0.9, keep_images=True)
    h = metrics.MetricHarness(m.rc)(on_dev["post_pred"], on_dev["post_gt"], name_fn=lambda s: "test_" + s)
    assert set(h) == {"test_psnr", "test_ssim"}
    assert h["test_psnr"] == on_dev["psnr"] and h["test_ssim"] == on_dev["ssim"], (h, on_dev["psnr"], on_dev["ssim"])
    _scalars({"psnr": h["test_psnr"], "ssim": h["test_ssim"]}, r64, r32, "MetricHarness", keys=("psnr", "ssim"))
    assert set(metrics.MetricHarness(m.rc, disable_ssim=True)(on_dev["post_pred"], on_dev["post_gt"])) == {"psnr"}
    post = metrics.postprocess(m.rc, img["rgb"], exposure=0.9)
    assert torch.equal(post * torch.from_numpy(mask).cuda()[..., None], on_dev["post_pred"])


def test_evaluate_view_transient():
    H = W = 11
    cfg = nrc_amd.cornell_transient_config(render_chunk_size=64)     # 121 rays: one whole chunk and one of 57
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_transient_np())
    p2c, c2w = _two_cameras(H, W, 2.5)
    ds = nrc_amd.DeviceDataset(m.rc, p2c, c2w, np.zeros((2, H, W, 3), np.float32), near=0.7, far=4.0)
    rays = ds.generate_ray_batch(0).rays
    fields = {k: v.reshape(H * W, -1) for k, v in rays.hot_fields().items() if k != "lossmult"}
    # chunk by chunk, as render_image and evaluate_view render: a ray's direct light past the last bin lands in the next
    # ray of its batch, so the batch boundaries are part of the result
    parts = [m.rc.render_transient({k: v[i: i + 64] for k, v in fields.items()}, None, outputs=["rgb"])["rgb"].cpu().numpy()
             for i in range(0, H * W, 64)]
    rgb = np.concatenate(parts).reshape(H, W, 700, 3)
    gt = (rgb * _rng(41).uniform(0.5, 1.5, size=rgb.shape)).astype(np.float32)
    scale = float(rgb.sum(-2).max()) / 1.5               # some bin sums above img_scale: the clip is taken
    got = metrics.evaluate_view(m, ds, 0, gt=gt, img_scale=scale)
    r64, r32 = ref.both(rgb, gt, img_scale=scale)
    _scalars(got, r64, r32, "transient view", keys=("mse", "psnr", "ssim", "transient_iou"))
    assert 0.0 < got["transient_iou"] < 1.0
    with pytest.raises(ValueError, match="gt"):
        metrics.evaluate_view(m, ds, 0)
