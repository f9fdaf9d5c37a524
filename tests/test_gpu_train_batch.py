"""rc_cast_rays_multi / rc_train_batch on the GPU: one launch for a batch that mixes cameras is bitwise
the per-camera rc_cast_rays and agrees with the float64 oracle; the training batch's picks are the host mirror's, its
colours the numpy gather's, its rays those of the multi-camera cast; model._cast_pixels and the render function on top of
it give the bytes of the per-camera path; cache_stage_fit trains a student towards its teacher's images."""
import dataclasses

import numpy as np
import pytest
import torch

import common
import nrc_amd
import train_batch_ref as ref
from nrc_amd import data, prng, rc_ext, train
from nrc_amd import model as M
from nrc_amd.config import ExtraOptParams, OptimizerConfig
from oracle import camera_ref

pytestmark = pytest.mark.gpu

FIELDS = ("origins", "directions", "viewdirs", "radii", "imageplane", "look", "up", "lights", "near", "far")
DIST = dict(k1=0.05, k2=-0.01, k3=0.002, k4=0.0, p1=0.001, p2=-0.0015)
KEY = prng.split(prng.PRNGKey(20200823))[1]
NCAM = 7


def _lookat(origin):
    o = np.asarray(origin, np.float64)
    look = -o / np.linalg.norm(o)
    right = np.cross(look, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
    up = np.cross(right, look)
    return np.concatenate([np.stack([right, up, -look], axis=1), o[:, None]], axis=1)       # OpenGL: right, up, -look


def _cameras(count, H, W, seed=3, radius=4.0, ndc=False, steep=False):
    """count look-at cameras on the upper shell with their own focal lengths, and lights next to them.  steep: on a cap
    above the scene, so that every ray points well downwards."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(count, 3)); o[:, 2] = np.abs(o[:, 2]) + 0.3
    if steep:
        o[:, :2] *= 0.2; o[:, 2] = 1.0
    o = radius * o / np.linalg.norm(o, axis=1, keepdims=True)
    c2w = np.stack([_lookat(v) for v in o])
    if ndc:       # forward facing: the cameras look down -z from slightly different places
        c2w = np.stack([np.concatenate([np.eye(3), [[0.2 * i - 0.5], [-0.1 * i], [3.0 + 0.05 * i]]], axis=1) for i in range(count)])
    p2c = np.stack([nrc_amd.get_pixtocam(f, W, H) for f in np.linspace(0.9 * W, 1.4 * W, count)])
    lights = c2w[:, :, 3] + rng.normal(scale=0.1, size=(count, 3))
    return p2c.astype(np.float32), c2w.astype(np.float32), lights.astype(np.float32)


CASES = {
    "perspective": {}, "pano": dict(camtype="pano"), "fisheye": dict(camtype="fisheye"),
    "fisheye_equisolid": dict(camtype="fisheye_equisolid"), "distortion": dict(distortion_params=DIST),
    "ndc": dict(ndc=True), "distortion+ndc": dict(distortion_params=DIST, ndc=True), "z_range": dict(z_range=(-0.75, 1.25)),
    "jitter": dict(jitter=True), "jitter+z_range+distortion": dict(jitter=True, z_range=(-0.75, 1.25), distortion_params=DIST),
}


def _case(case, n=1500, H=30, W=44):
    kw = dict(CASES[case])
    ndc, jitter = kw.pop("ndc", False), kw.pop("jitter", False)
    # z_range divides by directions.z (t = (z_plane - origin.z) / directions.z): the crop amplifies the float32 rounding
    # of a ray by |d| / |d.z|, without bound for a ray along the planes.  The bound of tests/test_camera.py is for a
    # camera that looks down on the slab (|viewdirs.z| >= 0.4 there), so the z_range cases take such cameras too; the
    # oracle test asserts that precondition on its inputs.
    p2c, c2w, lights = _cameras(NCAM, H, W, ndc=ndc, steep="z_range" in kw)
    if kw.get("camtype") == "pano":
        p2c = np.stack([np.diag([2.0 * np.pi / W, np.pi / H, 1.0])] * NCAM).astype(np.float32)
    if ndc:
        kw["pixtocam_ndc"] = p2c[0]
    rng = np.random.default_rng(12)
    cam_idx = rng.permutation(np.arange(n) % NCAM).astype(np.int32)             # shuffled, every camera present
    px, py = rng.integers(0, W, n).astype(np.int32), rng.integers(0, H, n).astype(np.int32)
    jit = (rng.uniform(-0.5, 0.5, n).astype(np.float32), (rng.normal(size=n) * 0.5).astype(np.float32)) if jitter else None
    return p2c, c2w, lights, kw, cam_idx, px, py, jit


def _per_camera(rc, p2c, c2w, lights, kw, cam_idx, px, py, jit, near=0.0, far=1.0):
    """The launch-per-camera way: rc_cast_rays for the pixels of each camera, scattered back into the batch order."""
    out = {}
    for c in range(p2c.shape[0]):
        sel = np.nonzero(cam_idx == c)[0]
        if sel.size == 0:
            continue
        cam = nrc_amd.Camera(p2c[c], c2w[c], light=None if lights is None else lights[c], near=near, far=far, **kw)
        r = rc.cast_rays(cam, px[sel], py[sel], pix_jitter=None if jit is None else (jit[0][sel], jit[1][sel]))
        for k in FIELDS:
            v = getattr(r, k)
            out.setdefault(k, torch.empty((cam_idx.size, v.shape[-1]), dtype=v.dtype, device=v.device))[torch.from_numpy(sel).cuda()] = v
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_multi_camera_cast_is_bitwise_the_per_camera_cast(case):
    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    p2c, c2w, lights, kw, cam_idx, px, py, jit = _case(case)
    cams = rc.camera_set(p2c, c2w, lights, 0.0, 1.0, **kw)
    got = rc.cast_rays_multi(cams, cam_idx, px, py, pix_jitter=jit)
    want = _per_camera(rc, p2c, c2w, lights, kw, cam_idx, px, py, jit)
    torch.cuda.synchronize()
    for k in FIELDS:
        g = getattr(got, k)
        assert g.shape == want[k].shape and torch.equal(g.view(torch.int32), want[k].view(torch.int32)), (case, k)
    assert torch.equal(got.cam_idx[:, 0].cpu(), torch.from_numpy(cam_idx)) and got.lossmult.shape == (cam_idx.size, 1)
    # lights = NULL: the camera centres, as Camera(light=None)
    got0 = rc.cast_rays_multi(rc.camera_set(p2c, c2w, None, 0.0, 1.0, **kw), cam_idx, px, py, pix_jitter=jit)
    want0 = _per_camera(rc, p2c, c2w, None, kw, cam_idx, px, py, jit)
    assert torch.equal(got0.lights, want0["lights"]) and torch.equal(got0.origins.view(torch.int32), want0["origins"].view(torch.int32))
    # batch shape carried through, cuda index tensors used where they are
    sh = (3, 500)
    dev = lambda a: torch.from_numpy(a).cuda().reshape(sh)
    got2 = rc.cast_rays_multi(cams, dev(cam_idx), dev(px), dev(py), pix_jitter=None if jit is None else tuple(dev(j) for j in jit))
    assert got2.directions.shape == sh + (3,) and torch.equal(got2.directions.reshape(-1, 3), got.directions)
    assert torch.equal(got2.radii.reshape(-1, 1), got.radii)


@pytest.mark.parametrize("case", list(CASES))
def test_multi_camera_cast_matches_the_oracle_in_float64(case):
    """Per camera against oracle.camera_ref.cast_ray_batch in float64, at the bounds tests/test_camera.py holds
    rc_cast_rays to: 2e-6 of the field's scale for the plain pinhole, 4e-6 with distortion / fisheye / NDC / z_range /
    jitter, 2e-5 for the radii of NDC rays (differences of two NDC origins ~1 apart)."""
    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    p2c, c2w, lights, kw, cam_idx, px, py, jit = _case(case)
    got = rc.cast_rays_multi(rc.camera_set(p2c, c2w, lights, 0.0, 1.0, **kw), cam_idx, px, py, pix_jitter=jit)
    torch.cuda.synchronize()
    worst = {}
    for c in range(NCAM):
        sel = np.nonzero(cam_idx == c)[0]
        o = camera_ref.cast_ray_batch(p2c[c], c2w[c], lights[c], px[sel], py[sel], 0.0, 1.0, np.float64,
                                      camtype=kw.get("camtype", "perspective"), distortion_params=kw.get("distortion_params"),
                                      pixtocam_ndc=kw.get("pixtocam_ndc"), z_range=kw.get("z_range"),
                                      pix_jitter=None if jit is None else (jit[0][sel], jit[1][sel]))
        if "z_range" in kw:
            assert np.abs(o["viewdirs"][:, 2]).min() >= 0.4, (c, np.abs(o["viewdirs"][:, 2]).min())
        for k in FIELDS:
            g = getattr(got, k).cpu().numpy()[sel].astype(np.float64)
            assert g.shape == o[k].shape, k
            tol = 2e-6 if case == "perspective" else (2e-5 if ("ndc" in case and k == "radii") else 4e-6)
            err, scale = float(np.abs(g - o[k]).max()), max(1.0, float(np.abs(o[k]).max()))
            worst[k] = max(worst.get(k, 0.0), err / scale)
            assert err <= tol * scale, (case, c, k, err, scale)
    print(case, {k: f"{v:.2e}" for k, v in worst.items()})


def _images(count, H, W, dtype, seed=5):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (count, H, W, 3), dtype=np.uint8)
    return rng.uniform(size=(count, H, W, 3)).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("patch,border,batching,batch_size", [(1, 0, "all_images", 1024), (3, 2, "all_images", 1000),
                                                              (2, 1, "single_image", 512)])
def test_train_batch(dtype, patch, border, batching, batch_size):
    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    H, W = 30, 44
    p2c, c2w, lights = _cameras(NCAM, H, W)
    images = _images(NCAM, H, W, dtype)
    lm = np.linspace(0.25, 2.0, NCAM).astype(np.float32)
    ds = data.DeviceDataset(rc, p2c, c2w, images, lights, near=2.0, far=6.0, distortion_params=DIST, cam_lossmult=lm,
                            patch_size=patch, border=border, batching=batching, batch_size=batch_size)
    n = (batch_size // patch ** 2) * patch ** 2
    assert ds.batch_size == n
    b = ds.next_train(KEY)
    torch.cuda.synchronize()
    cam, xs, ys = ds.host_indices(KEY)
    want = ref.indices(KEY, n // patch ** 2, patch, border, H, W, NCAM, batching)
    for g, h_, w_ in zip((b.rays.cam_idx, b.rays.pix_x_int, b.rays.pix_y_int), (cam, xs, ys), want):
        assert g.dtype == torch.int32 and g.shape == (n, 1)
        assert np.array_equal(g.cpu().numpy()[:, 0], h_) and np.array_equal(h_, w_)
    if batching == "single_image":
        assert len(set(cam.tolist())) == 1
    else:
        assert len(set(cam.tolist())) == NCAM
    gather = ref.gather(images, cam, ys, xs)
    assert b.rgb.shape == (n, 3) and np.array_equal(b.rgb.cpu().numpy().view(np.int32), gather.view(np.int32))
    assert np.array_equal(b.rays.lossmult.cpu().numpy()[:, 0], lm[cam])
    # the rays are those of the multi-camera cast (and so of rc_cast_rays) for these picks
    rays = rc.cast_rays_multi(ds.cameras, cam, xs, ys)
    for k in FIELDS:
        assert torch.equal(getattr(b.rays, k).view(torch.int32), getattr(rays, k).view(torch.int32)), k
    assert float(b.rays.near.min()) == 2.0 == float(b.rays.near.max()) and float(b.rays.far.min()) == 6.0
    # a pure function of the key
    again = ds.next_train(KEY)
    for k in FIELDS + ("cam_idx", "pix_x_int", "pix_y_int", "lossmult"):
        assert torch.equal(getattr(again.rays, k), getattr(b.rays, k)), k
    assert torch.equal(again.rgb, b.rgb)
    other = ds.next_train(prng.split(KEY)[0])
    assert not torch.equal(other.rays.pix_x_int, b.rays.pix_x_int) and not torch.equal(other.rays.pix_y_int, b.rays.pix_y_int)
    # no lossmult table: ones; jitter offsets as arrays
    ds1 = data.DeviceDataset(rc, p2c, c2w, images, lights, near=2.0, far=6.0, distortion_params=DIST, patch_size=patch,
                             border=border, batching=batching, batch_size=batch_size)
    rng = np.random.default_rng(8)
    jit = (rng.uniform(-0.5, 0.5, n).astype(np.float32), rng.uniform(-0.5, 0.5, n).astype(np.float32))
    bj = ds1.next_train(KEY, pix_jitter=jit)
    assert float(bj.rays.lossmult.min()) == 1.0 == float(bj.rays.lossmult.max())
    rj = rc.cast_rays_multi(ds.cameras, cam, xs, ys, pix_jitter=jit)
    assert torch.equal(bj.rays.directions.view(torch.int32), rj.directions.view(torch.int32)) and torch.equal(bj.rgb, b.rgb)
    assert not torch.equal(bj.rays.directions, b.rays.directions)


def test_train_batch_errors_and_empty_batch():
    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    p2c, c2w, lights = _cameras(3, 8, 8)
    img = torch.from_numpy(_images(3, 8, 8, np.float32)).cuda()
    cams = rc.camera_set(p2c, c2w, lights, 2.0, 6.0)
    rays, rgb = rc.train_batch(cams, img, KEY, 0)
    assert rays.origins.shape == (0, 3) and rgb.shape == (0, 3)
    with pytest.raises(rc_ext.RcError, match="n must be P"):
        rc.train_batch(cams, img, KEY, 10, patch_size=2)
    with pytest.raises(rc_ext.RcError, match="no admissible patch position"):
        rc.train_batch(cams, img, KEY, 16, patch_size=1, border=4)
    with pytest.raises(ValueError):
        rc.train_batch(cams, img[:2], KEY, 16)
    full = data.DeviceDataset(rc, p2c, c2w, img, lights).generate_ray_batch(1)
    one = rc.cast_rays(nrc_amd.Camera(p2c[1], c2w[1], light=lights[1], near=2.0, far=6.0), rect=(0, 0, 8, 8))
    assert full.rays.origins.shape == (8, 8, 3) and torch.equal(full.rgb, img[1])
    for k in FIELDS:
        assert torch.equal(getattr(full.rays, k), getattr(one, k)), k
    torch.cuda.synchronize()


class _Dataset:
    camtype = "perspective"
    mesh = env_map = env_map_pmf = env_map_pdf = env_map_dirs = env_map_w = env_map_h = albedo_ratio = None


def test_cast_pixels_is_bitwise_the_per_camera_path():
    """model._cast_pixels on a 7-camera Pixels batch, host arrays and cuda tensors: every Rays field is bitwise what one
    rc_cast_rays per camera yields, and render_eval_pfn renders the same bytes from it."""
    cfg = nrc_amd.hotdog_config(render_chunk_size=256)
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_np())
    H = W = 24
    p2c, c2w, lights = _cameras(NCAM, H, W, radius=4.0)
    n = 700
    rng = np.random.default_rng(0)
    px, py = rng.integers(0, W, n).astype(np.int32), rng.integers(0, H, n).astype(np.int32)
    cam_idx = rng.permutation(np.arange(n) % NCAM).astype(np.int32)
    col = lambda v, dt=np.float32: np.full((1, n, 1), v, dt)
    pixels = nrc_amd.Pixels(pix_x_int=px[None], pix_y_int=py[None], lossmult=col(1.0), near=col(2.0), far=col(6.0),
                            cam_idx=cam_idx[None, :, None], light_idx=col(0, np.int32))
    cameras = (p2c[None], c2w[None], DIST, None, None)                    # replicated: leading device axis
    want = _per_camera(m.rc, p2c, c2w, lights, dict(distortion_params=DIST), cam_idx, px, py, None)
    on_dev = pixels.tree_map(lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    for pix in (pixels, on_dev):
        rays = M._cast_pixels(m, cameras, lights[None], pix, "perspective")
        for k in FIELDS:
            if k not in ("near", "far"):
                g = getattr(rays, k)
                assert g.shape == (1, n, want[k].shape[-1]) and torch.equal(g[0].view(torch.int32), want[k].view(torch.int32)), k
        assert float(rays.near.min()) == 2.0 and float(rays.far.max()) == 6.0
        assert torch.equal(rays.cam_idx[0, :, 0].cpu(), torch.from_numpy(cam_idx)) and rays.cam_idx.dtype == torch.int32
    pfn = M.create_render_fn(m, _Dataset())
    out, _ = pfn(None, None, 1.0, cameras, lights[None], pixels, ("cache",), None)
    out_dev, _ = pfn(None, None, 1.0, cameras, lights[None], on_dev, ("cache",), None)
    fields = {k: want[k] for k in ("origins", "directions", "viewdirs", "lights")}
    fields.update(near=torch.full((n, 1), 2.0).cuda(), far=torch.full((n, 1), 6.0).cuda(), lossmult=torch.ones(n, 1).cuda())
    rays_ref = nrc_amd.synthetic_rays(n).tree_map(lambda a: torch.from_numpy(np.asarray(a)).cuda()).replace(
        **fields, radii=want["radii"], imageplane=want["imageplane"], look=want["look"], up=want["up"], cam_origins=want["origins"])
    ref_img = m.apply(None, None, rays_ref)["render"]
    for k in ("rgb", "acc"):
        assert torch.equal(out[k][0, 0], ref_img[k]) and torch.equal(out_dev[k][0, 0], ref_img[k]), k
    # one camera for the whole batch: the single-camera branch
    one = dataclasses.replace(pixels, cam_idx=np.full((1, n, 1), 4, np.int32))
    r1 = M._cast_pixels(m, cameras, lights[None], one, "perspective")
    w1 = _per_camera(m.rc, p2c, c2w, lights, dict(distortion_params=DIST), np.full(n, 4, np.int32), px, py, None)
    assert torch.equal(r1.directions[0], w1["directions"]) and torch.equal(r1.lights[0], w1["lights"])
    with pytest.raises(IndexError):
        M._cast_pixels(m, cameras, lights[None], dataclasses.replace(pixels, cam_idx=(cam_idx[None, :, None] + 1)), "perspective")


# The criterion of tests/test_gpu_data_loss.py's Adam loop (LOOP_LR, LOOP_STEPS, LOOP_DROP = 1e-3, 40, 0.5): 40 steps of
# Adam at 1e-3 must halve the data loss.  The optimizer runs from count 0, so the schedule is that constant rate without
# the reference's 2500-step delay (whose first steps are 1e-8 of the rate and move nothing in 40 steps).
FIT_LR, FIT_STEPS, FIT_DROP = 1e-3, 40, 0.5


def test_cache_stage_fit_lowers_the_data_loss():
    """Teacher-student: four 32 x 32 cameras rendered by the handle's own weights (render_camera) are the data set; the
    student starts from the same density fields with the shader side of another seed; the data loss on ONE held-out
    batch, evaluated before and after cache_stage_fit, halves."""
    cfg = nrc_amd.hotdog_config()
    teacher = M.Model(cfg, 0)
    w_teacher = common.weights_np()
    teacher.load_variables(w_teacher)
    H = W = 32
    p2c, c2w, _ = _cameras(4, H, W, seed=9, radius=4.03)
    images = torch.stack([nrc_amd.render_camera(teacher, nrc_amd.Camera(p2c[c], c2w[c], near=2.0, far=6.0), H, W, keys=("rgb",),
                                                to_host=False)["rgb"] for c in range(4)])
    assert images.shape == (4, H, W, 3) and float(images.std()) > 1e-3
    rc = common.make_rc()
    shader = {name for name, _, _ in rc.shader_grad_layout()[0]}
    w_other = common.weights_np(seed=2)
    w_student = {k: (w_other[k] if k in shader else v) for k, v in w_teacher.items()}
    ocfg = OptimizerConfig(lr_init=FIT_LR, lr_final=FIT_LR, lr_delay_steps=0,
                           extra_opt_params=(ExtraOptParams("Cache", FIT_LR, FIT_LR, 0, FIT_LR, FIT_LR, 0),))
    opt = train.CacheStageOptimizer(rc, ocfg)
    opt.init_from(w_student)
    ds = data.DeviceDataset(rc, p2c, c2w, images, near=2.0, far=6.0, batch_size=1024)
    k_fit, k_held = prng.split(prng.PRNGKey(17))
    held = ds.next_train(k_held)
    held_jit = [rc.prng_fill(k, (ds.batch_size, 1), "uniform") for k in prng.split(k_held, 3)]

    def held_loss():
        _, loss = rc.data_backward(held.rays.hot_fields(), held.rgb, held_jit, train.anneal_at(1.0), grads=False)
        return float(loss)

    before = held_loss()
    history = train.cache_stage_fit(rc, opt, ds, k_fit, FIT_STEPS)
    after = held_loss()
    per_step = [float(h["data"]) for h in history]
    print("cache_stage_fit: held-out data loss", before, "->", after, "; per-step data loss", [round(v, 5) for v in per_step])
    assert opt.count == FIT_STEPS and len(history) == FIT_STEPS
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for h in history for v in h.values())
    assert np.isfinite(per_step).all() and np.isfinite([before, after]).all()
    assert after < FIT_DROP * before, (before, after)
    # the same key replays the same run
    opt2 = train.CacheStageOptimizer(rc, ocfg)
    opt2.init_from(w_student)
    again = train.cache_stage_fit(rc, opt2, ds, k_fit, 2)
    assert float(again[0]["data"]) == pytest.approx(per_step[0], rel=1e-5)
