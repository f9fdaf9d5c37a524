"""rc_probe_rays and rc_vmf_panorama on the GPU against the fp64 restatement (tests/probe_ref.py), the lobes read from the
handle against the oracle's light head, nrc_amd.probe.surface_probe's composition, and the argument checks.

Every float comparison is loss_cases.check: |got - fp64| <= 3 |fp32 restatement - fp64| + 1e-6 max|fp64|; both distances
are printed.  Eight-bit pictures follow test_gpu_vis._check_u8 with its 1 % budget per case."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import nrc_amd
import probe_ref as ref
from nrc_amd import camera, prng, probe, rc_ext
from nrc_amd import model as M
from oracle import material_ref, mathx

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
FLT_EPS = float(np.finfo(np.float32).eps)
VIEW_H, VIEW_W = 7, 9                                          # not square: a swapped x / y or H / W shows
CORNERS_AND_INTERIOR = [0, VIEW_W - 1, (VIEW_H - 1) * VIEW_W, VIEW_H * VIEW_W - 1, 3 * VIEW_W + 4]
PANORAMAS = [(1, 1), (3, 5), (8, 16), (5, 67)]                 # one ray; less than a wave; two waves; across a 256-thread block
BROADCAST = ("lights", "imageplane", "look", "up")
SENTINEL = -777.25


@pytest.fixture(scope="module")
def rc():
    return rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)   # the two calls need no weights


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- rc_probe_rays -------------------------------------------------------------------------------------------------------

def make_view(seed=3):
    r = _rng(seed)
    n = VIEW_H * VIEW_W
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    return dict(origins=f32(r.normal(size=(n, 3)) * 2.0), directions=f32(unit(r.normal(size=(n, 3))) * r.uniform(0.8, 1.3, (n, 1))),
                distance_median=f32(r.uniform(2.0, 6.0, n)), normals=f32(unit(r.normal(size=(n, 3)))),
                lights=f32(r.normal(size=(n, 3))), imageplane=f32(r.uniform(-0.5, 0.5, (n, 2))),
                look=f32(unit(r.normal(size=(n, 3)))), up=f32(unit(r.normal(size=(n, 3)))))


def probe_pixels(P):
    return (CORNERS_AND_INTERIOR * 4)[:P] if P != 1 else [CORNERS_AND_INTERIOR[-1]]


def call_probe_rays(rc, view, pixels, h, w, near, far, offset, flip, skip=(), positions=True):
    """rc_probe_rays through ctypes on sentinel-filled outputs -> (status, {field: tensor}, positions); `skip`: the members
    of rc_cast_outputs left NULL."""
    pix = np.ascontiguousarray(pixels, dtype=np.int64)
    P = pix.size
    v, held = rc_ext.rc_probe_view(), []
    for k in ("origins", "directions", "distance_median", "normals") + BROADCAST:
        if view.get(k) is not None:
            held.append(torch.from_numpy(view[k]).cuda())
            setattr(v, k, held[-1].data_ptr())
    v.n_view = VIEW_H * VIEW_W
    out, t = rc_ext.rc_cast_outputs(), {}
    for k, width in rc_ext.CAST_OUTPUTS:
        if k not in skip:
            t[k] = torch.full((max(P, 1) * max(h, 1) * max(w, 1), width), SENTINEL, device="cuda")
            setattr(out, k, t[k].data_ptr())
    pos = torch.full((max(P, 1), 3), SENTINEL, device="cuda") if positions else None
    code = rc.lib.rc_probe_rays(rc._h, C.byref(v), pix.ctypes.data_as(C.c_void_p), P, h, w, near, far, offset, int(flip),
                                C.byref(out), None if pos is None else pos.data_ptr(), rc._stream())
    torch.cuda.synchronize()
    return code, t, pos


def check_probe_rays(got, pos, view, pixels, h, w, near, far, offset, flip, what):
    r64, p64 = ref.probe_rays(view, pixels, h, w, near, far, offset, flip, np.float64)
    r32, p32 = ref.probe_rays(view, pixels, h, w, near, far, offset, flip, np.float32)
    for k, g in list(got.items()) + [("positions", pos)]:
        a64, a32 = (p64, p32) if k == "positions" else (r64[k], r32[k])
        g = g.cpu().numpy().astype(np.float64).reshape(a64.shape)
        print(f"{what} {k}: max|got - fp64| {np.abs(g - a64).max():.3e} max|fp32 - fp64| {np.abs(a32 - a64).max():.3e}")
        lc.check(g, a64, a32.astype(np.float64), f"{what} {k}")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("h,w", PANORAMAS)
@pytest.mark.parametrize("P", [1, 3, 16])
def test_probe_rays_against_fp64(rc, P, h, w, flip):
    view, pixels = make_view(), probe_pixels(P)
    code, got, pos = call_probe_rays(rc, view, pixels, h, w, 0.05, 2.0, 0.4, flip)
    assert code == 0, rc.lib.rc_last_error(rc._h)
    check_probe_rays(got, pos, view, pixels, h, w, 0.05, 2.0, 0.4, flip, f"P {P} {h}x{w} flip {flip}")
    assert _same_bits(got["directions"], got["viewdirs"])
    code, again, pos2 = call_probe_rays(rc, view, pixels, h, w, 0.05, 2.0, 0.4, flip)
    assert all(_same_bits(got[k], again[k]) for k in got) and _same_bits(pos, pos2)


def test_probe_rays_without_the_optional_view_arrays(rc):
    view = {k: v for k, v in make_view(5).items() if k not in BROADCAST}
    pixels, (h, w) = probe_pixels(3), (5, 67)
    code, got, pos = call_probe_rays(rc, view, pixels, h, w, 0.1, 3.0, 0.25, False)
    assert code == 0
    check_probe_rays(got, pos, view, pixels, h, w, 0.1, 3.0, 0.25, False, "no optional arrays")
    assert torch.equal(got["lights"], got["origins"])


def test_probe_rays_with_null_outputs(rc):
    view, pixels, (h, w) = make_view(), probe_pixels(3), (8, 16)
    code, full, pos = call_probe_rays(rc, view, pixels, h, w, 0.05, 2.0, 0.4, True)
    code2, part, none = call_probe_rays(rc, view, pixels, h, w, 0.05, 2.0, 0.4, True, skip=("viewdirs", "imageplane", "far"),
                                        positions=False)
    assert code == 0 and code2 == 0 and none is None and set(part) == set(full) - {"viewdirs", "imageplane", "far"}
    assert all(_same_bits(full[k], part[k]) for k in part)


def test_probe_radii_are_bitwise_the_panoramic_cast(rc):
    view, (h, w) = make_view(), (5, 67)
    code, got, pos = call_probe_rays(rc, view, probe_pixels(1), h, w, 0.05, 2.0, 0.4, False)
    assert code == 0
    c2w = np.concatenate([np.eye(3, dtype=np.float32), pos.cpu().numpy().reshape(3, 1)], axis=1)
    cast = camera.cast_spherical_rays(rc, c2w, h, w, 0.05, 2.0)
    assert _same_bits(cast.radii.reshape(-1, 1), got["radii"])
    assert _same_bits(cast.origins.reshape(-1, 3), got["origins"]) and _same_bits(cast.near.reshape(-1, 1), got["near"])
    assert not torch.equal(cast.directions.reshape(-1, 3), got["directions"])       # the reference's mismatch, kept
    # the binding's wrapper: the same rays, shaped [P, H, W, .]
    rays, positions = rc.probe_rays(view, probe_pixels(1), h, w, 0.05, 2.0)
    assert _same_bits(positions, pos) and tuple(rays.radii.shape) == (1, h, w, 1) and rays.cam_origins is None
    for k, width in rc_ext.CAST_OUTPUTS:
        assert _same_bits(getattr(rays, k).reshape(-1, width), got[k]), k


# ---- rc_vmf_panorama -----------------------------------------------------------------------------------------------------

KAPPAS = np.array([0.0, 1e-9, FLT_EPS, 2 * FLT_EPS, 0.3, 7.0, 50.0], np.float32)
LOGITS = np.array([-50.0, -3.0, 0.0, 12.0, 69.0, 75.0], np.float32)           # 75 is clipped at 70
VMF_CASES = [(V, h, w, P) for V in (1, 5, 128) for (h, w) in PANORAMAS[1:] for P in (1, 3)]


def make_lobes(P, V, seed):
    """Raw means of length in [0.2, 3], one lobe with a zero mean and one of length 1e-7 (for V = 1: in the second and the
    third mixture), kappas and logits drawn from the sets above."""
    r = _rng(seed)
    d = r.normal(size=(P, V, 3))
    means = d / np.linalg.norm(d, axis=-1, keepdims=True) * r.uniform(0.2, 3.0, (P, V, 1))
    if V >= 3:
        means[:, 1] = 0.0
        means[:, 2] = means[:, 2] / np.linalg.norm(means[:, 2], axis=-1, keepdims=True) * 1e-7
    elif P >= 3:
        means[1] = 0.0
        means[2] = means[2] / np.linalg.norm(means[2], axis=-1, keepdims=True) * 1e-7
    kappas = KAPPAS[r.integers(0, len(KAPPAS), (P, V))]
    logits = LOGITS[r.integers(0, len(LOGITS), (P, V))]
    return means.astype(np.float32), kappas, logits


def vmf_case(V, h, w, P):
    flip = (V + h + P) % 2 == 1
    return make_lobes(P, V, seed=1000 * V + 10 * h + P) + (flip,)


def check_vmf(got, means, kappas, logits, h, w, flip, what):
    """The three outputs of one call against the restatement; returns (close pixels, pixels) of the 8-bit budget."""
    from test_gpu_vis import _check_float, _check_u8
    lin64, s64 = ref.vmf_image(means, kappas, logits, h, w, flip, np.float64)
    lin32, s32 = ref.vmf_image(means, kappas, logits, h, w, flip, np.float32)
    assert np.isfinite(lin64).all() and np.isfinite(lin32).all()
    _check_float(got["linear"].cpu().numpy(), lin64, lin32, f"{what} linear")
    _, bound = _check_float(got["srgb"].cpu().numpy(), s64, s32, f"{what} srgb")
    budget = [0]
    u8 = got["u8"].cpu().numpy()
    assert u8.dtype == np.uint8 and u8.shape == s64.shape
    _check_u8(u8, s64, bound, f"{what} u8", budget)
    print(f"{what}: {budget[0]} of {u8.size} values may differ by one step")
    assert budget[0] <= 0.01 * u8.size, (what, budget[0], u8.size)


@pytest.mark.parametrize("V,h,w,P", VMF_CASES)
def test_vmf_panorama_against_fp64(rc, V, h, w, P):
    means, kappas, logits, flip = vmf_case(V, h, w, P)
    got = rc.vmf_panorama(means, kappas, logits, h, w, flip=flip, linear=True, srgb=True, u8=True)
    assert tuple(got["linear"].shape) == (P, h, w) and tuple(got["srgb"].shape) == (P, h, w, 3)
    check_vmf(got, means, kappas, logits, h, w, flip, f"V {V} {h}x{w} P {P} flip {flip}")
    # each output alone is bitwise what it is together with the others
    for k in ("linear", "srgb", "u8"):
        alone = rc.vmf_panorama(means, kappas, logits, h, w, flip=flip, **{"linear": False, "srgb": False, "u8": False, k: True})
        assert set(alone) == {k} and _same_bits(alone[k], got[k]), k


# ---- the lobes of a handle ------------------------------------------------------------------------------------------------

def test_light_lobes_against_the_oracle_light_head():
    cfg = nrc_amd.hotdog_config()
    m = M.Model(cfg, 0)
    w = common.weights_material_np()
    m.load_variables(w)
    n = 5
    rays, rnd = lc.material_case(n, seed=41)
    means, kappas, logits, normals = probe.light_lobes(m, rays, rnd)
    assert tuple(means.shape) == (n, 128, 3) and tuple(kappas.shape) == (n, 128) and tuple(logits.shape) == (n, 128)
    pts = m.rc.workspace("m_pts")[: 3 * n].reshape(n, 3)           # the shading points the device's head was evaluated at
    assert np.array_equal(normals.cpu().numpy(), m.rc.workspace("m_nrm")[: 3 * n].reshape(n, 3))
    refs = {}
    for dt in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
        o = material_ref.light_vmfs({k: t(v) for k, v in w.items() if "LightSampler" in k}, cfg, t(pts), t(rnd["vmf_noise"]))
        refs[dt] = (mathx.l2_normalize(o["vmf_means"]).double().numpy(), o["vmf_kappas"][..., 0].double().numpy(),
                    o["vmf_logits"][..., 0].double().numpy())
    for name, g, a64, a32 in zip(("means", "kappas", "logits"), (means, kappas, logits), refs[torch.float64], refs[torch.float32]):
        g = g.cpu().numpy().astype(np.float64)
        print(f"light_lobes {name}: max|got - fp64| {np.abs(g - a64).max():.3e} max|fp32 - fp64| {np.abs(a32 - a64).max():.3e}")
        lc.check(g, a64, a32, f"light_lobes {name}")
    # the panorama of these lobes against the restatement fed the same device values
    h, wd = 8, 16
    got = m.rc.vmf_panorama(means, kappas, logits, h, wd, linear=True, srgb=True, u8=True)
    check_vmf(got, means.cpu().numpy(), kappas.cpu().numpy(), logits.cpu().numpy(), h, wd, False, "lobes of the handle")


# ---- the whole block ------------------------------------------------------------------------------------------------------

H, W, HL, WL = 12, 16, 6, 12


def _camera():
    from test_gpu_eval_metrics import _two_cameras
    p2c, c2w = _two_cameras(H, W, 4.0)
    return nrc_amd.Camera(pixtocam=p2c[0], camtoworld=c2w[0], near=2.0, far=6.0)


def test_surface_probe_composition(tmp_path):
    cfg = nrc_amd.hotdog_config(render_chunk_size=30)            # 2 whole panorama rows per chunk: 3 chunks a panorama
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_material_np())
    cam = _camera()
    rendering = camera.render_camera(m, cam, H, W, to_host=False, keys=("rgb", "acc", "distance_median", "normals_to_use"))
    pixels = [probe.default_pixel(H, W), (0, 0), (W - 1, H - 1)]
    res = probe.surface_probe(m, cam, rendering, pixels, size=(HL, WL))
    assert set(res) == {"pixels", "positions", "secondary", "secondary_vis", "vmf"} and res["pixels"].tolist() == [[5, 7], [0, 0], [15, 11]]
    P = len(pixels)
    # the same rays through rc.probe_rays and ONE model.apply
    view = probe.probe_view(m, cam, rendering, pixels)
    rays, positions = m.rc.probe_rays(view, np.arange(P), HL, WL, cfg.secondary_near, cfg.secondary_far, 0.4)
    assert _same_bits(positions, res["positions"])
    n = P * HL * WL
    flat = {k: v.reshape((n,) + tuple(v.shape[3:])) for k, v in rays.hot_fields().items()}
    key, chunk, drawn = prng.PRNGKey(0), probe.probe_chunk(m, WL), []       # the chunks' random tensors, end to end
    assert chunk == 24
    for i0 in range(0, n, chunk):
        apply_key, key = prng.chunk_keys(key)
        drawn.append(probe.secondary_randoms(m, apply_key, min(chunk, n - i0)))
    randoms = {"jitter": [torch.cat([d["jitter"][lvl] for d in drawn]) for lvl in range(cfg.num_levels)],
               "gumbel": torch.cat([d["gumbel"] for d in drawn])}
    want = m.apply(None, randoms, flat, passes=("cache", "is_secondary"))["render"]
    assert {"rgb", "acc", "distance_median", "normals_to_use", "env_map_rgb", "cache_rgb"} <= set(res["secondary"])
    assert set(res["secondary"]) == set(want)
    for k, v in res["secondary"].items():
        assert tuple(v.shape[:3]) == (P, HL, WL), k
        assert _same_bits(v.reshape(want[k].shape), want[k].contiguous()), k
    # the hit point, from the view's own arrays on the host
    full = camera.cast_ray_batch(m.rc, cam, rect=(0, 0, W, H))
    x, y = pixels[0]
    hit = ref.position(full.origins[y, x].cpu().numpy(), full.directions[y, x].cpu().numpy(),
                       rendering["distance_median"][y, x].cpu().numpy(), rendering["normals_to_use"][y, x].cpu().numpy())
    assert np.abs(res["positions"][0].cpu().numpy() - hit).max() <= 1e-5
    assert len(res["secondary_vis"]) == P
    for pics in res["secondary_vis"]:
        assert {"acc", "color", "color_cache", "depth_median", "normals"} <= set(pics)
        for k, pic in pics.items():
            assert tuple(pic.shape) == (HL, WL, 3) and pic.dtype == torch.uint8, k
    assert tuple(res["vmf"].shape) == (P, HL, WL, 3) and res["vmf"].dtype == torch.uint8
    again = probe.surface_probe(m, cam, rendering, pixels, size=(HL, WL))
    assert _same_bits(again["vmf"], res["vmf"]) and _same_bits(again["positions"], res["positions"])
    assert all(_same_bits(again["secondary"][k], v) for k, v in res["secondary"].items())
    assert all(_same_bits(a[k], b[k]) for a, b in zip(again["secondary_vis"], res["secondary_vis"]) for k in b)
    # the default pixel and the default size of the view; no vMF panorama when it is not asked for
    one = probe.surface_probe(m, cam, rendering, vmf=False)
    assert "vmf" not in one and one["pixels"].tolist() == [[5, 7]] and tuple(one["secondary"]["rgb"].shape) == (1, 12, 32, 3)
    try:
        from PIL import Image
    except ImportError:
        return
    paths = probe.save_probe(res, str(tmp_path), 3, probe=1)
    assert paths["vmfs"].endswith(os.path.join("vmfs", "0003.png"))
    assert paths["color"].endswith(os.path.join("color", "secondary", "0003.png"))
    assert np.array_equal(np.asarray(Image.open(paths["vmfs"])), res["vmf"][1].cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(paths["color"])), res["secondary_vis"][1]["color"].cpu().numpy())


def test_surface_probe_refusals():
    cam = _camera()
    rendering = {"distance_median": torch.full((H, W), 3.0, device="cuda"),
                 "normals_to_use": torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(H, W, 3).contiguous()}
    bare = M.Model(nrc_amd.hotdog_config(), 0)
    bare.load_variables(common.weights_np())                     # cache-only weights: no light sampler
    with pytest.raises(ValueError, match="light sampler"):
        probe.surface_probe(bare, cam, rendering, size=(HL, WL))
    ok = probe.surface_probe(bare, cam, rendering, size=(HL, WL), vmf=False)       # the handle is usable afterwards
    assert tuple(ok["secondary"]["rgb"].shape) == (1, HL, WL, 3)
    tr = M.Model(nrc_amd.cornell_transient_config(), 0)
    tr.load_variables(common.weights_transient_np())
    with pytest.raises(NotImplementedError, match="time-resolved cache renders primary rays"):
        probe.surface_probe(tr, cam, rendering, size=(HL, WL))
    with pytest.raises(ValueError):
        probe.surface_probe(bare, cam, rendering, pixels=[(W, 0)], vmf=False)


# ---- argument checks ------------------------------------------------------------------------------------------------------

def test_probe_rays_refusals_leave_outputs_and_handle_alone(rc):
    view, (h, w) = make_view(), (3, 5)
    n = VIEW_H * VIEW_W
    good = dict(pixels=[4, 7], h=h, w=w)

    def attempt(what, view=view, pixels=good["pixels"], h=h, w=w, **kw):
        code, t, pos = call_probe_rays(rc, view, pixels, h, w, 0.05, 2.0, 0.4, False, **kw)
        assert code == INVALID_ARG, (what, code)
        assert all(bool((x == SENTINEL).all()) for x in t.values()) and (pos is None or bool((pos == SENTINEL).all())), what
        assert b"rc_probe_rays" in (rc.lib.rc_last_error(rc._h) or b""), what

    attempt("P = 0", pixels=[])
    attempt("P = 17", pixels=[0] * 17)
    attempt("pixel < 0", pixels=[3, -1])
    attempt("pixel = n_view", pixels=[n, 2])
    attempt("height", h=0)
    attempt("width", w=-3)
    for k in ("origins", "directions", "distance_median", "normals"):
        attempt(f"null {k}", view={**view, k: None})
    attempt("no output", skip=tuple(k for k, _ in rc_ext.CAST_OUTPUTS), positions=False)
    # 2^31 rays, a NULL view / pixel / out: nothing is read, so no arrays are needed
    v = rc_ext.rc_probe_view(n_view=1)
    dummy = torch.zeros(4, device="cuda")
    for k in ("origins", "directions", "distance_median", "normals"):
        setattr(v, k, dummy.data_ptr())
    out = rc_ext.rc_cast_outputs(radii=dummy.data_ptr())
    pix = np.zeros(16, np.int64)
    args = lambda view=C.byref(v), pixel=pix.ctypes.data_as(C.c_void_p), P=1, h=1, w=1, o=C.byref(out): (
        rc._h, view, pixel, P, h, w, 0.05, 2.0, 0.4, 0, o, None, rc._stream())
    assert rc.lib.rc_probe_rays(*args(P=16, h=2 ** 14, w=2 ** 13)) == INVALID_ARG
    assert rc.lib.rc_probe_rays(*args(view=None)) == INVALID_ARG
    assert rc.lib.rc_probe_rays(*args(pixel=None)) == INVALID_ARG
    assert rc.lib.rc_probe_rays(*args(o=None)) == INVALID_ARG
    assert rc.lib.rc_probe_rays(None, *args()[1:]) == INVALID_ARG                   # a NULL handle
    torch.cuda.synchronize()
    assert float(dummy.abs().max()) == 0.0
    code, got, pos = call_probe_rays(rc, view, good["pixels"], h, w, 0.05, 2.0, 0.4, False)      # the next good call
    assert code == 0
    check_probe_rays(got, pos, view, good["pixels"], h, w, 0.05, 2.0, 0.4, False, "after the refusals")


def test_vmf_panorama_refusals_leave_outputs_and_handle_alone(rc):
    h, w, P, V = 3, 5, 2, 5
    means, kappas, logits = (torch.from_numpy(a).cuda() for a in make_lobes(P, V, seed=9))
    outs = {"linear": torch.full((P, h, w), SENTINEL, device="cuda"), "srgb": torch.full((P, h, w, 3), SENTINEL, device="cuda"),
            "u8": torch.full((P, h, w, 3), 201, dtype=torch.uint8, device="cuda")}

    def call(m=means, k=kappas, l=logits, P=P, V=V, h=h, w=w, handle=True, wanted=("linear", "srgb", "u8")):
        ptr = lambda name: outs[name].data_ptr() if name in wanted else None
        return rc.lib.rc_vmf_panorama(rc._h if handle else None, None if m is None else m.data_ptr(),
                                      None if k is None else k.data_ptr(), None if l is None else l.data_ptr(), P, V, h, w, 0,
                                      ptr("linear"), ptr("srgb"), ptr("u8"), rc._stream())

    cases = [("P = 0", call(P=0)), ("P = 17", call(P=17)), ("V = 0", call(V=0)), ("V = 129", call(V=129)),
             ("height", call(h=0)), ("width", call(w=-1)), ("2^31", call(P=16, h=2 ** 14, w=2 ** 13)),
             ("null means", call(m=None)), ("null kappas", call(k=None)), ("null logits", call(l=None)),
             ("no output", call(wanted=())), ("null handle", call(handle=False))]
    for what, code in cases:
        assert code == INVALID_ARG, (what, code)
    torch.cuda.synchronize()
    assert bool((outs["linear"] == SENTINEL).all()) and bool((outs["srgb"] == SENTINEL).all()) and bool((outs["u8"] == 201).all())
    assert call(wanted=()) == INVALID_ARG
    msg = (rc.lib.rc_last_error(rc._h) or b"").decode()
    assert "rc_vmf_panorama" in msg and "no output" in msg, msg
    assert call() == 0                                                               # the next good call
    torch.cuda.synchronize()
    want = rc.vmf_panorama(means, kappas, logits, h, w, linear=True, srgb=True, u8=True)
    assert all(_same_bits(outs[k], want[k]) for k in outs)
    with pytest.raises(ValueError):
        rc.vmf_panorama(means, kappas[:, :4], logits, h, w)
    with pytest.raises(ValueError):
        rc.vmf_panorama(means, kappas, logits, h, w, srgb=False)
