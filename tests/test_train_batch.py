"""rc_train_batch / rc_cast_rays_multi without a GPU: the index rule's known answers, the numpy mirror
against the restatement of tests/train_batch_ref.py, the struct layouts against a C compiler, and the argument checks,
which both calls make before they look at the handle."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import train_batch_ref as ref
from nrc_amd import data, prng, rc_ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RC_ERR_INVALID_ARG = -1
KEY = prng.split(prng.PRNGKey(20200823))[1]
LAST = 2 ** 32 - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return rc_ext.load_library()


@pytest.mark.parametrize("lo,hi", [(0, 1), (0, 100), (0, 800), (3, 790), (7, 8), (0, 2 ** 31 - 1)])
def test_first_and_last_word_hit_the_ends_of_the_range(lo, hi):
    assert ref.map_word(0, lo, hi) == lo and ref.map_word(LAST, lo, hi) == hi - 1
    got = data.pick(np.array([0, LAST, 1 << 31], np.uint32), lo, hi - lo)
    assert got.dtype == np.int32 and got[0] == lo and got[1] == hi - 1 and got[2] == lo + (hi - lo) // 2
    w = np.random.default_rng(1).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    m = data.pick(w, lo, hi - lo)
    assert m.min() >= lo and m.max() < hi
    assert np.array_equal(m, [ref.map_word(v, lo, hi) for v in w])
    assert np.all(np.diff(data.pick(np.sort(w), lo, hi - lo)) >= 0)           # monotone in the word


def test_border_and_patch_ranges():
    """x in [border, W - border - p + 1): the patch's last column W - border - 1 stays inside the unmasked image."""
    H, W, p, border = 20, 30, 4, 3
    lo_x, hi_x, lo_y, hi_y = border, W - border - p + 1, border, H - border - p + 1
    assert (ref.map_word(0, lo_x, hi_x), ref.map_word(LAST, lo_x, hi_x)) == (3, 23)
    assert (ref.map_word(0, lo_y, hi_y), ref.map_word(LAST, lo_y, hi_y)) == (3, 13)
    cam, xs, ys = data.patch_indices(KEY, 500, p, border, H, W, 9)
    assert xs.min() >= border and xs.max() <= W - border - 1 and ys.min() >= border and ys.max() <= H - border - 1
    assert cam.min() >= 0 and cam.max() <= 8 and len(set(cam.tolist())) == 9
    # the only admissible position
    cam, xs, ys = data.patch_indices(KEY, 5, 4, 3, 10, 10, 1)
    assert np.all(cam == 0) and np.array_equal(xs[:16].reshape(4, 4), np.tile(np.arange(3, 7), (4, 1)))
    with pytest.raises(ValueError):
        data.patch_indices(KEY, 5, 4, 4, 10, 10, 1)            # 10 - 8 - 4 + 1 < 1
    with pytest.raises(ValueError):
        data.patch_indices(KEY, 5, 1, 0, 10, 10, 0)


def test_patch_pixels_are_the_block_in_row_major_order():
    p = 3
    cam, xs, ys = data.patch_indices(KEY, 11, p, 1, 17, 19, 5)
    assert cam.shape == xs.shape == ys.shape == (11 * p * p,)
    for q in range(11):
        bx, by, bc = (a[q * p * p:(q + 1) * p * p].reshape(p, p) for a in (xs, ys, cam))
        dx, dy = np.meshgrid(np.arange(p), np.arange(p), indexing="xy")       # camera_utils.pixel_coordinates(p, p)
        assert np.array_equal(bx, bx[0, 0] + dx) and np.array_equal(by, by[0, 0] + dy)
        assert np.all(bc == bc[0, 0])


def test_single_image_uses_one_camera():
    cam, xs, ys = data.patch_indices(KEY, 64, 2, 0, 16, 16, 100, "single_image")
    cam_all, xs_all, ys_all = data.patch_indices(KEY, 64, 2, 0, 16, 16, 100, "all_images")
    assert np.all(cam == cam_all[0]) and len(set(cam_all.tolist())) > 20
    assert np.array_equal(xs, xs_all) and np.array_equal(ys, ys_all)
    with pytest.raises(ValueError):
        data.patch_indices(KEY, 4, 1, 0, 8, 8, 2, "some_images")


@pytest.mark.parametrize("P,p,border,H,W,Cn,batching", [
    (1024, 1, 0, 800, 800, 100, "all_images"), (37, 2, 1, 9, 13, 7, "all_images"), (5, 4, 0, 4, 4, 3, "single_image"),
    (33, 1, 2, 32, 32, 4, "single_image"), (1, 1, 0, 1, 1, 1, "all_images"), (0, 1, 0, 8, 8, 2, "all_images")])
def test_host_indices_equal_the_restatement(P, p, border, H, W, Cn, batching):
    want = ref.indices(KEY, P, p, border, H, W, Cn, batching)
    got = data.patch_indices(KEY, P, p, border, H, W, Cn, batching)
    for g, w_ in zip(got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w_)
    ds = types.SimpleNamespace(num_patches=P, patch_size=p, border=border, height=H, width=W, batching=batching,
                               cameras=types.SimpleNamespace(count=Cn))
    for g, w_ in zip(data.DeviceDataset.host_indices(ds, KEY), want):
        assert np.array_equal(g, w_)
    other = data.patch_indices(prng.split(KEY)[0], P, p, border, H, W, Cn, batching)
    if P >= 33:
        assert not np.array_equal(other[1], got[1])


def test_words_are_prngs_bits():
    """The words are prng.random_bits(key, (P, 3)); a lane's own evaluation of one element gives the same word."""
    for P in (1, 2, 5, 1024):
        w = ref.words(KEY, P)
        assert w.dtype == np.uint32 and np.array_equal(w, prng.random_bits(KEY, (P, 3)))
        n = 3 * P
        for e in sorted({0, 1, 2, n // 2, (n + 1) // 2, max(0, (n + 1) // 2 - 1), n - 1}):
            assert ref.bits_at(KEY, e, n) == int(w.reshape(-1)[e]), (P, e)


def test_gather_restatement():
    rng = np.random.default_rng(3)
    img8 = rng.integers(0, 256, (3, 5, 6, 3), dtype=np.uint8)
    cam, ys, xs = np.array([0, 2, 1]), np.array([4, 0, 2]), np.array([5, 1, 3])
    g = ref.gather(img8, cam, ys, xs)
    assert g.dtype == np.float32 and g.shape == (3, 3)
    assert np.array_equal(g[1], np.float32(img8[2, 0, 1]) / np.float32(255))
    assert ref.gather(np.full((1, 1, 1, 3), 255, np.uint8), [0], [0], [0]).max() == 1.0
    imgf = rng.uniform(size=(3, 5, 6, 3)).astype(np.float32)
    assert np.array_equal(ref.gather(imgf, cam, ys, xs)[2], imgf[1, 2, 3])


def test_struct_layouts_match_c():
    """rc_camera_set and rc_train_batch_outputs as a C compiler lays them out == the ctypes mirrors."""
    fields_set = [n for n, _ in rc_ext.rc_camera_set._fields_]
    fields_out = [n for n, _ in rc_ext.rc_train_batch_outputs._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "rc_abi.h"\nint main(void) {\n'
            '  printf("%zu %zu %zu %d %d %d %d\\n", sizeof(rc_camera_set), sizeof(rc_train_batch_outputs), sizeof(rc_cast_outputs),\n'
            '         (int)RC_IMAGE_F32, (int)RC_IMAGE_U8, (int)RC_BATCHING_ALL_IMAGES, (int)RC_BATCHING_SINGLE_IMAGE);\n'
            + "".join(f'  printf("%zu\\n", offsetof(rc_camera_set, {f}));\n' for f in fields_set)
            + "".join(f'  printf("%zu\\n", offsetof(rc_train_batch_outputs, {f}));\n' for f in fields_out)
            + '  return 0;\n}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [C.sizeof(rc_ext.rc_camera_set), C.sizeof(rc_ext.rc_train_batch_outputs), C.sizeof(rc_ext.rc_cast_outputs)]
    assert out[3:7] == [rc_ext.RC_IMAGE_F32, rc_ext.RC_IMAGE_U8, rc_ext.BATCHING["all_images"], rc_ext.BATCHING["single_image"]]
    offs = out[7:]
    assert offs[:len(fields_set)] == [getattr(rc_ext.rc_camera_set, f).offset for f in fields_set]
    assert offs[len(fields_set):] == [getattr(rc_ext.rc_train_batch_outputs, f).offset for f in fields_out]
    assert fields_out[0] == "rays" and [n for n, _ in rc_ext.rc_cast_outputs._fields_] == [k for k, _ in rc_ext.CAST_OUTPUTS]


def test_symbols_are_exported_and_bound(lib):
    for name in ("rc_cast_rays_multi", "rc_train_batch"):
        assert hasattr(lib, name) and name in rc_ext.EXPORTS
        assert getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) in (10, 14)
    assert lib.rc_abi_version() == rc_ext.RC_ABI_VERSION == 5
    for name in ("camera_set", "cast_rays_multi", "train_batch"):
        assert callable(getattr(rc_ext.RadianceCache, name))


def _set(count=2, tables=True, **kw):
    s = rc_ext.rc_camera_set()
    s.count = count
    if tables:
        s.pixtocams, s.camtoworlds = 0x1000, 0x2000          # never dereferenced: every call below fails before a launch
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_train_batch_argument_checks_need_no_device(lib):
    """Every malformed call comes back as RC_ERR_INVALID_ARG with its reason in rc_last_error, handle or no handle; a
    well-formed call without a handle is refused for the handle alone."""
    key = (C.c_uint32 * 2)(1, 2)
    out = rc_ext.rc_train_batch_outputs()
    img = 0x3000

    def call(s=None, images=img, dtype=0, H=8, W=8, key_=key, p=2, border=1, batching=0, n=16, out_=out):
        s = _set() if s is None else s
        code = lib.rc_train_batch(None, C.byref(s) if s is not False else None, images, dtype, H, W, None, key_, p, border,
                                  batching, n, C.byref(out_) if out_ is not None else None, None)
        return code, (lib.rc_last_error(None) or b"").decode()

    cases = {
        "n must be P": dict(n=15),
        "negative n": dict(n=-4),
        "count must be at least 1": dict(s=_set(count=0)),
        "pixtocams / camtoworlds are NULL": dict(s=_set(tables=False)),
        "no admissible patch position": dict(W=5, border=2, p=2),                  # 5 - 4 - 2 + 1 = 0
        "no admissible patch position ": dict(H=3, border=0, p=4, n=16),
        "images is NULL": dict(images=None),
        "null key": dict(key_=None),
        "null camera set/outputs": dict(s=False),
        "null camera set/outputs ": dict(out_=None),
        "image_dtype": dict(dtype=2),
        "unknown batching": dict(batching=2),
        "must be positive": dict(p=0),
        "must be positive ": dict(border=-1),
        "camtype": dict(s=_set(camtype=4)),
        "pixtocam_ndc": dict(s=_set(has_ndc=1)),
        "pix_dx and pix_dy go together": dict(s=_set(pix_dx=0x4000)),
    }
    for msg, kw in cases.items():
        code, text = call(**kw)
        assert code == RC_ERR_INVALID_ARG and msg.strip() in text and text.startswith("rc_train_batch:"), (msg, code, text)
    for kw in (dict(), dict(n=0), dict(W=6, border=2, p=2, n=4), dict(dtype=1, batching=1)):
        code, text = call(**kw)
        assert code == RC_ERR_INVALID_ARG and text == "rc_train_batch: null handle", (kw, code, text)


def test_cast_rays_multi_argument_checks_need_no_device(lib):
    out = rc_ext.rc_cast_outputs()
    idx = 0x5000

    def call(s=None, cam=idx, px=idx, py=idx, n=4, dx=None, dy=None, out_=out):
        s = _set() if s is None else s
        code = lib.rc_cast_rays_multi(None, C.byref(s) if s is not False else None, cam, px, py, n, dx, dy,
                                      C.byref(out_) if out_ is not None else None, None)
        return code, (lib.rc_last_error(None) or b"").decode()

    cases = {
        "null camera set/outputs": dict(s=False),
        "null camera set/outputs ": dict(out_=None),
        "negative n": dict(n=-1),
        "count must be at least 1": dict(s=_set(count=-3)),
        "pixtocams / camtoworlds are NULL": dict(s=_set(tables=False)),
        "cam_idx, pix_x and pix_y are required": dict(cam=None),
        "cam_idx, pix_x and pix_y are required ": dict(py=None),
        "pix_dx and pix_dy go together": dict(dx=idx),
        "camtype": dict(s=_set(camtype=-1)),
    }
    for msg, kw in cases.items():
        code, text = call(**kw)
        assert code == RC_ERR_INVALID_ARG and msg.strip() in text and text.startswith("rc_cast_rays_multi:"), (msg, code, text)
    for kw in (dict(), dict(n=0, cam=None, px=None, py=None), dict(dx=idx, dy=idx)):
        code, text = call(**kw)
        assert code == RC_ERR_INVALID_ARG and text == "rc_cast_rays_multi: null handle", (kw, code, text)
