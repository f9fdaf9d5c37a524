"""The training batch's index rule, patch layout and gather, restated in plain Python integers and numpy (DESIGN.md
§4.14): what nrc_amd.data.patch_indices and the k_train_batch kernel are checked against.  Nothing here is shared with the
product but prng.random_bits (pinned by tests/test_prng.py) and prng.threefry2x32."""
import numpy as np

from nrc_amd import prng


def words(key, num_patches):
    """Three 32-bit words per patch: random_bits(key, (P, 3)), row q = (w_cam, w_x, w_y) of patch q."""
    return prng.random_bits(key, (3 * int(num_patches),)).reshape(int(num_patches), 3)


def bits_at(key, e, n):
    """Element e of random_bits(key, (n,)) computed alone, the way a kernel lane does it: the counters iota(n) are cut in
    two halves, block i = (i, i + half), an odd n is padded with a zero counter."""
    half = (n + 1) // 2
    i = e if e < half else e - half
    x0, x1 = prng.threefry2x32(key, [i], [i + half if i + half < n else 0])
    return int(x0[0] if e < half else x1[0])


def map_word(w, lo, hi):
    """A word to [lo, hi): lo + floor(w (hi - lo) / 2^32) in exact integers."""
    return int(lo) + (int(w) * (int(hi) - int(lo))) // (1 << 32)


def indices(key, num_patches, patch_size, border, height, width, num_cameras, batching="all_images"):
    """(cam_idx, pix_x, pix_y) int32 [P p^2]: ranges of Dataset._next_train (x in [border, W - border - p + 1), y likewise,
    the camera in [0, C) per patch, or ONE camera from the first word), patch offsets in row-major order."""
    w = words(key, num_patches)
    p = int(patch_size)
    cam, xs, ys = [], [], []
    for q in range(int(num_patches)):
        c = map_word(w[0, 0] if batching == "single_image" else w[q, 0], 0, num_cameras)
        x0 = map_word(w[q, 1], border, width - border - p + 1)
        y0 = map_word(w[q, 2], border, height - border - p + 1)
        for row in range(p):
            for col in range(p):
                cam.append(c)
                xs.append(x0 + col)
                ys.append(y0 + row)
    return np.asarray(cam, np.int32), np.asarray(xs, np.int32), np.asarray(ys, np.int32)


def gather(images, cam, ys, xs):
    """images[cam, y, x, 0:3] as float32; uint8 is float32(u) / float32(255) (one IEEE division)."""
    px = np.asarray(images)[cam, ys, xs]
    if px.dtype == np.uint8:
        return px.astype(np.float32) / np.float32(255.0)
    return px.astype(np.float32)
