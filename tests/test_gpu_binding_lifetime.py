"""The binding owns the device copies of host-side inputs while the kernels run.

Every entry point enqueues asynchronously and returns; inputs given as numpy arrays are copied to the device by the
binding, and those copies have no other owner than the binding's `held` / `_keep`.  Each case runs a method once with
cuda tensors the test holds, then with the same values as numpy arrays, allocates and fills scratch tensors of the same
sizes before synchronising (a copy released too early goes back to torch's caching allocator and is handed out again),
and requires bitwise-equal results.

One part of the results cannot be bitwise: the hash-grid table segments of a gradient buffer are accumulated with float
atomics, so two identical calls already differ there in the last bits (64 rays, identical cuda inputs, four calls each:
288 to 616 of 1.9 M / 2.4 M entries per interlevel buffer, 2140 to 2796 of 11.7 M per data-loss buffer).  Those entries
are held to the bound tests/test_gpu_interlevel.py::test_semantics holds them to between two calls (rtol 1e-5, atol 1e-6
of the buffer's largest entry); the losses and the dense layers' segments, which every input feeds, are bitwise."""
import numpy as np
import pytest
import torch

import common
import nrc_amd

pytestmark = pytest.mark.gpu

N = 64
INT_KEYS = ("vmf_lobe", "resample_inds", "cam_idx", "pix_x_int", "pix_y_int")


@pytest.fixture(scope="module")
def rc():
    return common.make_rc(weights=common.weights_material_np(False))


def _to_cuda(x, key=None):
    """numpy arrays (and lists / tuples / dicts of them) as cuda tensors of the dtype the binding passes on."""
    if isinstance(x, dict):
        return {k: _to_cuda(v, k) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_cuda(v, key) for v in x)
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x, np.int32 if key in INT_KEYS else np.float32)).cuda()
    return x


def _arrays(x):
    if isinstance(x, dict):
        return [a for v in x.values() for a in _arrays(v)]
    if isinstance(x, (list, tuple)):
        return [a for v in x for a in _arrays(v)]
    return [x] if isinstance(x, np.ndarray) else []


def _tensors(x):
    """The cuda tensors of a method's result (dicts, tuples, Rays), in a fixed order."""
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in _tensors(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _tensors(v)]
    if hasattr(x, "__dataclass_fields__"):
        return [t for k in sorted(x.__dataclass_fields__) for t in _tensors(getattr(x, k))]
    return []


def _rays(seed):
    return {k: np.ascontiguousarray(v, np.float32) for k, v in nrc_amd.synthetic_rays(N, seed=seed).hot_fields().items()
            if v is not None}


def _case_render_rays(rc):
    inputs = dict(rays=_rays(11), randoms={"jitter": common.jitters(N, seed=3)})
    return inputs, lambda a: rc.render_rays(a["rays"], a["randoms"], outputs=["rgb", "acc", "distance_median", "normals_pred"]), None


def _case_interlevel(rc):
    inputs = dict(rays=_rays(12), jitters=common.jitters(N, seed=4),
                  lossmult=np.random.default_rng(1).uniform(0.5, 1.5, N).astype(np.float32))
    return inputs, lambda a: rc.interlevel_backward(a["rays"], a["jitters"], lossmult=a["lossmult"]), [0, 1, None]


def _case_data(rc):
    rng = np.random.default_rng(2)
    inputs = dict(rays=_rays(13), rgb=rng.uniform(size=(N, 3)).astype(np.float32), jitters=common.jitters(N, seed=5),
                  lossmult=rng.uniform(0.5, 1.5, N).astype(np.float32))
    call = lambda a: rc.data_backward(a["rays"], a["rgb"], a["jitters"], lossmult=a["lossmult"])
    return inputs, call, [rc.cfg.num_levels - 1, "shader", None]


def _case_material(rc):
    from oracle import material_ref
    inputs = dict(rays=_rays(14), randoms=material_ref.draw_randoms(rc.cfg, N, seed=6))
    return inputs, lambda a: rc.render_material(a["rays"], a["randoms"]), None


def _case_cast_multi(rc):
    rng = np.random.default_rng(7)
    count, H, W = 3, 12, 16
    c2w = np.stack([np.concatenate([np.eye(3), [[0.2 * i], [-0.1 * i], [3.0 + 0.1 * i]]], axis=1) for i in range(count)])
    p2c = np.stack([nrc_amd.get_pixtocam(f, W, H) for f in (15.0, 18.0, 21.0)])
    cams = rc.camera_set(p2c.astype(np.float32), c2w.astype(np.float32), None, 0.1, 4.0)
    inputs = dict(cam_idx=rng.integers(0, count, N).astype(np.int32), pix_x_int=rng.integers(0, W, N).astype(np.int32),
                  pix_y_int=rng.integers(0, H, N).astype(np.int32),
                  pix_jitter=(rng.uniform(-0.5, 0.5, N).astype(np.float32), rng.uniform(-0.5, 0.5, N).astype(np.float32)))
    call = lambda a: rc.cast_rays_multi(cams, a["cam_idx"], a["pix_x_int"], a["pix_y_int"], pix_jitter=a["pix_jitter"])
    return inputs, call, None


CASES = {"render_rays": _case_render_rays, "interlevel_backward": _case_interlevel, "data_backward": _case_data,
         "render_material": _case_material, "cast_rays_multi": _case_cast_multi}


def _table_mask(rc, key, like):
    """True on the hash-grid table segments of gradient layout `key` (everything but the dense layers' kernel / bias)."""
    mask = torch.ones_like(like, dtype=torch.bool)
    for name, off, shape in rc._grad_layout(key)[0]:
        if name.endswith(("/kernel", "/bias")):
            mask[off: off + int(np.prod(shape))] = False
    return mask


@pytest.mark.parametrize("method", list(CASES))
def test_host_inputs_stay_alive_until_the_kernels_ran(rc, method):
    """Each case: (inputs as numpy, the call, per result tensor the gradient layout it is laid out in or None)."""
    inputs, call, layouts = CASES[method](rc)
    held_by_test = _to_cuda(inputs)
    want = [t.clone() for t in _tensors(call(held_by_test))]
    torch.cuda.synchronize()
    got = call(inputs)                                  # numpy inputs: the binding's device copies have no other owner
    scratch = [torch.full(a.shape, 7, dtype=torch.int32 if a.dtype.kind == "i" else torch.float32, device="cuda")
               for _ in range(3) for a in _arrays(inputs)]
    torch.cuda.synchronize()
    got = _tensors(got)
    assert len(got) == len(want) > 0 and len(scratch) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (method, i)
        same = g.view(torch.int32) == w.view(torch.int32)                                  # bitwise (NaN-safe)
        if layouts is None or layouts[i] is None:
            assert bool(same.all()), (method, i)
            continue
        tables = _table_mask(rc, layouts[i], w)
        assert not bool(tables.all()) and bool(same[~tables].all()), (method, i)
        assert float(w[~tables].abs().max()) > 0.0 and float(w[tables].abs().max()) > 0.0, (method, i)
        bound = 1e-5 * w[tables].abs() + 1e-6 * float(w.abs().max())
        print(f"{method}[{i}]: {int((~same).sum())} table entries differ, worst |diff| / bound = "
              f"{float(((g[tables] - w[tables]).abs() / bound).max()):.3g}")
        assert bool(((g[tables] - w[tables]).abs() <= bound).all()), (method, i)
    assert any(float(w.float().abs().sum()) > 0.0 for w in want)
