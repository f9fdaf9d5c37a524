"""The loss calls behind tests/golden/loss_call_pin.json and tests/test_gpu_loss_call_pin.py: every per-ray loss entry point
through the binding, once without a gradient buffer and once with one, at the ray counts that reach each seam of the host
layer in front of the kernels.  Seeded cases of loss_cases.py; a case "<entry>/n<k>/<grad|nograd>" renders

  {"losses": [float, ...], "arrays": {name: float32 array}}

arrays: every tensor of every gradient flat ("grad:<tensor>", "sampler_grad:<tensor>", ...) and the workspace intermediates
the per-loss tests read by name, as the call left them.  Hash-grid table segments are accumulated with float atomics; the
pin tool leaves out what differs between two runs, and only tables may.

  cache handle (hotdog weights)           interlevel, data, geometry, geometry_smoothness, mask, density_regularizer
  time-resolved handle (cornell weights)  transient_interlevel, transient_geometry, transient_mask, transient_density_regularizer,
                                          transient_data, transient_data_kind, transient_data_sampler
  material handle                         light_sampling, material_smoothness, material_data

Ray counts: 1; 1025 for the cache, sampler and material losses (32 last-level samples: the density backward's chunk of
32768 samples ends at 1024 rays, so a second chunk of 32 samples and a second K slice run); 257 for the transient data calls
(chunks of 256 rays).  The regularizers take no rays: one size.

refusals(): from one valid 1-ray call of each entry point, as the binding marshals it, one call of the export per single
argument fault (status, message) and the valid n = 0 call; every fault is refused by the host layer before any launch.

Run as a program it writes the cases into the .json named on its command line (tools/make_loss_call_pin.py runs it on a
build of the parent commit): losses as numbers, every array as its shape and the SHA-256 of its float32 bytes.
"""
import dataclasses
import hashlib
import json
import sys

import numpy as np
import torch

import common
import loss_cases as lc
import nrc_amd

ANNEAL = 0.4
K_SEC = 8                                    # secondary samples of the material-stage calls
CACHE_SIZES, DATA_SIZES = (1, 1025), (1, 257)
CACHE_ENTRIES = ("interlevel", "data", "geometry", "geometry_smoothness", "mask")
SAMPLER_ENTRIES = ("transient_interlevel", "transient_geometry", "transient_mask")
DATA_ENTRIES = ("transient_data", "transient_data_kind", "transient_data_sampler")
MATERIAL_ENTRIES = ("light_sampling", "material_smoothness", "material_data")
REGULARIZERS = ("density_regularizer", "transient_density_regularizer")
HANDLE_OF = {**{e: "cache" for e in CACHE_ENTRIES + ("density_regularizer",)},
             **{e: "transient" for e in SAMPLER_ENTRIES + DATA_ENTRIES + ("transient_density_regularizer",)},
             **{e: "material" for e in MATERIAL_ENTRIES}}


def case_names():
    names = []
    for entries, sizes in ((CACHE_ENTRIES, CACHE_SIZES), (SAMPLER_ENTRIES, CACHE_SIZES), (DATA_ENTRIES, DATA_SIZES),
                           (MATERIAL_ENTRIES, CACHE_SIZES)):
        names += [f"{e}/n{n}/{g}" for e in entries for n in sizes for g in ("nograd", "grad")]
    return names + [f"{e}/n0/{g}" for e in REGULARIZERS for g in ("nograd", "grad")]


def lossmult(n, seed):
    """loss_cases.lossmult without its leading zero: ray 0 counts (the single-ray cases carry a real gradient), rays 6, 13, ...
    have weight 0."""
    return lc.lossmult(n + 1, seed=seed)[1:].copy()


def is_table(name):
    """A hash-grid table segment of a gradient flat (float atomics: not reproducible bit for bit)."""
    return name.split(":", 1)[0].endswith("grad") and "grid" in name


def make_handles():
    from nrc_amd import rc_ext
    t = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    t.load_weights(common.weights_transient_np())
    return {"cache": common.make_rc(), "transient": t, "material": lc.make_material_rc()}


def _flat(rc, what, flat, layout):
    """{array name: the segment, still on the device} of a gradient flat"""
    if flat is None:
        return {}
    return {f"{what}:{name}": flat[off: off + int(np.prod(shape))].reshape(shape) for name, off, shape in layout}


def _ws(rc, names):
    return {k: rc.workspace(k).copy() for k in names}


def _geo_terms():
    from nrc_amd import train
    return train.geometry_terms(1.0)


def render(handles, name, want=None):
    """One case on the handle of its kind (make_handles).  want: the arrays to bring to the host (default all; the test
    leaves the tables on the device)."""
    from nrc_amd import config, train
    entry, n, grad = name.split("/")
    n, grad = int(n[1:]), grad == "grad"
    rc = handles[HANDLE_OF[entry]]
    g = None if grad else False
    L2 = rc.cfg.num_levels - 1
    dens = lambda l: rc.density_grad_layout(l)[0]
    sampler = lambda: rc.transient_sampler_grad_layout()[0]
    arrays = {}
    if entry in REGULARIZERS:
        if entry == "density_regularizer":
            flat, losses = rc.density_regularizer(L2, 0.1, g)
            arrays = _flat(rc, "grad", flat, dens(L2))
        else:
            flat, losses = rc.transient_density_regularizer(L2, 0.1, g)
            arrays = _flat(rc, "grad", flat, sampler())
    elif entry in CACHE_ENTRIES + SAMPLER_ENTRIES:
        tr = entry.startswith("transient_")
        kind = entry[len("transient_"):] if tr else entry
        rays, jit = lc.transient_batch(n, seed=31, jitter_seed=32) if tr else lc.cache_case(n, seed=31)
        lm = lossmult(n, seed=33)
        if kind == "interlevel":
            if tr:
                flat, losses = rc.transient_interlevel_backward(rays, jit, ANNEAL, lossmult=lm, grad=g)
                arrays = _flat(rc, "grad", flat, sampler())
            else:
                flats, losses = rc.interlevel_backward(rays, jit, ANNEAL, lossmult=lm, levels=None if grad else ())
                for l in range(L2):
                    arrays.update(_flat(rc, f"level{l}_grad", flats[l], dens(l)))
            arrays.update(_ws(rc, ["i:loss_ray"] + [f"i:d_density{l}" for l in range(L2)] + ([f"i:points{l}" for l in range(L2)] if grad else [])))
        elif kind == "data":
            flats, losses = rc.data_backward(rays, lc.uniform_gt(n, 34), jit, ANNEAL, lm, grads=g)
            arrays = {**_flat(rc, "density_grad", flats[0], dens(L2)), **_flat(rc, "shader_grad", flats[1], rc.shader_grad_layout()[0]),
                      **_ws(rc, ["d:loss_ray", "d:d_density", "d:d_rgbs"] + (["d:points"] if grad else []))}
        elif kind == "geometry":
            if tr:
                flat, losses = rc.transient_geometry_backward(rays, jit, ANNEAL, lm, _geo_terms(), grad=g)
                arrays = _flat(rc, "grad", flat, sampler())
            else:
                flats, losses = rc.geometry_backward(rays, jit, ANNEAL, lm, _geo_terms(), grads=g)
                arrays = {**_flat(rc, "density_grad", flats[0], dens(L2)), **_flat(rc, "shader_grad", flats[1], rc.shader_grad_layout()[0])}
            arrays.update(_ws(rc, ["g:loss_ray"] + (["g:d_density", "g:d_pred", "g:points"] if grad else [])))
        elif kind == "geometry_smoothness":
            S2 = rc.cfg.sampling_strategy[-1][2]
            noise = np.random.Generator(np.random.PCG64(35)).standard_normal((n, S2, 3)).astype(np.float32)
            terms = dict(train.geometry_smoothness_terms(1.0), weight_density=0.01)
            flat, losses = rc.geometry_smoothness_backward(rays, jit, ANNEAL, noise, lm, terms, grads=g)
            arrays = {**_flat(rc, "grad", flat, dens(L2)), **_ws(rc, ["gs:loss_ray", "gs:points", "gs:points_p"] + (["gs:d_density", "gs:d_density_p"] if grad else []))}
        else:
            masks = (np.arange(n) % 3 != 1).astype(np.float32)
            fn = rc.transient_mask_backward if tr else rc.mask_backward
            flat, losses = fn(rays, jit, ANNEAL, masks, lm, **({"grad": g} if tr else {"grads": g}))
            arrays = {**_flat(rc, "grad", flat, sampler() if tr else dens(L2)), **_ws(rc, ["mk:loss_ray", "mk:d_density"] + (["mk:points"] if grad else []))}
    elif entry in DATA_ENTRIES:
        rays, jit = lc.transient_batch(n, seed=41, jitter_seed=42)
        gt = lc.transient_target(rc, rays, jit, 43)
        lm = lossmult(n, seed=44)
        heads = rc.transient_head_grad_layout()[0]
        cfg = None if entry == "transient_data" else dataclasses.replace(config.TransientDataLossConfig(), loss_type="mse")
        if entry == "transient_data_sampler":
            flat, sflat, losses = rc.transient_data_backward_sampler(rays, {"jitter": jit}, gt, lossmult=lm, cfg=cfg, grad=g, sampler_grad=g)
            arrays = {**_flat(rc, "sampler_grad", sflat, sampler()), **(_ws(rc, ["td:d_density", "td:points"]) if grad else {})}
        else:
            flat, losses = rc.transient_data_backward(rays, {"jitter": jit}, gt, lossmult=lm, cfg=cfg, grad=g)
        arrays.update({**_flat(rc, "grad", flat, heads), **_ws(rc, ["td:loss_ray", "td:G", "td:d_weights"])})
    else:
        rays, rnd = lc.material_case(n, K_SEC, seed=51)
        lm = lossmult(n, seed=53)
        mat = rc.material_grad_layout()[0]
        if entry == "light_sampling":
            flat, losses = rc.light_sampling_backward(rays, rnd, K_SEC, lossmult=lm, grad=g)
            arrays = {**_flat(rc, "grad", flat, rc.light_grad_layout()[0]), **_ws(rc, ["ls:loss_ray"])}
        elif entry == "material_smoothness":
            flat, losses = rc.material_smoothness_backward(rays, rnd, lc.normal_noise(n, 54), lossmult=lm, grad=g)
            arrays = {**_flat(rc, "grad", flat, mat), **_ws(rc, ["ms:loss_ray"])}
        else:
            flat, losses = rc.material_data_backward(rays, rnd, lc.uniform_gt(n, 55), K_SEC, lossmult=lm, grad=g)
            arrays = {**_flat(rc, "grad", flat, mat), **_ws(rc, ["md:loss_ray"] + (["md:dmat"] if grad else []))}
    torch.cuda.synchronize()
    render.alive = (arrays, losses)            # refusals() calls the export again with these buffers
    return {"losses": [float(v) for v in losses.cpu().numpy().reshape(-1)],
            "arrays": {k: np.ascontiguousarray(v.cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32)
                       for k, v in arrays.items() if want is None or k in want}}


def digest(case):
    """A case as the pin stores it: the losses as numbers, every array as its shape and the SHA-256 of its float32 bytes."""
    return {"losses": case["losses"],
            "arrays": {k: {"shape": list(v.shape), "sha256": hashlib.sha256(v.tobytes()).hexdigest()} for k, v in case["arrays"].items()}}


# ---- the refusal table ---------------------------------------------------------------------------------------------------

ENTRY_FN = {**{e: f"rc_{e}_backward" for e in CACHE_ENTRIES + SAMPLER_ENTRIES + MATERIAL_ENTRIES},
            "transient_data": "rc_transient_data_backward", "transient_data_kind": "rc_transient_data_backward_kind",
            "transient_data_sampler": "rc_transient_data_backward_sampler", "density_regularizer": "rc_density_regularizer",
            "transient_density_regularizer": "rc_transient_density_regularizer"}
# one setting of the entry's config struct made NaN, and the entry's own refusals: {label: (field, value)}
NONFINITE = {"rc_mask_loss": "weight_opaque"}          # every other struct: its first field
OWN_FAULTS = {"geometry": {"distortion_p 0": ("distortion_p", 0.0), "distortion_p 1": ("distortion_p", 1.0)},
              "transient_geometry": {"distortion_p 0": ("distortion_p", 0.0), "distortion_p 1": ("distortion_p", 1.0)},
              "mask": {"charb_padding 0": ("charb_padding", 0.0)}, "transient_mask": {"charb_padding 0": ("charb_padding", 0.0)},
              "geometry_smoothness": {"weight_normals_pred 1": ("weight_normals_pred", 1.0)},
              "transient_data_kind": {"loss_type 99": ("loss_type", 99), "loss_type -1": ("loss_type", -1)},
              "transient_data_sampler": {"loss_type 99": ("loss_type", 99), "loss_type -1": ("loss_type", -1)}}


class _Recorder:
    """Stands in for the binding's library: every call goes through, its arguments are kept."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def _valid_call(handles, entry):
    """The export and the argument list of one valid call of `entry` (1 ray, with a gradient buffer), as the binding made it."""
    rc = handles[HANDLE_OF[entry]]
    lib = rc.lib
    rc.lib = rec = _Recorder(lib)
    try:
        render(handles, f"{entry}/n{0 if entry in REGULARIZERS else 1}/grad", want=set())
    finally:
        rc.lib = lib
    return rc, [list(a) for f, a in rec.calls if f == ENTRY_FN[entry]][-1]


def _edited(byref_arg, field, value):
    """A copy of the struct behind a byref argument with one field changed ("base.mult": a member of a member)."""
    import ctypes as C
    obj = byref_arg._obj
    c = type(obj).from_buffer_copy(obj)
    tgt = c
    *path, leaf = field.split(".")
    for k in path:
        tgt = getattr(tgt, k)
    setattr(tgt, leaf, value)
    return C.byref(c), c


def refusals(handles):
    """{entry: {fault: [status, message]}}: from one valid call of each entry point, one call per single fault -- every one an
    argument fault the host layer refuses before any launch -- and the valid call with n = 0, whose loss tensor must keep its
    canary ("n 0": [status, "", canary kept])."""
    import ctypes as C
    from nrc_amd import rc_ext as X
    nan = float("nan")
    table = {}
    for entry, fn_name in ENTRY_FN.items():
        rc, args = _valid_call(handles, entry)
        alive = render.alive
        types = X._PROTOTYPES[fn_name][1]
        fn = getattr(rc.lib, fn_name)
        other = handles["cache" if HANDLE_OF[entry] == "transient" else "transient"]
        keep, out = [], {}

        def call(label, edits, handle=rc):
            a = list(args)
            a[0] = handle._h
            for i, v in edits.items():
                a[i] = v
            code = int(fn(*a))
            out[label] = [code, (handle.lib.rc_last_error(handle._h) or b"").decode() if code else ""]

        loss_i = len(types) - 2
        call("null loss", {loss_i: None})
        call("wrong handle kind", {}, other)
        if entry in REGULARIZERS:
            call("level -1", {1: -1})
            call("level 3", {1: 3})
            call("mult nan", {2: nan})
            table[entry] = out
            continue
        ri, ni = types.index(X._RAYS), types.index(X._I64)
        call("null rays", {ri: None})
        call("n -1", {ni: -1})
        for field in ("origins", "directions", "far"):
            ref, obj = _edited(args[ri], field, None)
            keep.append(obj)
            call("rays without " + field, {ri: ref})
        ai = types.index(X._RND) + 1
        if types[ai] is X._F:
            call("anneal -1", {ai: -1.0})
            call("anneal nan", {ai: nan})
        ci = [i for i, t in enumerate(types) if t not in (X._RAYS, X._RND, X._MRND) and isinstance(getattr(t, "_type_", None), type)
              and issubclass(t._type_, C.Structure)]
        if ci:
            ci = ci[0]
            call("null cfg", {ci: None})
            struct = type(args[ci]._obj)
            first = struct._fields_[0][0]
            field = NONFINITE.get(struct.__name__, "base.mult" if first == "base" else first)
            edits = {"setting nan": (field, nan), **OWN_FAULTS.get(entry, {})}
            for label, (f, v) in edits.items():
                ref, obj = _edited(args[ci], f, v)
                keep.append(obj)
                call(label, {ci: ref})
        elif entry.endswith("interlevel"):
            mi = types.index(C.POINTER(C.c_float))
            call("null mults", {mi: None})
            call("null blurs", {mi + 1: None})
            for label, i, v in (("mults nan", mi, nan), ("blurs nan", mi + 1, nan), ("blurs -1", mi + 1, -1.0)):
                arr = type(args[i])(*args[i])
                arr[0] = v
                keep.append(arr)
                call(label, {i: arr})
        else:                                  # data: charb_padding and mult follow the anneal
            call("null gt_rgb", {ri + 1: None})
            call("charb_padding nan", {ai + 1: nan})
            call("mult nan", {ai + 2: nan})
        if entry in MATERIAL_ENTRIES:
            call("null material randoms", {types.index(X._MRND): None})
        canary = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
        call("n 0", {ni: 0, loss_i: canary.data_ptr()})
        torch.cuda.synchronize()
        out["n 0"].append(bool((canary == 7.0).all()))
        table[entry] = out
        del alive
    return table


if __name__ == "__main__":
    from nrc_amd import rc_ext
    handles = make_handles()
    out = {"mlp_arithmetic": rc_ext.mlp_arithmetic(), "source_hash": rc_ext.source_hash(),
           "cases": {name: digest(render(handles, name)) for name in case_names()}, "refusals": refusals(handles)}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
