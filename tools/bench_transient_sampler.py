"""The time-resolved cache stage's sampler-side calls, ms per call by tools/bench_transient_grad.py's
protocol (device events after warm-up, distinct batches cycled, the median of the repetitions).  One JSON line per ray count:

  kind            rc_transient_data_backward_kind with the heads' gradient (the yardstick: runs on a library from before the
                  sampler calls too)
  sampler_null    rc_transient_data_backward_sampler, sampler_grads = NULL (must cost what `kind` costs)
  sampler         rc_transient_data_backward_sampler with both gradient buffers
  interlevel / geometry / mask / regularizer      the four sampler calls with the sampler buffer (regularizer: the three levels)
  step            train.transient_cache_stage_step (every loss, the backward mask term, one rc_adam_update, both refreshes)

--library PATH measures another build of the same ABI (RC_HIP_LIBRARY); the calls it lacks are left out, so a parent build
gives the `kind` line to alternate with this build's in one session:

  python tools/bench_transient_sampler.py --rays 1024 --library /path/to/parent/librc_hip.so --only kind
  python tools/bench_transient_sampler.py --rays 1024
"""
import argparse
import ctypes
import os

import bench_common as bc


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [1024])
    bc.add_loop(ap, 3, 10)
    ap.add_argument("--only", nargs="+", default=None, help="time only these calls")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--library", default=None, help="another build of the library (RC_HIP_LIBRARY)")
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    if a.library:
        os.environ["RC_HIP_LIBRARY"] = a.library
    import numpy as np
    import torch

    import common
    import nrc_amd
    from nrc_amd import config, rc_ext, train

    probe = ctypes.CDLL(rc_ext.library_path())
    lacking = [k for k in rc_ext._PROTOTYPES if not hasattr(probe, k)]
    for k in lacking:                      # an older build: bind what it has
        del rc_ext._PROTOTYPES[k]
    new = not lacking
    w = common.weights_transient_np()
    rc = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    rc.load_weights(w)
    il, ge, mk = (config.cornell_transient_interlevel_config(), config.cornell_transient_geometry_config(),
                  config.cornell_transient_mask_config())
    for n in a.rays:
        batches = []
        for i in range(a.batches):
            rays = bc.to_device(nrc_amd.synthetic_transient_rays(n, seed=100 + i).hot_fields())
            jit = bc.to_device([j.reshape(-1) for j in common.jitters(n, seed=200 + i)])
            rgb = rc.render_transient(rays, {"jitter": jit}, outputs=["rgb"])["rgb"]
            gt = (rgb * torch.empty_like(rgb).uniform_(0.5, 1.5)).contiguous()
            o = rays["origins"]
            look = (-o / o.norm(dim=-1, keepdim=True)).contiguous()
            back = {"u1": torch.rand(n, device="cuda"), "u2": torch.rand(n, device="cuda"),
                    "jitter": bc.to_device([j.reshape(-1) for j in common.jitters(n, seed=300 + i)])}
            batches.append((rays, jit, gt, look, back))
        heads = torch.zeros(rc.transient_head_grad_layout()[1], device="cuda")
        state = {"i": 0}

        def nxt():
            state["i"] += 1
            return batches[state["i"] % len(batches)]

        def kind():
            rays, jit, gt, _, _ = nxt()
            cfg, _, r, held, m, cam, rnd_p, lm, gt_p, rn_p, gn_p = rc._transient_data_args(rays, {"jitter": jit}, gt, None, None,
                                                                                           None, None)
            ck = rc_ext.transient_data_loss_kind_c(cfg)
            losses = torch.zeros(2, device="cuda")
            rc._check(rc.lib.rc_transient_data_backward_kind(rc._h, ctypes.byref(r), cam.data_ptr(), m, rnd_p, gt_p, rn_p, gn_p, None,
                                                             ctypes.byref(ck), heads.data_ptr(), losses.data_ptr(), rc._stream()))
            rc._keep = [held]

        calls = {"kind": kind}
        if new:
            flat = torch.zeros(rc.transient_sampler_grad_layout()[1], device="cuda")
            terms = train.mask_terms(1.0, mk)["mask"]
            gterms = train.geometry_terms(1.0, ge)

            def sampler_null():
                rays, jit, gt, _, _ = nxt()
                rc.transient_data_backward_sampler(rays, {"jitter": jit}, gt, grad=heads, sampler_grad=False)

            def sampler():
                rays, jit, gt, _, _ = nxt()
                rc.transient_data_backward_sampler(rays, {"jitter": jit}, gt, grad=heads, sampler_grad=flat)

            def interlevel():
                rays, jit, _, _, _ = nxt()
                rc.transient_interlevel_backward(rays, jit, 0.4, il.mults, il.blurs, None, flat)

            def geometry():
                rays, jit, _, _, _ = nxt()
                rc.transient_geometry_backward(rays, jit, 0.4, None, gterms, flat)

            def mask():
                rays, jit, _, _, _ = nxt()
                rc.transient_mask_backward(rays, jit, 0.4, None, None, terms, flat)

            def regularizer():
                for l in range(rc.cfg.num_levels):
                    rc.transient_density_regularizer(l, ge.density_grid_mult, flat)

            lr = 1e-4
            ocfg = config.OptimizerConfig(lr_init=lr, lr_final=lr, lr_delay_steps=0, extra_opt_params=tuple(
                config.ExtraOptParams(g, lr, lr, 0, lr, lr, 0) for g in ("Cache", "SurfaceLightField")))
            opt = {}

            def step():
                if not opt:                # built on first use: its refresh reloads the handle's weights
                    opt["o"] = train.TransientSamplerOptimizer(rc, ocfg)
                    opt["o"].init_from(w)
                rays, jit, gt, look, back = nxt()
                train.transient_cache_stage_step(rc, opt["o"], rays, None, jit, gt, look=look, backward_randoms=back)

            calls.update(sampler_null=sampler_null, sampler=sampler, interlevel=interlevel, geometry=geometry, mask=mask,
                         regularizer=regularizer, step=step)
        res = {"rays": n, "label": a.label or ("this build" if new else "older build"),
               **bc.time_calls(calls, a.warmup, a.reps, a.only)}
        bc.emit(res)


if __name__ == "__main__":
    main()
