"""Times the relighting calls per call by device events, one case and size per process, each beside its
yardstick in the same process:

  python tools/bench_relight.py --case stage --rays 1024 [--warmup 5] [--reps 30] [--rounds 5] [--out profiles/relight_bench.jsonl]
      rc_render_relight in both modes under a 1024 x 2048 image against rc_render_material on the same rays and randoms;
      the calls alternate over `rounds` rounds and the spread of the yardstick's round medians is reported, so a
      difference can be read against it;
  python tools/bench_relight.py --case pick
      rc_env_pick at T = 256 on that image against rc_prng_fill of the same T H W Gumbel values into HBM followed by
      torch.argmax over the texels of (noise + safe_log(pmf)), and against the threefry issue floor (36 vector
      instructions per output: 20 rounds of add / rotate / xor and the key injections of one counter block, two outputs
      per block; 256 CUs x 4 SIMDs x 32 lanes per cycle at 2.4 GHz);
  python tools/bench_relight.py --case lookup
      rc_env_lookup at 262 144 directions against its byte floor (12 B read + 12 B written per direction and four 16-byte
      texel reads) at the 6.3 TB/s copy rate.
Prints one JSON line per measurement (and appends it to --out)."""
import argparse
import json

import bench_common as bc

COPY_RATE_TBS = 6.3                 # measured device copy rate
VALU_LANE_RATE = 256 * 4 * 32 * 2.4e9
THREEFRY_INSTR_PER_OUTPUT = 36
H, W = 1024, 2048


def hdr_image(seed=0):
    """A synthetic HDR panorama: a smooth sky, a bright lobe and noise, in [0, ~50]."""
    import numpy as np
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.linspace(0, 1, H, dtype=np.float32), np.linspace(0, 1, W, dtype=np.float32), indexing="ij")
    sky = 0.2 + 0.8 * (1 - i)
    sun = 50.0 * np.exp(-((i - 0.3) ** 2 + (j - 0.6) ** 2) / 0.002)
    img = (sky + sun)[..., None] * np.asarray([1.0, 0.9, 0.8], np.float32) + rng.uniform(0, 0.05, size=(H, W, 3)).astype(np.float32)
    return img.astype(np.float32)


def rounds_of(calls, warmup, reps, rounds):
    """Median ms per call and round for each call, the calls alternating: {name: [ms per round]}."""
    out = {k: [] for k in calls}
    for r in range(rounds):
        res = bc.time_calls(calls, warmup if r == 0 else 1, reps)
        for k in calls:
            out[k].append(res[k + "_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("stage", "pick", "lookup"), required=True)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    bc.add_loop(ap, 5, 30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import common
    import nrc_amd
    from nrc_amd import prng, rc_ext, relight
    from oracle import material_ref

    cfg = nrc_amd.hotdog_config()
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(common.weights_material_np(False))
    env = relight.EnvImage(rc, hdr_image())
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"case": a.case, "image": [H, W], "library": rc_ext.source_hash(), "arithmetic": rc_ext.mlp_arithmetic()}
    if a.case == "stage":
        n = a.rays
        Ks, Kd = relight.leg_counts(cfg)
        rays = bc.to_device(nrc_amd.synthetic_rays(n, seed=77).hot_fields())
        rnd = bc.to_device(material_ref.draw_randoms(cfg, n, seed=3))
        ps = env.picks(prng.PRNGKey(1), relight.expected_T(n, Ks))
        pd = env.picks(prng.PRNGKey(2), relight.expected_T(n, Kd))
        calls = {"render_material": lambda: rc.render_material(rays, rnd),
                 "relight_brdf": lambda: rc.render_relight(rays, rnd, "brdf"),
                 "relight_env": lambda: rc.render_relight(rays, rnd, "env", ps, pd)}
        per = rounds_of(calls, a.warmup, a.reps, a.rounds)
        base = med(per["render_material"])
        res.update(rays=n, rounds=per, spread_of_yardstick=round((max(per["render_material"]) - min(per["render_material"])) / base, 4))
        for k in calls:
            res[k + "_ms"] = med(per[k])
            res[k + "_vs_material"] = round(med(per[k]) / base, 4)
    elif a.case == "pick":
        T = 256
        hw = H * W
        key = prng.PRNGKey(5)
        logp = torch.log(torch.clamp(env.pmf, min=float(np.finfo(np.float32).tiny)))

        def materialised():
            g = rc.prng_fill(key, (T, hw), "gumbel")
            return torch.argmax(g + logp[None, :], dim=1)

        calls = {"env_pick": lambda: env.picks(key, T), "fill_then_argmax": materialised}
        per = rounds_of(calls, a.warmup, max(a.reps // 3, 5), a.rounds)
        got, want = env.picks(key, T).cpu().numpy(), materialised().cpu().numpy()
        floor_ms = THREEFRY_INSTR_PER_OUTPUT * T * hw / VALU_LANE_RATE * 1e3
        res.update(T=T, outputs=T * hw, rounds=per, env_pick_ms=med(per["env_pick"]), fill_then_argmax_ms=med(per["fill_then_argmax"]),
                   noise_GB=round(4 * T * hw / 1e9, 2), picks_equal=float(np.mean(got == want)),
                   threefry_issue_floor_ms=round(floor_ms, 4), env_pick_times_floor=round(med(per["env_pick"]) / floor_ms, 2),
                   env_pick_vs_materialised=round(med(per["env_pick"]) / med(per["fill_then_argmax"]), 4))
    else:
        n = 262144
        d = torch.randn(n, 3, device="cuda")
        d = (d / d.norm(dim=-1, keepdim=True)).contiguous()
        out = torch.empty_like(d)
        st = rc._stream()
        calls = {"env_lookup": lambda: rc._check(rc.lib.rc_env_lookup(rc._h, d.data_ptr(), n, out.data_ptr(), st))}
        per = rounds_of(calls, a.warmup, a.reps, a.rounds)
        nbytes = n * (12 + 12 + 4 * 16)
        floor_ms = nbytes / (COPY_RATE_TBS * 1e12) * 1e3
        res.update(directions=n, rounds=per, env_lookup_ms=med(per["env_lookup"]), bytes=nbytes, byte_floor_ms=round(floor_ms, 5),
                   env_lookup_times_floor=round(med(per["env_lookup"]) / floor_ms, 2))
    bc.emit(res)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
