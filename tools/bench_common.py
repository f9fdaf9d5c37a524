"""Shared body of the per-loss bench tools (bench_interlevel, bench_data_backward, bench_geometry_backward,
bench_light_sampling, bench_material_smoothness, bench_material_data): the import path, the common command-line options,
the device-resident inputs, the timed loops and the splitters of a rocprofv3 kernel_stats.csv.  Each tool keeps its
kernel groups, its derived figure and its table of calls."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def add_rays(ap, default):
    ap.add_argument("--rays", type=int, nargs="+", default=default)


def add_loop(ap, warmup, reps):
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--reps", type=int, default=reps)


def add_stats(ap, per_call=False):
    """--stats; per_call: also --calls and --only, of the tools that time several calls and profile one of them."""
    ap.add_argument("--stats", default=None)
    if per_call:
        ap.add_argument("--calls", type=int, default=0, help="--stats: gradient calls in the profiled run")
        ap.add_argument("--only", nargs="+", default=None, help="time only these calls (backward, loss_only, ...)")


def emit(res):
    print(json.dumps(res), flush=True)


def to_device(v):
    """Inputs resident on the device: the calls' host work is argument marshalling only."""
    import numpy as np
    import torch
    if isinstance(v, dict):
        return {k: to_device(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [to_device(x) for x in v]
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def time_calls(calls, warmup, reps, only=None):
    """{name + "_ms": ms per call} of a {name: callable} table: after the warm-up calls, device events bracket each call
    on the caller's stream; the median of the repetitions."""
    import torch
    res = {}
    for name, fn in calls.items():
        if only and name not in only:
            continue
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        res[name + "_ms"] = round(times[len(times) // 2], 4)
    return res


def time_whole_call(fn, warmup, reps, flats):
    """One gradient call into the buffers `flats`: steady-state ms per call (one device-event pair around all the
    repetitions) and the device memory the call's workspaces took during the warm-up calls."""
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ws_gb = (free0 - torch.cuda.mem_get_info()[0]) / 1e9
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return {"ms_per_call": round(e0.elapsed_time(e1) / reps, 4), "workspace_GB": round(ws_gb, 2),
            "grad_MB": [round(f.numel() * 4 / 1e6, 1) for f in flats]}


def kernel_rows(stats_path):
    """(kernel name, total ns) of a rocprofv3 kernel_stats.csv (or its results .db)."""
    if stats_path.endswith(".db"):
        import sqlite3
        return sqlite3.connect(stats_path).execute("select name, sum(end - start) from kernels group by name").fetchall()
    with open(stats_path) as f:
        return [(r["Name"], r["TotalDurationNs"]) for r in csv.DictReader(f)]


def split_groups(stats_path, groups, calls=1, other=None):
    """Kernel ms by group ({group: name fragments}; a kernel counts in the first group that names it), divided by
    `calls`; kernels no group names go to `other` where one is given."""
    out = {k: 0.0 for k in groups}
    if other:
        out[other] = 0.0
    for name, total_ns in kernel_rows(stats_path):
        g = next((g for g, pre in groups.items() if any(p in name for p in pre)), other)
        if g:
            out[g] += float(total_ns) / 1e6 / calls
    return out


def split_own(stats_path, own):
    """Kernel ms per kernel over the whole profiled run: ({fragment of `own`: ms}, {other kernel name: ms})."""
    mine, other = {}, {}
    for name, total_ns in kernel_rows(stats_path):
        ms = float(total_ns) / 1e6
        key = next((k for k in own if k in name), None)
        into, key = (mine, key) if key else (other, name[:60])
        into[key] = into.get(key, 0.0) + ms
    return mine, other


def own_report(stats_path, own, rays, calls):
    """The --stats line of the tools that split by their own kernels; with `calls` also per gradient call."""
    mine, other = split_own(stats_path, own)
    res = {"rays": rays, "kernel_ms_per_run_own": {k: round(v, 4) for k, v in mine.items()},
           "kernel_ms_per_run_other_total": round(sum(other.values()), 4)}
    if calls:
        res["own_ms_per_grad_call"] = {k: round(v / calls, 4) for k, v in mine.items()}
        res["own_total_ms_per_grad_call"] = round(sum(mine.values()) / calls, 4)
        res["other_ms_per_grad_call"] = round(sum(other.values()) / calls, 4)
    return res
