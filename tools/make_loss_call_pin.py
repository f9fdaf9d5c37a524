#!/usr/bin/env python
"""Writes tests/golden/loss_call_pin.json: the cases of tests/loss_call_cases.py (every per-ray loss entry point, without and
with a gradient buffer, at the ray counts of the host layer's seams) as the library of THIS checkout computes them.  Run
once, on the parent of a change to the host layer or the binding in front of the loss kernels;
tests/test_gpu_loss_call_pin.py then holds the changed library to it with exact equality.

  make -C neural-radiance-caching_amd/csrc -j16
  python tools/make_loss_call_pin.py [out.json]

The cases are rendered twice, each time in a fresh child process.  The hash-grid table segments of a backward call's
gradient flats are accumulated with float atomics: they are left out, whether or not the two runs happen to agree on them
(the regularizers write theirs without atomics: kept).  Every other array, and every loss, must agree bit for bit between
the two runs, or the tool ends.  The file also holds the refusal table of loss_call_cases.refusals (status and message of one
call per single argument fault of every entry point, and the n = 0 call), equal in both runs.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)


def render_child(path):
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")])}
    r = subprocess.run([sys.executable, os.path.join(TESTS, "loss_call_cases.py"), path], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"the cases ended with {r.returncode}: {r.stderr[-3000:]}")
    with open(path) as f:
        return json.load(f)


def main():
    import loss_call_cases as cases

    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(TESTS, "golden", "loss_call_pin.json")
    with tempfile.TemporaryDirectory() as tmp:
        a, b = (render_child(os.path.join(tmp, f"run{i}.json")) for i in range(2))
    assert a["source_hash"] == b["source_hash"] and a["mlp_arithmetic"] == b["mlp_arithmetic"]
    assert list(a["cases"]) == list(b["cases"]) == cases.case_names()
    assert a["refusals"] == b["refusals"], "the refusal table differs between two runs"
    dropped = 0
    for name, ca in a["cases"].items():
        cb = b["cases"][name]
        assert ca["losses"] == cb["losses"], (name, ca["losses"], cb["losses"])
        assert set(ca["arrays"]) == set(cb["arrays"]), name
        for k in list(ca["arrays"]):
            if cases.is_table(k) and name.split("/")[0] not in cases.REGULARIZERS:
                del ca["arrays"][k]
                dropped += 1
            else:
                assert ca["arrays"][k] == cb["arrays"][k], f"{name}: {k} differs between two runs and is no table segment"
    with open(dst, "w") as f:
        json.dump(a, f, indent=0, sort_keys=True)
        f.write("\n")
    kept = sum(len(c["arrays"]) for c in a["cases"].values())
    print(f"{dst}: {len(a['cases'])} cases, {kept} arrays pinned, {dropped} table segments left out, {os.path.getsize(dst)} bytes, "
          f"source {a['source_hash']}, {a['mlp_arithmetic']}")


if __name__ == "__main__":
    main()
