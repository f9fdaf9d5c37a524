"""`make prngcheck`: the material stage's random_split tree (csrc/rc_prng_host.h) compiled for the CPU under
AddressSanitizer + UBSan as a stand-alone program (csrc/prngcheck.cpp) and run here; the segment tables it prints are
compared with prng.material_stage_plan, case by case.  A sanitizer report makes the program exit non-zero."""
import os
import subprocess

import pytest

import material_randoms_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")


@pytest.fixture(scope="module")
def tables():
    subprocess.run(["make", "-C", CSRC, "prngcheck"], check=True, capture_output=True)
    run = subprocess.run([os.path.join(CSRC, "prngcheck")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    cases, refusals, cur = {}, {}, None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = cases[tuple(int(v) for v in w[1:7])] = dict(rc=int(w[8]), count=int(w[10]), words=int(w[12]), segs=[])
        elif w[0] == "seg":
            cur["segs"].append(tuple(int(v) for v in w[1:]))
        else:
            assert w[0] == "refuse", line
            refusals[w[1]] = int(w[2])
    return cases, refusals


def test_tables_are_the_python_plan(tables):
    cases, _ = tables
    assert len(cases) == len(mc.SIZES) * len(mc.FLAGS)
    for n, K in mc.SIZES:
        for train, env, loss, vmf in mc.FLAGS:
            c = cases[(n, K, int(train), int(env), int(loss), int(vmf))]
            want = mc.rows_of(mc.python_plan(n, K, train, env, loss, vmf))
            assert c["rc"] == 0 and c["count"] == len(want) == len(c["segs"])
            assert [(s[0], s[1], s[2], s[3], s[4]) for s in c["segs"]] == want, (n, K, train, env, loss, vmf)


def test_tables_are_the_library_s(tables):
    """The same header compiled into the product: offsets and arena size agree with rc_material_randoms_plan."""
    import __graft_entry__ as g
    g.build()
    cases, _ = tables
    for n, K in mc.SIZES:
        for train, env, loss, vmf in mc.FLAGS:
            c = cases[(n, K, int(train), int(env), int(loss), int(vmf))]
            segs, words = mc.c_plan(n, K, train, env, loss, vmf)
            assert words == c["words"]
            assert [(g_.id, g_.mode, g_.n, g_.key[0], g_.key[1], g_.offset, g_.offset2) for g_ in segs] == c["segs"]


def test_refusals(tables):
    _, refusals = tables
    assert refusals == {"K5": -5, "null_key": -1, "null_segs": -1, "null_count": -1, "null_levels": -1}
