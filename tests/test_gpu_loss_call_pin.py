"""The host layer and the binding in front of the loss kernels, held to the parent of the change that consolidated them:
tests/golden/loss_call_pin.json (tools/make_loss_call_pin.py, taken on that parent) pins every case of loss_call_cases.py --
each per-ray loss entry point without and with a gradient buffer, at 1 ray and at the ray count behind the first chunk
seam -- and this library must give the same losses and the same bytes in every dense segment of every gradient flat and in
the workspace intermediates.  Exact equality: nothing on the device changed, so nothing may move.  The same file holds the
parent's refusal table (status and message per single argument fault, the n = 0 call), replayed here."""
import hashlib
import json
import os

import pytest

import loss_call_cases as cases

pytestmark = pytest.mark.gpu
PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_call_pin.json")


@pytest.fixture(scope="module")
def pin():
    with open(PIN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def handles():
    return cases.make_handles()


def test_pin_covers_the_described_set(pin):
    """Every entry point, both gradient modes, the seam sizes; the tables of the backward calls are the only arrays left out."""
    assert list(pin["cases"]) == sorted(cases.case_names()) and len(pin["cases"]) == 60
    entries = {n.split("/")[0] for n in pin["cases"]}
    assert entries == set(cases.HANDLE_OF) and len(entries) == 16
    for e in cases.CACHE_ENTRIES + cases.SAMPLER_ENTRIES + cases.MATERIAL_ENTRIES:
        assert {n for n in pin["cases"] if n.startswith(e + "/")} == {f"{e}/n{k}/{g}" for k in (1, 1025) for g in ("grad", "nograd")}
    for e in cases.DATA_ENTRIES:
        assert {n for n in pin["cases"] if n.startswith(e + "/")} == {f"{e}/n{k}/{g}" for k in (1, 257) for g in ("grad", "nograd")}
    for name, c in pin["cases"].items():
        entry, _, grad = name.split("/")
        assert c["losses"] and all(v == v for v in c["losses"]), name
        tables = [k for k in c["arrays"] if cases.is_table(k)]
        assert not tables or entry in cases.REGULARIZERS, (name, tables)
        flats = [k for k in c["arrays"] if k.split(":", 1)[0].endswith("grad")]
        assert bool(flats) == (grad == "grad"), name                 # dense segments of a flat exactly when one was asked for
        assert entry in cases.REGULARIZERS or any(k.endswith("loss_ray") for k in c["arrays"]), name


@pytest.mark.parametrize("name", cases.case_names())
def test_case_equals_the_pin(pin, handles, name):
    from nrc_amd import rc_ext
    assert rc_ext.mlp_arithmetic() == pin["mlp_arithmetic"]
    want = pin["cases"][name]
    got = cases.digest(cases.render(handles, name, want=set(want["arrays"])))
    assert got["losses"] == want["losses"], (name, got["losses"], want["losses"])
    assert set(got["arrays"]) == set(want["arrays"])
    diff = [k for k in want["arrays"] if got["arrays"][k] != want["arrays"][k]]
    assert not diff, (name, diff)


REQUIRED = ("null rays", "null loss", "n -1", "n 0", "wrong handle kind", "rays without origins", "rays without directions",
            "rays without far")


def test_refusals_equal_the_parent(pin, handles):
    """One call per single argument fault of every entry point, and the valid n = 0 call: status and message are the parent's,
    the n = 0 call returns RC_OK and leaves the loss tensor's canary alone.  Every fault is refused before any launch.  Then
    one valid 1-ray call per handle still gives the pinned result."""
    want = pin["refusals"]
    assert set(want) == set(cases.HANDLE_OF)
    for entry, table in want.items():
        assert all(code != 0 and msg for label, (code, msg, *_) in table.items() if label != "n 0"), (entry, table)
        if entry in cases.REGULARIZERS:
            assert {"null loss", "wrong handle kind", "level -1", "mult nan"} <= set(table), entry
            continue
        assert set(REQUIRED) <= set(table), (entry, sorted(table))
        assert table["n 0"] == [0, "", True], (entry, table["n 0"])
        assert any("nan" in label for label in table) and (entry in cases.MATERIAL_ENTRIES + cases.DATA_ENTRIES or "anneal -1" in table)
        assert entry == "data" or entry.endswith("interlevel") or "null cfg" in table, entry
    got = json.loads(json.dumps(cases.refusals(handles)))
    diff = {(e, k): (got[e].get(k), v) for e, t in want.items() for k, v in t.items() if got[e].get(k) != v}
    assert not diff and {e: set(t) for e, t in got.items()} == {e: set(t) for e, t in want.items()}, diff
    for name in ("mask/n1/grad", "transient_data_sampler/n1/grad", "material_data/n1/grad"):
        w = pin["cases"][name]
        assert cases.digest(cases.render(handles, name, want=set(w["arrays"]))) == w, name


def test_single_ray_cases_carry_a_gradient(pin):
    """Ray 0 has a non-zero loss weight and mask: the 1-ray cases pin real losses, not the hashes of zero buffers."""
    for name, c in pin["cases"].items():
        if "/n1/" in name:
            assert any(v != 0.0 for v in c["losses"]), (name, c["losses"])
