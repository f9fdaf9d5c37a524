"""`hostcheck --rows`: the output rows of the fused streams as a table (csrc/rc_pack_host.h pack_dot_rows, rc_rows_stride,
rc_rows_at) and the fragment offsets of the fused stream in both layouts, from the ASan/UBSan build of the host-only
packing code (a stand-alone program; a sanitizer report makes it exit non-zero), against numpy restatements:

  * the table of a 3-output / 2-tile block equals what lanes 0 and 32 of pack_dot's fragments hold, bit for bit, its
    biases what a bias fragment holds, everything else is zero padding, and the two rows lie 128 bytes apart modulo the
    256 bytes of an LDS bank row;
  * the offsets F_L0 .. F_SH, the shader's layer offsets, NF_FUSED and the chunk count match the formulas, restated
    here from the layer shapes, in the fragment form (the parent's 3452 fragments = 54 chunks) and in the table form;
  * no row table straddles a chunk of the ring, and every split layer starts on a whole 1-KiB piece.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
CHUNK = 64


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    r = subprocess.run(["make", "-C", CSRC, "hostcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    d = tmp_path_factory.mktemp("hostcheck_rows")
    rng = np.random.default_rng(13)
    k = rng.normal(size=(64, 3)).astype(np.float32)
    b = rng.normal(size=(3,)).astype(np.float32)
    k.tofile(d / "in_d_kernel.bin")
    b.tofile(d / "in_d_bias.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(CSRC, "hostcheck"), "--rows", str(d)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "hostcheck rows ok" in r.stdout, r.stdout + r.stderr       # non-zero: a sanitizer report
    lines = {}
    for line in r.stdout.splitlines():
        kv = dict((a, int(v)) for a, v in re.findall(r"(\w+)=(-?\d+)", line))
        if line.split()[0] in ("fused", "dens", "shader"):
            lines[(line.split()[0], kv["rows"])] = kv
        elif kv:
            lines[line.split()[0]] = kv
    return d, k, b, lines


def _out(d, name):
    return np.fromfile(d / f"out_{name}.bin", dtype=np.float32)


def acc_feat(t, r, h):
    return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h


def rows_stride(no, nt):
    """Floats between the two half-wave rows: the row length in 128-byte units, made odd."""
    units = (no * nt * 16 + 31) // 32
    return 32 * (units + (units % 2 == 0))


def test_row_table_equals_lanes_0_and_32_of_the_dot_fragments(rows):
    d, k, b, lines = rows
    NO, NT = 3, 2
    n, stride = NO * NT * 16, rows_stride(NO, NT)
    assert lines["rows"]["stride"] == stride == 96 and stride * 4 % 256 == 128
    dot = _out(d, "rows_dot").view(np.uint32).reshape(NO * NT * 16 + NO, 64)
    # pack_dot itself against the layer (what tests/test_hostcheck.py pins), then the two floats of every fragment
    for o in range(NO):
        for t in range(NT):
            for r in range(16):
                frag = dot[(o * NT + t) * 16 + r]
                assert (frag[:32] == frag[0]).all() and (frag[32:] == frag[32]).all()
                assert frag[0] == k[acc_feat(t, r, 0), o].view(np.uint32) and frag[32] == k[acc_feat(t, r, 1), o].view(np.uint32)
        assert (dot[NO * NT * 16 + o] == b[o].view(np.uint32)).all()
    for name, frags in (("rows", lines["rows"]["frags"]), ("rows_piece", lines["rows"]["piece_frags"])):
        tab = _out(d, name).view(np.uint32)
        assert tab.size == frags * 64
        want = np.zeros(tab.size, np.uint32)
        want[0:n] = dot[:n, 0]
        want[stride:stride + n] = dot[:n, 32]
        want[stride + n:stride + n + NO] = dot[n:, 0]
        assert np.array_equal(tab, want), name
    assert lines["rows"]["floats"] == stride + n + NO
    assert lines["rows"]["frags"] == -(-(stride + n + NO) // 64)
    assert lines["rows"]["piece_frags"] == 4 * -(-(stride + n + NO) // 256)


def _formulas(rows_layout, split):
    """Fragment offsets of the fused stream from the layer shapes (rc_pack_host.h rc_lfr, rc_dfr, rc_rfr, rc_rows_at)."""
    lfr = (lambda ks, nt: -(-ks // 8) * nt * 12) if split else (lambda ks, nt: ks * nt)
    dfr = (lambda no, nt: -(-(no * (nt * 16 + 1)) // 4) * 4) if split else (lambda no, nt: no * (nt * 16 + 1))
    piece = (lambda f: -(-f // 4) * 4) if split else (lambda f: f)

    def rfr(no, nt, to_piece):
        fl = rows_stride(no, nt) + no * nt * 16 + no
        return 4 * -(-fl // 256) if to_piece else -(-fl // 64)

    def place(f, nfr):          # a row table lies in one chunk
        return -(-f // CHUNK) * CHUNK if f // CHUNK != (f + nfr - 1) // CHUNK else f

    def block(f, no, nt, to_piece, fragments):
        if not rows_layout:
            return f, f + fragments
        at = place(f, rfr(no, nt, to_piece))
        return at, at + rfr(no, nt, to_piece)

    out, f, blocks = {}, 0, []
    for l, (ks0, no) in enumerate(((4, 1), (5, 1), (17, 4))):
        out[f"F_L{l}"] = f
        f += ks0 * 2 + 33 * 2                                   # density MLPs: fp32 fragments in every build
        at, f = block(f, no, 2, False, no * 33)
        out[f"DO{l}"] = at
        blocks.append((at, f))
    out["B1_2"] = f
    f += 32 * 2 + 32 * 1                                        # the backward fragments of level 2
    out["END2"] = f
    out["F_SH"] = sh = piece(f)
    s = {"F_H": 0}
    s["F_S0"] = s["F_H"] + lfr(49, 1)
    s["F_I0"] = s["F_S0"] + lfr(85, 8)
    s["F_I1"] = s["F_I0"] + lfr(49, 2)
    at, end = block(sh + s["F_I1"] + lfr(33, 2), 1, 2, split, dfr(1, 2))
    s["F_IO"], s["F_S1"] = at - sh, end - sh
    blocks.append((at, end))
    s["F_S2"] = s["F_S1"] + lfr(65, 4)
    s["F_SB"] = s["F_S2"] + lfr(65, 4)
    at, end = block(sh + s["F_SB"] + lfr(64, 4), 3, 4, split, dfr(3, 4))
    s["F_SO"], s["COUNT"] = at - sh, end - sh
    blocks.append((at, end))
    out["NF_FUSED"] = sh + s["COUNT"]
    out["chunks"] = -(-out["NF_FUSED"] // CHUNK)
    return out, s, blocks


@pytest.mark.parametrize("rows_layout", [0, 1])
def test_fused_offsets_match_the_formulas(rows, rows_layout):
    _, _, _, lines = rows
    split = bool(lines["rows"]["split"])
    want, shader, blocks = _formulas(bool(rows_layout), split)
    got = dict(lines[("fused", rows_layout)], **lines[("dens", rows_layout)])
    got.pop("rows")
    assert got == want, (got, want)
    sh = dict(lines[("shader", rows_layout)])
    sh.pop("rows")
    assert sh == shader, (sh, shader)
    if rows_layout:
        for lo, hi in blocks:
            assert lo // CHUNK == (hi - 1) // CHUNK, ("a row table straddles a chunk", lo, hi)
    if split:
        assert want["F_SH"] % 4 == 0
        assert all((want["F_SH"] + shader[k]) % 4 == 0 for k in ("F_H", "F_S0", "F_I0", "F_I1", "F_S1", "F_S2", "F_SB"))


def test_table_form_shortens_the_split_stream(rows):
    _, _, _, lines = rows
    assert lines["rows"]["split"] == 1           # `make hostcheck` builds the default arithmetic
    frag, tab = lines[("fused", 0)], lines[("fused", 1)]
    assert (frag["NF_FUSED"], frag["chunks"], frag["F_SH"]) == (3452, 54, 544)       # the fragment form, as before
    # five blocks of 33 + 33 + 132 + 36 + 196 = 430 fragments become 2 + 2 + 5 + 4 + 8 = 21, and level 2's table moves
    # from fragment 254 to the chunk start 256 (2 fragments of padding); F_SH's padding to a piece goes from 0 to 3
    assert frag["NF_FUSED"] - tab["NF_FUSED"] == 430 - 21 - 2 - 3
    assert tab["chunks"] == 48
    assert lines["layout"]["rows"] == 1 and lines["layout"]["NF_FUSED"] == tab["NF_FUSED"]
