"""`make hostcheck`: the host-only parts of the weight packing (csrc/rc_pack_host.h -- MFMA A-fragment packing, the
folded shader bottleneck, the cell-table index rule, the directional-encoding table) compiled for the CPU under
AddressSanitizer + UBSan and compared with numpy restatements of the layouts (sanitizers on the CPU build;
GPU sanitizers are not available on the pool).  A sanitizer report makes the program exit non-zero."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")


def acc_feat(t, r, h):
    """Feature that accumulator register r of tile t holds on half-wave h (v_mfma_f32_32x32x2_f32 D layout)."""
    return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h


def np_pack(steps, tiles, layers):
    """steps: [(row_h0, row_h1)], >= 0 input row, -1 zero, -2 bias.  tiles: [[(layer, col, bias_ok) or None] * 32]."""
    out = np.zeros((len(steps), len(tiles), 64), np.float32)
    for s, rows in enumerate(steps):
        for t, tile in enumerate(tiles):
            for lane in range(64):
                h, i = lane >> 5, lane & 31
                ent = tile[i]
                if ent is None:
                    continue
                name, col, bias_ok = ent
                k, b = layers[name]
                row = rows[h]
                if row == -2:
                    out[s, t, lane] = b[col] if bias_ok else 0.0
                elif row >= 0 and row < k.shape[0]:
                    out[s, t, lane] = k[row, col]
    return out.reshape(-1)


def unsplit(words, n_steps, n_tiles):
    """The split form of a layer (rc_pack_host.h pack_split: [block of 8 k-steps][tile][piece][lane][4 dwords], a dword = the
    bf16 of an even step in its low half and of the following step in its high half) back to [step][tile][lane] float32:
    the three pieces must add up to the packed weight EXACTLY, each must be the truncated top 16 bits of what the pieces
    in front of it leave, and the steps that pad the last block must be zero."""
    nb = (n_steps + 7) // 8
    w = np.asarray(words).view(np.uint32).reshape(nb, n_tiles, 3, 64, 4)
    halves = np.stack([w & 0xFFFF, w >> 16], axis=-1).reshape(nb, n_tiles, 3, 64, 8)          # [..., j] = step 8 q + j
    pieces = (halves.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    total = pieces.sum(axis=2)                                                                 # exact in float64
    val = total.astype(np.float32)
    assert np.array_equal(val.astype(np.float64), total)
    rest = val.astype(np.float32)
    for p in range(3):
        top = (rest.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        assert np.array_equal(top.astype(np.float64), pieces[:, :, p])
        rest = (rest - top).astype(np.float32)
    assert not rest.any()
    out = val.transpose(0, 3, 1, 2).reshape(nb * 8, n_tiles, 64)                                # [step][tile][lane]
    assert not out[n_steps:].any()
    return out[:n_steps].reshape(-1)


def natural(K):
    return [(2 * i, 2 * i + 1 if 2 * i + 1 < K else -1) for i in range((K + 1) // 2)]


def full_tile(name, t, out_dim, bias_ok=True):
    return [(name, 32 * t + i, bias_ok) if 32 * t + i < out_dim else None for i in range(32)]


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    r = subprocess.run(["make", "-C", CSRC, "hostcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    d = tmp_path_factory.mktemp("hostcheck")
    rng = np.random.default_rng(11)
    layers = {}
    for name, (i, o) in dict(a=(37, 70), b=(64, 40), c=(9, 5), d=(64, 3), bott=(12, 16), cons=(21, 9)).items():
        k = rng.normal(size=(i, o)).astype(np.float32)
        b = rng.normal(size=(o,)).astype(np.float32)
        k.tofile(d / f"in_{name}_kernel.bin")
        b.tofile(d / f"in_{name}_bias.bin")
        layers[name] = (k, b)
    grid = rng.normal(size=(5, 5, 5, 2)).astype(np.float32)          # [z, y, x, F] = entry ((k2-1) N + (k1-1)) N + (k0-1)
    grid.tofile(d / "in_grid.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(CSRC, "hostcheck"), str(d)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "hostcheck ok" in r.stdout, r.stdout + r.stderr       # non-zero: a sanitizer report
    return d, layers, grid


@pytest.fixture(scope="module")
def tbins(tmp_path_factory):
    """`hostcheck --tbins`: the two per-bin head layers of the time-resolved cache through the three packing functions."""
    r = subprocess.run(["make", "-C", CSRC, "hostcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    d = tmp_path_factory.mktemp("hostcheck_tbins")
    rng = np.random.default_rng(12)
    layers = {}
    for name, (i, o) in dict(slf=(128, 71), irr=(64, 70)).items():
        k = rng.normal(size=(i, o)).astype(np.float32)
        b = rng.normal(size=(o,)).astype(np.float32)
        k.tofile(d / f"in_{name}_kernel.bin")
        b.tofile(d / f"in_{name}_bias.bin")
        layers[name] = (k, b)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(CSRC, "hostcheck"), "--tbins", str(d)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "hostcheck tbins ok" in r.stdout, r.stdout + r.stderr       # non-zero: a sanitizer report
    return d, layers


def _out(d, name):
    return np.fromfile(d / f"out_{name}.bin", dtype=np.float32)


def test_fragment_packing_matches_numpy(hostcheck):
    d, layers, _ = hostcheck
    want = np_pack(natural(37) + [(-2, -1)], [full_tile("a", t, 70) for t in range(3)], layers)
    assert np.array_equal(unsplit(_out(d, "pack"), 20, 3), want)
    acc_steps = [(acc_feat(t, r, 0), acc_feat(t, r, 1)) for t in range(2) for r in range(16)]
    want = np_pack(acc_steps, [full_tile("b", t, 40, False) for t in range(2)], layers)
    assert np.array_equal(unsplit(_out(d, "pack_acc"), 32, 2), want)
    # "by register": output r sits in accumulator register r of BOTH half-waves = tile rows (r & 3) + 8 (r >> 2) + 4 h
    tile = [None] * 32
    for i in range(32):
        r = (i & 3) + 4 * (i >> 3)
        if r < 5:
            tile[i] = ("c", r, True)
    want = np_pack(natural(9) + [(-2, -1)], [tile], layers)
    assert np.array_equal(unsplit(_out(d, "by_reg"), 6, 1), want)


def _head_tiles(layers, t):
    """[step][lane] float32 of column tile t of the two per-bin heads: slf over 4 accumulator tiles + bias, irr over 2."""
    s4 = [(acc_feat(q, r, 0), acc_feat(q, r, 1)) for q in range(4) for r in range(16)] + [(-2, -1)]
    s2 = [(acc_feat(q, r, 0), acc_feat(q, r, 1)) for q in range(2) for r in range(16)] + [(-2, -1)]
    pa = np_pack(s4, [full_tile("slf", t, 71)], layers).reshape(65, 64)
    pb = np_pack(s2, [full_tile("irr", t, 70)], layers).reshape(33, 64)
    return pa, pb


def test_transient_bins_stream_matches_numpy(tbins):
    """rc_pack_host.h pack_bins_stream, what repack_transient uploads for k_transient_bins, in both forms: per column tile
    [slf | irr], zero fragments up to the tile's whole chunks.  cols = 70 is no multiple of 32: the last tile's entries
    71..95 are zero columns; entry 70 holds slf's column 70 (the alpha of output_rgba_layer, entry 2100 of the library's
    stream, which k_transient_bins never stores) and a zero irr column."""
    d, layers = tbins
    split = _out(d, "tbins_split").reshape(3, 192 * 64)
    f32 = _out(d, "tbins_f32").reshape(3, 128, 64)
    for t in range(3):
        pa, pb = _head_tiles(layers, t)
        # split form: 9 blocks of the slf head (108 fragments), 5 of the irr head (60), zeros behind
        assert np.array_equal(unsplit(split[t, :108 * 64], 65, 1).reshape(65, 64), pa)
        assert np.array_equal(unsplit(split[t, 108 * 64:168 * 64], 33, 1).reshape(33, 64), pb)
        assert not split[t, 168 * 64:].view(np.uint32).any()
        # fp32 form: 16 groups of [slf 4 g .. 4 g + 3 | irr 2 g, 2 g + 1], then [slf 64 | irr 32], zeros behind
        want = []
        for g in range(16):
            want += [pa[4 * g + q] for q in range(4)] + [pb[2 * g + q] for q in range(2)]
        want += [pa[64], pb[32]]
        assert np.array_equal(f32[t, :98].view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
        assert not f32[t, 98:].view(np.uint32).any()
    pa, pb = _head_tiles(layers, 2)
    assert not pa[:, [l for l in range(64) if (l & 31) >= 7]].any() and pa[:, :7].all()
    assert not pb[:, [l for l in range(64) if (l & 31) >= 6]].any() and pb[:, :6].all()


def test_transient_slice_columns_match_numpy(tbins):
    """pack_slice_columns: column f of a head is `stride` floats, value j = 2 step + half of the accumulator-order steps
    (feature acc_feat(j // 32, (j // 2) % 16, j & 1)), the bias at 2 x steps, zeros behind."""
    d, layers = tbins
    for name, ntiles, stride in (("slf", 4, 132), ("irr", 2, 68)):
        k, b = layers[name]
        got = _out(d, "tslice_" + name).reshape(70, stride)
        K = 32 * ntiles
        rows = [acc_feat(j // 32, (j // 2) % 16, j & 1) for j in range(K)]
        assert sorted(rows) == list(range(K))
        want = np.zeros((70, stride), np.float32)
        want[:, :K] = k[rows, :70].T
        want[:, K] = b[:70]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_temporal_taps_match_numpy(tbins):
    """temporal_taps (render.py:406-408): float32 arithmetic step by step, the sum in tap order; bit for bit."""
    d, _ = tbins
    v = _out(d, "ttaps")
    at = 0
    for sigma, count in ((3.0, 25), (4.0, 33), (0.7, 7), (0.0, 0)):
        assert int(v[at]) == count
        got = v[at + 1:at + 1 + count]
        at += 1 + count
        if not count:
            continue
        half = (count - 1) // 2
        assert half == int(np.floor(4.0 * sigma + 0.5))
        kk = np.arange(-half, half + 1).astype(np.float32)
        sg = np.float32(sigma)
        arg = -(kk * kk) / (np.float32(2.0) * sg * sg)
        e64 = np.exp(arg.astype(np.float64))
        raw = e64.astype(np.float32) - np.float32(np.exp(-8.0))
        tot = np.float32(0.0)
        for x in raw:
            tot = np.float32(tot + x)
        want = raw / tot
        # (expf returns the float nearest to the exact value at these 33 arguments: the fp64 exp, rounded once)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
        assert np.array_equal(got, got[::-1]) and abs(float(got.astype(np.float64).sum()) - 1.0) < count * 2.0 ** -24
    assert at == v.size


def test_dot_fragments_match_numpy(hostcheck):
    d, layers, _ = hostcheck
    k, b = layers["d"]
    want = []
    for o in range(3):
        for t in range(2):
            for r in range(16):
                want.append([k[acc_feat(t, r, lane >> 5), o] for lane in range(64)])
    for o in range(3):
        want.append([b[o]] * 64)
    want = np.asarray(want, np.float32).reshape(-1)
    got = _out(d, "dot")                     # padded with zero fragments to whole 1-KiB pieces (rc_dfr)
    assert got.size == (3 * 33 + 3) // 4 * 4 * 64 and np.array_equal(got[:want.size], want) and not got[want.size:].any()


def test_folded_bottleneck_matches_fp64_product(hostcheck):
    d, layers, _ = hostcheck
    (kb, bb), (kc, _) = layers["bott"], layers["cons"]
    wk = np.concatenate([(kb.astype(np.float64) @ kc[:16].astype(np.float64)).astype(np.float32), kc[16:21]])
    wb = (bb.astype(np.float64) @ kc[:16].astype(np.float64)).astype(np.float32)
    got_k, got_b = _out(d, "fold_kernel").reshape(17, 9), _out(d, "fold_bias")
    # the C++ sums its 16 products in index order in fp64; numpy's dot may pair them differently: one float32 ulp
    assert np.allclose(got_k, wk, rtol=0, atol=1e-6) and np.array_equal(got_k[12:], kc[16:21])
    assert np.allclose(got_b, wb, rtol=0, atol=1e-6)


def test_cell_table_matches_padded_volume(hostcheck):
    d, _, grid = hostcheck
    N, F, M = 5, 2, 8
    pad = np.zeros((N + 2, N + 2, N + 2, F), np.float32)             # [k2, k1, k0]: zero padding at 0 and N + 1
    pad[1:-1, 1:-1, 1:-1] = grid
    want = np.zeros((M, M, M, 8, F), np.float32)                     # [q2, q1, q0, corner]
    for q2 in range(M):
        for q1 in range(M):
            for q0 in range(M):
                for c in range(8):
                    b0, b1, b2 = (c >> 2) & 1, (c >> 1) & 1, c & 1
                    k0, k1, k2 = (min(max(q - 1 + b, 0), N + 1) for q, b in ((q0, b0), (q1, b1), (q2, b2)))
                    want[q2, q1, q0, c] = pad[k2, k1, k0]
    assert np.array_equal(_out(d, "cells"), want.reshape(-1))


def test_ide_table_matches_the_oracle(hostcheck):
    import sys
    sys.path.insert(0, ROOT)
    from oracle import mathx
    d, _, _ = hostcheck
    v = _out(d, "ide")
    coef = v[: 36 * 17].reshape(36, 17)
    m = v[36 * 17: 36 * 17 + 36]
    sigma = v[36 * 17 + 36:]
    ml, mat = mathx.ide_tables(5)                                    # ml [2, 36] (m, l), mat [k, term]
    ml, mat = np.asarray(ml), np.asarray(mat, np.float64)
    assert np.array_equal(m, ml[0].astype(np.float32))
    l = ml[1].astype(np.float64)
    assert np.allclose(sigma, 0.5 * l * (l + 1))
    assert np.allclose(coef[:, : mat.shape[0]], mat.T.astype(np.float32), rtol=1e-6, atol=0)
    assert not coef[:, mat.shape[0]:].any()


# ---- the workspace registry (csrc/rc_ws.h) ---------------------------------------------------------------------------
# The table as it stood before the registry moved into its own header: the 21 structs in the order of the set's variant
# (RenderWs first: every set has one), the prefix of the set that holds each, and their buffers.  "name#" is a per-level
# buffer ("name0" ..).
WS_STRUCTS = [
    ("RenderWs", "", "sdist# tdist# means# feat# density# weights# hbuf normals_pred normals_grad jac app shade debug env_rgb "
                     "rgb_noenv acc_ws inds src_idx filt_weight acc_sel feat_sel hbuf_sel normals_sel density_sel t_irr t_slf tshade"),
    ("ExtraWs", "", "m_pts m_nrm m_feat m_mat m_feat_all m_mat_all l_feat l_vmf l_vmf_logit sec_origins sec_dirs sec_near sec_far "
                    "sec_lights sec_samples m_local_view sec_rgb sec_acc sec_env sh_origins sh_dirs sh_near sh_far sh_normals "
                    "sh_lights sh_acc"),
    ("TrainWs", "t:", "feat dfeat a1 a2 d1 d2 fe graw density partial"),
    ("InterlevelWs", "i:", "d_density# points# loss_ray"),
    ("DataWs", "d:", "rgb loss_ray d_density d_rgbs points f96 heads p3 ib_in x328 s0 s1 sb i1 i2 io so dheads dio dso dsb dx328 "
                     "ds1 ds0 di2 di1 dib_in db128 dp3 df96 dfeat dapp part ones"),
    ("GeometryWs", "g:", "loss_ray d_density d_pred points h64 dfeat part ones reg_part"),
    ("OptimWs", "o:", "part norm mult stage"),
    ("LightWs", "ls:", "cache_rgb cache_acc h0 h1 vp dvp dh1 dh0 dfeat loss_ray part ones reg_part"),
    ("MaterialWs", "ms:", "cache_rgb cache_acc pts feat mat_p loss_ray loss_part dfeat part reg_part"),
    ("MatDataWs", "md:", "cache_rgb cache_acc rgb loss_ray dmat dfeat part loss_part d_env e_h0 e_h1 e_xb e_hb e_raw e_draw e_dhb "
                         "e_dxb e_dh1 e_dh0 e_part e_ones"),
    ("TransDataWs", "td:", "rgb G Gt loss_ray dz_irr dz_slf x_irr x_slf part ones d_t_irr d_t_slf d_tint_ibrdf d_direct d_weights "
                           "d_density points"),
    ("EvalWs", "ev:", "binsum_pred binsum_gt post_pred post_gt part si_metric si_state si_part"),
    ("AlbedoWs", "ea:", "pairs wg state part"),
    ("VisWs", "vz:", "state part maxpart binsum"),
    ("MaskWs", "mk:", "loss_ray d_density points"),
    ("RelightWs", "rl:", "part best"),
    ("NormalsWs", "nb:", "feat jac gf ghat u t0 a0 t1 a2 ones partial normals"),
    ("GSmoothWs", "gs:", "means_p feat_p jac_p density_p normals_p points points_p d_normals d_normals_p d_density d_density_p "
                         "loss_ray"),
    ("QueryWs", "q:", "means feat jac density normals_pred normals_grad m_feat"),
    ("IsoWs", "iso:", "mask tcount tile_v tile_t group_v group_t group_off vbase state"),
    ("AtlasWs", "atlas:", "points owner hidden app_feat"),
]
WS_BARE_PREFIXES = ("p1:", "p2:", "p3:", "s:")          # WS_RENDER1-3 and WS_SECONDARY: a RenderWs and nothing else
WS_MAX_LEVELS = 3                                      # RC_MAX_LEVELS
WS_PROBES = ("bogus:feat", "x:hbuf", "zz", "i:nothing", "hbuf9", "hbuf0", "sdist", "sdist3", "i:points", "i:d_density2", "d:f97",
             "T:feat", "atlas", ":hbuf", "q:", "td:g")


def _ws_fields(k):
    """{leaf: per-level?} of struct k of WS_STRUCTS"""
    return {f.rstrip("#"): f.endswith("#") for f in WS_STRUCTS[k][2].split()}


def _ws_expected(kind, leaf, digit, num_levels):
    """(struct index, field, level) that "<leaf><digit>" reaches in a set holding struct `kind` (0: none beside its RenderWs),
    or None: RenderWs first, then the held struct; a per-level buffer takes the digits 0 .. num_levels - 1, InterlevelWs' only
    0 .. num_levels - 2, any other buffer no digit."""
    for k in ([0, kind] if kind else [0]):
        per_level = _ws_fields(k).get(leaf)
        if per_level is None:
            continue
        if not per_level and digit is None:
            return k, leaf, -1
        if per_level and digit is not None and digit < num_levels - (1 if WS_STRUCTS[k][0] == "InterlevelWs" else 0):
            return k, leaf, digit
    return None


@pytest.mark.parametrize("num_levels", [3, 2])
def test_workspace_registry_resolves_the_table(num_levels):
    """`hostcheck --ws`: every set holds the struct of its kind and is asked for every name of the whole table under its own
    prefix, bare and with the digits 0 .. RC_MAX_LEVELS.  What resolves, and to which buffer, is what the literal table
    above and the lookup rule say; nothing else resolves; the sanitizers report nothing."""
    r = subprocess.run(["make", "-C", CSRC, "hostcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(CSRC, "hostcheck"), "--ws", str(num_levels), *WS_PROBES], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.endswith("hostcheck ws ok\n") and not r.stderr, r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    hits = {}
    for ln in lines:
        if ln.startswith("hit "):
            _, full, kind, field, level, off = ln.split()
            assert hits.setdefault(full, (int(kind), field, int(level), int(off))) == (int(kind), field, int(level), int(off))
    assert len(WS_STRUCTS) == 21 and len({s[0] for s in WS_STRUCTS}) == 21
    sets = [(prefix, k) for k, (_, prefix, _) in enumerate(WS_STRUCTS) if k] + [(p, 0) for p in WS_BARE_PREFIXES]
    assert len({p for p, _ in sets}) == 24
    leaves = sorted({leaf for k in range(len(WS_STRUCTS)) for leaf in _ws_fields(k)})
    want, lookups = {}, 0
    for prefix, kind in sets:
        for leaf in leaves:
            for digit in [None] + list(range(WS_MAX_LEVELS + 1)):
                e = _ws_expected(kind, leaf, digit, num_levels)
                if e is not None:
                    want[prefix + leaf + ("" if digit is None else str(digit))] = e
    assert {k: v[:3] for k, v in hits.items()} == want
    # the program asked for every row of the table, 5 spellings each, in each of the 24 sets, then for the probes
    rows = sum(len(_ws_fields(k)) for k in range(len(WS_STRUCTS)))
    assert lines[-2].split() == ["lookups", str(24 * rows * (WS_MAX_LEVELS + 2) + len(WS_PROBES)), "buffers",
                                 str(sum((WS_MAX_LEVELS if lv else 1) for p, k in sets for kk in {0, k} for lv in _ws_fields(kk).values()))]
    # every name of a struct resolves under its set's prefix (a name RenderWs has too reaches RenderWs), to distinct buffers
    for prefix, kind in sets:
        for k in {0, kind}:
            offs = []
            for leaf, per_level in _ws_fields(k).items():
                top = num_levels - (1 if WS_STRUCTS[k][0] == "InterlevelWs" else 0)
                for name in ([f"{leaf}{d}" for d in range(top)] if per_level else [leaf]):
                    got = hits[prefix + name]
                    assert got[0] in (0, k) and got[1] == leaf, (prefix, name, got)
                    if got[0] == k:
                        offs.append(got[3])
            assert len(set(offs)) == len(offs), (prefix, k)
    probes = {ln.split()[1]: ln.split()[2:] for ln in lines if ln.startswith("probe ")}
    assert set(probes) == set(WS_PROBES)
    for name, (set_id, off) in probes.items():
        assert off == "-", name
        assert (set_id == "-1") == (":" in name and name.split(":")[0] + ":" not in {p for p, _ in sets}), name
