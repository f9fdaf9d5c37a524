"""k_gemm (csrc/rc_data.hip) and k_gemm_tile (csrc/rc_envmap_bwd.hip) on their own contract, RcGemmArgs (csrc/rc_internal.h):
the cases, an fp64 reference, fp32 / bf16 emulations and the file format of the driver tests/gemm_check.hip.  numpy only.

A case is a dict of RcGemmArgs' fields as element counts, strides and offsets in floats into numbered backing buffers.
Every backing buffer has GUARD floats in front and behind, and every float that is not a logical element of an operand is
a canary NaN (CANARY): a read outside an operand turns C into NaN, a write outside C changes a canary; neither needs a
fault to be seen.

Case file (little endian): int64 [magic, n_buf, n_case, len(FIELDS)], int64 [n_buf][2] (first float, floats; first float
-1: a buffer of canaries alone, not stored), int64 [n_case][len(FIELDS)], then the float32 data of the stored buffers.
Result file: int64 [magic, CUs, n_case, driver wall time in us], int64 [n_case][2][5] (address & 15 of the a, b, c, bias and
mask bases per launcher, -1 for a null pointer), then per case and launcher (0 k_gemm, 1 k_gemm_tile) the whole backing
buffer of C (all parts) and, for a case with `g_buf`, the whole buffer of the sums after k_sum_parts."""
import os
import re

import numpy as np

GUARD = 64
CANARY = 0x7FC0BEEF
MAGIC_CASES, MAGIC_RESULTS = 0x47454D4D43415345, 0x47454D4D52534C54
FIELDS = ("M", "N", "K", "a_buf", "a_off", "sai", "sak", "b_buf", "b_off", "sbk", "sbj", "c_buf", "c_off", "sci", "scj",
          "bias_buf", "bias_off", "mask_buf", "mask_off", "smi", "smj", "relu", "accumulate", "kslice", "spart", "kparts",
          "g_buf", "g_off")
MASK_VALUES = np.array([1.0, 1e-30, 0.0, -0.0, -1.0, np.nan], np.float32)
MUTATIONS = ("drop_last_k", "bias_jm1", "mask_ge", "relu_first", "b_shift")
U = 2.0 ** -24                               # unit roundoff of fp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
HOST_FILES = ("rc_data_host.inc", "rc_geometry_host.inc", "rc_light_host.inc", "rc_material_data_host.inc",
              "rc_transient_bwd_host.inc")
ROWS_M, ROWS_K, KSLICE = 257, 1031, 1024    # rows of a production descriptor where they are M / K; kDataKSlice


def canary(n):
    return np.full(n, CANARY, np.uint32).view(np.float32)


def is_canary(x):
    return x.view(np.uint32) == CANARY


def strided(buf, off, shape, strides):
    """The view v[i, j] = buf[off + i strides[0] + j strides[1]] (off counts from the buffer's first float, guard included)."""
    return np.lib.stride_tricks.as_strided(buf[off:], shape, tuple(4 * int(s) for s in strides), writeable=buf.flags.writeable)


def extent(shape, strides):
    """Floats from the base to one past the last logical element (0 for an empty operand)."""
    if min(shape) <= 0:
        return 0
    return sum((n - 1) * s for n, s in zip(shape, strides)) + 1


def parts_of(K, kslice):
    return max(1, -(-K // kslice)) if kslice > 0 else 1


# ---------------------------------------------------------------------------------------------------------------------------
# reference


def operand_views(c, bufs):
    A = strided(bufs[c["a_buf"]], c["a_off"], (c["M"], c["K"]), (c["sai"], c["sak"]))
    B = strided(bufs[c["b_buf"]], c["b_off"], (c["K"], c["N"]), (c["sbk"], c["sbj"]))
    bias = bufs[c["bias_buf"]][c["bias_off"]: c["bias_off"] + c["N"]] if c["bias_buf"] >= 0 else None
    mask = strided(bufs[c["mask_buf"]], c["mask_off"], (c["M"], c["N"]), (c["smi"], c["smj"])) if c["mask_buf"] >= 0 else None
    return A, B, bias, mask


def c_view(c, cbuf, z):
    return strided(cbuf, c["c_off"] + z * c["spart"], (c["M"], c["N"]), (c["sci"], c["scj"]))


def slice_bounds(c, z):
    k0 = min(c["K"], z * c["kslice"])
    return k0, min(c["K"], k0 + c["kslice"])


def reference(c, bufs, mutation=None):
    """RcGemmArgs' comment in fp64, in its order: C(i, j) (+)= sum_k A(i, k) B(k, j) (+ bias[j]), then ReLU, then zero where
    !(mask > 0) (-0.0, 0.0, negatives and NaN), per K slice z at z spart; a slice wholly beyond K sums nothing.  Returns
    {"parts": fp64 [kparts][M][N], "C": the expected backing buffer of C in fp32, "G": that of the sums (or None)}:
    G = out + (((p0 + p1) + p2) ...) in slice order in fp32, as k_sum_parts.  `mutation`: one of MUTATIONS, a deliberately
    wrong reading of the contract (tests/test_gemm_ref.py)."""
    c = dict(c)
    if mutation == "b_shift":
        c["b_off"] += 1
    if mutation == "bias_jm1":
        c["bias_off"] -= 1
    A, B, bias, mask = operand_views(c, bufs)
    cbuf = bufs[c["c_buf"]].copy()
    parts = []
    for z in range(c["kparts"]):
        k0, k1 = slice_bounds(c, z)
        if mutation == "drop_last_k" and k1 > k0:
            k1 -= 1
        v = A[:, k0:k1].astype(np.float64) @ B[k0:k1].astype(np.float64) + 0.0
        if bias is not None:
            v = v + bias.astype(np.float64)[None, :]
        cv = c_view(c, cbuf, z)
        if mutation == "relu_first" and c["relu"]:
            v = np.maximum(v, 0.0)
        if c["accumulate"]:
            v = cv.astype(np.float64) + v
        if c["relu"] and mutation != "relu_first":
            v = np.maximum(v, 0.0)
        if mask is not None:
            with np.errstate(invalid="ignore"):
                keep = (mask >= 0) if mutation == "mask_ge" else (mask > 0)
            v = np.where(keep, v, 0.0)
        parts.append(v)
        cv[...] = v.astype(np.float32)
    out = {"parts": np.stack(parts), "C": cbuf, "G": None}
    if c["g_buf"] >= 0:
        gbuf = bufs[c["g_buf"]].copy()
        n = c["spart"]
        s = np.zeros(n, np.float32)
        for z in range(c["kparts"]):
            s = s + cbuf[c["c_off"] + z * n: c["c_off"] + (z + 1) * n]                 # fp32 + fp32, rounded once
        gbuf[c["g_off"]: c["g_off"] + n] += s
        out["G"] = gbuf
    return out


def triple_loop(c, bufs):
    """`reference` as literal loops over flat indices (tests/test_gemm_ref.py holds the two against each other)."""
    a, b = bufs[c["a_buf"]], bufs[c["b_buf"]]
    cbuf = bufs[c["c_buf"]].copy()
    for z in range(c["kparts"]):
        k0, k1 = slice_bounds(c, z)
        for i in range(c["M"]):
            for j in range(c["N"]):
                s = 0.0
                for k in range(k0, k1):
                    s += float(a[c["a_off"] + i * c["sai"] + k * c["sak"]]) * float(b[c["b_off"] + k * c["sbk"] + j * c["sbj"]])
                if c["bias_buf"] >= 0:
                    s += float(bufs[c["bias_buf"]][c["bias_off"] + j])
                at = c["c_off"] + z * c["spart"] + i * c["sci"] + j * c["scj"]
                if c["accumulate"]:
                    s = float(cbuf[at]) + s
                if c["relu"]:
                    s = max(s, 0.0)
                if c["mask_buf"] >= 0 and not float(bufs[c["mask_buf"]][c["mask_off"] + i * c["smi"] + j * c["smj"]]) > 0.0:
                    s = 0.0
                cbuf[at] = np.float32(s)
    return cbuf


def exact_precondition(c):
    """Operands are multiples of 1/8 in [-1, 1]: every product is a multiple of 2^-6, every partial sum of at most K products,
    the bias, the old C and the sums of k_sum_parts a multiple of 2^-6 below (K + 3): exact in fp32 while (K + 3) 64 < 2^24."""
    return (c["K"] + 3) * 64 < 2 ** 24


def rounding_bound(c, bufs):
    """Per element and part: 2 (K + 2) 2^-24 (sum_k |a||b| + |bias| + |old C|), the sequential-sum bound of round-to-nearest,
    doubled (whether the matrix pipe rounds each product and add to nearest is not measured here)."""
    A, B, bias, _ = operand_views(c, bufs)
    out = []
    for z in range(c["kparts"]):
        k0, k1 = slice_bounds(c, z)
        m = np.abs(A[:, k0:k1].astype(np.float64)) @ np.abs(B[k0:k1].astype(np.float64))
        if bias is not None:
            m = m + np.abs(bias.astype(np.float64))[None, :]
        if c["accumulate"]:
            m = m + np.abs(c_view(c, bufs[c["c_buf"]], z).astype(np.float64))
        out.append(2.0 * (c["K"] + 2) * U * m)
    return np.stack(out)


def emulate_f32(c, bufs, truncate_bf16=False):
    """The kernels' arithmetic in numpy fp32, in their k order: per step two k (the lanes l >> 5 of v_mfma_f32_32x32x2_f32),
    each product and each add rounded on its own; then bias, old C.  truncate_bf16: the operands cut to their top 16 bits
    first (what a reduced-precision pipe would see)."""
    A, B, bias, _ = operand_views(c, bufs)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    if truncate_bf16:
        A = (A.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        B = (B.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    parts = []
    for z in range(c["kparts"]):
        k0, k1 = slice_bounds(c, z)
        acc = np.zeros((c["M"], c["N"]), np.float32)
        for k in range(k0, k1):
            acc = acc + A[:, k, None] * B[None, k, :]                    # float32 product, float32 add
        if bias is not None:
            acc = acc + bias[None, :]
        if c["accumulate"]:
            acc = c_view(c, bufs[c["c_buf"]], z) + acc
        if c["relu"]:
            acc = np.maximum(acc, np.float32(0))
        parts.append(acc.astype(np.float64))
    return np.stack(parts)


# ---------------------------------------------------------------------------------------------------------------------------
# the launcher's choices, restated (csrc/rc_envmap_bwd.hip: panel_mode, rc_launch_gemm_tile)


def panel_mode(align, s_mn, s_k, kslice):
    aligned = align == 0
    if s_k == 1:
        return 2 if (aligned and s_mn % 4 == 0 and kslice % 4 == 0) else 0
    if s_mn == 1:
        return 1 | (2 if (aligned and s_k % 4 == 0) else 0)
    return 0


def big_instantiation(c, cus):
    return ((c["M"] + 127) // 128) * ((c["N"] + 127) // 128) * c["kparts"] >= cus


# ---------------------------------------------------------------------------------------------------------------------------
# cases


class Cases:
    def __init__(self, seed=20250711):
        self.rng = np.random.default_rng(seed)
        self.bufs, self.cases = [], []

    def eighths(self, shape, nonzero=False):
        """Integers in [-8, 8] / 8 (A and B: without 0, so that no single product vanishes)."""
        v = self.rng.integers(-8, 9, size=shape)
        if nonzero:
            v = np.where(v == 0, 8, v)
        return (v / 8.0).astype(np.float32)

    def uniform(self, shape):
        return (self.rng.random(size=shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)

    def buffer(self, floats):
        self.bufs.append(canary(floats + 2 * GUARD))
        return len(self.bufs) - 1

    def operand(self, off, shape, strides, values):
        """A new backing buffer with `values` at base offset `off` and the given strides; returns (buffer, offset field)."""
        b = self.buffer(off + extent(shape, strides))
        if min(shape) > 0:
            strided(self.bufs[b], GUARD + off, shape, strides)[...] = values
        return b, GUARD + off

    def add(self, name, group, M, N, K, A, B, C, *, bias=False, mask=None, relu=0, accumulate=0, kslice=None, kparts=None,
            sum_parts=False, family="exact", src=None, spart=None, share=None):
        """A, B, C, mask: (stride of the first index, of the second, base offset in floats).  share: a case whose A and B
        buffers this one reads (at its own offsets and strides)."""
        draw = (lambda s, nz=False: self.eighths(s, nz)) if family == "exact" else (lambda s, nz=False: self.uniform(s))
        kslice = K if kslice is None else kslice
        kparts = parts_of(K, kslice) if kparts is None else kparts
        c = dict(name=name, group=group, family=family, src=src, M=M, N=N, K=K, relu=int(relu), accumulate=int(accumulate),
                 kslice=kslice, kparts=kparts)
        c["sai"], c["sak"], c["sbk"], c["sbj"], c["sci"], c["scj"] = A[0], A[1], B[0], B[1], C[0], C[1]
        if share is None:
            a_shape = tuple(n if s else 1 for n, s in zip((M, K), A[:2]))           # a 0 stride: one value, broadcast
            b_shape = tuple(n if s else 1 for n, s in zip((K, N), B[:2]))
            c["a_buf"], c["a_off"] = self.operand(A[2], a_shape, [s or 1 for s in A[:2]], draw(a_shape, True))
            c["b_buf"], c["b_off"] = self.operand(B[2], b_shape, [s or 1 for s in B[:2]], draw(b_shape, True))
        else:
            c["a_buf"], c["b_buf"] = share["a_buf"], share["b_buf"]
            c["a_off"], c["b_off"] = GUARD + A[2], GUARD + B[2]
        c["spart"] = (extent((M, N), C[:2]) if kparts > 1 else 0) if spart is None else spart
        c["c_buf"] = self.buffer(C[2] + (kparts - 1) * c["spart"] + extent((M, N), C[:2]))
        c["c_off"] = GUARD + C[2]
        if accumulate:
            for z in range(kparts):
                c_view(c, self.bufs[c["c_buf"]], z)[...] = draw((M, N))
        c["bias_buf"], c["bias_off"] = self.operand(0, (N,), (1,), draw((N,))) if bias else (-1, 0)
        c["mask_buf"], c["mask_off"], c["smi"], c["smj"] = -1, 0, 0, 0
        if mask is not None:
            vals = np.resize(MASK_VALUES, M * N)                        # every value present (M N >= 6), in random places
            self.rng.shuffle(vals)
            c["mask_buf"], c["mask_off"] = self.operand(mask[2], (M, N), mask[:2], vals.reshape(M, N))
            c["smi"], c["smj"] = mask[0], mask[1]
        c["g_buf"], c["g_off"] = -1, 0
        if sum_parts:
            g = draw((c["spart"],))
            c["g_buf"], c["g_off"] = self.operand(0, g.shape, (1,), np.where(g == 0, np.float32(0.5), g))
        self.cases.append(c)
        return c

    def unsliced(self, c):
        """Slice z of `c` as a launch of its own on rows [z kslice, min(K, (z + 1) kslice)) of the same buffers."""
        for z in range(c["kparts"]):
            k0, k1 = slice_bounds(c, z)
            C = (c["sci"], c["scj"], c["c_off"] - GUARD)
            d = self.add(f"{c['name']}/slice{z}", "unsliced", c["M"], c["N"], k1 - k0,
                         (c["sai"], c["sak"], c["a_off"] - GUARD + k0 * c["sak"]),
                         (c["sbk"], c["sbj"], c["b_off"] - GUARD + k0 * c["sbk"]), C, share=c, family=c["family"])
            d["parent"], d["slice"] = c["name"], z
            d["bias_buf"], d["bias_off"] = c["bias_buf"], c["bias_off"]
            d["mask_buf"], d["mask_off"], d["smi"], d["smj"] = c["mask_buf"], c["mask_off"], c["smi"], c["smj"]
            d["relu"] = c["relu"]
            if c["accumulate"]:
                d["accumulate"] = 1
                c_view(d, self.bufs[d["c_buf"]], 0)[...] = c_view(c, self.bufs[c["c_buf"]], z)


# The production descriptors: every dense_fwd / dense_dx / dense_wgrad call (and _tile form) of the five host files and the
# hand-built descriptor of rc_material_data_host.inc, by source line.  Layer = (in, out).
#   ("fwd", in, out, ldx, x_off, ldy, y_off, relu)
#   ("dx", in, out, ldy, y_off, ldx, x_off, j0, nj, mask row stride or None, accumulate)
#   ("wgrad", in, out, ldx, x_off, ldy, y_off)            -> two descriptors: the kernel's pass and the bias pass
_D, _G, _L, _M, _T = HOST_FILES
PRODUCTION = [
    # rc_data_host.inc: the recompute
    (_D, 122, ("fwd", 96, 1, 96, 0, 10, 0, 0)), (_D, 123, ("fwd", 96, 3, 96, 0, 10, 1, 0)),
    (_D, 124, ("fwd", 96, 3, 96, 0, 10, 4, 0)), (_D, 125, ("fwd", 96, 3, 96, 0, 10, 7, 0)),
    (_D, 126, ("fwd", 64, 3, 96, 0, 3, 0, 0)), (_D, 127, ("fwd", 96, 128, 96, 0, 328, 128, 0)),
    (_D, 128, ("fwd", 96, 128, 96, 0, 129, 0, 0)), (_D, 130, ("fwd", 129, 64, 129, 0, 64, 0, 1)),
    (_D, 131, ("fwd", 64, 64, 64, 0, 64, 0, 1)), (_D, 132, ("fwd", 64, 1, 64, 0, 1, 0, 0)),
    (_D, 133, ("fwd", 200, 128, 328, 128, 128, 0, 1)), (_D, 134, ("fwd", 128, 128, 128, 0, 128, 0, 1)),
    (_D, 135, ("fwd", 128, 128, 128, 0, 328, 0, 1)), (_D, 136, ("fwd", 328, 128, 328, 0, 128, 0, 1)),
    (_D, 137, ("fwd", 128, 3, 128, 0, 3, 0, 0)),
    # the input gradients
    (_D, 140, ("dx", 128, 3, 3, 0, 128, 0, 0, 128, 128, 0)), (_D, 141, ("dx", 328, 128, 128, 0, 328, 0, 0, 128, 328, 0)),
    (_D, 142, ("dx", 328, 128, 128, 0, 328, 0, 128, 200, None, 0)), (_D, 143, ("dx", 128, 128, 328, 0, 128, 0, 0, 128, 128, 0)),
    (_D, 144, ("dx", 128, 128, 128, 0, 128, 0, 0, 128, 128, 0)), (_D, 145, ("dx", 200, 128, 128, 0, 328, 128, 0, 200, None, 1)),
    (_D, 146, ("dx", 64, 1, 1, 0, 64, 0, 0, 64, 64, 0)), (_D, 147, ("dx", 64, 64, 64, 0, 64, 0, 0, 64, 64, 0)),
    (_D, 148, ("dx", 129, 64, 64, 0, 129, 0, 0, 129, None, 0)), (_D, 150, ("dx", 96, 128, 128, 0, 96, 0, 0, 96, None, 0)),
    (_D, 151, ("dx", 96, 1, 10, 0, 96, 0, 0, 96, None, 1)), (_D, 152, ("dx", 96, 3, 10, 1, 96, 0, 0, 96, None, 1)),
    (_D, 153, ("dx", 96, 3, 10, 4, 96, 0, 0, 96, None, 1)), (_D, 154, ("dx", 96, 3, 10, 7, 96, 0, 0, 96, None, 1)),
    (_D, 155, ("dx", 64, 3, 3, 0, 96, 0, 0, 64, None, 1)),
    # the weight gradients (the lambda of line 160 at each of its calls)
    (_D, 162, ("wgrad", 64, 3, 96, 0, 3, 0)), (_D, 163, ("wgrad", 96, 128, 96, 0, 128, 0)),
    (_D, 164, ("wgrad", 96, 1, 96, 0, 10, 0)), (_D, 165, ("wgrad", 96, 3, 96, 0, 10, 1)),
    (_D, 166, ("wgrad", 96, 3, 96, 0, 10, 4)), (_D, 167, ("wgrad", 96, 3, 96, 0, 10, 7)),
    (_D, 168, ("wgrad", 129, 64, 129, 0, 64, 0)), (_D, 169, ("wgrad", 64, 64, 64, 0, 64, 0)),
    (_D, 170, ("wgrad", 64, 1, 64, 0, 1, 0)), (_D, 171, ("wgrad", 200, 128, 328, 128, 128, 0)),
    (_D, 172, ("wgrad", 128, 128, 128, 0, 128, 0)), (_D, 173, ("wgrad", 128, 128, 128, 0, 328, 0)),
    (_D, 174, ("wgrad", 328, 128, 328, 0, 128, 0)), (_D, 175, ("wgrad", 128, 3, 128, 0, 3, 0)),
    # rc_geometry_host.inc: pred_normals_layer (no bias in the forward; d_pred offset by 3 c0)
    (_G, 110, ("wgrad", 64, 3, 64, 0, 3, 3)), (_G, 112, ("dx", 64, 3, 3, 3, 64, 0, 0, 64, None, 0)),
    # rc_light_host.inc: the three layers of each loop
    (_L, 73, ("fwd", 32, 64, 32, 0, 64, 0, 1)), (_L, 73, ("fwd", 64, 64, 64, 0, 64, 0, 1)), (_L, 73, ("fwd", 64, 640, 64, 0, 640, 0, 0)),
    (_L, 99, ("wgrad", 32, 64, 32, 0, 64, 0)), (_L, 99, ("wgrad", 64, 64, 64, 0, 64, 0)), (_L, 99, ("wgrad", 64, 640, 64, 0, 640, 0)),
    (_L, 100, ("dx", 32, 64, 64, 0, 32, 0, 0, 32, None, 0)), (_L, 100, ("dx", 64, 64, 64, 0, 64, 0, 0, 64, 64, 0)),
    (_L, 100, ("dx", 64, 640, 640, 0, 64, 0, 0, 64, 64, 0)),
    # rc_material_data_host.inc: the EnvMap (enc = xb + 256, row stride 288)
    (_M, 62, ("fwd", 27, 256, 288, 256, 256, 0, 1)), (_M, 63, ("fwd", 256, 256, 256, 0, 256, 0, 1)),
    (_M, 64, ("fwd", 256, 256, 256, 0, 288, 0, 1)), (_M, 65, ("fwd", 283, 128, 288, 0, 128, 0, 1)),
    (_M, 66, ("fwd", 128, 4, 128, 0, 4, 0, 0)), (_M, 69, ("dx", 128, 4, 4, 0, 128, 0, 0, 128, 128, 0)),
    (_M, 72, ("dx", 283, 128, 128, 0, 256, 0, 0, 256, 288, 0)),          # hand-built: the mask's row stride is not dX's
    (_M, 78, ("dx", 256, 256, 256, 0, 256, 0, 0, 256, 256, 0)), (_M, 79, ("dx", 256, 256, 256, 0, 256, 0, 0, 256, 256, 0)),
    (_M, 83, ("wgrad", 128, 4, 128, 0, 4, 0)), (_M, 84, ("wgrad", 283, 128, 288, 0, 128, 0)),
    (_M, 85, ("wgrad", 256, 256, 256, 0, 256, 0)), (_M, 86, ("wgrad", 256, 256, 256, 0, 256, 0)),
    (_M, 87, ("wgrad", 27, 256, 288, 256, 256, 0)),
    # rc_transient_bwd_host.inc: the per-bin heads (dX at chunk r0 = 1: 32 rows of 64 / 128 in)
    (_T, 114, ("dx", 64, 2100, 2100, 0, 64, 2048, 0, 64, None, 0)), (_T, 115, ("dx", 128, 2101, 2104, 0, 128, 4096, 0, 128, None, 0)),
    (_T, 117, ("wgrad", 64, 2100, 64, 0, 2100, 0)), (_T, 118, ("wgrad", 128, 2101, 128, 0, 2104, 0)),
]
# lines that hold a dense_* name without being a call site of their own: the two wgrad lambdas and the launch of the
# hand-built descriptor (listed above under the line that starts it)
NOT_CALL_SITES = {(_D, 159), (_D, 160), (_M, 76), (_M, 80), (_M, 81)}
_CALL = re.compile(r"\b(dense_(?:fwd|dx|wgrad)(?:_tile)?|wgrad|RcGemmArgs|rc_launch_gemm(?:_tile)?)\b")


def call_sites():
    """(file, line) of every line of the five host files that names a dense GEMM helper, a launcher or the descriptor."""
    out = set()
    for f in HOST_FILES:
        with open(os.path.join(CSRC, f)) as fh:
            for n, line in enumerate(fh, 1):
                if _CALL.search(line.split("//")[0]):
                    out.add((f, n))
    return out


def _production(cs):
    for f, line, d in PRODUCTION:
        src = f"{f}:{line}"
        if d[0] == "fwd":
            _, i, o, ldx, xo, ldy, yo, relu = d
            cs.add(f"prod/{src}/fwd{i}x{o}", "prod", ROWS_M, o, i, (ldx, 1, xo), (o, 1, 0), (ldy, 1, yo), bias=True, relu=relu, src=src)
        elif d[0] == "dx":
            _, i, o, ldy, yo, ldx, xo, j0, nj, mld, acc = d
            cs.add(f"prod/{src}/dx{i}x{o}@{j0}", "prod", ROWS_M, nj, o, (ldy, 1, yo), (1, o, j0 * o), (ldx, 1, xo + j0),
                   mask=None if mld is None else (mld, 1, j0), accumulate=acc, src=src)
        else:
            _, i, o, ldx, xo, ldy, yo = d
            w = cs.add(f"prod/{src}/dW{i}x{o}", "prod", i, o, ROWS_K, (1, ldx, xo), (ldy, 1, yo), (o, 1, 0), kslice=KSLICE,
                       spart=i * o, sum_parts=True, src=src)
            # the bias pass: A = `ones`, a single 1.0f with both strides 0, the same dY
            b = cs.add(f"prod/{src}/db{i}x{o}", "prod", 1, o, ROWS_K, (0, 0, 0), (ldy, 1, yo), (o, 1, 0), kslice=KSLICE, spart=o,
                       sum_parts=True, src=src, share=w)
            b["a_buf"], b["a_off"] = cs.operand(0, (1, 1), (1, 1), np.ones((1, 1), np.float32))
            cs.unsliced(w)
            cs.unsliced(b)


EDGE_MN = ((1, 1), (1, 129), (129, 1), (31, 31), (32, 32), (33, 33), (33, 65), (65, 33), (63, 64), (64, 63), (127, 4), (128, 128),
           (129, 129))
EDGE_K = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)
LAY = (65, 33, 37)
KINDS = ("kc", "mc", "nn", "bc")            # k-contiguous, mn-contiguous, neither stride unit, broadcast 0 / 0


def _strides(kind, mn, k, ld4):
    """(stride along mn, stride along k) of an mn x k operand; ld4: the leading dimension a multiple of 4 or not."""
    if kind == "kc":
        return (k + 3) // 4 * 4 if ld4 else (k + 3) // 4 * 4 + 1, 1
    if kind == "mc":
        return 1, (mn + 3) // 4 * 4 if ld4 else (mn + 3) // 4 * 4 + 1
    if kind == "nn":
        return (2 * k + 3) // 4 * 4 + (4 if ld4 else 5), 2
    return 0, 0


def layout_variants():
    """32 pairs of an A and a B layout: each of the 16 (kind, ld % 4 == 0, base offset) forms of A once with a B form of each
    parity, so that every pair of kinds, every form of A and every form of B occurs."""
    forms = [(kind, ld4, off) for kind in KINDS for ld4 in (1, 0) for off in (0, 1)]
    out = []
    for n, fa in enumerate(forms):
        ka, va = divmod(n, 4)
        out.append((fa, forms[4 * va + ka]))
        out.append((fa, forms[4 * ((va + 1) % 4) + (ka + 2) % 4]))
    return out


def _layouts(cs, group, K, kslices, unsliced, only=None):
    M, N, _ = LAY
    for (ka, la, oa), (kb, lb, ob) in layout_variants():
        if only and (ka, la, oa) != only and (kb, lb, ob) != only:
            continue
        sai, sak = _strides(ka, M, K, la)
        sbj, sbk = _strides(kb, N, K, lb)
        for ks in kslices:
            c = cs.add(f"{group}/A{ka}{la}{oa}/B{kb}{lb}{ob}/K{K}/ks{ks}", group, M, N, K, (sai, sak, oa), (sbk, sbj, ob), (36, 1, 0),
                       bias=True, kslice=ks)
            if unsliced and c["kparts"] > 1:
                cs.unsliced(c)
    # C and the mask transposed or with no unit stride, A row-major, B both ways
    for n, (C, mk) in enumerate((((1, 68, 0), (1, 65, 0)), ((1, 65, 1), (35, 1, 1)), ((70, 2, 0), (1, 67, 1)), ((33, 1, 0), (2, 131, 0)))):
        B = (N + 3, 1, 0) if n % 2 else (1, (K + 3) // 4 * 4, 0)
        for ks in kslices:
            c = cs.add(f"{group}/C{C[0]}.{C[1]}/mask{mk[0]}.{mk[1]}/K{K}/ks{ks}", group, M, N, K, ((K + 3) // 4 * 4, 1, 0), B, C,
                       bias=True, mask=mk, kslice=ks)
            if unsliced and c["kparts"] > 1:
                cs.unsliced(c)


def build_cases(cus):
    """All cases for a device of `cus` compute units (the 128 x 128 instantiation needs big tiles * K slices >= cus)."""
    cs = Cases()
    _production(cs)
    for M, N in EDGE_MN:
        for K in EDGE_K:
            cs.add(f"edge/{M}x{N}x{K}", "edge", M, N, K, (K + 1, 1, 0), (N, 1, 0), (N, 1, 0), bias=True)
    _layouts(cs, "layout", LAY[2], (37, 16, 12, 5), True)
    # a launch with more slices than K has: the last one lies wholly beyond K and writes bias alone
    cs.add("layout/beyondK", "layout", 65, 33, 37, (40, 1, 0), (33, 1, 0), (36, 1, 0), bias=True, kslice=12, kparts=5)
    for bits in range(16):
        bias, relu, mask, acc = bits & 1, bits >> 1 & 1, bits >> 2 & 1, bits >> 3 & 1
        cs.add(f"epilogue/bias{bias}relu{relu}mask{mask}acc{acc}", "epilogue", 65, 33, 37, (40, 1, 0), (33, 1, 0), (36, 1, 0),
               bias=bias, relu=relu, mask=(36, 1, 0) if mask else None, accumulate=acc)
    # the 128 x 128 instantiation
    cs.add("big/4097x1025x19/ragged", "big", 4097, 1025, 19, (19, 1, 0), (1025, 1, 0), (1025, 1, 0), bias=True)
    cs.add("big/4097x1025x19/aligned", "big", 4097, 1025, 19, (20, 1, 0), (1028, 1, 0), (1028, 1, 0), bias=True)
    _layouts(cs, "biglayout", 4 * cus + 3, (4, 5), False)
    # K = 4 cus + 3 in slices of 5 is fewer slices than CUs; 5 cus + 3 puts a slice length that is no multiple of 4 on
    # the 128 x 128 instantiation too, for the layouts whose mode depends on it (k-contiguous and 16-byte aligned)
    _layouts(cs, "biglayout5", 5 * cus + 3, (5,), False, only=("kc", 1, 0))
    # the rounding family
    for K in (27, 96, 129):
        for lay in ("rowmajor", "transposed"):
            A, B = ((K + 1, 1, 0), (65, 1, 0)) if lay == "rowmajor" else ((1, 132, 0), (1, K + 3, 0))
            for inst, parts in (("small", 1), ("big", (cus + 1) // 2)):
                cs.add(f"round/{lay}/K{K}/{inst}", "round", 129, 65, K, A, B, (65, 1, 0), bias=True, accumulate=1, kparts=parts,
                       spart=129 * 65 + 7 if parts > 1 else 0, family="round")
    assert len({c["name"] for c in cs.cases}) == len(cs.cases)
    for c in cs.cases:
        check_bounds(c, cs.bufs)
        assert c["family"] != "exact" or exact_precondition(c), c["name"]
    return cs.bufs, cs.cases


def check_bounds(c, bufs):
    """Every logical element of every operand lies inside its backing buffer, guards excluded."""
    def inside(buf, off, shape, strides):
        n = extent(shape, strides)
        assert min(strides, default=0) >= 0 and off >= GUARD and off + n <= bufs[buf].size - GUARD, (c["name"], buf, off, n)
    inside(c["a_buf"], c["a_off"], (c["M"], c["K"]), (c["sai"], c["sak"]))
    inside(c["b_buf"], c["b_off"], (c["K"], c["N"]), (c["sbk"], c["sbj"]))
    inside(c["c_buf"], c["c_off"], (c["M"], c["N"]), (c["sci"], c["scj"]))
    inside(c["c_buf"], c["c_off"] + (c["kparts"] - 1) * c["spart"], (c["M"], c["N"]), (c["sci"], c["scj"]))
    if c["bias_buf"] >= 0:
        inside(c["bias_buf"], c["bias_off"], (c["N"],), (1,))
    if c["mask_buf"] >= 0:
        inside(c["mask_buf"], c["mask_off"], (c["M"], c["N"]), (c["smi"], c["smj"]))
    if c["g_buf"] >= 0:
        inside(c["g_buf"], c["g_off"], (c["spart"],), (1,))
        assert c["spart"] == c["M"] * c["N"] and c["sci"] == c["N"] and c["scj"] == 1        # k_sum_parts: dense parts
    assert c["kparts"] >= 1 and (c["kparts"] == 1 or c["spart"] >= extent((c["M"], c["N"]), (c["sci"], c["scj"])))


# ---------------------------------------------------------------------------------------------------------------------------
# files


def write_case_file(path, bufs, cases):
    table = np.zeros((len(bufs), 2), np.int64)
    at = 0
    stored = [not is_canary(b).all() for b in bufs]
    for n, b in enumerate(bufs):
        table[n] = (at if stored[n] else -1), b.size
        at += b.size if stored[n] else 0
    fields = np.array([[c[f] for f in FIELDS] for c in cases], np.int64).reshape(len(cases), len(FIELDS))
    with open(path, "wb") as fh:
        np.array([MAGIC_CASES, len(bufs), len(cases), len(FIELDS)], np.int64).tofile(fh)
        table.tofile(fh)
        fields.tofile(fh)
        for n, b in enumerate(bufs):
            if stored[n]:
                b.tofile(fh)


class Results:
    """The driver's result file: cus, wall_us, align [case][launcher][a, b, c, bias, mask]; C(n, launcher) and
    G(n, launcher) read one backing buffer."""

    def __init__(self, path, bufs, cases):
        self.path = path
        head = np.fromfile(path, np.int64, 4)
        assert head[0] == MAGIC_RESULTS and head[2] == len(cases), head
        self.cus, self.wall_us = int(head[1]), int(head[3])
        self.align = np.fromfile(path, np.int64, len(cases) * 10, offset=32).reshape(len(cases), 2, 5)
        at = 32 + 80 * len(cases)
        self.where = []
        for c in cases:
            per = []
            for _ in range(2):
                nc = bufs[c["c_buf"]].size
                ng = bufs[c["g_buf"]].size if c["g_buf"] >= 0 else 0
                per.append((at, nc, at + 4 * nc, ng))
                at += 4 * (nc + ng)
            self.where.append(per)
        assert os.path.getsize(path) == at, (os.path.getsize(path), at)

    def C(self, n, launcher):
        at, nc, _, _ = self.where[n][launcher]
        return np.fromfile(self.path, np.float32, nc, offset=at)

    def G(self, n, launcher):
        _, _, at, ng = self.where[n][launcher]
        return np.fromfile(self.path, np.float32, ng, offset=at) if ng else None
