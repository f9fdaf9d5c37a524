// Host-only part of the weight packing (no HIP in this header): Flax layers -> MFMA A-fragment streams, the folded
// shader bottleneck, the directional-encoding coefficient table, and the index rule of the dense levels' cell tables.
// rc_api.hip uses it at rc_load_weights time; csrc/hostcheck.cpp compiles the same code for the CPU with
// -fsanitize=address,undefined and tests/test_hostcheck.py compares its results with numpy restatements
// (`make hostcheck`: SURVEY 5, sanitizers on the CPU build only).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <array>
#include <vector>

#ifndef RC_IDE_TERMS
#define RC_IDE_TERMS 36
#define RC_IDE_ZPOW 17
struct RcIdeTable {
  float coef[RC_IDE_TERMS][RC_IDE_ZPOW];
  int32_t m[RC_IDE_TERMS];
  float sigma[RC_IDE_TERMS];
};
#endif

#if defined(__HIPCC__)
#define RC_HD __host__ __device__
#else
#define RC_HD
#endif

// Cell tables of the dense levels (rc_fused.hip k_build_cells): record i = cell * 8 + corner of the zero-padded
// volume, (N + 3)^3 cells whose origin runs over [-1, N + 1] per axis; corner bits (b0 b1 b2) in combine order.
// Returns true and the entry index ((k2 - 1) N + (k1 - 1)) N + (k0 - 1) of the source level when the corner lies
// inside the level, false for the zero padding (grid_utils.py:384-390).
RC_HD inline bool rc_cell_corner(int N, int64_t i, int64_t* entry) {
  const int M = N + 3;
  const int c = (int)(i & 7);
  int64_t cell = i >> 3;
  const int q0 = (int)(cell % M); cell /= M;
  const int q1 = (int)(cell % M);
  const int q2 = (int)(cell / M);
  const int b0 = (c >> 2) & 1, b1 = (c >> 1) & 1, b2 = c & 1;
  const int lo = 0, hi = N + 1;
  int k0 = q0 - 1 + b0, k1 = q1 - 1 + b1, k2 = q2 - 1 + b2;
  k0 = k0 < lo ? lo : (k0 > hi ? hi : k0); k1 = k1 < lo ? lo : (k1 > hi ? hi : k1); k2 = k2 < lo ? lo : (k2 > hi ? hi : k2);
  const bool inside = (k0 >= 1) & (k0 <= N) & (k1 >= 1) & (k1 <= N) & (k2 >= 1) & (k2 <= N);
  *entry = ((int64_t)(k2 - 1) * N + (k1 - 1)) * N + (k0 - 1);
  return inside;
}


// ---------------------------------------------------------------------------------------------
// Arithmetic of the MLP layers (compile-time, the whole library): RC_SPLIT_MFMA = 1 (default) runs every weight layer on
// the bf16 matrix pipe with each fp32 operand split EXACTLY into three bf16 pieces (8 + 8 + 8 significand bits:
// hi + mid + lo == x bit for bit) and the six piece products whose weight is >= 2^-16 of the full product
// (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid; what is dropped is <= 2^-23 of |a b|, the size of one fp32 rounding),
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16: 6 x 32 cycles per 16 k where v_mfma_f32_32x32x2_f32 takes 8 x 64
// (tools/micro/split_mfma.hip: 1.9 x the layer rate at the same error against fp64).  RC_SPLIT_MFMA = 0 is the exact
// fp32 MFMA chain of rounds 1-4 (`make diag DIAG_EXTRA=-DRC_SPLIT_MFMA=0`).
// Stream geometry: a layer of KS k-steps (= pairs of inputs) and NT 32-row tiles is KS * NT fragments of 256 bytes in
// the fp32 form; in the split form ceil(KS / 8) blocks x NT tiles x 3 pieces x 1 KiB (= 4 fragments each: lane l holds
// the 8 bf16 of steps 8 q .. 8 q + 7, half l / 32, row l % 32).
// ---------------------------------------------------------------------------------------------
#ifndef RC_SPLIT_MFMA
#define RC_SPLIT_MFMA 1
#endif
constexpr bool kRcSplit = RC_SPLIT_MFMA != 0;
// The two-wave kernel k_cache_fused_team (rc_fused2.hip) is built where the shader is the fp32 MFMA chain.  Its split form
// shares a SIMD between waves of two workgroups, the configuration rc_dev_mlp.h INSTABILITY calls unstable, so a split
// build compiles it only for diagnosis (`make diag DIAG_STAMPS= DIAG_EXTRA=-DRC_TEAM_SPLIT_DIAG`); elsewhere rc_set_fused(1) runs the
// one-wave kernel (tests/test_code_objects.py holds every bf16-MFMA kernel of the product to the whole register file).
#if !RC_SPLIT_MFMA || defined(RC_TEAM_SPLIT_DIAG)
#define RC_TEAM_KERNEL 1
#else
#define RC_TEAM_KERNEL 0
#endif
// fragments of a weight layer / of a dot_out block (NO outputs over NT hidden tiles + NO bias fragments; padded to whole
// 1-KiB pieces in the split form so that every layer behind it starts on one)
constexpr int rc_lfr(int ks, int nt) { return kRcSplit ? ((ks + 7) / 8) * nt * 12 : ks * nt; }
constexpr int rc_dfr(int no, int nt) { return kRcSplit ? ((no * (nt * 16 + 1) + 3) / 4) * 4 : no * (nt * 16 + 1); }
// The density MLPs of the proposal levels stay on the fp32 MFMA in every build (mlp_layer_d, rc_dev_mlp.h: with them in
// the split form the two-wave kernel was unstable -- see INSTABILITY there): their
// layers and dot blocks keep the fp32 geometry, and a stream that continues with split layers is padded to a whole piece.
constexpr int rc_lfr32(int ks, int nt) { return ks * nt; }
constexpr int rc_dfr32(int no, int nt) { return no * (nt * 16 + 1); }
constexpr int rc_align_piece(int f) { return kRcSplit ? (f + 3) / 4 * 4 : f; }

// ---------------------------------------------------------------------------------------------
// Output rows as a table (the fused streams of the one-wave kernel only: kRcFusedRows).  A dot_out fragment holds two
// distinct floats (one per half-wave; a bias fragment one), so a block of NO outputs over NT tiles ships NO (16 NT + 1)
// fragments for 2 NO 16 NT + NO values.  The table form of the same block, in floats from the block's first fragment:
//   [0, n)            half-wave 0: [output][tile][register]      n = NO * NT * 16
//   [S, S + n)        half-wave 1, S = rc_rows_stride: n, or n + 32 where n is a multiple of 64 -- the two rows then lie
//                     128 bytes apart modulo the 256 bytes of a bank row, and the two addresses of a read (lanes 0-31 one,
//                     lanes 32-63 the other) never meet on a bank
//   [S + n, S + n + NO)  the biases
// padded with zeros to whole fragments (to whole 1-KiB pieces where a split layer follows).  dot_rows (rc_dev_mlp.h) reads
// it; a block never straddles a chunk of the ring (rc_rows_at moves it to the next chunk's start if it would): a lane's
// address depends on its half-wave, so both rows must be resident together.
// ---------------------------------------------------------------------------------------------
constexpr int kRcChunkFrags = 64;                  // fragments per chunk of the weight ring (rc_dev_mlp.h kChunk)
constexpr bool kRcFusedRows = kRcSplit && !RC_TEAM_KERNEL;
constexpr int rc_rows_stride(int no, int nt) { return (no * nt * 16 + 31) / 32 * 32 + (((no * nt * 16 + 31) / 32) % 2 == 0 ? 32 : 0); }
constexpr int rc_rows_floats(int no, int nt) { return rc_rows_stride(no, nt) + no * nt * 16 + no; }
constexpr int rc_rfr(int no, int nt, bool piece) { return piece ? (rc_rows_floats(no, nt) + 255) / 256 * 4 : (rc_rows_floats(no, nt) + 63) / 64; }
constexpr int rc_rows_at(int f, int nfr) {
  return f / kRcChunkFrags != (f + nfr - 1) / kRcChunkFrags ? (f + kRcChunkFrags - 1) / kRcChunkFrags * kRcChunkFrags : f;
}

// fragment offsets of the shader's layers inside its weight stream (host: rc_api.hip, same order).  ROWS: the two output
// blocks as row tables, the stream starting at fragment F0 of its kernel's stream (the fused streams); the fragment form
// (k_cache_shader, the texture atlas, the material stage, the two-wave kernel) does not depend on F0.
namespace rcdev {
template <bool ROWS, int F0 = 0>
struct ShaderFragsL {
  static constexpr bool kRows = ROWS;
  static constexpr int F_H = 0, F_S0 = F_H + rc_lfr(49, 1), F_I0 = F_S0 + rc_lfr(85, 8), F_I1 = F_I0 + rc_lfr(49, 2),
                       F_IO = ROWS ? rc_rows_at(F0 + F_I1 + rc_lfr(33, 2), rc_rfr(1, 2, kRcSplit)) - F0 : F_I1 + rc_lfr(33, 2),
                       F_S1 = F_IO + (ROWS ? rc_rfr(1, 2, kRcSplit) : rc_dfr(1, 2)), F_S2 = F_S1 + rc_lfr(65, 4), F_SB = F_S2 + rc_lfr(65, 4),
                       F_SO = ROWS ? rc_rows_at(F0 + F_SB + rc_lfr(64, 4), rc_rfr(3, 4, kRcSplit)) - F0 : F_SB + rc_lfr(64, 4),
                       COUNT = F_SO + (ROWS ? rc_rfr(3, 4, kRcSplit) : rc_dfr(3, 4));
  static_assert((F0 + F_S1) % 4 == 0 || !kRcSplit, "the layer behind a row table starts on a whole piece");
};
using ShaderFrags = ShaderFragsL<false>;
}  // namespace rcdev

// fragments of the fused weight stream [density MLP 0 | 1 | 2 (+ backward fragments) | shader]
namespace rcfused {
template <int KS0, bool ROWS = false, int FB = 0> struct DensFrags {
  static constexpr int NO = KS0 == 17 ? 4 : 1;       // output rows: density (+ 3 predicted normals on the last level)
  static constexpr int D0 = 0, D1 = rc_lfr32(KS0, 2),
                       DO = ROWS ? rc_rows_at(FB + D1 + rc_lfr32(33, 2), rc_rfr(NO, 2, false)) - FB : D1 + rc_lfr32(33, 2),
                       B1 = DO + (ROWS ? rc_rfr(NO, 2, false) : rc_dfr32(NO, 2)), B0 = B1 + rc_lfr32(32, 2), END = B0 + rc_lfr32(32, 1);
};
template <bool ROWS> struct FusedFrags {
  static constexpr int L0 = 0;                                          // K = 6: KS0 = 4
  static constexpr int L1 = L0 + DensFrags<4, ROWS, L0>::B1;            // K = 7: KS0 = 5
  static constexpr int L2 = L1 + DensFrags<5, ROWS, L1>::B1;            // K = 32: KS0 = 17, with the 96 backward fragments
  static constexpr int SH = rc_align_piece(L2 + DensFrags<17, ROWS, L2>::END);      // the shader's split layers start on a whole piece
  static constexpr int NF = SH + rcdev::ShaderFragsL<ROWS, SH>::COUNT;
  static_assert(SH % 4 == 0 || !kRcSplit, "F_SH: the shader's split layers start on a whole 1-KiB piece");
};
constexpr int F_L0 = FusedFrags<kRcFusedRows>::L0, F_L1 = FusedFrags<kRcFusedRows>::L1, F_L2 = FusedFrags<kRcFusedRows>::L2,
              F_SH = FusedFrags<kRcFusedRows>::SH, NF_FUSED = FusedFrags<kRcFusedRows>::NF;
template <int KS0, int FB> using FusedDens = DensFrags<KS0, kRcFusedRows, FB>;       // a density MLP of the fused stream at fragment FB
using FusedShader = rcdev::ShaderFragsL<kRcFusedRows, F_SH>;
}  // namespace rcfused

namespace rcpack {

struct HostLayer {
  std::vector<float> kernel, bias;
  int in = 0, out = 0;
  bool have_kernel = false, have_bias = false;
};

// ---------------------------------------------------------------------------------------------
// MFMA fragment packing
// ---------------------------------------------------------------------------------------------
struct Step { int row[2]; };               // >= 0 input row, -1 zero, -2 bias
struct Col {
  const HostLayer* L = nullptr;            // nullptr -> zero column
  int col = 0;
  int row_off = 0;
  bool bias_ok = true;
};
using Tile = std::array<Col, 32>;

inline int acc_feat(int t, int r, int h) { return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h; }

inline void steps_natural(std::vector<Step>& s, int K, int base) {
  for (int i = 0; i < (K + 1) / 2; ++i) s.push_back({{base + 2 * i, (2 * i + 1 < K) ? base + 2 * i + 1 : -1}});
}
inline void steps_acc(std::vector<Step>& s, int ntiles, int base) {
  for (int t = 0; t < ntiles; ++t)
    for (int r = 0; r < 16; ++r) s.push_back({{base + acc_feat(t, r, 0), base + acc_feat(t, r, 1)}});
}
inline void step_bias(std::vector<Step>& s) { s.push_back({{-2, -1}}); }

inline Tile tile_full(const HostLayer* L, int t, int row_off = 0, bool bias_ok = true) {
  Tile tl;
  for (int i = 0; i < 32; ++i) {
    const int c = 32 * t + i;
    if (c < L->out) tl[i] = Col{L, c, row_off, bias_ok};
  }
  return tl;
}
// Output `regs[r]` lands in accumulator register r of BOTH half-waves.
inline Tile tile_by_reg(const std::vector<Col>& regs) {
  Tile tl;
  for (int i = 0; i < 32; ++i) {
    const int r = (i & 3) + 4 * (i >> 3);
    if (r < (int)regs.size()) tl[i] = regs[r];
  }
  return tl;
}

// Fragments of dot_out (rc_dev_mlp.h): per output, per tile, per accumulator register the weight of the feature that
// register holds on each half-wave; then one bias fragment per output.
inline std::vector<float> pack_dot(const std::vector<Col>& outs, int ntiles, bool pad_to_piece = kRcSplit) {
  std::vector<float> v;
  for (const Col& c : outs)
    for (int t = 0; t < ntiles; ++t)
      for (int r = 0; r < 16; ++r)
        for (int lane = 0; lane < 64; ++lane) {
          const int row = acc_feat(t, r, lane >> 5) + c.row_off;
          v.push_back((c.L && row < c.L->in) ? c.L->kernel[(size_t)row * c.L->out + c.col] : 0.0f);
        }
  for (const Col& c : outs)
    for (int lane = 0; lane < 64; ++lane) v.push_back(c.L ? c.L->bias[c.col] : 0.0f);
  if (pad_to_piece) v.resize((size_t)rc_dfr((int)outs.size(), ntiles) * 64, 0.0f);
  return v;
}

// The same block as a row table (rc_rows_stride above, dot_rows in rc_dev_mlp.h): the two distinct floats of every weight
// fragment of pack_dot -- what lanes 0 and 32 hold -- and the one of every bias fragment.
inline std::vector<float> pack_dot_rows(const std::vector<Col>& outs, int ntiles, bool pad_to_piece = kRcSplit) {
  const int no = (int)outs.size(), n = no * ntiles * 16, stride = rc_rows_stride(no, ntiles);
  std::vector<float> v((size_t)rc_rfr(no, ntiles, pad_to_piece) * 64, 0.0f);
  for (int h = 0; h < 2; ++h)
    for (int o = 0; o < no; ++o)
      for (int t = 0; t < ntiles; ++t)
        for (int r = 0; r < 16; ++r) {
          const Col& c = outs[o];
          const int row = acc_feat(t, r, h) + c.row_off;
          v[(size_t)h * stride + (o * ntiles + t) * 16 + r] = (c.L && row < c.L->in) ? c.L->kernel[(size_t)row * c.L->out + c.col] : 0.0f;
        }
  for (int o = 0; o < no; ++o) v[(size_t)stride + n + o] = outs[o].L ? outs[o].L->bias[outs[o].col] : 0.0f;
  return v;
}

// weight of k-step s, half-wave h, for the output row lane i of a tile holds
inline float pack_value(const Step& st, int h, const Col& c) {
  if (!c.L) return 0.0f;
  const int row = st.row[h];
  if (row == -2) return c.bias_ok ? c.L->bias[c.col] : 0.0f;
  if (row >= 0) {
    const int rr = row + c.row_off;
    if (rr < c.L->in) return c.L->kernel[(size_t)rr * c.L->out + c.col];
  }
  return 0.0f;
}

// x == hi + mid + lo exactly, each piece the TRUNCATED top 16 bits of what is left (a bf16): 8 significand bits apiece
inline void split3(float x, uint16_t (&piece)[3]) {
  float r = x;
  for (int p = 0; p < 3; ++p) {
    uint32_t u;
    memcpy(&u, &r, 4);
    u &= 0xffff0000u;
    float top;
    memcpy(&top, &u, 4);
    piece[p] = (uint16_t)(u >> 16);
    r = r - top;               // exact: top shares r's leading bits
  }
}

inline std::vector<float> pack_f32(const std::vector<Step>& steps, const std::vector<Tile>& tiles) {
  const size_t NT = tiles.size();
  std::vector<float> out(steps.size() * NT * 64, 0.0f);
  for (size_t s = 0; s < steps.size(); ++s)
    for (size_t t = 0; t < NT; ++t)
      for (int lane = 0; lane < 64; ++lane) out[(s * NT + t) * 64 + lane] = pack_value(steps[s], lane >> 5, tiles[t][lane & 31]);
  return out;
}

// split form (see rc_lfr): [block q][tile t][piece p][lane][4 dwords]; dword d of a lane = bf16 of step 8 q + 2 d in the low
// half, of step 8 q + 2 d + 1 in the high half; steps past the layer's last are zero
inline std::vector<float> pack_split(const std::vector<Step>& steps, const std::vector<Tile>& tiles) {
  const size_t NT = tiles.size(), NB = (steps.size() + 7) / 8;
  std::vector<uint32_t> out(NB * NT * 3 * 64 * 4, 0u);
  for (size_t s = 0; s < steps.size(); ++s)
    for (size_t t = 0; t < NT; ++t)
      for (int lane = 0; lane < 64; ++lane) {
        uint16_t pc[3];
        split3(pack_value(steps[s], lane >> 5, tiles[t][lane & 31]), pc);
        const size_t q = s / 8, j = s % 8;
        for (int p = 0; p < 3; ++p) {
          uint32_t& d = out[((((q * NT + t) * 3 + p) * 64) + lane) * 4 + j / 2];
          d = (j & 1) ? ((d & 0x0000ffffu) | ((uint32_t)pc[p] << 16)) : ((d & 0xffff0000u) | pc[p]);
        }
      }
  std::vector<float> f(out.size());
  memcpy(f.data(), out.data(), out.size() * 4);
  return f;
}

inline std::vector<float> pack(const std::vector<Step>& steps, const std::vector<Tile>& tiles) {
  return kRcSplit ? pack_split(steps, tiles) : pack_f32(steps, tiles);
}


// ---------------------------------------------------------------------------------------------
// The two per-bin heads of the time-resolved cache (rc_transient.hip k_transient_bins, rc_transient_slice.hip): `slf` is
// output_rgba_layer [128 -> cols + 1], `irr` transient_indirect_layer [64 -> cols], cols = 3 n_bins histogram entries.
// rc_transient_host.inc packs the library's weights with these; tests/transient_check.hip a case file's.
// ---------------------------------------------------------------------------------------------
// k_transient_bins' stream: per column tile of 32 entries [slf (128 + bias) | irr (64 + bias)], every tile padded with zeros
// to `frags_per_tile` fragments (whole chunks of the kernel's LDS ring).  Split form (tile_xw2_split): the pieces of the SLF
// head's 9 blocks, then of the irradiance head's 5.  fp32 form (tile_xw2's consumption order): 16 groups of [SLF head 4
// steps | irradiance head 2 steps], then the two bias steps.
inline std::vector<float> pack_bins_stream(const HostLayer& slf, const HostLayer& irr, int cols, int frags_per_tile,
                                           bool split = kRcSplit) {
  std::vector<float> stream;
  std::vector<Step> s4, s2;
  steps_acc(s4, 4, 0); step_bias(s4);
  steps_acc(s2, 2, 0); step_bias(s2);
  const int tiles = (cols + 31) / 32;
  const size_t tile_floats = (size_t)frags_per_tile * 64;
  auto append = [&](const std::vector<float>& b) { stream.insert(stream.end(), b.begin(), b.end()); };
  for (int t = 0; t < tiles; ++t) {
    if (split) {
      append(pack_split(s4, {tile_full(&slf, t)}));
      append(pack_split(s2, {tile_full(&irr, t)}));
    } else {
      const std::vector<float> pa = pack_f32(s4, {tile_full(&slf, t)}), pb = pack_f32(s2, {tile_full(&irr, t)});
      auto frag = [&](const std::vector<float>& p, int i) { stream.insert(stream.end(), p.begin() + (size_t)i * 64, p.begin() + (size_t)(i + 1) * 64); };
      for (int g = 0; g < 16; ++g) {
        for (int q = 0; q < 4; ++q) frag(pa, 4 * g + q);
        for (int q = 0; q < 2; ++q) frag(pb, 2 * g + q);
      }
      frag(pa, 64); frag(pb, 32);
    }
    stream.resize((size_t)(t + 1) * tile_floats, 0.0f);
  }
  return stream;
}

// k_transient_slice's plain columns of one head (`ntiles` accumulator tiles of inputs: 4 for slf, 2 for irr).  The
// activations k_transient_shader stores are in MFMA operand order -- value 2 k + h of a sample is half h of step k -- so the
// columns are built from the same step tables: row j of a column is the weight that meets value j, then the bias.
inline std::vector<float> pack_slice_columns(const HostLayer& L, int ntiles, int cols, int stride) {
  std::vector<Step> st;
  steps_acc(st, ntiles, 0); step_bias(st);
  std::vector<float> v((size_t)cols * stride, 0.0f);
  for (int col = 0; col < cols; ++col)
    for (size_t k = 0; k < st.size(); ++k)
      for (int hh = 0; hh < 2; ++hh)
        if ((int)(2 * k + hh) < stride) v[(size_t)col * stride + 2 * k + hh] = pack_value(st[k], hh, Col{&L, col, 0, true});
  return v;
}

// temporal filter of the direct part (render.py:411-413): taps -round(4 sigma) .. round(4 sigma), exp(-k^2 / 2 sigma^2) -
// exp(-8), normalised; none for sigma = 0
inline std::vector<float> temporal_taps(float sigma) {
  std::vector<float> taps;
  if (sigma != 0.0f) {
    const int half = (int)lround(4.0 * sigma);
    float sum = 0.0f;
    for (int k = -half; k <= half; ++k) {
      const float kk = (float)k;
      const float v = expf(-(kk * kk) / (2.0f * sigma * sigma)) - (float)exp(-8.0);
      taps.push_back(v);
      sum += v;
    }
    for (float& v : taps) v = v / sum;
  }
  return taps;
}

// A linear layer `b` (no activation) folded into the layer L that consumes it: rows [row0, row0 + b.out) of L take b's
// output, the following `extra_rows` rows are kept as they are.  W' = W_b W[rows], b' = b_b W[rows] (fp64 products,
// rounded once); L's own bias is added where the result is packed.
inline HostLayer fold_linear(const HostLayer& b, const HostLayer& L, int row0, int extra_rows) {
  const int FE = b.in, BW = b.out;
  HostLayer f;
  f.in = FE + extra_rows; f.out = L.out;
  f.kernel.assign((size_t)f.in * f.out, 0.0f); f.bias.assign(f.out, 0.0f);
  f.have_kernel = f.have_bias = true;
  for (int o = 0; o < L.out; ++o) {
    for (int i = 0; i < FE; ++i) {
      double a = 0.0;
      for (int m = 0; m < BW; ++m) a += (double)b.kernel[(size_t)i * BW + m] * (double)L.kernel[(size_t)(row0 + m) * L.out + o];
      f.kernel[(size_t)i * f.out + o] = (float)a;
    }
    double bb = 0.0;
    for (int m = 0; m < BW; ++m) bb += (double)b.bias[m] * (double)L.kernel[(size_t)(row0 + m) * L.out + o];
    f.bias[o] = (float)bb;
    for (int e = 0; e < extra_rows; ++e) f.kernel[(size_t)(FE + e) * f.out + o] = L.kernel[(size_t)(row0 + BW + e) * L.out + o];
  }
  return f;
}

// ref_utils.py:75-153 coefficient table for deg_view = 5, rounded to float32 like `mat` is.
inline double fact(int n) { double f = 1; for (int i = 2; i <= n; ++i) f *= i; return f; }
inline double gen_binom(double a, int k) { double p = 1; for (int j = 0; j < k; ++j) p *= (a - j); return p / fact(k); }
inline double sph_coeff(int l, int m, int k) {
  const double al = ((m & 1) ? -1.0 : 1.0) * pow(2.0, l) * fact(l) / fact(k) / fact(l - k - m) *
                    gen_binom(0.5 * (l + k + m - 1.0), l);
  return sqrt((2.0 * l + 1.0) * fact(l - m) / (4.0 * M_PI * fact(l + m))) * al;
}
inline void build_ide_table(RcIdeTable& tb) {
  memset(&tb, 0, sizeof(tb));
  int i = 0;
  for (int d = 0; d < 5; ++d) {
    const int l = 1 << d;
    for (int m = 0; m <= l; ++m, ++i) {
      tb.m[i] = m;
      tb.sigma[i] = (float)(0.5 * l * (l + 1));
      for (int k = 0; k <= l - m; ++k) tb.coef[i][k] = (float)sph_coeff(l, m, k);
    }
  }
}


}  // namespace rcpack
