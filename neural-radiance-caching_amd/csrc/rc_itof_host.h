// Host-only builder of the iToF modulation table (no HIP in this header), beside rc_pack_host.h: the rows of
// render_utils.dtof_to_itof (internal/inverse_render/render_utils.py:1648-1676) as k_transient_loss_kinds and
// k_dtof_to_itof read them (rc_transient_bwd.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

// W[2 n_pairs + 1][n_bins]: per (frequency, phase) pair a cos row then a sin row, then the constant row:
//   t_b = b exposure_time / c   (linspace(0, n_bins exposure_time, n_bins, endpoint=False) / 299792458)
//   W_cos[b] = cos(2 pi f t_b + phi) + 1,  W_sin[b] = sin(2 pi f t_b + phi) + 1,  W_const[b] = 1/2
// evaluated in double and rounded once to float32, as the temporal filter's window is.
inline std::vector<float> rc_itof_table(int n_bins, double exposure_time, int n_pairs, const double* frequency,
                                        const double* phase_shift) {
  const double c = 299792458.0, two_pi = 6.283185307179586476925286766559;
  const int rows = 2 * n_pairs + 1;
  std::vector<float> w((size_t)rows * (size_t)n_bins);
  for (int p = 0; p < n_pairs; ++p)
    for (int b = 0; b < n_bins; ++b) {
      const double ph = two_pi * frequency[p] * ((double)b * exposure_time / c) + phase_shift[p];
      w[(size_t)(2 * p) * n_bins + b] = (float)(cos(ph) + 1.0);
      w[(size_t)(2 * p + 1) * n_bins + b] = (float)(sin(ph) + 1.0);
    }
  for (int b = 0; b < n_bins; ++b) w[(size_t)(rows - 1) * n_bins + b] = 0.5f;
  return w;
}
