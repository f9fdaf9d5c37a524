// Host-only part of rc_vis_images (rc_vis_host.inc): the checks of an item table and the plan of its bin sums.  No HIP in
// here, so the hostcheck program runs it under the sanitizers.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rc_abi.h"

namespace rcvis {

constexpr int64_t kMaxElems = (int64_t)1 << 31;            // pixels and elements are indexed in 32 bits

inline bool sums_bins(int op) { return op == RC_VIS_BINSUM_SRGB || op == RC_VIS_BINSUM_CLIP_SRGB; }

// One sum over the bins: items that read the same histogram share it.
struct BinSum { const float* src; int32_t channels, n_bins; };
struct Plan {
  std::vector<BinSum> sums;
  std::vector<int> slot;                                   // per item: its index in `sums`, or -1
};

// Empty string: the table is fine and `plan` is filled; otherwise what is wrong with it.
inline std::string plan_items(const rc_vis_item* items, int32_t n_items, int32_t height, int32_t width, Plan& plan) {
  if (!items) return "null items";
  if (n_items < 1) return "n_items must be at least 1";
  if (height < 1 || width < 1) return "height and width must be at least 1";
  if ((int64_t)height * width >= kMaxElems) return "2^31 pixels or more";
  plan.sums.clear();
  plan.slot.assign((size_t)n_items, -1);
  for (int32_t i = 0; i < n_items; ++i) {
    const rc_vis_item& it = items[i];
    const std::string who = "item " + std::to_string(i) + ": ";
    if (!it.src) return who + "null src";
    if (!it.out_f32 && !it.out_u8) return who + "no output";
    if (it.channels != 1 && it.channels != 3) return who + "channels must be 1 or 3";
    if (it.op < 0 || it.op >= RC_VIS_OP_COUNT) return who + "unknown operation";
    if (sums_bins(it.op) ? it.n_bins < 1 : it.n_bins != 0) return who + "n_bins must be > 0 exactly on an operation that sums bins";
    if (it.op == RC_VIS_TURBO && (!it.bounds || it.channels != 1)) return who + "RC_VIS_TURBO needs bounds and one channel";
    if (!sums_bins(it.op)) continue;
    size_t s = 0;
    while (s < plan.sums.size() && !(plan.sums[s].src == it.src && plan.sums[s].channels == it.channels && plan.sums[s].n_bins == it.n_bins)) ++s;
    if (s == plan.sums.size()) plan.sums.push_back(BinSum{it.src, it.channels, it.n_bins});
    plan.slot[(size_t)i] = (int)s;
  }
  return std::string();
}

}  // namespace rcvis
