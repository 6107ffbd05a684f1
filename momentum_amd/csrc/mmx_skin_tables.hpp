// mmx_skin_tables.hpp -- host-side bookkeeping of linear-blend skinning (mmx_skin_points / mmx_skin_points_backward): no HIP
// here, so it is checked bit-exactly on the CPU (tests/test_skin_tables_host.py through mmx_host_skin_tables).
//
// The backward pass is a vertex-to-joint reduction.  Its summation order is fixed by ONE table, the joint-sorted influence
// list: every (vertex, slot) pair with a non-zero weight, sorted by (joint, vertex, slot), with jointStart [J + 1] as the
// index.  A zero-weight slot is padding and has no entry; a joint repeated in two slots of a vertex keeps both entries.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmx.h"

namespace mmx {
#pragma GCC visibility push(hidden)

// Bytes of LDS the forward kernel needs for the posed affines of a rig of J joints (12 floats each)
inline size_t skinLdsBytes(int32_t J) {
  return size_t(J) * 12 * sizeof(float);
}
// null, or why a rig of J joints is outside the kernels' LDS budget (the 160 KB rule of the other kernels)
const char* skinRefusal(int32_t J);

// Every check of a skin descriptor that needs no device: null pointers, V >= 1, K in 1 .. MMX_MAX_SKIN_INFLUENCES, every
// joint index (zero-weight slots included) in [0, J), finite weights; with `payload` also finite inverse-bind entries and
// rest positions and a non-null rest_positions.  MMX_OK or MMX_ERR_INVALID_ARGUMENT with `err` set.
int32_t validateSkinDesc(int32_t J, const mmx_skin_desc* d, bool payload, std::string& err);

struct SkinTables {
  std::vector<int32_t> jointStart; // [J + 1]
  std::vector<int32_t> entryVertex, entrySlot; // [numEntries] sorted by (joint, vertex, slot)
  std::vector<float> entryWeight; // [numEntries] weight[vertex][slot]: what the backward kernel reads instead of the slot
  // The backward kernel's wave partition: wave w takes the joints waveStart[w] .. waveStart[w + 1] - 1, one after the other.
  // Consecutive joints are packed while their cost (entries + kSkinJointCost each) stays within the heaviest single joint's:
  // no wave is slower than the one that carries that joint, and a joint's sum is one wave's whatever the packing.
  std::vector<int32_t> waveStart; // [numWaves + 1], waveStart[numWaves] = J
};
constexpr int32_t kSkinJointCost = 16; // a joint's fixed work (state row, cross-lane tree, eight channels) in entries
// (the descriptor must have passed validateSkinDesc)
SkinTables buildSkinTables(int32_t J, const mmx_skin_desc* d);

#pragma GCC visibility pop
} // namespace mmx
