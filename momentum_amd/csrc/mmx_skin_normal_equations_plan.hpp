// mmx_skin_normal_equations_plan.hpp -- the split of mmx_skin_normal_equations_split as pure host functions (no HIP here, no
// device): the part ranges, the effective parts, the workspace's size and layout, the plan of parts = 0 and the split's
// refusals.  The launcher and the reducer's indexing (mmx_skin_normal_equations.hip), the executor (mmx_capi.hip) and the
// exported queries read them from here, and so do the tests (tests/test_skin_normal_equations_plan_host.py,
// tests/cpp/test_skin_normal_equations_plan.cpp, which links mmx_skin_normal_equations_plan.cpp alone).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mmx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMX_SNE_HD __host__ __device__
#else
#define MMX_SNE_HD
#endif

namespace mmx {

constexpr int32_t kSkinNeTileRows = 32; // residual rows of a tile (kSneTileRows of the kernel)
constexpr int32_t kSkinNeMaxParts = MMX_SKIN_NE_MAX_PARTS;
constexpr int32_t kSkinNeSplitMaxSolved = 128; // == kSkinNeMaxSolved (mmx_kernels.hpp)
constexpr int32_t kSkinNeBlockFloats = 16 * 64; // a 32 x 32 block of H as a wave holds it: [reg][lane]

// rows and tiles of a descriptor: C rows for plane constraints, 3 C for position constraints; 0 for count < 1
MMX_SNE_HD inline int64_t skinNeRows(int32_t type, int32_t count) {
  return count < 1 ? 0 : (type == MMX_VC_PLANE ? int64_t(count) : 3 * int64_t(count));
}
MMX_SNE_HD inline int32_t skinNeTiles(int32_t type, int32_t count) {
  return int32_t((skinNeRows(type, count) + kSkinNeTileRows - 1) / kSkinNeTileRows);
}
// Pe = min(parts, T) (parts >= 1, T >= 1)
MMX_SNE_HD inline int32_t skinNeEffectiveParts(int32_t parts, int32_t tiles) {
  return parts < tiles ? parts : tiles;
}
// first tile of part p of Pe: floor(p T / Pe); part p owns [begin(p), begin(p + 1)), never empty for Pe <= T
MMX_SNE_HD inline int32_t skinNePartBegin(int32_t p, int32_t tiles, int32_t effectiveParts) {
  return int32_t(int64_t(p) * int64_t(tiles) / int64_t(effectiveParts));
}
// lower blocks of the 32-wide block triangle of n enabled parameters, and the padded width
MMX_SNE_HD inline int32_t skinNePaddedSolved(int32_t n) {
  return (n + 31) & ~31;
}
MMX_SNE_HD inline int32_t skinNeNumBlocks(int32_t n) {
  const int32_t nb = skinNePaddedSolved(n) >> 5;
  return nb * (nb + 1) / 2;
}

// The workspace of a call with `parts` parts per instance: three arrays, each [instance][part][...], the part innermost of
// the two so that the reducer's loads of one entry over the parts are a fixed stride apart and a wave's are contiguous.
//   acc  float  [B][parts][numBlocks][16 regs][64 lanes]   the MFMA accumulators as the waves hold them
//   g    double [B][parts][nPad]                           h0 + h1 of a column
//   err  double [B][parts]
struct SkinNeWorkspace {
  int32_t parts = 0, numBlocks = 0, nPad = 0;
  int64_t accOffset = 0, gOffset = 0, errOffset = 0; // bytes, multiples of 16
  int64_t bytes = 0; // multiple of 16
  MMX_SNE_HD int64_t accIndex(int64_t b, int32_t part, int32_t block) const { // in floats from accOffset
    return ((b * parts + part) * numBlocks + block) * kSkinNeBlockFloats;
  }
  MMX_SNE_HD int64_t gIndex(int64_t b, int32_t part) const { // in doubles from gOffset
    return (b * parts + part) * nPad;
  }
  MMX_SNE_HD int64_t errIndex(int64_t b, int32_t part) const { // in doubles from errOffset
    return b * parts + part;
  }
};
// false for batch < 1, numEnabled outside 1..128 or parts outside 1..512
bool skinNeWorkspaceLayout(int32_t batch, int32_t numEnabled, int32_t parts, SkinNeWorkspace* out);
// bytes a call needs: 0 for parts <= 1, -1 for an argument out of range (parts outside 0..512)
int64_t skinNeWorkspaceBytes(int32_t batch, int32_t numEnabled, int32_t parts);

// the split a call with parts = 0 takes: min(workgroup slots per instance, tiles, 512), at least 1 -- a part may be a single
// tile (measured on humanoid72 p128 only: DESIGN.md).  false (nothing written) for batch < 1, count < 1, an unknown type,
// computeUnits < 1 or workgroupsPerCu < 1
bool skinNePlan(int32_t batch, int32_t type, int32_t count, int32_t computeUnits, int32_t workgroupsPerCu, int32_t* partsOut);

// The split's own refusals, after the unsplit call's (checkVertexConstraints) have passed.  `parts` is the requested value
// already resolved (0 replaced by the plan's); `requested` the value the caller gave.  MMX_OK, or the status with a message.
struct SkinNeSplitFacts {
  int32_t batch = 0, solved = 0, type = 0, count = 0;
  int32_t requested = 0; // the caller's `parts`
  int32_t parts = 0; // resolved: == requested unless requested == 0
  bool haveWorkspace = false;
  uintptr_t workspaceAddress = 0;
  int64_t workspaceBytes = 0;
};
int32_t checkSkinNeParts(int32_t requested, std::string& err); // the range of `parts` alone: needs nothing else
int32_t checkSkinNeSplit(const SkinNeSplitFacts& f, std::string& err);

} // namespace mmx
