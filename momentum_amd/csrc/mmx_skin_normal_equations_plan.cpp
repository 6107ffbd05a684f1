// mmx_skin_normal_equations_plan.cpp -- see mmx_skin_normal_equations_plan.hpp
#include "mmx_skin_normal_equations_plan.hpp"

#include <algorithm>

namespace mmx {

namespace {

constexpr int64_t alignUp16(int64_t v) {
  return (v + 15) & ~int64_t(15);
}

} // namespace

bool skinNeWorkspaceLayout(int32_t batch, int32_t numEnabled, int32_t parts, SkinNeWorkspace* out) {
  if (batch < 1 || numEnabled < 1 || numEnabled > kSkinNeSplitMaxSolved || parts < 1 || parts > kSkinNeMaxParts) {
    return false;
  }
  SkinNeWorkspace w;
  w.parts = parts, w.numBlocks = skinNeNumBlocks(numEnabled), w.nPad = skinNePaddedSolved(numEnabled);
  const int64_t records = int64_t(batch) * int64_t(parts); // < 2^40; times at most 40 KB of accumulators: < 2^56
  w.accOffset = 0;
  w.gOffset = alignUp16(w.accOffset + records * w.numBlocks * kSkinNeBlockFloats * int64_t(sizeof(float)));
  w.errOffset = alignUp16(w.gOffset + records * w.nPad * int64_t(sizeof(double)));
  w.bytes = alignUp16(w.errOffset + records * int64_t(sizeof(double)));
  if (out != nullptr) {
    *out = w;
  }
  return true;
}

int64_t skinNeWorkspaceBytes(int32_t batch, int32_t numEnabled, int32_t parts) {
  if (batch < 1 || numEnabled < 1 || numEnabled > kSkinNeSplitMaxSolved || parts < 0 || parts > kSkinNeMaxParts) {
    return -1;
  }
  if (parts <= 1) {
    return 0;
  }
  SkinNeWorkspace w;
  skinNeWorkspaceLayout(batch, numEnabled, parts, &w);
  return w.bytes;
}

bool skinNePlan(int32_t batch, int32_t type, int32_t count, int32_t computeUnits, int32_t workgroupsPerCu, int32_t* partsOut) {
  if (batch < 1 || count < 1 || (type != MMX_VC_POSITION && type != MMX_VC_PLANE) || computeUnits < 1 || workgroupsPerCu < 1) {
    return false;
  }
  const int64_t tiles = skinNeTiles(type, count);
  const int64_t slots = int64_t(computeUnits) * int64_t(workgroupsPerCu) / int64_t(batch);
  const int64_t most = std::min<int64_t>(kSkinNeMaxParts, tiles);
  if (partsOut != nullptr) {
    *partsOut = int32_t(std::min(std::max<int64_t>(slots, 1), most));
  }
  return true;
}

int32_t checkSkinNeParts(int32_t requested, std::string& err) {
  if (requested < 0) {
    err = "parts is negative (1..MMX_SKIN_NE_MAX_PARTS, or 0 for the plan's choice)";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  if (requested > kSkinNeMaxParts) {
    err = "parts exceeds MMX_SKIN_NE_MAX_PARTS (512)";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  return MMX_OK;
}

int32_t checkSkinNeSplit(const SkinNeSplitFacts& f, std::string& err) {
  const int32_t rc = checkSkinNeParts(f.requested, err);
  if (rc != MMX_OK) {
    return rc;
  }
  auto bad = [&](const char* what) {
    err = what;
    return int32_t(MMX_ERR_INVALID_ARGUMENT);
  };
  if (f.parts < 1 || f.parts > kSkinNeMaxParts) {
    return bad("the resolved parts is outside 1..MMX_SKIN_NE_MAX_PARTS");
  }
  const int32_t tiles = skinNeTiles(f.type, f.count);
  if (tiles < 1 || skinNeEffectiveParts(f.parts, tiles) <= 1) {
    return MMX_OK; // one part: the unsplit launch, no workspace read or written
  }
  const int64_t need = skinNeWorkspaceBytes(f.batch, f.solved, f.parts); // for the parts asked for, not for min(parts, T)
  if (need < 0) {
    return bad("batch or the enabled parameters are outside the workspace's range");
  }
  if (!f.haveWorkspace) {
    return bad("the workspace is null and more than one part is in effect");
  }
  if (f.workspaceBytes < need) {
    err = "workspace_bytes is below mmx_skin_normal_equations_workspace_bytes for this batch, enabled parameters and parts (" +
        std::to_string(f.workspaceBytes) + " < " + std::to_string(need) + ")";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  if ((f.workspaceAddress & 15u) != 0) {
    return bad("the workspace is not 16-byte aligned");
  }
  return MMX_OK;
}

} // namespace mmx
