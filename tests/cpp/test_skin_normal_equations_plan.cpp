// The split of mmx_skin_normal_equations_split on the CPU (momentum_amd/csrc/mmx_skin_normal_equations_plan.cpp: a stand-alone
// program that links that host file and nothing else): the part ranges tile the tiles, the workspace's regions do not overlap
// and end within the reported size, every refusal of the split returns its status with a message naming the condition, in the
// documented order, and what is inside passes.  The unsplit refusals come first in the entry point because it runs
// checkVertexConstraints before these functions (mmx_capi.hip); here that order shows as: these functions read nothing of the
// descriptor but its type and count.
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../momentum_amd/csrc/mmx_skin_normal_equations_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                        \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL line %d: %s\n", __LINE__, #cond);  \
      ++failures;                                          \
    }                                                      \
  } while (0)

int main() {
  using namespace mmx;
  // ---- rows, tiles, ranges
  CHECK(skinNeTiles(MMX_VC_PLANE, 1) == 1 && skinNeTiles(MMX_VC_PLANE, 32) == 1 && skinNeTiles(MMX_VC_PLANE, 33) == 2);
  CHECK(skinNeTiles(MMX_VC_POSITION, 10) == 1 && skinNeTiles(MMX_VC_POSITION, 11) == 2 && skinNeTiles(MMX_VC_POSITION, 22) == 3);
  CHECK(skinNeTiles(MMX_VC_POSITION, 2147483647) == 201326592 && skinNeTiles(MMX_VC_PLANE, 0) == 0);
  for (int32_t T = 1; T <= 70; ++T) {
    for (int32_t parts = 1; parts <= 71; ++parts) {
      const int32_t asked = parts == 71 ? 512 : parts;
      const int32_t pe = skinNeEffectiveParts(asked, T);
      CHECK(pe == (asked < T ? asked : T));
      CHECK(skinNePartBegin(0, T, pe) == 0 && skinNePartBegin(pe, T, pe) == T);
      for (int32_t p = 0; p < pe; ++p) {
        CHECK(skinNePartBegin(p + 1, T, pe) > skinNePartBegin(p, T, pe)); // no part is empty; consecutive by construction
      }
    }
  }
  CHECK(skinNePartBegin(511, 201326592, 512) == int32_t(int64_t(511) * 201326592 / 512)); // no 32-bit overflow
  // ---- the workspace: regions of (instance, part, field) do not overlap and end within the size
  for (int32_t n : {1, 32, 33, 96, 97, 128}) {
    for (int32_t parts : {2, 3, 7}) {
      for (int32_t batch : {1, 3}) {
        SkinNeWorkspace w;
        CHECK(skinNeWorkspaceLayout(batch, n, parts, &w));
        CHECK(w.bytes == skinNeWorkspaceBytes(batch, n, parts) && w.parts == parts);
        CHECK(w.numBlocks == skinNeNumBlocks(n) && w.nPad == skinNePaddedSolved(n) && w.nPad >= n && w.nPad % 32 == 0);
        CHECK(w.accOffset % 16 == 0 && w.gOffset % 16 == 0 && w.errOffset % 16 == 0 && w.bytes % 16 == 0);
        std::vector<std::pair<int64_t, int64_t>> regions;
        for (int32_t b = 0; b < batch; ++b) {
          for (int32_t p = 0; p < parts; ++p) {
            for (int32_t k = 0; k < w.numBlocks; ++k) {
              const int64_t at = w.accOffset + w.accIndex(b, p, k) * 4;
              regions.push_back({at, at + int64_t(kSkinNeBlockFloats) * 4});
            }
            const int64_t g = w.gOffset + w.gIndex(b, p) * 8, e = w.errOffset + w.errIndex(b, p) * 8;
            regions.push_back({g, g + int64_t(w.nPad) * 8});
            regions.push_back({e, e + 8});
          }
        }
        for (size_t i = 0; i < regions.size(); ++i) {
          CHECK(regions[i].first >= 0 && regions[i].second <= w.bytes);
          for (size_t j = i + 1; j < regions.size(); ++j) {
            CHECK(regions[i].second <= regions[j].first || regions[j].second <= regions[i].first);
          }
        }
      }
    }
  }
  CHECK(skinNeWorkspaceBytes(1, 5, 0) == 0 && skinNeWorkspaceBytes(1, 5, 1) == 0 && skinNeWorkspaceBytes(1, 5, 2) > 0);
  CHECK(skinNeWorkspaceBytes(0, 5, 2) == -1 && skinNeWorkspaceBytes(1, 0, 2) == -1 && skinNeWorkspaceBytes(1, 129, 2) == -1);
  CHECK(skinNeWorkspaceBytes(1, 5, -1) == -1 && skinNeWorkspaceBytes(1, 5, 513) == -1);
  CHECK(!skinNeWorkspaceLayout(1, 5, 0, nullptr) && !skinNeWorkspaceLayout(1, 5, 513, nullptr) && skinNeWorkspaceLayout(1, 5, 512, nullptr));
  // ---- the plan
  int32_t parts = -7;
  CHECK(!skinNePlan(0, MMX_VC_PLANE, 5, 256, 2, &parts) && parts == -7);
  CHECK(!skinNePlan(1, MMX_VC_PLANE, 0, 256, 2, &parts) && parts == -7);
  CHECK(!skinNePlan(1, 2, 5, 256, 2, &parts) && parts == -7);
  CHECK(!skinNePlan(1, MMX_VC_PLANE, 5, 0, 2, &parts) && parts == -7);
  CHECK(!skinNePlan(1, MMX_VC_PLANE, 5, 256, 0, &parts) && parts == -7);
  CHECK(skinNePlan(1, MMX_VC_PLANE, 5, 256, 2, &parts) && parts == 1); // one tile
  CHECK(skinNePlan(512, MMX_VC_POSITION, 20000, 256, 2, &parts) && parts == 1); // a workgroup per slot already
  CHECK(skinNePlan(16, MMX_VC_POSITION, 20000, 256, 2, &parts) && parts == 32);
  CHECK(skinNePlan(1, MMX_VC_POSITION, 20000, 256, 2, &parts) && parts == 512); // 1875 tiles, 512 slots
  CHECK(skinNePlan(1, MMX_VC_POSITION, 2147483647, 2147483647, 2, &parts) && parts == 512);
  CHECK(skinNePlan(1, MMX_VC_PLANE, 5, 256, 2, nullptr));
  // ---- the refusals, in order: the range of parts, then the workspace (null, short, misaligned)
  std::string err;
  auto status = [&](const SkinNeSplitFacts& f, const char* word) {
    err.clear();
    const int32_t rc = checkSkinNeSplit(f, err);
    if (rc != MMX_OK && std::strstr(err.c_str(), word) == nullptr) {
      std::printf("message '%s' lacks '%s'\n", err.c_str(), word);
      return int32_t(-1);
    }
    return rc;
  };
  SkinNeSplitFacts ok;
  ok.batch = 3, ok.solved = 40, ok.type = MMX_VC_PLANE, ok.count = 100; // four tiles
  ok.requested = ok.parts = 3;
  ok.haveWorkspace = true, ok.workspaceAddress = 0x1000, ok.workspaceBytes = skinNeWorkspaceBytes(3, 40, 3);
  CHECK(status(ok, "") == MMX_OK && err.empty());
  auto with = [&](auto change) {
    SkinNeSplitFacts f = ok;
    change(f);
    return f;
  };
  CHECK(status(with([](auto& f) { f.requested = f.parts = -1; }), "negative") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.requested = f.parts = 513; }), "MMX_SKIN_NE_MAX_PARTS") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(checkSkinNeParts(-1, err) == MMX_ERR_INVALID_ARGUMENT && checkSkinNeParts(513, err) == MMX_ERR_INVALID_ARGUMENT);
  CHECK(checkSkinNeParts(0, err) == MMX_OK && checkSkinNeParts(1, err) == MMX_OK && checkSkinNeParts(512, err) == MMX_OK);
  CHECK(status(with([](auto& f) { f.haveWorkspace = false, f.workspaceAddress = 0; }), "null") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.workspaceBytes -= 1; }), "workspace_bytes") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.workspaceBytes = 0; }), "workspace_bytes") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.workspaceBytes = -5; }), "workspace_bytes") == MMX_ERR_INVALID_ARGUMENT);
  for (uintptr_t off : {1u, 4u, 8u, 15u}) {
    CHECK(status(with([off](auto& f) { f.workspaceAddress += off; }), "16-byte") == MMX_ERR_INVALID_ARGUMENT);
  }
  // the range of parts wins over the workspace, a null workspace over its size, the size over the alignment
  CHECK(status(with([](auto& f) { f.requested = f.parts = 513, f.haveWorkspace = false; }), "MMX_SKIN_NE_MAX_PARTS") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.haveWorkspace = false, f.workspaceBytes = 0; }), "null") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.workspaceBytes = 16, f.workspaceAddress = 0x1004; }), "workspace_bytes") == MMX_ERR_INVALID_ARGUMENT);
  // the size is taken for the parts asked for, not for min(parts, tiles): 512 parts of four tiles need 512 parts' bytes
  CHECK(status(with([](auto& f) { f.requested = f.parts = 512; }), "workspace_bytes") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.requested = f.parts = 512, f.workspaceBytes = skinNeWorkspaceBytes(3, 40, 512); }), "") == MMX_OK);
  CHECK(status(with([](auto& f) { f.workspaceBytes += 1000; }), "") == MMX_OK);
  // an effective parts of one needs no workspace: parts 1, or one tile
  CHECK(status(with([](auto& f) { f.requested = f.parts = 1, f.haveWorkspace = false, f.workspaceBytes = 0, f.workspaceAddress = 0; }), "") == MMX_OK);
  CHECK(status(with([](auto& f) { f.count = 32, f.haveWorkspace = false, f.workspaceBytes = 0, f.workspaceAddress = 0; }), "") == MMX_OK);
  CHECK(status(with([](auto& f) { f.requested = f.parts = 1, f.workspaceAddress = 0x1001; }), "") == MMX_OK); // (not read)
  // parts = 0 resolved by the plan: checked with the resolved value
  CHECK(status(with([](auto& f) { f.requested = 0, f.parts = 3; }), "") == MMX_OK);
  CHECK(status(with([](auto& f) { f.requested = 0, f.parts = 4; }), "workspace_bytes") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& f) { f.requested = 0, f.parts = 0; }), "resolved") == MMX_ERR_INVALID_ARGUMENT);
  if (failures != 0) {
    std::printf("FAIL: %d check(s)\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
