// mmx_closest_points_plan.hpp -- the launch decision of mmx_closest_points as a pure host function (no HIP here, no device):
// what the launcher in mmx_closest_points.hip asks and what mmx_closest_points_plan reports, so the tests take their edge
// shapes from the same place as the kernel (tests/test_closest_points_plan_host.py).
#pragma once

#include <cstdint>

namespace mmx {
#pragma GCC visibility push(hidden)

constexpr int32_t kCpThreads = 256; // a workgroup: four wavefronts
constexpr int32_t kCpBlock = 4; // sources a lane owns in registers (64 apart)
constexpr int32_t kCpWaveSources = 64 * kCpBlock; // sources of one wavefront
constexpr int32_t kCpTile = 1024, kCpTileNormals = 512; // targets of a staged tile: both fill 12 KB per buffer
constexpr int32_t kCpWays = kCpThreads / 64; // the waves a tile's targets are divided over
// One form for every size: the four waves of a workgroup hold the SAME kCpWaveSources sources and each scans a quarter of every
// tile.  The other form (every wave scanning whole tiles for sources of its own, four times the sources per workgroup) was
// measured: 0.5-1.4 % faster at 4096 x 2000 x 2000 and 1.4-1.9 times SLOWER at N = 500 and N = 1100, where its workgroups
// are half empty, so it is not built.

struct ClosestPointsPlan {
  int32_t sourcesPerWorkgroup = 0; // S
  int32_t targetTile = 0; // T
  int32_t targetWays = 0; // W = kCpWays
  int64_t workgroups = 0; // batch * ceil(N / S)
};

// false: a size below 1, or more than 2^31 - 1 workgroups
bool closestPointsPlan(int32_t batch, int32_t numSource, int32_t numTarget, bool withNormals, ClosestPointsPlan* plan);

#pragma GCC visibility pop
} // namespace mmx
