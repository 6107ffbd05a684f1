// mmx_closest_points_on_mesh_plan.hpp -- the launch decision of mmx_closest_points_on_mesh as a pure host function (no HIP
// here, no device): what the launcher in mmx_closest_points_on_mesh.hip asks and what mmx_closest_points_on_mesh_plan
// reports, so the tests take their edge shapes from the same place as the kernel
// (tests/test_closest_points_on_mesh_plan_host.py).
#pragma once

#include <cstdint>

namespace mmx {
#pragma GCC visibility push(hidden)

constexpr int32_t kCpmThreads = 256; // a workgroup: four wavefronts
constexpr int32_t kCpmBlock = 4; // sources a lane owns in registers (64 apart), taken two at a time
constexpr int32_t kCpmWaveSources = 64 * kCpmBlock; // sources of one wavefront = of one workgroup
constexpr int32_t kCpmTile = kCpmThreads; // triangles of a staged tile: a thread stages ONE record per tile
constexpr int32_t kCpmRecord = 15; // floats of a triangle's record (a, e1, e2, d11, d12, d22, i11, i22, ibc)
constexpr int32_t kCpmWays = kCpmThreads / 64; // the waves a tile's triangles are divided over
// One form for every size, as in mmx_closest_points_plan.hpp: the four waves of a workgroup hold the SAME sources and each
// scans a quarter of every tile.

struct ClosestPointsOnMeshPlan {
  int32_t sourcesPerWorkgroup = 0; // S
  int32_t triangleTile = 0; // T_t
  int32_t triangleWays = 0; // W
  int64_t workgroups = 0; // batch * ceil(N / S)
};

// false: a size below 1, or more than 2^31 - 1 workgroups
bool closestPointsOnMeshPlan(int32_t batch, int32_t numSource, int32_t numTriangles, ClosestPointsOnMeshPlan* plan);

#pragma GCC visibility pop
} // namespace mmx
