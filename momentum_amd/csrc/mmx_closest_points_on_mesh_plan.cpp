// mmx_closest_points_on_mesh_plan.cpp -- see mmx_closest_points_on_mesh_plan.hpp.  No HIP, no device.
#include "mmx_closest_points_on_mesh_plan.hpp"

namespace mmx {

bool closestPointsOnMeshPlan(int32_t batch, int32_t numSource, int32_t numTriangles, ClosestPointsOnMeshPlan* plan) {
  if (batch < 1 || numSource < 1 || numTriangles < 1) {
    return false;
  }
  ClosestPointsOnMeshPlan p;
  p.triangleTile = kCpmTile;
  p.triangleWays = kCpmWays;
  p.sourcesPerWorkgroup = kCpmWaveSources;
  p.workgroups = int64_t(batch) * ((int64_t(numSource) + p.sourcesPerWorkgroup - 1) / p.sourcesPerWorkgroup);
  if (p.workgroups > 0x7fffffffLL) {
    return false;
  }
  *plan = p;
  return true;
}

} // namespace mmx
