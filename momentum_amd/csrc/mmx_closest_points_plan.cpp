// mmx_closest_points_plan.cpp -- see mmx_closest_points_plan.hpp.  No HIP, no device.
#include "mmx_closest_points_plan.hpp"

namespace mmx {

bool closestPointsPlan(int32_t batch, int32_t numSource, int32_t numTarget, bool withNormals, ClosestPointsPlan* plan) {
  if (batch < 1 || numSource < 1 || numTarget < 1) {
    return false;
  }
  ClosestPointsPlan p;
  p.targetTile = withNormals ? kCpTileNormals : kCpTile;
  p.targetWays = kCpWays;
  p.sourcesPerWorkgroup = kCpWaveSources;
  p.workgroups = int64_t(batch) * ((int64_t(numSource) + p.sourcesPerWorkgroup - 1) / p.sourcesPerWorkgroup);
  if (p.workgroups > 0x7fffffffLL) {
    return false;
  }
  *plan = p;
  return true;
}

} // namespace mmx
