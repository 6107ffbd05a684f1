// GPU smoke test of the joint-to-joint distance function in the C++ shell (include/momentum_amd/momentum_amd.hpp):
// on momentum's test chain (createTestCharacter(24), momentum/test/character/character_helpers.cpp:38-55,106-149) the
// tip is pulled towards joint 12 while joint 5 stays put; the error of the pair row collapses, the Distance setter of
// ABI 12 goes through the same block path, and data that does not fit its function throws std::runtime_error.
#include <cmath>
#include <cstdio>

#include "momentum_amd/momentum_amd.hpp"

using namespace momentum_amd;

static Character createTestCharacter(size_t n) {
  Character c;
  Joint j;
  j.name = "root";
  c.skeleton.joints.push_back(j);
  for (size_t i = 1; i < n; ++i) {
    j.name = "joint" + std::to_string(i);
    j.parent = i - 1;
    j.translationOffset = {0.f, 1.f, 0.f};
    c.skeleton.joints.push_back(j);
  }
  auto& pt = c.parameterTransform;
  pt.name = {"root_tx", "root_ty", "root_tz", "root_rx", "root_ry", "root_rz", "scale_global", "joint1_rx", "shared_rz"};
  const int rxStart = int(pt.name.size());
  for (size_t i = 2; i < n; ++i) {
    pt.name.push_back("joint" + std::to_string(i) + "_rx");
  }
  std::vector<ParameterTransform::Triplet> t;
  for (int d = 0; d < 7; ++d) {
    t.push_back({d, d, 1.f});
  }
  t.push_back({1 * 7 + 3, 7, 1.f});
  t.push_back({1 * 7 + 5, 8, 0.5f});
  t.push_back({2 * 7 + 5, 8, 0.5f});
  for (size_t i = 2; i < n; ++i) {
    t.push_back({int(i * 7 + 3), rxStart + int(i) - 2, 1.f});
  }
  pt.setFromTriplets(n, t);
  return c;
}

template <typename F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

int main() {
  const size_t n = 24, B = 4;
  const Character character = createTestCharacter(n);
  DeviceCharacter dev(character, 0);
  BatchedSkeletonSolverFunction fn(dev, B, {5}, {});
  const size_t pairFn = fn.addJointToJointDistanceErrorFunction({23, 20}, {12, 20});
  const size_t distFn = fn.addJointErrorFunction(JointErrorFunctionType::Distance, {5});
  int bad = 0;
  for (size_t b = 0; b < B; ++b) {
    std::vector<PositionData> anchor(1);
    anchor[0].parent = 5;
    anchor[0].target = {0.f, 5.f, 0.f}; // where the rest pose has it
    fn.setPositionConstraints(b, anchor);
    std::vector<JointToJointDistanceData> pairs(2);
    pairs[0].joint1 = 23, pairs[0].joint2 = 12;
    pairs[0].offset1 = {0.f, 0.5f, 0.f};
    pairs[0].targetDistance = 8.f + float(b); // straight chain: 11.5, the bent start of the solve: about 11.1
    pairs[1].joint1 = 20, pairs[1].joint2 = 20; // two points of one joint, already at their distance
    pairs[1].offset2 = {0.3f, 0.f, 0.4f};
    pairs[1].targetDistance = 0.5f;
    fn.setConstraints(pairFn, b, pairs);
    std::vector<DistanceData> dist(1);
    dist[0].parent = 5;
    dist[0].origin = {0.f, 0.f, 0.f};
    dist[0].target = 5.f; // holds at the rest pose
    fn.setConstraints(distFn, b, dist);
  }
  GaussNewtonSolverOptions opt;
  opt.minIterations = 10;
  opt.maxIterations = 10;
  opt.regularization = 0.05f;
  BatchedGaussNewtonSolver solver(opt, &fn);
  const size_t P = fn.getNumParameters();
  std::vector<float> theta(B * P, 0.f);
  for (size_t b = 0; b < B; ++b) {
    for (size_t i = 14; i <= 20; ++i) {
      theta[b * P + i + 7] = 0.1f; // joint<i>_rx: off the straight chain, whose distances do not change to first order
    }
  }
  std::vector<float> jac, res;
  std::vector<double> e0;
  fn.getJacobian(theta, jac, res, e0);
  if (res.size() != B * (3 + 2 + 1)) {
    std::printf("FAIL: %zu residual rows\n", res.size() / B);
    ++bad;
  }
  const std::vector<double> e = solver.solve(theta);
  for (size_t b = 0; b < B; ++b) {
    std::printf("instance %zu: error %.6g -> %.3g, status %d\n", b, e0[b], e[b], solver.getStatus()[b]);
    if (!(e0[b] > 1e-3) || !(e[b] < 1e-3 * e0[b]) || (solver.getStatus()[b] & MMX_SOLVE_ERROR_MASK) != 0) {
      ++bad;
    }
  }
  // a pair function takes two parent lists; its data must name the joints it was added with
  bad += throws([&] { fn.addJointErrorFunction(JointErrorFunctionType::JointToJointDistance, {1, 2}); }) ? 0 : 1;
  bad += throws([&] { fn.addJointToJointDistanceErrorFunction({1, 2}, {3}); }) ? 0 : 1;
  bad += throws([&] {
    std::vector<JointToJointDistanceData> wrong(2);
    wrong[0].joint1 = 23, wrong[0].joint2 = 11;
    wrong[1].joint1 = 20, wrong[1].joint2 = 20;
    fn.setConstraints(pairFn, 0, wrong);
  }) ? 0 : 1;
  bad += throws([&] { fn.setConstraints(distFn, 0, std::vector<JointToJointDistanceData>(1)); }) ? 0 : 1;
  // a second joint outside the skeleton is refused by the library when the payload is uploaded
  bad += throws([&] {
    BatchedSkeletonSolverFunction other(dev, 1, {5}, {});
    other.addJointToJointDistanceErrorFunction({3}, {n});
    other.sync();
  }) ? 0 : 1;
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
