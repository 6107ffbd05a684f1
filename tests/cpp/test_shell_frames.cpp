// GPU smoke test of warm-started frame sequences in the C++ shell (include/momentum_amd/momentum_amd.hpp,
// BatchedGaussNewtonSolver::solveFrames over mmx_solve_frames_host): on momentum's 3-joint test character
// (createTestCharacter(3), momentum/test/character/character_helpers.cpp:38-55,106-149), S = 3 sequences of F = 4 frames
// whose targets drift from frame to frame.  One solveFrames call must equal -- bit for bit, parameters, errors, iterations
// and status -- four chained solve calls on the same handle pinned to the one-wavefront route, call f started from call
// f - 1's rows of frame f - 1 (the per-frame loop of marker_tracker.cpp:905-913).
#include <cmath>
#include <cstdio>
#include <cstring>

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

int main() {
  const size_t n = 3, S = 3, F = 4, B = F * S;
  const Character character = createTestCharacter(n);
  DeviceCharacter dev(character, 0);
  BatchedSkeletonSolverFunction fn(dev, B, {0, 1, 2}, {2});
  for (size_t f = 0; f < F; ++f) {
    for (size_t s = 0; s < S; ++s) { // element f S + s: frame f of sequence s
      const float t = 0.15f * float(f) + 0.4f * float(s);
      std::vector<PositionData> pos(3);
      for (size_t k = 0; k < 3; ++k) {
        pos[k].parent = k;
        pos[k].offset = {0.1f * float(k), 0.f, 0.05f};
        pos[k].target = {0.3f * std::sin(t + float(k)), float(k) + 0.2f * std::cos(t), 0.25f * float(k) * std::sin(2.f * t)};
      }
      fn.setPositionConstraints(f * S + s, pos);
      std::vector<OrientationData> ori(1);
      ori[0].parent = 2;
      ori[0].target = {std::sin(0.5f * t), 0.f, 0.f, std::cos(0.5f * t)};
      fn.setOrientationConstraints(f * S + s, ori);
    }
  }
  GaussNewtonSolverOptions opt; // the batched driver's defaults (tensor_ik.h:66-82) with the line search on
  opt.minIterations = 4;
  opt.maxIterations = 50;
  opt.threshold = 10.f;
  opt.regularization = 0.01f;
  opt.doLineSearch = true;
  BatchedGaussNewtonSolver solver(opt, &fn);
  fn.sync();
  mmx_tuning tuning{};
  tuning.route = MMX_ROUTE_WAVE; // the chained reference runs the kernels solveFrames runs
  check(mmx_problem_set_tuning(fn.handle(), &tuning));

  const size_t P = fn.getNumParameters();
  std::vector<float> init(S * P, 0.f);
  for (size_t s = 0; s < S; ++s) {
    init[s * P + 7] = 0.1f + 0.05f * float(s);
    init[s * P + 8] = -0.1f;
  }
  int bad = 0;
  // the loop a caller writes today: one solve per frame, frame f's rows seeded from frame f - 1's results
  std::vector<float> ref(B * P, 0.f);
  std::vector<double> refErr(B);
  std::vector<int32_t> refIt(B), refSt(B);
  std::vector<float> prev = init;
  for (size_t f = 0; f < F; ++f) {
    std::vector<float> theta(B * P, 0.f);
    std::memcpy(&theta[f * S * P], prev.data(), S * P * sizeof(float));
    const std::vector<double> e = solver.solve(theta);
    for (size_t s = 0; s < S; ++s) {
      const size_t b = f * S + s;
      std::memcpy(&ref[b * P], &theta[b * P], P * sizeof(float));
      refErr[b] = e[b], refIt[b] = solver.getIterations()[b], refSt[b] = solver.getStatus()[b];
    }
    std::memcpy(prev.data(), &theta[f * S * P], S * P * sizeof(float));
  }
  // one launch; the rows of frames >= 1 are not read
  std::vector<float> theta(B * P, std::nanf(""));
  std::memcpy(theta.data(), init.data(), S * P * sizeof(float));
  const std::vector<double> e = solver.solveFrames(theta, F);
  for (size_t b = 0; b < B; ++b) {
    const bool same = std::memcmp(&theta[b * P], &ref[b * P], P * sizeof(float)) == 0 && std::memcmp(&e[b], &refErr[b], sizeof(double)) == 0 &&
        solver.getIterations()[b] == refIt[b] && solver.getStatus()[b] == refSt[b];
    std::printf("frame %zu sequence %zu: error %.6g, %d iterations, status %d%s\n", b / S, b % S, e[b], solver.getIterations()[b], solver.getStatus()[b], same ? "" : "  != chained solve");
    if (!same || (solver.getStatus()[b] & MMX_SOLVE_ERROR_MASK) != 0 || solver.getIterations()[b] < 4) {
      ++bad;
    }
  }
  if (mmx_problem_last_route(fn.handle()) != MMX_ROUTE_WAVE) {
    std::printf("FAIL: last route %d\n", mmx_problem_last_route(fn.handle()));
    ++bad;
  }
  // a frame count that does not divide the batch is refused, and the parameters stay as they were
  std::vector<float> keep = init;
  keep.resize(B * P, 0.f);
  std::vector<float> again = keep;
  bool threw = false;
  try {
    solver.solveFrames(again, 5);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  if (!threw || std::memcmp(again.data(), keep.data(), B * P * sizeof(float)) != 0) {
    std::printf("FAIL: num_frames = 5 on a batch of %zu\n", B);
    ++bad;
  }
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
