// GPU smoke test of the matrix-free gradient in the C++ shell (include/momentum_amd/momentum_amd.hpp,
// BatchedSkeletonSolverFunction::getGradient / SkeletonSolverFunction::getGradient over mmx_eval_gradient_host): on momentum's
// 3-joint test character (createTestCharacter(3), momentum/test/character/character_helpers.cpp:38-55,106-149) with position and
// orientation constraints and a model-parameter prior, the gradient equals 2 J^T r contracted in double from the same
// function's getJacobian, and the error its error.
//
// Bound: both sides are single-precision evaluations.  The CPU oracle's own float32 gradient deviates from its float64 one by
// 5.2e-7 max|g| on this character; four times that is what each side is allowed against the truth (the summation orders
// differ: subtree sums against row order), so the two may differ by 2 x 4 x 5.2e-7 = 4.2e-6 max|g|; the errors likewise by
// 2 x 4 x 4.2e-7 = 3.4e-6 relative.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

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

template <class Fn>
static void fill(Fn& fn, size_t b, float t, size_t P) {
  std::vector<PositionData> pos(3);
  for (size_t k = 0; k < 3; ++k) {
    pos[k].parent = k;
    pos[k].offset = {0.1f * float(k), 0.f, 0.05f};
    pos[k].target = {0.3f * std::sin(t + float(k)), float(k) + 0.2f * std::cos(t), 0.25f * float(k) * std::sin(2.f * t)};
    pos[k].weight = 0.5f + 0.25f * float(k);
  }
  std::vector<OrientationData> ori(1);
  ori[0].parent = 2;
  ori[0].target = {std::sin(0.5f * t), 0.f, 0.f, std::cos(0.5f * t)};
  std::vector<float> target(P), weights(P);
  for (size_t p = 0; p < P; ++p) {
    target[p] = 0.05f * float(p) - 0.1f * t;
    weights[p] = p % 3 == 0 ? 0.f : 0.5f + 0.1f * float(p);
  }
  if constexpr (std::is_same<Fn, SkeletonSolverFunction>::value) {
    (void)b;
    fn.setPositionConstraints(pos);
    fn.setOrientationConstraints(ori);
    fn.setTargetParameters(target, weights, 0.7f);
  } else {
    fn.setPositionConstraints(b, pos);
    fn.setOrientationConstraints(b, ori);
    fn.setTargetParameters(b, target, weights, 0.7f);
  }
}

int main() {
  const size_t n = 3, B = 4;
  const Character character = createTestCharacter(n);
  DeviceCharacter dev(character, 0);
  BatchedSkeletonSolverFunction fn(dev, B, {0, 1, 2}, {2});
  const size_t P = fn.getNumParameters();
  std::vector<float> theta(B * P);
  for (size_t b = 0; b < B; ++b) {
    fill(fn, b, 0.3f + 0.4f * float(b), P);
    for (size_t p = 0; p < P; ++p) {
      theta[b * P + p] = 0.2f * std::sin(1.7f * float(p) + float(b));
    }
  }
  std::vector<float> jac, res, grad;
  std::vector<double> errJ, errG;
  fn.getJacobian(theta, jac, res, errJ);
  fn.getGradient(theta, grad, errG);
  const size_t M = res.size() / B;
  int bad = 0;
  for (size_t b = 0; b < B; ++b) {
    double gmax = 0.0, dmax = 0.0;
    for (size_t p = 0; p < P; ++p) {
      double g = 0.0;
      for (size_t i = 0; i < M; ++i) {
        g += double(jac[(b * P + p) * M + i]) * double(res[b * M + i]);
      }
      g *= 2.0;
      gmax = std::fmax(gmax, std::fabs(g));
      dmax = std::fmax(dmax, std::fabs(g - double(grad[b * P + p])));
    }
    const double de = std::fabs(errG[b] - errJ[b]);
    const bool ok = dmax <= 4.2e-6 * gmax && de <= 3.4e-6 * errJ[b] && gmax > 0.0;
    std::printf("element %zu: max|g| %.6g, max|g - 2 J^T r| %.3g (%.3g of max|g|, bound 4.2e-6), error %.9g against %.9g (%.3g relative, bound 3.4e-6)%s\n", b, gmax, dmax,
                dmax / gmax, errG[b], errJ[b], de / errJ[b], ok ? "" : "  FAIL");
    bad += ok ? 0 : 1;
  }
  // the single-instance function: element 1's problem alone gives element 1's row, bit for bit (a row depends on its own inputs only)
  SkeletonSolverFunction one(dev, {0, 1, 2}, {2});
  fill(one, 0, 0.3f + 0.4f * 1.f, P);
  std::vector<float> th1(theta.begin() + P, theta.begin() + 2 * P), g1;
  const double e1 = one.getGradient(th1, g1);
  if (g1.size() != P || std::memcmp(g1.data(), &grad[P], P * sizeof(float)) != 0 || std::memcmp(&e1, &errG[1], sizeof(double)) != 0) {
    std::printf("FAIL: SkeletonSolverFunction::getGradient != element 1 of the batch\n");
    ++bad;
  }
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
