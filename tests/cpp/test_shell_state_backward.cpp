// GPU smoke test of the skeleton state's backward pass in the C++ shell (include/momentum_amd/momentum_amd.hpp,
// BatchedSkeletonState::backward over mmx_eval_skeleton_state_backward_host): on momentum's 3-joint test character
// (createTestCharacter(3), momentum/test/character/character_helpers.cpp:38-55,106-149) the gradient of L = sum(c . state)
// equals central differences (h = 1e-6) of a forward kinematics written here in double, and the forward the shell returns
// is that forward kinematics.
//
// Bound: the float32 run of the pure-torch reference (tests/skeleton_state_reference.py) deviates from its float64 run by
// 1.5e-7 max|g| on these inputs (largest of the four elements); four times that, 6.0e-7 max|g|, is what the GPU is allowed against
// the double gradient -- the rule of tests/test_gpu_skeleton_state_backward.py.  The central differences themselves are good
// to 1e-9.
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

// the 3-joint character's forward kinematics in double: theta [10] -> state [3][8]
struct Q {
  double x, y, z, w;
};
static Q mul(const Q& a, const Q& b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x,
          a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
static void rot(const Q& q, const double* v, double* o) {
  const double ux = 2 * (q.y * v[2] - q.z * v[1]), uy = 2 * (q.z * v[0] - q.x * v[2]), uz = 2 * (q.x * v[1] - q.y * v[0]);
  o[0] = v[0] + q.w * ux + (q.y * uz - q.z * uy);
  o[1] = v[1] + q.w * uy + (q.z * ux - q.x * uz);
  o[2] = v[2] + q.w * uz + (q.x * uy - q.y * ux);
}
static void forward(const double* th, double* st) {
  double jp[3][7] = {};
  for (int d = 0; d < 7; ++d) {
    jp[0][d] = th[d];
  }
  jp[1][3] = th[7], jp[1][5] = 0.5 * th[8], jp[2][5] = 0.5 * th[8], jp[2][3] = th[9];
  double tp[3] = {0, 0, 0}, sp = 1.0;
  Q qp{0, 0, 0, 1};
  for (int j = 0; j < 3; ++j) {
    const double* p = jp[j];
    const Q ql = mul(mul(Q{0, 0, std::sin(0.5 * p[5]), std::cos(0.5 * p[5])}, Q{0, std::sin(0.5 * p[4]), 0, std::cos(0.5 * p[4])}), Q{std::sin(0.5 * p[3]), 0, 0, std::cos(0.5 * p[3])});
    const double tl[3] = {sp * p[0], sp * ((j > 0 ? 1.0 : 0.0) + p[1]), sp * p[2]};
    double r[3];
    rot(qp, tl, r);
    for (int k = 0; k < 3; ++k) {
      tp[k] += r[k];
    }
    qp = mul(qp, ql);
    sp *= std::exp2(p[6]);
    double* o = st + 8 * j;
    o[0] = tp[0], o[1] = tp[1], o[2] = tp[2], o[3] = qp.x, o[4] = qp.y, o[5] = qp.z, o[6] = qp.w, o[7] = sp;
  }
}

int main() {
  const size_t n = 3, B = 4;
  const Character character = createTestCharacter(n);
  DeviceCharacter dev(character, 0);
  BatchedSkeletonSolverFunction fn(dev, B, {0}, {});
  const size_t P = fn.getNumParameters(), J = n;
  if (P != 10) {
    std::printf("FAIL: P = %zu\n", P);
    return 1;
  }
  std::vector<float> theta(B * P), cot(B * J * 8);
  for (size_t b = 0; b < B; ++b) {
    for (size_t p = 0; p < P; ++p) {
      theta[b * P + p] = 0.4f * std::sin(1.7f * float(p) + float(b));
    }
    for (size_t i = 0; i < J * 8; ++i) {
      cot[b * J * 8 + i] = std::cos(0.9f * float(i) + 0.5f * float(b));
    }
  }
  const std::vector<float> grad = BatchedSkeletonState::backward(fn, theta, cot);
  const BatchedSkeletonState state(fn, theta);
  int bad = 0;
  if (grad.size() != B * P) {
    std::printf("FAIL: grad.size() = %zu\n", grad.size());
    return 1;
  }
  for (size_t b = 0; b < B; ++b) {
    double th[10], st[24];
    for (size_t p = 0; p < P; ++p) {
      th[p] = double(theta[b * P + p]);
    }
    forward(th, st);
    double fmax = 0.0;
    for (size_t j = 0; j < J; ++j) {
      const Transform& t = state[b].jointState[j].transform;
      const double got[8] = {t.translation[0], t.translation[1], t.translation[2], t.rotation[0], t.rotation[1], t.rotation[2], t.rotation[3], t.scale};
      for (int c = 0; c < 8; ++c) {
        fmax = std::fmax(fmax, std::fabs(got[c] - st[8 * j + c]));
      }
    }
    auto loss = [&](const double* x) {
      double s[24], l = 0.0;
      forward(x, s);
      for (size_t i = 0; i < J * 8; ++i) {
        l += double(cot[b * J * 8 + i]) * s[i];
      }
      return l;
    };
    double gmax = 0.0, dmax = 0.0;
    for (size_t p = 0; p < P; ++p) {
      const double h = 1e-6, keep = th[p];
      th[p] = keep + h;
      const double lp = loss(th);
      th[p] = keep - h;
      const double lm = loss(th);
      th[p] = keep;
      const double g = (lp - lm) / (2 * h);
      gmax = std::fmax(gmax, std::fabs(g));
      dmax = std::fmax(dmax, std::fabs(g - double(grad[b * P + p])));
    }
    const bool ok = dmax <= 6.0e-7 * gmax && gmax > 0.1 && fmax <= 5e-6;
    std::printf("element %zu: max|g| %.6g, max|g - central differences| %.3g (%.3g of max|g|, bound 6.0e-7), forward off by %.3g%s\n", b, gmax, dmax, dmax / gmax, fmax,
                ok ? "" : "  FAIL");
    bad += ok ? 0 : 1;
  }
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
