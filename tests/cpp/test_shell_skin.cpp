// GPU smoke test of linear-blend skinning in the C++ shell (include/momentum_amd/momentum_amd.hpp, DeviceSkin over
// mmx_skin_points_host / mmx_skin_points_backward_host): on momentum's 3-joint test character with the five-vertex, K = 4 skin
// of the Python tests (zero-weight padding, joint 2 named by padding only: tests/skinning_reference.py hand_skin), a perturbed
// inverse bind and per-element rest positions, the posed vertices equal the formula written here in double, and the state and
// rest gradients of L = sum(c . vertices) equal central differences (h = 1e-6) of it.
//
// Bounds: the float32 run of the torch reference (tests/skinning_reference.py) deviates from its float64 run on these inputs
// by 1.55e-7 max|out|, 1.51e-7 max|state_grad| and 1.41e-7 max|rest_grad| (largest of the four elements); four times that is
// what the GPU is allowed against the double values -- the rule of tests/test_gpu_skin_points.py.  The central differences
// themselves are good to 1e-9.
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

constexpr size_t B = 4, J = 3, V = 5, K = 4;
static const int32_t kJoint[V * K] = {0, 1, 2, 2, 1, 0, 2, 0, 0, 2, 2, 2, 1, 1, 2, 0, 0, 1, 0, 1};
static const float kWeight[V * K] = {0.7f, 0.3f, 0.f, 0.f, 0.25f, 0.75f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.5f, 0.125f, 0.f, 0.375f, 0.4f, 0.3f, 0.2f, 0.1f};
static const float kRest[V * 3] = {0.1f, 0.2f, -0.3f, 0.3f, 1.1f, 0.2f, -0.2f, 0.4f, 0.1f, 0.05f, 1.6f, -0.1f, 0.2f, 0.9f, 0.3f};

// one element in double: state [J][8], rest [V][3] -> vertices [V][3]; the polynomial p + 2 w (u x p) + 2 u x (u x p)
static void skin(const double* st, const float* inv, const double* rest, double* out) {
  for (size_t v = 0; v < V; ++v) {
    double acc[3] = {0, 0, 0};
    for (size_t k = 0; k < K; ++k) {
      const double w = double(kWeight[v * K + k]);
      if (w == 0.0) {
        continue;
      }
      const size_t j = size_t(kJoint[v * K + k]);
      const float* m = inv + 12 * j;
      const double* r = rest + 3 * v;
      double p[3];
      for (int i = 0; i < 3; ++i) {
        p[i] = double(m[4 * i]) * r[0] + double(m[4 * i + 1]) * r[1] + double(m[4 * i + 2]) * r[2] + double(m[4 * i + 3]);
      }
      const double* s = st + 8 * j;
      const double qx = s[3], qy = s[4], qz = s[5], qw = s[6];
      const double ux = 2 * (qy * p[2] - qz * p[1]), uy = 2 * (qz * p[0] - qx * p[2]), uz = 2 * (qx * p[1] - qy * p[0]);
      const double rot[3] = {p[0] + qw * ux + (qy * uz - qz * uy), p[1] + qw * uy + (qz * ux - qx * uz), p[2] + qw * uz + (qx * uy - qy * ux)};
      for (int i = 0; i < 3; ++i) {
        acc[i] += w * (s[i] + s[7] * rot[i]);
      }
    }
    out[3 * v] = acc[0], out[3 * v + 1] = acc[1], out[3 * v + 2] = acc[2];
  }
}

int main() {
  const Character character = createTestCharacter(J);
  DeviceCharacter dev(character, 0);
  std::vector<float> state(B * J * 8), cot(B * V * 3), rest(B * V * 3), inv(J * 12);
  for (size_t b = 0; b < B; ++b) {
    for (size_t j = 0; j < J; ++j) {
      float* s = state.data() + (b * J + j) * 8;
      double q[4] = {std::sin(0.9 * j + 0.4 * b + 1), std::cos(1.1 * j + 0.3 * b), std::sin(0.5 * j - 0.2 * b + 2), 1.0 + 0.1 * std::cos(double(j + b))};
      const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int c = 0; c < 3; ++c) {
        s[c] = float(0.5 * std::sin(1.3 * c + 0.7 * j + double(b)));
      }
      for (int c = 0; c < 4; ++c) {
        s[3 + c] = float(q[c] / n);
      }
      s[7] = float(1 + 0.2 * std::sin(j + 0.5 * b));
    }
    for (size_t v = 0; v < V; ++v) {
      for (size_t c = 0; c < 3; ++c) {
        cot[(b * V + v) * 3 + c] = float(std::cos(0.9 * double(3 * v + c) + 0.5 * b));
        rest[(b * V + v) * 3 + c] = float(double(kRest[3 * v + c]) + 0.05 * std::sin(double(b + v + c)));
      }
    }
  }
  for (size_t j = 0; j < J; ++j) { // the rest pose's inverse (joint j sits at (0, j, 0)), every entry perturbed
    for (size_t i = 0; i < 12; ++i) {
      const double base = (i == 0 || i == 5 || i == 10) ? 1.0 : (i == 7 ? -double(j) : 0.0);
      inv[12 * j + i] = float(base + 0.1 * std::sin(double(i + 2 * j)));
    }
  }
  const DeviceSkin skinDev(
      dev, K, std::vector<int32_t>(kJoint, kJoint + V * K), std::vector<float>(kWeight, kWeight + V * K), inv, std::vector<float>(kRest, kRest + V * 3));
  if (skinDev.numVertices() != V || mmx_skin_num_vertices(skinDev.handle()) != int32_t(V)) {
    std::printf("FAIL: numVertices\n");
    return 1;
  }
  const std::vector<float> out = skinDev.skinPoints(B, state, rest);
  const DeviceSkin::Gradients grad = skinDev.skinPointsBackward(B, state, cot, rest, true);
  const DeviceSkin::Gradients noRest = skinDev.skinPointsBackward(B, state, cot, rest);
  if (out.size() != B * V * 3 || grad.state.size() != B * J * 8 || grad.restPositions.size() != B * V * 3 || !noRest.restPositions.empty() ||
      noRest.state != grad.state) {
    std::printf("FAIL: sizes, or the state gradient depends on whether the rest gradient is asked for\n");
    return 1;
  }
  int bad = 0;
  for (size_t b = 0; b < B; ++b) {
    double st[J * 8], rs[V * 3], ref[V * 3];
    for (size_t i = 0; i < J * 8; ++i) {
      st[i] = double(state[b * J * 8 + i]);
    }
    for (size_t i = 0; i < V * 3; ++i) {
      rs[i] = double(rest[b * V * 3 + i]);
    }
    skin(st, inv.data(), rs, ref);
    double omax = 0.0, odiff = 0.0;
    for (size_t i = 0; i < V * 3; ++i) {
      omax = std::fmax(omax, std::fabs(ref[i]));
      odiff = std::fmax(odiff, std::fabs(ref[i] - double(out[b * V * 3 + i])));
    }
    auto loss = [&]() {
      double o[V * 3], l = 0.0;
      skin(st, inv.data(), rs, o);
      for (size_t i = 0; i < V * 3; ++i) {
        l += double(cot[b * V * 3 + i]) * o[i];
      }
      return l;
    };
    auto central = [&](double& x) {
      const double h = 1e-6, keep = x;
      x = keep + h;
      const double lp = loss();
      x = keep - h;
      const double lm = loss();
      x = keep;
      return (lp - lm) / (2 * h);
    };
    double smax = 0.0, sdiff = 0.0, rmax = 0.0, rdiff = 0.0;
    bool zeroRow = true;
    for (size_t i = 0; i < J * 8; ++i) {
      const double g = central(st[i]);
      smax = std::fmax(smax, std::fabs(g));
      sdiff = std::fmax(sdiff, std::fabs(g - double(grad.state[b * J * 8 + i])));
      if (i >= 16) { // joint 2 has no influence: exact zeros
        zeroRow = zeroRow && grad.state[b * J * 8 + i] == 0.f;
      }
    }
    for (size_t i = 0; i < V * 3; ++i) {
      const double g = central(rs[i]);
      rmax = std::fmax(rmax, std::fabs(g));
      rdiff = std::fmax(rdiff, std::fabs(g - double(grad.restPositions[b * V * 3 + i])));
    }
    const bool ok = odiff <= 6.2e-7 * omax && sdiff <= 6.0e-7 * smax && rdiff <= 5.6e-7 * rmax && omax > 0.1 && smax > 0.1 && rmax > 0.1 && zeroRow;
    std::printf(
        "element %zu: vertices off by %.3g of max|out| (bound 6.2e-7), state gradient by %.3g of max|g| (bound 6.0e-7), rest gradient by %.3g (bound "
        "5.6e-7), joint 2's row %s%s\n",
        b, odiff / omax, sdiff / smax, rdiff / rmax, zeroRow ? "zero" : "NOT zero", ok ? "" : "  FAIL");
    bad += ok ? 0 : 1;
  }
  // a refusal becomes std::runtime_error
  bool threw = false;
  try {
    (void)skinDev.skinPoints(B, std::vector<float>(3), rest);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  try {
    std::vector<int32_t> badJoint(kJoint, kJoint + V * K);
    badJoint[3] = 3; // (a zero-weight slot)
    const DeviceSkin refused(dev, K, badJoint, std::vector<float>(kWeight, kWeight + V * K), inv, std::vector<float>(kRest, kRest + V * 3));
    threw = false;
  } catch (const std::runtime_error&) {
  }
  if (!threw) {
    std::printf("FAIL: a refusal did not throw\n");
    return 1;
  }
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
