// GPU smoke test of the split form of the vertex constraints' Gauss-Newton terms in the C++ shell
// (include/momentum_amd/momentum_amd.hpp, DeviceSkin::normalEquations with `parts` over mmx_skin_normal_equations_split_host):
// on momentum's 3-joint test character with a five-vertex, K = 4 skin, 100 plane constraints on single vertices (100 rows: four
// tiles of 32) for two elements.
//   parts = 1 gives the bits of the form without `parts`; parts = 4 and parts = 512 give the same bits (min(parts, tiles)).
//   parts = 3 against parts = 1: H is bitwise symmetric; the error within 2^-40 (non-negative terms summed in double); g
//   within 2^-23 max|g| (one float32 rounding of double sums that differ in association); H within 2 x 100 x 2^-24 max|H| --
//   both are float32 accumulations of the same 100 products per entry in different association, each within
//   rows x 2^-24 x sqrt(H_ii H_jj) <= rows x 2^-24 x max|H| of the exact sum.
//   parts = 0 (the library's plan) has the bits of the explicit parts that normalEquationsAutoParts reports for the descriptor;
//   normalEquationsWorkspaceBytes is the C function's value; parts = 513 and a negative value throw.
// The device-memory overload is not run here: the program links the library alone and has no device allocator.
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

constexpr size_t B = 2, J = 3, P = 10, V = 5, K = 4, C = 100;
static const int32_t kJoint[V * K] = {0, 1, 2, 2, 1, 0, 2, 0, 0, 2, 2, 2, 1, 1, 2, 0, 0, 1, 0, 1};
static const float kWeight[V * K] = {0.7f, 0.3f, 0.f, 0.f, 0.25f, 0.75f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.5f, 0.125f, 0.f, 0.375f, 0.4f, 0.3f, 0.2f, 0.1f};
static const float kRest[V * 3] = {0.1f, 0.2f, -0.3f, 0.3f, 1.1f, 0.2f, -0.2f, 0.4f, 0.1f, 0.05f, 1.6f, -0.1f, 0.2f, 0.9f, 0.3f};

static bool sameBits(const VertexNormalEquations& a, const VertexNormalEquations& b) {
  return a.n == b.n && a.jtj == b.jtj && a.jtr == b.jtr && a.error == b.error;
}

int main() {
  const Character character = createTestCharacter(J);
  DeviceCharacter dev(character, 0);
  BatchedSkeletonSolverFunction fn(dev, B, {0}, {});
  std::vector<float> inv(J * 12), theta(B * P);
  for (size_t j = 0; j < J; ++j) {
    for (size_t i = 0; i < 12; ++i) {
      const double base = (i == 0 || i == 5 || i == 10) ? 1.0 : (i == 7 ? -double(j) : 0.0);
      inv[12 * j + i] = float(base + 0.1 * std::sin(double(i + 2 * j)));
    }
  }
  for (size_t b = 0; b < B; ++b) {
    for (size_t p = 0; p < P; ++p) {
      theta[b * P + p] = float(0.4 * std::sin(1.7 * double(p) + double(b)));
    }
  }
  const DeviceSkin skinDev(
      dev, K, std::vector<int32_t>(kJoint, kJoint + V * K), std::vector<float>(kWeight, kWeight + V * K), inv, std::vector<float>(kRest, kRest + V * 3));
  VertexConstraints c;
  c.corners = 1;
  c.functionWeight = 0.7f;
  for (size_t b = 0; b < B; ++b) {
    for (size_t i = 0; i < C; ++i) {
      c.vertex.push_back(int32_t((3 * i + b) % V));
      for (int k = 0; k < 3; ++k) {
        c.target.push_back(float(0.5 * std::sin(1.1 * double(3 * i + size_t(k)) + 0.7 * double(b))));
        c.normal.push_back(float(std::cos(0.8 * double(3 * i + size_t(k)) + 0.3 * double(b))));
      }
      c.weight.push_back(float(1.0 + 0.5 * std::sin(double(i) + 0.4 * double(b))));
    }
  }
  const VertexNormalEquations unsplit = skinDev.normalEquations(fn, theta, c);
  const VertexNormalEquations one = skinDev.normalEquations(fn, theta, c, 1), three = skinDev.normalEquations(fn, theta, c, 3);
  const VertexNormalEquations four = skinDev.normalEquations(fn, theta, c, 4), many = skinDev.normalEquations(fn, theta, c, 512);
  const VertexNormalEquations planned = skinDev.normalEquations(fn, theta, c, 0);
  int bad = 0;
  auto expect = [&](bool ok, const char* what) {
    if (!ok) {
      std::printf("FAIL: %s\n", what);
      ++bad;
    }
  };
  const size_t N = unsplit.n;
  expect(N == P && three.n == N && three.jtj.size() == B * N * N && three.jtr.size() == B * N && three.error.size() == B, "sizes");
  expect(sameBits(one, unsplit), "parts = 1 has the bits of the unsplit form");
  expect(sameBits(four, many), "parts = 512 has the bits of parts = 4 (four tiles)");
  mmx_vertex_constraints shape{}; // type, count and corners are read; the arrays are not
  shape.type = MMX_VC_PLANE, shape.count = int32_t(C), shape.corners = 1, shape.function_weight = c.functionWeight;
  const int32_t autoParts = skinDev.normalEquationsAutoParts(fn, shape);
  std::printf("auto parts: %d\n", autoParts);
  expect(autoParts >= 1 && autoParts <= 4, "auto parts within the four tiles");
  expect(sameBits(planned, skinDev.normalEquations(fn, theta, c, autoParts)), "parts = 0 has the bits of the parts the query reports");
  for (size_t b = 0; b < B && bad == 0; ++b) {
    double hmax = 0, hdiff = 0, gmax = 0, gdiff = 0;
    bool symmetric = true;
    for (size_t i = 0; i < N; ++i) {
      gmax = std::fmax(gmax, std::fabs(double(unsplit.jtr[b * N + i])));
      gdiff = std::fmax(gdiff, std::fabs(double(three.jtr[b * N + i]) - double(unsplit.jtr[b * N + i])));
      for (size_t j = 0; j < N; ++j) {
        const size_t at = (b * N + i) * N + j;
        hmax = std::fmax(hmax, std::fabs(double(unsplit.jtj[at])));
        hdiff = std::fmax(hdiff, std::fabs(double(three.jtj[at]) - double(unsplit.jtj[at])));
        symmetric = symmetric && three.jtj[at] == three.jtj[(b * N + j) * N + i];
      }
    }
    const double ediff = std::fabs(three.error[b] - unsplit.error[b]);
    const bool ok = symmetric && hmax > 0.1 && gmax > 0.1 && unsplit.error[b] > 0.01 && hdiff <= 2.0 * double(C) * std::ldexp(1.0, -24) * hmax &&
        gdiff <= std::ldexp(1.0, -23) * gmax && ediff <= std::ldexp(1.0, -40) * unsplit.error[b];
    std::printf(
        "element %zu, parts 3 against parts 1: H off by %.3g of max|H| (bound %.3g), g by %.3g of max|g| (bound 1.19e-7), the error by %.3g (bound 9.1e-13), H %s%s\n",
        b, hdiff / hmax, 2.0 * double(C) * std::ldexp(1.0, -24), gdiff / gmax, ediff / unsplit.error[b], symmetric ? "symmetric" : "NOT symmetric",
        ok ? "" : "  FAIL");
    bad += ok ? 0 : 1;
  }
  expect(DeviceSkin::normalEquationsWorkspaceBytes(fn, 1) == 0 && DeviceSkin::normalEquationsWorkspaceBytes(fn, 513) == -1, "workspace bytes: edges");
  for (int32_t parts : {2, 3, 512}) {
    const int64_t bytes = DeviceSkin::normalEquationsWorkspaceBytes(fn, parts);
    // n = 10: one block of 16 x 64 floats, 32 padded doubles and the error's double per (instance, part), 16-byte pieces
    expect(bytes == mmx_skin_normal_equations_workspace_bytes(int32_t(B), int32_t(N), parts) && bytes >= int64_t(B) * parts * (4096 + 256 + 8), "workspace bytes");
  }
  for (int32_t parts : {513, -1}) {
    bool threw = false;
    try {
      (void)skinDev.normalEquations(fn, theta, c, parts);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    expect(threw, "parts out of range throws");
  }
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
