// The intake of mmx_skin_normal_equations on the CPU (checkVertexConstraints, momentum_amd/csrc/mmx_vertex_constraints.cpp: a
// stand-alone program that links that host file and nothing else): every refusal of include/mmx.h returns its status with a
// message naming the condition, in the documented order (argument errors before scope limits), and what is inside passes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../momentum_amd/csrc/mmx_vertex_constraints.hpp"

static int failures = 0;
#define CHECK(cond)                                        \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL line %d: %s\n", __LINE__, #cond);  \
      ++failures;                                          \
    }                                                      \
  } while (0)

int main() {
  using namespace mmx;
  const float f[3] = {0.f, 0.f, 0.f};
  const int32_t v[3] = {0, 0, 0};
  mmx_vertex_constraints ok{};
  ok.type = MMX_VC_PLANE, ok.count = 7, ok.corners = 3, ok.function_weight = 0.5f;
  ok.vertex = v, ok.barycentric = f, ok.target = f, ok.normal = f, ok.weight = f;
  VertexConstraintsFacts in;
  in.sameRig = in.haveTheta = in.haveOutput = true;
  in.skinVertices = 40, in.solved = 128, in.ldsBytes = kVertexConstraintsLdsBudget;
  std::string err;
  auto status = [&](const mmx_vertex_constraints& c, const VertexConstraintsFacts& facts, const char* word) {
    err.clear();
    const int32_t rc = checkVertexConstraints(&c, facts, err);
    if (rc != MMX_OK && std::strstr(err.c_str(), word) == nullptr) {
      std::printf("message '%s' lacks '%s'\n", err.c_str(), word);
      return int32_t(-1);
    }
    return rc;
  };
  CHECK(status(ok, in, "") == MMX_OK && err.empty());
  CHECK(checkVertexConstraints(nullptr, in, err) == MMX_ERR_INVALID_ARGUMENT && err.find("descriptor") != std::string::npos);
  {
    VertexConstraintsFacts x = in;
    x.haveTheta = false;
    CHECK(status(ok, x, "theta") == MMX_ERR_INVALID_ARGUMENT);
    x = in, x.haveOutput = false;
    CHECK(status(ok, x, "all null") == MMX_ERR_INVALID_ARGUMENT);
    x = in, x.sameRig = false;
    CHECK(status(ok, x, "another rig") == MMX_ERR_INVALID_ARGUMENT);
    x = in, x.solved = 129;
    CHECK(status(ok, x, "128") == MMX_ERR_UNSUPPORTED);
    x = in, x.solved = 0;
    CHECK(status(ok, x, "no enabled parameter") == MMX_ERR_UNSUPPORTED);
    x = in, x.ldsBytes = kVertexConstraintsLdsBudget + 1;
    CHECK(status(ok, x, "LDS budget") == MMX_ERR_UNSUPPORTED);
    // an argument error wins over a scope limit
    x = in, x.solved = 500;
    mmx_vertex_constraints c = ok;
    c.count = 0;
    CHECK(status(c, x, "count") == MMX_ERR_INVALID_ARGUMENT);
  }
  auto with = [&](auto change) {
    mmx_vertex_constraints c = ok;
    change(c);
    return c;
  };
  CHECK(status(with([](auto& c) { c.type = 2; }), in, "type") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.type = -1; }), in, "type") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.count = -5; }), in, "count") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.corners = 2; }), in, "corners") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.corners = 4; }), in, "corners") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.function_weight = -0.f - 1e-30f; }), in, "function_weight") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.function_weight = std::numeric_limits<float>::quiet_NaN(); }), in, "function_weight") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.function_weight = std::numeric_limits<float>::infinity(); }), in, "function_weight") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.function_weight = 0.f; }), in, "") == MMX_OK); // (zero is allowed: every row is zero)
  CHECK(status(with([](auto& c) { c.target = nullptr; }), in, "target") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.normal = nullptr; }), in, "normals") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.vertex = nullptr; }), in, "vertex") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.barycentric = nullptr; }), in, "barycentric") == MMX_ERR_INVALID_ARGUMENT);
  // the optional arrays: position constraints need no normals, single vertices no barycentrics, weights default to 1
  CHECK(status(with([](auto& c) { c.type = MMX_VC_POSITION, c.normal = nullptr, c.weight = nullptr; }), in, "") == MMX_OK);
  CHECK(status(with([](auto& c) { c.corners = 1, c.barycentric = nullptr; }), in, "") == MMX_OK);
  // vertex = NULL: corners = 1 and count = V only
  CHECK(status(with([](auto& c) { c.corners = 1, c.vertex = nullptr, c.count = 40; }), in, "") == MMX_OK);
  CHECK(status(with([](auto& c) { c.corners = 1, c.vertex = nullptr, c.count = 39; }), in, "vertex") == MMX_ERR_INVALID_ARGUMENT);
  CHECK(status(with([](auto& c) { c.corners = 1, c.vertex = nullptr, c.count = 41; }), in, "vertex") == MMX_ERR_INVALID_ARGUMENT);
  if (failures != 0) {
    std::printf("FAIL: %d check(s)\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
