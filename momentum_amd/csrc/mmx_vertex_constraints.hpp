// mmx_vertex_constraints.hpp -- host-side intake of mmx_skin_normal_equations: the descriptor's checks and the kernel's scope
// rules in one pure function (no HIP, no device), so that every refusal is decided -- and testable -- before anything runs.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mmx.h"

namespace mmx {

constexpr int32_t kVertexConstraintsMaxSolved = 128; // == kSkinNeMaxSolved (mmx_kernels.hpp), MMX_SKIN_NE_MAX_SOLVED
constexpr size_t kVertexConstraintsLdsBudget = 160 * 1024 - 64;

struct VertexConstraintsFacts {
  bool sameRig = false; // the skin was created on the problem's rig
  bool haveTheta = false;
  bool haveOutput = false; // at least one of jtj / jtr / err
  int32_t skinVertices = 0; // V
  int32_t solved = 0; // n: enabled parameters
  size_t ldsBytes = 0; // skinNormalEquationsLdsBytes for the call
};

// MMX_OK, or the status of the first condition that applies with a message naming it in `err`.
int32_t checkVertexConstraints(const mmx_vertex_constraints* c, const VertexConstraintsFacts& f, std::string& err);

} // namespace mmx
