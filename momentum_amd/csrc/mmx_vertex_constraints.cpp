// mmx_vertex_constraints.cpp -- see mmx_vertex_constraints.hpp
#include "mmx_vertex_constraints.hpp"

#include <cmath>

namespace mmx {

int32_t checkVertexConstraints(const mmx_vertex_constraints* c, const VertexConstraintsFacts& f, std::string& err) {
  auto bad = [&](const char* what) {
    err = what;
    return int32_t(MMX_ERR_INVALID_ARGUMENT);
  };
  if (c == nullptr) {
    return bad("the constraint descriptor is null");
  }
  if (!f.haveTheta) {
    return bad("theta is null");
  }
  if (!f.haveOutput) {
    return bad("jtj, jtr and err are all null: nothing to compute");
  }
  if (!f.sameRig) {
    return bad("the skin was created on another rig than the problem's");
  }
  if (c->type != MMX_VC_POSITION && c->type != MMX_VC_PLANE) {
    return bad("unknown constraint type (MMX_VC_POSITION or MMX_VC_PLANE)");
  }
  if (c->count < 1) {
    return bad("count must be >= 1");
  }
  if (c->corners != 1 && c->corners != 3) {
    return bad("corners must be 1 (a vertex) or 3 (a triangle with barycentric weights)");
  }
  if (!(c->function_weight >= 0.f) || !std::isfinite(c->function_weight)) {
    return bad("function_weight must be finite and >= 0");
  }
  if (c->target == nullptr) {
    return bad("target is null");
  }
  if (c->type == MMX_VC_PLANE && c->normal == nullptr) {
    return bad("MMX_VC_PLANE without normals");
  }
  if (c->corners == 3 && (c->vertex == nullptr || c->barycentric == nullptr)) {
    return bad("corners = 3 needs vertex and barycentric");
  }
  if (c->vertex == nullptr && c->count != f.skinVertices) {
    return bad("vertex may be null only with corners = 1 and count = the skin's vertex count");
  }
  if (f.solved < 1) {
    err = "no enabled parameter";
    return MMX_ERR_UNSUPPORTED;
  }
  if (f.solved > kVertexConstraintsMaxSolved) {
    err = "more enabled parameters than the kernel's accumulators take (MMX_SKIN_NE_MAX_SOLVED = 128)";
    return MMX_ERR_UNSUPPORTED;
  }
  if (f.ldsBytes > kVertexConstraintsLdsBudget) {
    err = "the rig's, the columns' and the tile's tables do not fit the kernel's LDS budget (160 KB)";
    return MMX_ERR_UNSUPPORTED;
  }
  return MMX_OK;
}

} // namespace mmx
