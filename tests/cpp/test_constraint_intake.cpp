// The constraint intake (momentum_amd/csrc/mmx_constraint_intake.{hpp,cpp}) against a transcription of the code it replaced,
// over generated requests on a small rig.  A stand-alone program: it links the host unit and mmx_host_tables.cpp, nothing else.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all test_constraint_intake.cpp
//       ../../momentum_amd/csrc/mmx_constraint_intake.cpp ../../momentum_amd/csrc/mmx_host_tables.cpp
//
// `referenceSetConstraints` / `referenceSetInstanceParents` below repeat, in their order and with their variable names, the
// validation, the derived integers and the comparison with the previous state of mmx_problem_set_constraints and
// mmx_problem_set_instance_parents as they stood in mmx_capi.hip before the intake existed -- the device work left out, every
// device call taken to succeed.  They are the specification: they are not edited to make this test pass.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../momentum_amd/csrc/mmx_constraint_intake.hpp"

namespace {

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// ---- the rig: a 6-joint tree; parameter 0 is shared by five joint-parameter rows, row 7 * 5 + 3 is driven by five parameters
struct Rig {
  std::vector<int32_t> parent{-1, 0, 1, 1, 0, 4};
  std::vector<int32_t> outer, inner;
  std::vector<float> value, preRot, offset, ptOffsets;
  int32_t J = 6, P = 9;
  Rig() {
    outer.push_back(0);
    for (int32_t row = 0; row < 7 * J; ++row) {
      const int32_t j = row / 7, dof = row % 7;
      if (dof == 3) { // rx of every joint: its own parameter (joint 5: parameters 4..8) ...
        if (j == 5) {
          for (int32_t p = 4; p < 9; ++p) {
            inner.push_back(p);
          }
        } else {
          inner.push_back(j < 4 ? j : 3);
        }
      } else if (dof == 4 && j < 5) { // ... ry: the shared parameter 0 and one more
        inner.push_back(0);
        inner.push_back(1 + j);
      }
      outer.push_back(int32_t(inner.size()));
    }
    value.assign(inner.size(), 1.f);
    preRot.assign(size_t(4 * J), 0.f);
    offset.assign(size_t(3 * J), 0.f);
    ptOffsets.assign(size_t(7 * J), 0.f);
  }
  mmx_rig_desc desc() const {
    mmx_rig_desc d{};
    d.num_joints = J;
    d.num_params = P;
    d.parent = parent.data();
    d.pre_rotation = preRot.data();
    d.translation_offset = offset.data();
    d.pt_outer = outer.data();
    d.pt_inner = inner.data();
    d.pt_value = value.data();
    d.pt_offsets = ptOffsets.data();
    return d;
  }
};

// ---- the transcription -------------------------------------------------------------------------------------------------
struct LossRef {
  int32_t type;
  float alpha, invC2, c;
};
struct JointBlockHost {
  int32_t type = 0, count = 0;
  std::vector<int32_t> parent;
  std::vector<int32_t> parentB;
};
struct BlockDevRef {
  int32_t type, count, first, rowStart;
  LossRef loss;
  float nearClip;
};
struct Handle { // the fields of mmx_problem the setters decide on
  int32_t J = 0, P = 0, Kp = 0, Ko = 0, U = 0, M = 0;
  std::vector<std::unique_ptr<JointBlockHost>> blocks;
  std::vector<BlockDevRef> blockDev;
  std::vector<mmx_ellipsoid_limit> ellipsoids;
  std::vector<mmx_parameter_limit> limits;
  int32_t genRows = 0, hasModel = 0, rowsJoint = 0, fnCols = 0;
  LossRef lossPos{0, 2.f, 1.f, 1.f}, lossOri{0, 2.f, 1.f, 1.f};
  bool tablesDirty = false;
  // mmx_problem_set_instance_parents
  std::vector<int32_t> unionPos, unionOri, instPosHost, instOriHost;
  bool instParentsFromHost = false, instPos = false, instOri = false;
};
struct Outcome {
  int32_t code = MMX_OK;
  std::string message;
  int site = -1; // which refusal of the reference
  bool blocksChanged = false, ellipsoidsChanged = false, structureChanged = false;
};
long reached[32] = {};
Outcome fail(int site, int32_t code, const std::string& msg) {
  ++reached[site];
  Outcome o;
  o.code = code;
  o.message = msg;
  o.site = site;
  return o;
}
int jointBlockFuncDim(int type) {
  return (type == MMX_JC_AIM_DIST || type == MMX_JC_AIM_DIR || type == MMX_JC_FIXED_AXIS_DIFF) ? 3 : type == MMX_JC_PROJECTION ? 2 : 1;
}

Outcome referenceSetConstraints(Handle* pb, const mmx_rig_desc& rigDesc, const mmx_constraint_data* c) {
  if (c == nullptr) {
    return fail(0, MMX_ERR_INVALID_ARGUMENT, "constraint data is null");
  }
  if (pb->Kp > 0 && (!c->pos_offset || !c->pos_target || !c->pos_weight)) {
    return fail(1, MMX_ERR_INVALID_ARGUMENT, "position constraint arrays are null");
  }
  if (pb->Ko > 0 && (!c->ori_offset || !c->ori_target || !c->ori_weight)) {
    return fail(2, MMX_ERR_INVALID_ARGUMENT, "orientation constraint arrays are null");
  }
  if (c->memory != MMX_MEM_DEVICE && c->memory != MMX_MEM_HOST) {
    return fail(3, MMX_ERR_INVALID_ARGUMENT, "constraint data: unknown memory space");
  }
  auto makeLoss = [](float alpha, float cc) {
    LossRef l{0, 2.f, 1.f, 1.f};
    if (cc > 0.f) {
      l.alpha = alpha;
      l.invC2 = 1.f / (cc * cc);
      l.c = cc;
      const float kEps = 1e-9f;
      if (alpha >= 2.f - kEps && alpha <= 2.f + kEps) {
        l.type = 0;
      } else if (alpha >= 1.f - kEps && alpha <= 1.f + kEps) {
        l.type = 1;
      } else if (alpha >= -kEps && alpha <= kEps) {
        l.type = 2;
      } else if (alpha == MMX_LOSS_WELSCH) {
        l.type = 3;
      } else {
        l.type = 4;
      }
    }
    return l;
  };
  const int32_t P = pb->P;
  if (c->num_limits < 0 || (c->num_limits > 0 && c->limits == nullptr)) {
    return fail(4, MMX_ERR_INVALID_ARGUMENT, "limits: negative count or null array");
  }
  if ((c->model_target == nullptr) != (c->model_weights == nullptr)) {
    return fail(5, MMX_ERR_INVALID_ARGUMENT, "model_target and model_weights must be given together");
  }
  for (int32_t l = 0; l < c->num_limits; ++l) {
    const mmx_parameter_limit& lm = c->limits[l];
    const bool model = lm.type == MMX_LIMIT_MINMAX || lm.type == MMX_LIMIT_LINEAR || lm.type == MMX_LIMIT_HALFPLANE;
    const bool joint = lm.type == MMX_LIMIT_MINMAX_JOINT || lm.type == MMX_LIMIT_LINEAR_JOINT;
    const bool two = lm.type == MMX_LIMIT_LINEAR || lm.type == MMX_LIMIT_HALFPLANE || lm.type == MMX_LIMIT_LINEAR_JOINT;
    if (lm.type == MMX_LIMIT_MINMAX_JOINT_PASSIVE) {
      continue;
    }
    if (!model && !joint) {
      return fail(
          6, MMX_ERR_UNSUPPORTED,
          "limit " + std::to_string(l) +
              ": MinMax, MinMaxJoint, MinMaxJointPassive (ignored like in the reference), Linear, LinearJoint and HalfPlane go here; "
              "Ellipsoid limits travel in mmx_constraint_data::ellipsoid_limits");
    }
    const int32_t bound = joint ? MMX_PARAMS_PER_JOINT * pb->J : P;
    if (lm.index0 < 0 || lm.index0 >= bound || (two && (lm.index1 < 0 || lm.index1 >= bound))) {
      return fail(7, MMX_ERR_INVALID_ARGUMENT, "limit " + std::to_string(l) + ": parameter index out of range");
    }
    if (mmx::limitParameters(&rigDesc, lm).size() > 4) {
      return fail(8, MMX_ERR_UNSUPPORTED, "limit " + std::to_string(l) + ": more than four model parameters drive the limited joint parameters");
    }
  }
  if (c->num_function_weights < 0 || c->num_function_weights > 4 + MMX_MAX_JOINT_BLOCKS) {
    return fail(9, MMX_ERR_INVALID_ARGUMENT, "num_function_weights out of range (columns: position, orientation, limits, model parameters, joint blocks)");
  }
  if (c->num_joint_blocks < 0 || c->num_joint_blocks > MMX_MAX_JOINT_BLOCKS || (c->num_joint_blocks > 0 && c->joint_blocks == nullptr)) {
    return fail(10, MMX_ERR_INVALID_ARGUMENT, "joint_blocks: count out of range or null array");
  }
  bool blocksChanged = size_t(c->num_joint_blocks) != pb->blocks.size();
  int32_t genRows = 0, genCount = 0;
  for (int32_t i = 0; i < c->num_joint_blocks; ++i) {
    const mmx_joint_constraint_block& jb = c->joint_blocks[i];
    const std::string tag = "joint block " + std::to_string(i);
    if (jb.type < MMX_JC_PLANE || jb.type > MMX_JC_JOINT_TO_JOINT_DISTANCE) {
      return fail(11, MMX_ERR_UNSUPPORTED, tag + ": unknown error-function type");
    }
    const bool pointOnly = jb.type == MMX_JC_PROJECTION || jb.type == MMX_JC_DISTANCE;
    const bool pairType = jb.type == MMX_JC_JOINT_TO_JOINT_DISTANCE;
    if ((pointOnly || pairType) && jb.loss_c > 0.f && !(jb.loss_alpha == 2.f && jb.loss_c == 1.f)) {
      return fail(12, MMX_ERR_UNSUPPORTED, tag + ": projection / distance / joint-to-joint distance blocks take the L2 loss only (loss_c <= 0 or (alpha, c) = (2, 1))");
    }
    if (jb.type == MMX_JC_PROJECTION && !std::isfinite(jb.near_clip)) {
      return fail(13, MMX_ERR_INVALID_ARGUMENT, tag + ": near_clip is not finite");
    }
    if (jb.count < 0 || (jb.count > 0 && (jb.parent == nullptr || (!pairType && jb.global == nullptr) || jb.weight == nullptr))) {
      return fail(14, MMX_ERR_INVALID_ARGUMENT, tag + ": negative count or null parent / global / weight array");
    }
    const bool plane = jb.type == MMX_JC_PLANE || jb.type == MMX_JC_HALF_PLANE;
    const bool fixedAxis = jb.type == MMX_JC_FIXED_AXIS_DIFF || jb.type == MMX_JC_FIXED_AXIS_COS || jb.type == MMX_JC_FIXED_AXIS_ANGLE;
    const bool needD = plane || jb.type == MMX_JC_DISTANCE || pairType;
    if (jb.count > 0 && ((!fixedAxis && jb.local_point == nullptr) || (!plane && !pointOnly && jb.local_dir == nullptr) || (needD && jb.plane_d == nullptr))) {
      return fail(15, MMX_ERR_INVALID_ARGUMENT, tag + ": a payload array its error function needs is null");
    }
    if (jb.count > 0 && jb.type == MMX_JC_PROJECTION && jb.projection == nullptr) {
      return fail(16, MMX_ERR_INVALID_ARGUMENT, tag + ": projection block without its projection matrices");
    }
    const int32_t numParents = pairType ? 2 * jb.count : jb.count;
    for (int32_t k = 0; k < numParents; ++k) {
      if (jb.parent[k] < 0 || jb.parent[k] >= pb->J) {
        return fail(17, MMX_ERR_INVALID_ARGUMENT, tag + ": parent joint out of range");
      }
    }
    genRows += jointBlockFuncDim(jb.type) * jb.count;
    genCount += jb.count;
    if (!blocksChanged) {
      const JointBlockHost& h = *pb->blocks[size_t(i)];
      blocksChanged = h.type != jb.type || h.count != jb.count || !std::equal(h.parent.begin(), h.parent.end(), jb.parent) ||
          h.parentB.size() != size_t(numParents - jb.count) || !std::equal(h.parentB.begin(), h.parentB.end(), jb.parent + jb.count);
    }
  }
  if (genCount > 1024) {
    return fail(18, MMX_ERR_UNSUPPORTED, "more than 1024 constraints in the further joint-constraint blocks");
  }
  if (c->num_ellipsoid_limits < 0 || c->num_ellipsoid_limits > 256 || (c->num_ellipsoid_limits > 0 && c->ellipsoid_limits == nullptr)) {
    return fail(19, MMX_ERR_INVALID_ARGUMENT, "ellipsoid_limits: count out of range or null array");
  }
  for (int32_t i = 0; i < c->num_ellipsoid_limits; ++i) {
    const mmx_ellipsoid_limit& e = c->ellipsoid_limits[i];
    if (e.parent < 0 || e.parent >= pb->J || e.ellipsoid_parent < 0 || e.ellipsoid_parent >= pb->J) {
      return fail(20, MMX_ERR_INVALID_ARGUMENT, "ellipsoid limit " + std::to_string(i) + ": joint index out of range");
    }
  }
  // ---- from here on the problem is modified
  if (c->function_weights != nullptr && c->num_function_weights > 0) {
    pb->fnCols = c->num_function_weights;
  } else {
    pb->fnCols = 0;
  }
  pb->lossPos = makeLoss(c->pos_loss_alpha, c->pos_loss_c);
  pb->lossOri = makeLoss(c->ori_loss_alpha, c->ori_loss_c);
  if (blocksChanged) {
    pb->tablesDirty = true;
    pb->blocks.clear();
    for (int32_t i = 0; i < c->num_joint_blocks; ++i) {
      auto h = std::make_unique<JointBlockHost>();
      h->type = c->joint_blocks[i].type;
      h->count = c->joint_blocks[i].count;
      h->parent.assign(c->joint_blocks[i].parent, c->joint_blocks[i].parent + h->count);
      if (h->type == MMX_JC_JOINT_TO_JOINT_DISTANCE) {
        h->parentB.assign(c->joint_blocks[i].parent + h->count, c->joint_blocks[i].parent + 2 * h->count);
      }
      pb->blocks.push_back(std::move(h));
    }
  }
  pb->blockDev.assign(size_t(c->num_joint_blocks), BlockDevRef{});
  {
    int32_t first = 0, row = 3 * pb->U;
    for (int32_t i = 0; i < c->num_joint_blocks; ++i) {
      const mmx_joint_constraint_block& jb = c->joint_blocks[i];
      BlockDevRef& k = pb->blockDev[size_t(i)];
      k.type = jb.type;
      k.count = jb.count;
      k.first = first;
      k.rowStart = row;
      k.loss = makeLoss(jb.loss_alpha, jb.loss_c);
      k.nearClip = jb.type == MMX_JC_PROJECTION ? jb.near_clip : 0.f;
      first += jb.count;
      row += jointBlockFuncDim(jb.type) * jb.count;
    }
  }
  pb->genRows = genRows;
  const bool ellipsoidsChanged = size_t(c->num_ellipsoid_limits) != pb->ellipsoids.size() ||
      (c->num_ellipsoid_limits > 0 &&
       std::memcmp(c->ellipsoid_limits, pb->ellipsoids.data(), size_t(c->num_ellipsoid_limits) * sizeof(mmx_ellipsoid_limit)) != 0);
  pb->ellipsoids.assign(c->ellipsoid_limits, c->ellipsoid_limits + c->num_ellipsoid_limits);
  std::vector<mmx_parameter_limit> kept;
  for (int32_t l = 0; l < c->num_limits; ++l) {
    if (c->limits[l].type != MMX_LIMIT_MINMAX_JOINT_PASSIVE) {
      kept.push_back(c->limits[l]);
    }
  }
  const bool structureChanged = pb->tablesDirty || blocksChanged || ellipsoidsChanged || (c->model_target != nullptr) != (pb->hasModel != 0) || kept.size() != pb->limits.size() ||
      (!kept.empty() && std::memcmp(kept.data(), pb->limits.data(), kept.size() * sizeof(mmx_parameter_limit)) != 0);
  pb->tablesDirty = pb->tablesDirty || structureChanged;
  pb->limits = std::move(kept);
  const int32_t NL = int32_t(pb->limits.size());
  pb->hasModel = c->model_target != nullptr ? 1 : 0;
  const int32_t rowsE = 3 * int32_t(pb->ellipsoids.size());
  pb->M = 3 * pb->U + pb->genRows + rowsE + NL + (pb->hasModel ? P : 0);
  pb->rowsJoint = 3 * pb->U + pb->genRows + rowsE;
  if (structureChanged) {
    pb->tablesDirty = false; // uploadProblemTables succeeded
  }
  Outcome o;
  o.blocksChanged = blocksChanged;
  o.ellipsoidsChanged = ellipsoidsChanged;
  o.structureChanged = structureChanged;
  return o;
}

struct ParentsOutcome {
  int32_t code = MMX_OK;
  std::string message;
  bool unchanged = false, sameTables = false;
};
ParentsOutcome referenceSetInstanceParents(Handle* pb, const std::vector<int32_t>& hpIn, const std::vector<int32_t>& hoIn, int32_t memory) {
  std::vector<int32_t> hp = hpIn, ho = hoIn;
  ParentsOutcome out;
  std::vector<uint8_t> seenP(size_t(pb->J), 0), seenO(size_t(pb->J), 0);
  for (int32_t j : hp) {
    if (j < 0 || j >= pb->J) {
      out.code = MMX_ERR_INVALID_ARGUMENT;
      out.message = "instance parents: position constraint parent joint out of range";
      return out;
    }
    seenP[size_t(j)] = 1;
  }
  for (int32_t j : ho) {
    if (j < 0 || j >= pb->J) {
      out.code = MMX_ERR_INVALID_ARGUMENT;
      out.message = "instance parents: orientation constraint parent joint out of range";
      return out;
    }
    seenO[size_t(j)] = 1;
  }
  if (memory == MMX_MEM_HOST && !pb->tablesDirty && pb->instParentsFromHost && hp == pb->instPosHost && ho == pb->instOriHost) {
    out.unchanged = true;
    return out;
  }
  const bool dp = !hp.empty(), dq = !ho.empty(); // place(): the device pointer is null exactly when the list is empty
  std::vector<int32_t> unionPos, unionOri;
  for (int32_t j = 0; j < pb->J; ++j) {
    if (seenP[size_t(j)]) {
      unionPos.push_back(j);
    }
    if (seenO[size_t(j)]) {
      unionOri.push_back(j);
    }
  }
  const bool sameTables = !pb->tablesDirty && dp == pb->instPos && dq == pb->instOri && unionPos == pb->unionPos && unionOri == pb->unionOri;
  pb->instPos = dp;
  pb->instOri = dq;
  pb->instParentsFromHost = memory == MMX_MEM_HOST;
  pb->instPosHost = std::move(hp);
  pb->instOriHost = std::move(ho);
  out.sameTables = sameTables;
  if (sameTables) {
    return out;
  }
  pb->tablesDirty = true;
  pb->unionPos = std::move(unionPos);
  pb->unionOri = std::move(unionOri);
  pb->tablesDirty = false; // uploadProblemTables succeeded
  return out;
}

// ---- the handle as the setters keep it now, written from the intake records the way mmx_capi.hip does -------------------------
struct NewHandle {
  int32_t Kp = 0, Ko = 0;
  std::vector<mmx::ProblemTopology::Block> blocks;
  std::vector<mmx_ellipsoid_limit> ellipsoids;
  std::vector<mmx_parameter_limit> limits;
  bool hasModel = false, tablesDirty = false;
  std::vector<int32_t> unionPos, unionOri, instPosHost, instOriHost;
  bool instParentsFromHost = false, instPos = false, instOri = false;
};
mmx::ConstraintIntake newSetConstraints(NewHandle* pb, const mmx_rig_desc& rig, const mmx_constraint_data* c) {
  mmx::ConstraintIntake in = mmx::intakeConstraints(rig, pb->Kp, pb->Ko, c, {pb->blocks, pb->ellipsoids, pb->limits, pb->hasModel, pb->tablesDirty});
  if (in.code != MMX_OK) {
    return in;
  }
  if (in.blocksChanged) {
    pb->blocks = in.blocks;
  }
  pb->ellipsoids.assign(c->ellipsoid_limits, c->ellipsoid_limits + c->num_ellipsoid_limits);
  pb->limits = in.limits;
  pb->hasModel = in.hasModel;
  if (in.structureChanged) {
    pb->tablesDirty = false;
  }
  return in;
}

// ---- generated requests ----------------------------------------------------------------------------------------------------
struct Rng {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  }
  int32_t below(int32_t n) {
    return int32_t(next() % uint32_t(n));
  }
  bool coin() {
    return (next() & 1) != 0;
  }
};
const float kPayload[4] = {0.f, 0.f, 0.f, 0.f}; // payload pointers are tested against null, never followed

struct Request { // owns the host arrays a mmx_constraint_data points to
  std::vector<mmx_parameter_limit> limits;
  std::vector<mmx_joint_constraint_block> blocks;
  std::vector<std::vector<int32_t>> parents;
  std::vector<mmx_ellipsoid_limit> ellipsoids;
  mmx_constraint_data c{};
  Request() = default;
  Request(const Request& o) : limits(o.limits), blocks(o.blocks), parents(o.parents), ellipsoids(o.ellipsoids), c(o.c) {}
  Request& operator=(const Request&) = delete;
  const mmx_constraint_data* data() { // re-points the struct at the arrays (call after every edit)
    c.num_limits = c.num_limits < 0 ? c.num_limits : int32_t(limits.size());
    c.limits = limits.empty() ? nullptr : limits.data();
    for (size_t i = 0; i < blocks.size(); ++i) {
      blocks[i].parent = parents[i].data();
    }
    c.num_joint_blocks = c.num_joint_blocks < 0 || c.num_joint_blocks > MMX_MAX_JOINT_BLOCKS ? c.num_joint_blocks : int32_t(blocks.size());
    c.joint_blocks = blocks.empty() ? nullptr : blocks.data();
    c.num_ellipsoid_limits = c.num_ellipsoid_limits < 0 || c.num_ellipsoid_limits > 256 ? c.num_ellipsoid_limits : int32_t(ellipsoids.size());
    c.ellipsoid_limits = ellipsoids.empty() ? nullptr : ellipsoids.data();
    return &c;
  }
};

const int32_t kLimitTypes[6] = {MMX_LIMIT_MINMAX, MMX_LIMIT_MINMAX_JOINT, MMX_LIMIT_MINMAX_JOINT_PASSIVE, MMX_LIMIT_LINEAR, MMX_LIMIT_LINEAR_JOINT, MMX_LIMIT_HALFPLANE};
mmx_parameter_limit validLimit(Rng& g, int32_t type) {
  mmx_parameter_limit lm{};
  lm.type = type;
  const bool joint = type == MMX_LIMIT_MINMAX_JOINT || type == MMX_LIMIT_LINEAR_JOINT || type == MMX_LIMIT_MINMAX_JOINT_PASSIVE;
  // joint rows 7 j + 3 / 7 j + 4 of joints 0..4: at most two parameters each, parameter 0 shared (a pair: at most three)
  lm.index0 = joint ? 7 * g.below(5) + 3 + g.below(2) : g.below(9);
  lm.index1 = joint ? 7 * g.below(5) + 3 + g.below(2) : g.below(9);
  lm.weight = 0.5f + float(g.below(4));
  lm.v[0] = -1.f, lm.v[1] = float(g.below(3)), lm.v[2] = 0.f, lm.v[3] = 1.f;
  return lm;
}
void addBlock(Request& r, Rng& g, int32_t type, int32_t count) {
  mmx_joint_constraint_block jb{};
  jb.type = type;
  jb.count = count;
  jb.local_point = jb.local_dir = jb.global = jb.plane_d = jb.weight = jb.projection = kPayload;
  jb.function_weight = 1.f + float(g.below(3));
  const bool l2Only = type == MMX_JC_PROJECTION || type == MMX_JC_DISTANCE || type == MMX_JC_JOINT_TO_JOINT_DISTANCE;
  const float alphas[6] = {2.f, 1.f, 0.f, MMX_LOSS_WELSCH, -2.f, 1.5f};
  jb.loss_alpha = l2Only ? 2.f : alphas[g.below(6)];
  jb.loss_c = l2Only ? float(g.below(2)) : float(g.below(3)) * 0.5f;
  jb.near_clip = 0.25f * float(g.below(8));
  if (g.coin()) { // what the type does not read may be anything
    const bool plane = type == MMX_JC_PLANE || type == MMX_JC_HALF_PLANE;
    const bool fixedAxis = type == MMX_JC_FIXED_AXIS_DIFF || type == MMX_JC_FIXED_AXIS_COS || type == MMX_JC_FIXED_AXIS_ANGLE;
    const bool pointOnly = type == MMX_JC_PROJECTION || type == MMX_JC_DISTANCE;
    if (fixedAxis) {
      jb.local_point = nullptr;
    }
    if (plane || pointOnly) {
      jb.local_dir = nullptr;
    }
    if (!plane && type != MMX_JC_DISTANCE && type != MMX_JC_JOINT_TO_JOINT_DISTANCE) {
      jb.plane_d = nullptr;
    }
    if (type == MMX_JC_JOINT_TO_JOINT_DISTANCE) {
      jb.global = nullptr;
    }
    if (type != MMX_JC_PROJECTION) {
      jb.projection = nullptr;
      jb.near_clip = g.coin() ? std::numeric_limits<float>::infinity() : std::nanf("");
    }
  }
  std::vector<int32_t> p(size_t(type == MMX_JC_JOINT_TO_JOINT_DISTANCE ? 2 * count : count));
  for (int32_t& j : p) {
    j = g.below(6);
  }
  r.blocks.push_back(jb);
  r.parents.push_back(std::move(p));
}
mmx_ellipsoid_limit validEllipsoid(Rng& g) {
  mmx_ellipsoid_limit e{};
  for (int i = 0; i < 12; ++i) {
    e.ellipsoid[i] = e.ellipsoid_inv[i] = float(g.below(5));
  }
  e.weight = 1.f;
  e.parent = g.below(6);
  e.ellipsoid_parent = g.below(6);
  return e;
}
Request validRequest(Rng& g) {
  Request r;
  r.c.pos_offset = r.c.pos_target = r.c.pos_weight = r.c.ori_offset = r.c.ori_target = r.c.ori_weight = kPayload;
  r.c.pos_function_weight = r.c.ori_function_weight = 1.f;
  r.c.memory = g.coin() ? MMX_MEM_HOST : MMX_MEM_DEVICE;
  if (g.coin()) {
    r.c.model_target = r.c.model_weights = kPayload;
  }
  const float alphas[7] = {2.f, 1.f, 0.f, MMX_LOSS_WELSCH, -2.f, 2.f + 1e-10f, 1.5f};
  r.c.pos_loss_alpha = alphas[g.below(7)], r.c.pos_loss_c = float(g.below(3)) - 0.5f;
  r.c.ori_loss_alpha = alphas[g.below(7)], r.c.ori_loss_c = float(g.below(3)) - 0.5f;
  for (int32_t l = g.below(5); l > 0; --l) {
    r.limits.push_back(validLimit(g, kLimitTypes[g.below(6)]));
  }
  for (int32_t b = g.below(4); b > 0; --b) {
    addBlock(r, g, g.below(MMX_JC_JOINT_TO_JOINT_DISTANCE + 1), g.below(4));
  }
  for (int32_t e = g.below(3); e > 0; --e) {
    r.ellipsoids.push_back(validEllipsoid(g));
  }
  if (g.coin()) {
    r.c.function_weights = kPayload;
  }
  r.c.num_function_weights = g.below(4 + MMX_MAX_JOINT_BLOCKS + 1);
  return r;
}

// One injector per refusal of the reference (its site number); site 0, the null request, is made by hand
constexpr int kNumSites = 21;
void inject(Request& r, Rng& g, int site) {
  auto someBlock = [&](int32_t type) -> size_t {
    if (r.blocks.size() >= size_t(MMX_MAX_JOINT_BLOCKS)) {
      r.blocks.pop_back(), r.parents.pop_back();
    }
    addBlock(r, g, type, 1 + g.below(3));
    return r.blocks.size() - 1;
  };
  switch (site) {
    case 1:
      (g.coin() ? r.c.pos_offset : g.coin() ? r.c.pos_target : r.c.pos_weight) = nullptr;
      break;
    case 2:
      (g.coin() ? r.c.ori_offset : g.coin() ? r.c.ori_target : r.c.ori_weight) = nullptr;
      break;
    case 3:
      r.c.memory = g.coin() ? 2 : -1;
      break;
    case 4:
      r.limits.clear();
      r.c.num_limits = g.coin() ? -1 : -7; // (a count > 0 with a null array cannot be kept apart from an empty list by data())
      break;
    case 5:
      r.c.model_target = kPayload, r.c.model_weights = nullptr;
      if (g.coin()) {
        std::swap(r.c.model_target, r.c.model_weights);
      }
      break;
    case 6: {
      mmx_parameter_limit lm = validLimit(g, MMX_LIMIT_MINMAX);
      lm.type = g.coin() ? 5 /* LimitType::Ellipsoid */ : g.coin() ? 7 : -1;
      r.limits.insert(r.limits.begin() + g.below(int32_t(r.limits.size()) + 1), lm);
      break;
    }
    case 7: {
      const int32_t rowTypes[5] = {MMX_LIMIT_MINMAX, MMX_LIMIT_MINMAX_JOINT, MMX_LIMIT_LINEAR, MMX_LIMIT_LINEAR_JOINT, MMX_LIMIT_HALFPLANE};
      mmx_parameter_limit lm = validLimit(g, rowTypes[g.below(5)]);
      const bool joint = lm.type == MMX_LIMIT_MINMAX_JOINT || lm.type == MMX_LIMIT_LINEAR_JOINT;
      const bool two = lm.type == MMX_LIMIT_LINEAR || lm.type == MMX_LIMIT_HALFPLANE || lm.type == MMX_LIMIT_LINEAR_JOINT;
      const int32_t bound = joint ? 42 : 9;
      (two && g.coin() ? lm.index1 : lm.index0) = g.coin() ? bound : g.coin() ? -1 : bound + 5;
      r.limits.insert(r.limits.begin() + g.below(int32_t(r.limits.size()) + 1), lm);
      break;
    }
    case 8: {
      mmx_parameter_limit lm = validLimit(g, g.coin() ? MMX_LIMIT_MINMAX_JOINT : MMX_LIMIT_LINEAR_JOINT);
      lm.index0 = 7 * 5 + 3; // five parameters
      if (lm.type == MMX_LIMIT_LINEAR_JOINT && g.coin()) {
        lm.index0 = 7 * 1 + 4, lm.index1 = 7 * 5 + 3;
      }
      r.limits.insert(r.limits.begin() + g.below(int32_t(r.limits.size()) + 1), lm);
      break;
    }
    case 9:
      r.c.num_function_weights = g.coin() ? -1 : 4 + MMX_MAX_JOINT_BLOCKS + 1;
      break;
    case 10:
      r.c.num_joint_blocks = g.coin() ? -1 : MMX_MAX_JOINT_BLOCKS + 1;
      break;
    case 11:
      r.blocks[someBlock(MMX_JC_PLANE)].type = g.coin() ? -1 : MMX_JC_JOINT_TO_JOINT_DISTANCE + 1;
      break;
    case 12: {
      const int32_t types[3] = {MMX_JC_PROJECTION, MMX_JC_DISTANCE, MMX_JC_JOINT_TO_JOINT_DISTANCE};
      mmx_joint_constraint_block& jb = r.blocks[someBlock(types[g.below(3)])];
      jb.loss_alpha = g.coin() ? 1.f : 2.f;
      jb.loss_c = jb.loss_alpha == 2.f ? 0.5f : 1.f;
      break;
    }
    case 13:
      r.blocks[someBlock(MMX_JC_PROJECTION)].near_clip = g.coin() ? std::numeric_limits<float>::infinity() : std::nanf("");
      break;
    case 14: {
      const int32_t type = g.below(MMX_JC_JOINT_TO_JOINT_DISTANCE + 1);
      mmx_joint_constraint_block& jb = r.blocks[someBlock(type)];
      switch (g.below(type == MMX_JC_JOINT_TO_JOINT_DISTANCE ? 2 : 3)) {
        case 0:
          jb.count = -1;
          break;
        case 1:
          jb.weight = nullptr;
          break;
        default:
          jb.global = nullptr;
      }
      break;
    }
    case 15: {
      const int32_t type = g.below(MMX_JC_JOINT_TO_JOINT_DISTANCE + 1);
      mmx_joint_constraint_block& jb = r.blocks[someBlock(type)];
      const bool plane = type == MMX_JC_PLANE || type == MMX_JC_HALF_PLANE;
      const bool fixedAxis = type == MMX_JC_FIXED_AXIS_DIFF || type == MMX_JC_FIXED_AXIS_COS || type == MMX_JC_FIXED_AXIS_ANGLE;
      const bool pointOnly = type == MMX_JC_PROJECTION || type == MMX_JC_DISTANCE;
      if (plane || type == MMX_JC_DISTANCE || (type == MMX_JC_JOINT_TO_JOINT_DISTANCE && g.coin())) {
        jb.plane_d = nullptr;
      } else if (fixedAxis || (!pointOnly && g.coin())) {
        jb.local_dir = nullptr;
      } else {
        jb.local_point = nullptr;
      }
      break;
    }
    case 16:
      r.blocks[someBlock(MMX_JC_PROJECTION)].projection = nullptr;
      break;
    case 17: {
      const size_t b = someBlock(g.coin() ? MMX_JC_JOINT_TO_JOINT_DISTANCE : g.below(MMX_JC_JOINT_TO_JOINT_DISTANCE));
      std::vector<int32_t>& p = r.parents[b];
      p[size_t(g.below(int32_t(p.size())))] = g.coin() ? 6 : -1; // (a pair block: in either half)
      break;
    }
    case 18:
      while (r.blocks.size() > 6) {
        r.blocks.pop_back(), r.parents.pop_back();
      }
      addBlock(r, g, MMX_JC_NORMAL, 1000);
      addBlock(r, g, MMX_JC_JOINT_TO_JOINT_DISTANCE, 25);
      break;
    case 19:
      if (g.coin()) {
        r.c.num_ellipsoid_limits = -1;
      } else {
        r.ellipsoids.assign(257, validEllipsoid(g));
      }
      break;
    case 20: {
      mmx_ellipsoid_limit e = validEllipsoid(g);
      (g.coin() ? e.parent : e.ellipsoid_parent) = g.coin() ? 6 : -1;
      r.ellipsoids.insert(r.ellipsoids.begin() + g.below(int32_t(r.ellipsoids.size()) + 1), e);
      break;
    }
    default:
      break;
  }
}

// ---- the comparison ----------------------------------------------------------------------------------------------------------
bool sameLoss(const LossRef& a, const mmx::LossHost& b) {
  return a.type == b.type && std::memcmp(&a.alpha, &b.alpha, 4) == 0 && std::memcmp(&a.invC2, &b.invC2, 4) == 0 && std::memcmp(&a.c, &b.c, 4) == 0;
}
long seen[3][2] = {}; // blocksChanged / ellipsoidsChanged / structureChanged, false / true
long accepted = 0, refused = 0;

struct Pair { // the same problem kept the old way and the new way
  Handle ref;
  NewHandle now;
  Pair(const Rig& rig, int32_t Kp, int32_t Ko) {
    ref.J = rig.J, ref.P = rig.P, ref.Kp = now.Kp = Kp, ref.Ko = now.Ko = Ko, ref.U = Kp + 3 * Ko;
  }
  void setDirty(bool dirty) { // a failed table upload leaves the flag set
    ref.tablesDirty = now.tablesDirty = dirty;
  }
};

Outcome step(Pair& h, const mmx_rig_desc& rig, const mmx_constraint_data* c) {
  const Outcome want = referenceSetConstraints(&h.ref, rig, c);
  const mmx::ConstraintIntake got = newSetConstraints(&h.now, rig, c);
  CHECK(got.code == want.code);
  CHECK(got.message == want.message);
  if (want.code != MMX_OK) {
    ++refused;
    return want;
  }
  ++accepted;
  const Handle& r = h.ref;
  CHECK(got.limits.size() == r.limits.size());
  CHECK(got.limits.empty() || std::memcmp(got.limits.data(), r.limits.data(), got.limits.size() * sizeof(mmx_parameter_limit)) == 0);
  CHECK(got.blockRows.size() == r.blockDev.size() && got.blocks.size() == r.blockDev.size());
  for (size_t i = 0; i < r.blockDev.size(); ++i) {
    CHECK(got.blockRows[i].first == r.blockDev[i].first && got.blockRows[i].rowStart == r.blockDev[i].rowStart);
    CHECK(sameLoss(r.blockDev[i].loss, got.blockRows[i].loss));
    CHECK(std::memcmp(&got.blockRows[i].nearClip, &r.blockDev[i].nearClip, 4) == 0);
  }
  CHECK(got.genRows == r.genRows && got.M == r.M && got.rowsJoint == r.rowsJoint && got.fnCols == r.fnCols);
  CHECK(sameLoss(r.lossPos, got.lossPos) && sameLoss(r.lossOri, got.lossOri));
  CHECK(got.hasModel == (r.hasModel != 0));
  CHECK(got.blocksChanged == want.blocksChanged && got.ellipsoidsChanged == want.ellipsoidsChanged && got.structureChanged == want.structureChanged);
  // ... and what the two handles hold afterwards
  CHECK(h.now.blocks.size() == r.blocks.size());
  for (size_t i = 0; i < r.blocks.size(); ++i) {
    CHECK(h.now.blocks[i].type == r.blocks[i]->type && h.now.blocks[i].parent == r.blocks[i]->parent && h.now.blocks[i].parentB == r.blocks[i]->parentB);
    CHECK(int32_t(r.blocks[i]->parent.size()) == c->joint_blocks[i].count); // the handle's topology is the request's, changed or not
  }
  CHECK(h.now.limits.size() == r.limits.size() && h.now.ellipsoids.size() == r.ellipsoids.size());
  CHECK(h.now.tablesDirty == r.tablesDirty && h.now.hasModel == (r.hasModel != 0));
  ++seen[0][want.blocksChanged], ++seen[1][want.ellipsoidsChanged], ++seen[2][want.structureChanged];
  return want;
}

void testRowsPerType() { // the "rows" column of the table in include/mmx.h
  const int32_t rows[11] = {/* PLANE */ 1, /* HALF_PLANE */ 1, /* AIM_DIST */ 3, /* AIM_DIR */ 3, /* FIXED_AXIS_DIFF */ 3, /* FIXED_AXIS_COS */ 1,
                            /* FIXED_AXIS_ANGLE */ 1, /* NORMAL */ 1, /* PROJECTION */ 2, /* DISTANCE */ 1, /* JOINT_TO_JOINT_DISTANCE */ 1};
  static_assert(MMX_JC_PLANE == 0 && MMX_JC_JOINT_TO_JOINT_DISTANCE == 10, "the table covers every type");
  static_assert(mmx::jointBlockRows(MMX_JC_PROJECTION) == 2, "constexpr");
  for (int32_t t = 0; t <= 10; ++t) {
    CHECK(mmx::jointBlockRows(t) == rows[t]);
  }
}

void testRefusals(const Rig& rig) {
  const mmx_rig_desc d = rig.desc();
  Rng g;
  Pair h(rig, 2, 1);
  CHECK(step(h, d, nullptr).site == 0);
  for (int round = 0; round < 40; ++round) {
    for (int a = 1; a < kNumSites; ++a) {
      for (int b = a; b < kNumSites; ++b) { // b == a: the defect alone; else a pair, injected in either order
        Request r = validRequest(g);
        step(h, d, r.data()); // (accepted: the previous state varies along the way)
        const bool swap = g.coin();
        inject(r, g, swap ? b : a);
        if (b != a) {
          inject(r, g, swap ? a : b);
        }
        const Outcome o = step(h, d, r.data());
        CHECK(o.code != MMX_OK);
        CHECK(b == a ? o.site == a : (o.site >= 1 && o.site < kNumSites));
        // a refused request leaves the handle as it was: the same valid request is no structure change afterwards
        Request again = validRequest(g);
        step(h, d, again.data());
        Request bad(again);
        inject(bad, g, a);
        CHECK(step(h, d, bad.data()).code != MMX_OK);
        const Outcome same = step(h, d, again.data());
        CHECK(same.code == MMX_OK && !same.structureChanged);
      }
    }
  }
  for (int s = 0; s < kNumSites; ++s) {
    if (reached[s] == 0) {
      std::printf("refusal %d never reached\n", s);
      std::exit(1);
    }
  }
  // the position / orientation arrays may be null exactly when the problem has no such constraint
  Pair none(rig, 0, 0), posOnly(rig, 2, 0), oriOnly(rig, 0, 1);
  Request r = validRequest(g);
  r.c.pos_offset = r.c.ori_weight = nullptr;
  CHECK(step(none, d, r.data()).code == MMX_OK);
  CHECK(step(posOnly, d, r.data()).site == 1 && step(oriOnly, d, r.data()).site == 2);
  r.c.pos_offset = kPayload;
  CHECK(step(posOnly, d, r.data()).code == MMX_OK && step(oriOnly, d, r.data()).site == 2);
  r.c.pos_offset = nullptr, r.c.ori_weight = kPayload;
  CHECK(step(posOnly, d, r.data()).site == 1 && step(oriOnly, d, r.data()).code == MMX_OK);
}

void testEdges(const Rig& rig) {
  const mmx_rig_desc d = rig.desc();
  Rng g;
  g.s = 77;
  Pair h(rig, 3, 2);
  // every limit type on its own, the passive one included: it is dropped and is no structure change
  for (int32_t type : kLimitTypes) {
    Request r = validRequest(g);
    r.limits.assign(1, validLimit(g, type));
    CHECK(step(h, d, r.data()).code == MMX_OK);
    CHECK(h.ref.limits.size() == (type == MMX_LIMIT_MINMAX_JOINT_PASSIVE ? 0u : 1u));
    Request p(r);
    p.limits.insert(p.limits.begin() + g.below(2), validLimit(g, MMX_LIMIT_MINMAX_JOINT_PASSIVE));
    CHECK(!step(h, d, p.data()).structureChanged);
    p.limits.push_back(validLimit(g, MMX_LIMIT_MINMAX));
    CHECK(step(h, d, p.data()).structureChanged);
    p.limits.back().weight += 1.f; // a limit's values are structure: the limit tables are built from them
    const Outcome o = step(h, d, p.data());
    CHECK(o.structureChanged && !o.blocksChanged && !o.ellipsoidsChanged);
  }
  // every block type with count 0 and > 0; payload, weight and loss are no structure
  for (int32_t type = MMX_JC_PLANE; type <= MMX_JC_JOINT_TO_JOINT_DISTANCE; ++type) {
    for (int32_t count : {0, 3}) {
      Request r = validRequest(g);
      r.blocks.clear(), r.parents.clear();
      addBlock(r, g, MMX_JC_NORMAL, 2);
      addBlock(r, g, type, count);
      addBlock(r, g, MMX_JC_AIM_DIR, 1);
      step(h, d, r.data());
      CHECK(h.ref.blockDev[2].first == 2 + count && h.ref.blockDev[2].rowStart == 3 * h.ref.U + 2 + mmx::jointBlockRows(type) * count);
      Request q(r);
      q.blocks[0].function_weight += 1.f, q.blocks[0].loss_alpha = 0.f, q.blocks[0].loss_c = 2.f, q.blocks[1].near_clip += 1.f;
      q.c.pos_function_weight = 3.f, q.c.memory = MMX_MEM_HOST + MMX_MEM_DEVICE - q.c.memory;
      const Outcome o = step(h, d, q.data());
      CHECK(!o.blocksChanged && !o.structureChanged);
      if (count > 0) { // one joint changed; a pair block: among the second joints alone
        q.parents[1].back() = (q.parents[1].back() + 1) % 6;
        const Outcome o2 = step(h, d, q.data());
        CHECK(o2.blocksChanged && o2.structureChanged && !o2.ellipsoidsChanged);
        CHECK(type != MMX_JC_JOINT_TO_JOINT_DISTANCE || h.ref.blocks[1]->parent == std::vector<int32_t>(r.parents[1].begin(), r.parents[1].begin() + count));
      }
      q.blocks[1].type = type == MMX_JC_PLANE ? MMX_JC_HALF_PLANE : MMX_JC_PLANE; // same count and joints, another function
      q.blocks[1].loss_c = 0.f;
      q.blocks[1].local_point = q.blocks[1].global = q.blocks[1].plane_d = kPayload;
      if (type != MMX_JC_JOINT_TO_JOINT_DISTANCE) {
        CHECK(step(h, d, q.data()).blocksChanged);
      }
    }
  }
  // exactly 1024 constraints, then 1025
  {
    Request r = validRequest(g);
    r.blocks.clear(), r.parents.clear();
    addBlock(r, g, MMX_JC_AIM_DIST, 1000);
    addBlock(r, g, MMX_JC_JOINT_TO_JOINT_DISTANCE, 24);
    CHECK(step(h, d, r.data()).code == MMX_OK);
    CHECK(h.ref.genRows == 3024);
    addBlock(r, g, MMX_JC_PLANE, 1);
    const Outcome o = step(h, d, r.data());
    CHECK(o.code == MMX_ERR_UNSUPPORTED && o.site == 18);
  }
  // ellipsoid counts 0, 256, 257; one value of one entry changed
  {
    Request r = validRequest(g);
    r.ellipsoids.clear();
    step(h, d, r.data());
    CHECK(!step(h, d, r.data()).ellipsoidsChanged);
    for (int i = 0; i < 256; ++i) {
      r.ellipsoids.push_back(validEllipsoid(g));
    }
    Outcome o = step(h, d, r.data());
    CHECK(o.code == MMX_OK && o.ellipsoidsChanged && o.structureChanged && !o.blocksChanged);
    CHECK(!step(h, d, r.data()).ellipsoidsChanged);
    r.ellipsoids[255].offset[2] += 1.f;
    CHECK(step(h, d, r.data()).ellipsoidsChanged);
    r.ellipsoids[255].parent = (r.ellipsoids[255].parent + 1) % 6; // the last word of the last entry
    CHECK(step(h, d, r.data()).ellipsoidsChanged);
    CHECK(!step(h, d, r.data()).ellipsoidsChanged);
    r.ellipsoids.push_back(validEllipsoid(g));
    o = step(h, d, r.data());
    CHECK(o.code == MMX_ERR_INVALID_ARGUMENT && o.site == 19);
  }
  // the model block alone; a dirty handle rebuilds whatever the request
  {
    Request r = validRequest(g);
    step(h, d, r.data());
    r.c.model_target = r.c.model_weights = r.c.model_target == nullptr ? kPayload : nullptr;
    const Outcome o = step(h, d, r.data());
    CHECK(o.structureChanged && !o.blocksChanged && !o.ellipsoidsChanged);
    CHECK(!step(h, d, r.data()).structureChanged);
    h.setDirty(true);
    const Outcome o2 = step(h, d, r.data());
    CHECK(o2.structureChanged && !o2.blocksChanged && !o2.ellipsoidsChanged && !h.ref.tablesDirty);
  }
}

// A walk: every request is the one before it with a few components edited, so that all three flags go both ways
void testWalk(const Rig& rig) {
  const mmx_rig_desc d = rig.desc();
  Rng g;
  g.s = 4242;
  Pair h(rig, 1, 1);
  std::unique_ptr<Request> r = std::make_unique<Request>(validRequest(g));
  for (int it = 0; it < 6000; ++it) {
    switch (g.below(12)) {
      case 0:
        r = std::make_unique<Request>(validRequest(g));
        break;
      case 1:
        if (!r->limits.empty()) {
          r->limits[size_t(g.below(int32_t(r->limits.size())))] = validLimit(g, kLimitTypes[g.below(6)]);
        }
        break;
      case 2:
        r->limits.push_back(validLimit(g, kLimitTypes[g.below(6)]));
        break;
      case 3:
        if (!r->limits.empty()) {
          r->limits.erase(r->limits.begin() + g.below(int32_t(r->limits.size())));
        }
        break;
      case 4:
        if (!r->blocks.empty()) {
          std::vector<int32_t>& p = r->parents[size_t(g.below(int32_t(r->blocks.size())))];
          if (!p.empty()) {
            p[size_t(g.below(int32_t(p.size())))] = g.below(6);
          }
        }
        break;
      case 5:
        if (r->blocks.size() < size_t(MMX_MAX_JOINT_BLOCKS)) {
          addBlock(*r, g, g.below(MMX_JC_JOINT_TO_JOINT_DISTANCE + 1), g.below(4));
        }
        break;
      case 6:
        if (!r->blocks.empty()) {
          r->blocks.pop_back(), r->parents.pop_back();
        }
        break;
      case 7:
        if (!r->ellipsoids.empty()) {
          r->ellipsoids[size_t(g.below(int32_t(r->ellipsoids.size())))] = validEllipsoid(g);
        } else {
          r->ellipsoids.push_back(validEllipsoid(g));
        }
        break;
      case 8:
        r->c.model_target = r->c.model_weights = g.coin() ? kPayload : nullptr;
        break;
      case 9:
        h.setDirty(g.below(4) == 0);
        break;
      default: // payload and weights only
        r->c.limit_function_weight += 1.f;
        r->c.memory = g.coin() ? MMX_MEM_HOST : MMX_MEM_DEVICE;
        break;
    }
    CHECK(step(h, d, r->data()).code == MMX_OK);
  }
  for (int f = 0; f < 3; ++f) {
    CHECK(seen[f][0] > 100 && seen[f][1] > 100);
  }
}

void testInstanceParents(const Rig& rig) {
  Rng g;
  g.s = 99;
  Pair h(rig, 2, 1);
  const int32_t B = 3;
  long sawUnchanged = 0, sawSame[2] = {}, sawRefusal[2] = {};
  std::vector<int32_t> pos, ori;
  for (int it = 0; it < 20000; ++it) {
    const int32_t memory = g.below(3) == 0 ? MMX_MEM_DEVICE : MMX_MEM_HOST;
    const int32_t span = 1 + g.below(3); // few joints: equal unions from different lists are common
    if (g.below(3) != 0) { // else: the lists of the call before, again
      pos.assign(g.below(5) == 0 ? 0u : size_t(B * h.ref.Kp), 0);
      ori.assign(g.below(5) == 0 ? 0u : size_t(B * h.ref.Ko), 0);
      for (int32_t& j : pos) {
        j = g.below(span);
      }
      for (int32_t& j : ori) {
        j = 3 + g.below(span);
      }
    }
    std::vector<int32_t> p = pos, o = ori;
    const int defect = g.below(12); // 0: position list, 1: orientation list, 2: both (the position list's refusal comes first)
    if ((defect == 0 || defect == 2) && !p.empty()) {
      p[size_t(g.below(int32_t(p.size())))] = g.coin() ? 6 : -1;
    }
    if ((defect == 1 || defect == 2) && !o.empty()) {
      o[size_t(g.below(int32_t(o.size())))] = g.coin() ? 6 : -2;
    }
    if (g.below(16) == 0) {
      h.setDirty(true);
    }
    const ParentsOutcome want = referenceSetInstanceParents(&h.ref, p, o, memory);
    NewHandle& n = h.now;
    mmx::InstanceParentsIntake got = mmx::intakeInstanceParents(
        rig.J, p, o, memory == MMX_MEM_HOST, {n.instPos, n.instOri, n.unionPos, n.unionOri, n.instParentsFromHost, n.instPosHost, n.instOriHost, n.tablesDirty});
    CHECK(got.code == want.code);
    if (want.code != MMX_OK) {
      CHECK(want.message == got.message);
      ++sawRefusal[want.message.find("orientation") != std::string::npos];
      continue;
    }
    CHECK(got.message == nullptr && got.unchanged == want.unchanged);
    if (want.unchanged) {
      ++sawUnchanged;
      continue;
    }
    CHECK(got.sameTables == want.sameTables);
    ++sawSame[want.sameTables];
    n.instPos = !p.empty(), n.instOri = !o.empty(), n.instParentsFromHost = memory == MMX_MEM_HOST; // as the setter writes them
    n.instPosHost = p, n.instOriHost = o;
    if (!got.sameTables) {
      n.unionPos = got.unionPos, n.unionOri = got.unionOri, n.tablesDirty = false;
    }
    CHECK(n.unionPos == h.ref.unionPos && n.unionOri == h.ref.unionOri && n.tablesDirty == h.ref.tablesDirty);
  }
  CHECK(sawUnchanged > 100 && sawSame[0] > 100 && sawSame[1] > 100 && sawRefusal[0] > 100 && sawRefusal[1] > 100);
}

void testJointsInRange() {
  const int32_t a[4] = {0, 5, 3, 5};
  CHECK(mmx::jointsInRange(a, 4, 6) && !mmx::jointsInRange(a, 4, 5) && mmx::jointsInRange(a, 1, 1) && mmx::jointsInRange(nullptr, 0, 6));
  const int32_t b[2] = {2, -1};
  CHECK(!mmx::jointsInRange(b, 2, 6) && mmx::jointsInRange(b, 1, 6));
}

} // namespace

int main() {
  const Rig rig;
  testRowsPerType();
  testJointsInRange();
  testRefusals(rig);
  testEdges(rig);
  testWalk(rig);
  testInstanceParents(rig);
  std::printf("%ld accepted and %ld refused requests\nOK\n", accepted, refused);
  return 0;
}
