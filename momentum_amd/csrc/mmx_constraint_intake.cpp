// mmx_constraint_intake.cpp -- see mmx_constraint_intake.hpp.  The checks fire in the order of this file: a request with
// several defects gets the first refusal listed here.
#include "mmx_constraint_intake.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mmx {

bool jointsInRange(const int32_t* joints, size_t count, int32_t numJoints) {
  return std::all_of(joints, joints + count, [numJoints](int32_t j) { return j >= 0 && j < numJoints; });
}

LossHost classifyLoss(float alpha, float c) {
  LossHost l{0, 2.f, 1.f, 1.f};
  if (c > 0.f) {
    l.alpha = alpha;
    l.invC2 = 1.f / (c * c);
    l.c = c;
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
}

namespace {

ConstraintIntake refuse(int32_t code, const std::string& message) {
  ConstraintIntake r;
  r.code = code;
  r.message = message;
  return r;
}

// null when the limit is accepted (the passive type is: it is dropped later)
const char* limitRefusal(const mmx_rig_desc& rig, const mmx_parameter_limit& lm, int32_t& code) {
  const bool model = lm.type == MMX_LIMIT_MINMAX || lm.type == MMX_LIMIT_LINEAR || lm.type == MMX_LIMIT_HALFPLANE;
  const bool joint = lm.type == MMX_LIMIT_MINMAX_JOINT || lm.type == MMX_LIMIT_LINEAR_JOINT;
  const bool two = lm.type == MMX_LIMIT_LINEAR || lm.type == MMX_LIMIT_HALFPLANE || lm.type == MMX_LIMIT_LINEAR_JOINT;
  if (lm.type == MMX_LIMIT_MINMAX_JOINT_PASSIVE) {
    return nullptr; // LimitErrorFunctionT skips the passive type: no error, no row (limit_error_function.cpp:836-837,1051-1052)
  }
  if (!model && !joint) {
    code = MMX_ERR_UNSUPPORTED;
    return ": MinMax, MinMaxJoint, MinMaxJointPassive (ignored like in the reference), Linear, LinearJoint and HalfPlane go here; "
           "Ellipsoid limits travel in mmx_constraint_data::ellipsoid_limits";
  }
  const int32_t bound = joint ? MMX_PARAMS_PER_JOINT * rig.num_joints : rig.num_params;
  if (lm.index0 < 0 || lm.index0 >= bound || (two && (lm.index1 < 0 || lm.index1 >= bound))) {
    code = MMX_ERR_INVALID_ARGUMENT;
    return ": parameter index out of range"; // MT_CHECK :574-575,:611-612
  }
  if (limitParameters(&rig, lm).size() > 4) {
    code = MMX_ERR_UNSUPPORTED;
    return ": more than four model parameters drive the limited joint parameters";
  }
  return nullptr;
}

// null when the block is accepted.  Payload pointers are only tested against null.
const char* blockRefusal(const mmx_joint_constraint_block& jb, int32_t numJoints, int32_t& code) {
  code = MMX_ERR_INVALID_ARGUMENT;
  if (jb.type < MMX_JC_PLANE || jb.type > MMX_JC_JOINT_TO_JOINT_DISTANCE) {
    code = MMX_ERR_UNSUPPORTED;
    return ": unknown error-function type";
  }
  const bool pointOnly = jb.type == MMX_JC_PROJECTION || jb.type == MMX_JC_DISTANCE; // (ABI 12)
  const bool pairType = jb.type == MMX_JC_JOINT_TO_JOINT_DISTANCE; // two points: parent is [2 * count], local_dir the second offset
  if ((pointOnly || pairType) && jb.loss_c > 0.f && !(jb.loss_alpha == 2.f && jb.loss_c == 1.f)) {
    code = MMX_ERR_UNSUPPORTED;
    return ": projection / distance / joint-to-joint distance blocks take the L2 loss only (loss_c <= 0 or (alpha, c) = (2, 1))";
  }
  if (jb.type == MMX_JC_PROJECTION && !std::isfinite(jb.near_clip)) {
    return ": near_clip is not finite";
  }
  if (jb.count < 0 || (jb.count > 0 && (jb.parent == nullptr || (!pairType && jb.global == nullptr) || jb.weight == nullptr))) {
    return ": negative count or null parent / global / weight array";
  }
  const bool plane = jb.type == MMX_JC_PLANE || jb.type == MMX_JC_HALF_PLANE;
  const bool fixedAxis = jb.type == MMX_JC_FIXED_AXIS_DIFF || jb.type == MMX_JC_FIXED_AXIS_COS || jb.type == MMX_JC_FIXED_AXIS_ANGLE;
  const bool needD = plane || jb.type == MMX_JC_DISTANCE || pairType;
  if (jb.count > 0 && ((!fixedAxis && jb.local_point == nullptr) || (!plane && !pointOnly && jb.local_dir == nullptr) || (needD && jb.plane_d == nullptr))) {
    return ": a payload array its error function needs is null";
  }
  if (jb.count > 0 && jb.type == MMX_JC_PROJECTION && jb.projection == nullptr) {
    return ": projection block without its projection matrices";
  }
  if (!jointsInRange(jb.parent, size_t(pairType ? 2 * jb.count : jb.count), numJoints)) {
    return ": parent joint out of range";
  }
  return nullptr;
}

} // namespace

ConstraintIntake intakeConstraints(const mmx_rig_desc& rig, int32_t Kp, int32_t Ko, const mmx_constraint_data* c, const ConstraintState& prev) {
  const int32_t J = rig.num_joints, P = rig.num_params, U = Kp + 3 * Ko;
  if (c == nullptr) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "constraint data is null");
  }
  if (Kp > 0 && (!c->pos_offset || !c->pos_target || !c->pos_weight)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "position constraint arrays are null");
  }
  if (Ko > 0 && (!c->ori_offset || !c->ori_target || !c->ori_weight)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "orientation constraint arrays are null");
  }
  if (c->memory != MMX_MEM_DEVICE && c->memory != MMX_MEM_HOST) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "constraint data: unknown memory space");
  }
  // ---- optional parameter-space blocks
  if (c->num_limits < 0 || (c->num_limits > 0 && c->limits == nullptr)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "limits: negative count or null array");
  }
  if ((c->model_target == nullptr) != (c->model_weights == nullptr)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "model_target and model_weights must be given together");
  }
  for (int32_t l = 0; l < c->num_limits; ++l) {
    int32_t code = MMX_OK;
    if (const char* why = limitRefusal(rig, c->limits[l], code)) {
      return refuse(code, "limit " + std::to_string(l) + why);
    }
  }
  if (c->num_function_weights < 0 || c->num_function_weights > 4 + MMX_MAX_JOINT_BLOCKS) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "num_function_weights out of range (columns: position, orientation, limits, model parameters, joint blocks)");
  }
  // ---- further joint-constraint blocks
  if (c->num_joint_blocks < 0 || c->num_joint_blocks > MMX_MAX_JOINT_BLOCKS || (c->num_joint_blocks > 0 && c->joint_blocks == nullptr)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "joint_blocks: count out of range or null array");
  }
  ConstraintIntake r;
  int32_t genCount = 0;
  for (int32_t i = 0; i < c->num_joint_blocks; ++i) {
    const mmx_joint_constraint_block& jb = c->joint_blocks[i];
    int32_t code = MMX_OK;
    if (const char* why = blockRefusal(jb, J, code)) {
      return refuse(code, "joint block " + std::to_string(i) + why);
    }
    ProblemTopology::Block b;
    b.type = jb.type;
    b.parent.assign(jb.parent, jb.parent + jb.count);
    if (jb.type == MMX_JC_JOINT_TO_JOINT_DISTANCE) { // the second joint of every constraint
      b.parentB.assign(jb.parent + jb.count, jb.parent + 2 * jb.count);
    }
    r.blocks.push_back(std::move(b));
    r.blockRows.push_back({genCount, 3 * U + r.genRows, classifyLoss(jb.loss_alpha, jb.loss_c), jb.type == MMX_JC_PROJECTION ? jb.near_clip : 0.f});
    r.genRows += jointBlockRows(jb.type) * jb.count;
    genCount += jb.count;
  }
  if (genCount > 1024) {
    return refuse(MMX_ERR_UNSUPPORTED, "more than 1024 constraints in the further joint-constraint blocks");
  }
  // ---- Ellipsoid entries of the limit block
  if (c->num_ellipsoid_limits < 0 || c->num_ellipsoid_limits > 256 || (c->num_ellipsoid_limits > 0 && c->ellipsoid_limits == nullptr)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "ellipsoid_limits: count out of range or null array");
  }
  for (int32_t i = 0; i < c->num_ellipsoid_limits; ++i) {
    const int32_t joints[2] = {c->ellipsoid_limits[i].parent, c->ellipsoid_limits[i].ellipsoid_parent};
    if (!jointsInRange(joints, 2, J)) {
      return refuse(MMX_ERR_INVALID_ARGUMENT, "ellipsoid limit " + std::to_string(i) + ": joint index out of range");
    }
  }
  // ---- accepted: the derived integers
  for (int32_t l = 0; l < c->num_limits; ++l) {
    if (c->limits[l].type != MMX_LIMIT_MINMAX_JOINT_PASSIVE) {
      r.limits.push_back(c->limits[l]);
    }
  }
  r.hasModel = c->model_target != nullptr;
  r.rowsJoint = 3 * U + r.genRows + 3 * c->num_ellipsoid_limits;
  r.M = r.rowsJoint + int32_t(r.limits.size()) + (r.hasModel ? P : 0);
  r.lossPos = classifyLoss(c->pos_loss_alpha, c->pos_loss_c);
  r.lossOri = classifyLoss(c->ori_loss_alpha, c->ori_loss_c);
  r.fnCols = c->function_weights != nullptr && c->num_function_weights > 0 ? c->num_function_weights : 0;
  // ---- what changed against the last accepted call.  Payload, weights and losses are no structure: the tables do not see them
  const auto sameBlock = [](const ProblemTopology::Block& a, const ProblemTopology::Block& b) {
    return a.type == b.type && a.parent == b.parent && a.parentB == b.parentB;
  };
  r.blocksChanged = r.blocks.size() != prev.blocks.size() || !std::equal(r.blocks.begin(), r.blocks.end(), prev.blocks.begin(), sameBlock);
  const size_t NE = size_t(c->num_ellipsoid_limits);
  r.ellipsoidsChanged = NE != prev.ellipsoids.size() || (NE > 0 && std::memcmp(c->ellipsoid_limits, prev.ellipsoids.data(), NE * sizeof(mmx_ellipsoid_limit)) != 0);
  const bool limitsChanged = r.limits.size() != prev.limits.size() ||
      (!r.limits.empty() && std::memcmp(r.limits.data(), prev.limits.data(), r.limits.size() * sizeof(mmx_parameter_limit)) != 0);
  r.structureChanged = prev.tablesDirty || r.blocksChanged || r.ellipsoidsChanged || r.hasModel != prev.hasModel || limitsChanged;
  return r;
}

InstanceParentsIntake intakeInstanceParents(
    int32_t numJoints, const std::vector<int32_t>& pos, const std::vector<int32_t>& ori, bool fromHost, const InstanceParentsState& prev) {
  InstanceParentsIntake r;
  r.code = MMX_ERR_INVALID_ARGUMENT;
  if (!jointsInRange(pos.data(), pos.size(), numJoints)) {
    r.message = "instance parents: position constraint parent joint out of range";
    return r;
  }
  if (!jointsInRange(ori.data(), ori.size(), numJoints)) {
    r.message = "instance parents: orientation constraint parent joint out of range";
    return r;
  }
  r.code = MMX_OK;
  // unchanged lists (the C++ shell re-sends them with every constraint update)
  r.unchanged = fromHost && !prev.tablesDirty && prev.listsFromHost && pos == prev.posLists && ori == prev.oriLists;
  const auto jointsOf = [numJoints](const std::vector<int32_t>& lists) {
    std::vector<uint8_t> seen(size_t(numJoints), 0);
    for (int32_t j : lists) {
      seen[size_t(j)] = 1;
    }
    std::vector<int32_t> joints;
    for (int32_t j = 0; j < numJoints; ++j) {
      if (seen[size_t(j)]) {
        joints.push_back(j);
      }
    }
    return joints;
  };
  r.unionPos = jointsOf(pos);
  r.unionOri = jointsOf(ori);
  r.sameTables = !prev.tablesDirty && pos.empty() != prev.instPos && ori.empty() != prev.instOri && r.unionPos == prev.unionPos && r.unionOri == prev.unionOri;
  return r;
}

} // namespace mmx
