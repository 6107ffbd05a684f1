// mmx_constraint_intake.hpp -- what a constraint update does to a problem, decided before anything is touched (no HIP here, no
// handle: pure functions of the caller's host arrays and of what the last accepted call left, unit-tested on the CPU against a
// transcription of the code they replaced: tests/cpp/test_constraint_intake.cpp).  mmx_problem_set_constraints and
// mmx_problem_set_instance_parents (mmx_capi.hip) ask for the intake record and either fail with its refusal or stage the
// payload and write the record into the handle: every check, every derived integer and the comparison with the previous state
// -- which decides whether the derived tables are rebuilt; a wrong "unchanged" solves with stale tables, silently -- are here.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmx.h"
#include "mmx_host_tables.hpp"

namespace mmx {
#pragma GCC visibility push(hidden)

// Jacobian rows per constraint of a joint-constraint block (FuncDim, the "rows" column of the table in include/mmx.h)
constexpr int32_t jointBlockRows(int32_t type) {
  return (type == MMX_JC_AIM_DIST || type == MMX_JC_AIM_DIR || type == MMX_JC_FIXED_AXIS_DIFF) ? 3 : type == MMX_JC_PROJECTION ? 2 : 1;
}

// Every entry names a joint of the rig (MT_CHECK(jntIndex < skeleton_.joints.size()), joint_error_function-inl.h:230)
bool jointsInRange(const int32_t* joints, size_t count, int32_t numJoints);

// mmx::LossDev (mmx_device.hpp) as the host sees it; mmx_capi.hip asserts that the layouts match
struct LossHost {
  int32_t type; // 0 L2, 1 L1 / pseudo-Huber, 2 Cauchy, 3 Welsch, 4 Barron's general form
  float alpha, invC2, c;
};
// GeneralizedLossT's constructor (generalized_loss.cpp:81-101); c <= 0: the default L2 loss with c = 1
LossHost classifyLoss(float alpha, float c);

// What the last accepted mmx_problem_set_constraints call left in the handle (views: nothing is copied)
struct ConstraintState {
  const std::vector<ProblemTopology::Block>& blocks;
  const std::vector<mmx_ellipsoid_limit>& ellipsoids;
  const std::vector<mmx_parameter_limit>& limits; // the kept ones
  bool hasModel;
  bool tablesDirty; // a table upload has failed since: the derived tables are not to be trusted
};

// The refusal (code and message) or everything the setter writes into the handle, no decision left to take
struct ConstraintIntake {
  int32_t code = MMX_OK;
  std::string message;
  std::vector<mmx_parameter_limit> limits; // the limits that produce a row (the passive type does not)
  std::vector<ProblemTopology::Block> blocks;
  struct BlockRows {
    int32_t first = 0; // index of the block's first constraint in the flattened list
    int32_t rowStart = 0; // first row of the block in J / r
    LossHost loss{};
    float nearClip = 0.f; // MMX_JC_PROJECTION, else 0
  };
  std::vector<BlockRows> blockRows; // [num_joint_blocks]
  int32_t genRows = 0; // rows of the further joint-constraint blocks
  int32_t M = 0, rowsJoint = 0; // all rows ; the rows ahead of the parameter-space rows
  LossHost lossPos{}, lossOri{};
  int32_t fnCols = 0; // columns of function_weights read (0: none given)
  bool hasModel = false;
  bool blocksChanged = false; // type, count or a joint of some block differs: the handle's block list is replaced
  bool ellipsoidsChanged = false;
  bool structureChanged = false; // ... or limits / model block differ, or the tables were dirty: uploadProblemTables runs
};

// The rig's counts come from the descriptor, Kp / Ko from the problem.  Reads the HOST arrays of `c` only (limits,
// joint_blocks[i].parent, ellipsoid_limits) and its scalars; payload pointers are tested against null, never followed.
ConstraintIntake intakeConstraints(const mmx_rig_desc& rig, int32_t Kp, int32_t Ko, const mmx_constraint_data* c, const ConstraintState& prev);

// mmx_problem_set_instance_parents: what the last accepted call left ...
struct InstanceParentsState {
  bool instPos, instOri; // per-instance lists are set
  const std::vector<int32_t>& unionPos;
  const std::vector<int32_t>& unionOri;
  bool listsFromHost; // posLists / oriLists are what the caller passed (host memory)
  const std::vector<int32_t>& posLists;
  const std::vector<int32_t>& oriLists;
  bool tablesDirty;
};
// ... and the refusal, or the joints that carry a position / orientation constraint in some element and what they mean for the
// tables: the integer bookkeeping (solve list, structurally zero columns) depends on the UNION of the batch's parents only, so
// new lists over the same joints need no rebuild -- the kernels read the lists themselves.
struct InstanceParentsIntake {
  int32_t code = MMX_OK;
  const char* message = nullptr;
  bool unchanged = false; // host lists equal to the last call's: nothing to do at all
  std::vector<int32_t> unionPos, unionOri; // ascending
  bool sameTables = false; // the derived tables can stay
};
// pos / ori: the host view of the [B][Kp] / [B][Ko] lists, empty when the caller passed none
InstanceParentsIntake intakeInstanceParents(
    int32_t numJoints, const std::vector<int32_t>& pos, const std::vector<int32_t>& ori, bool fromHost, const InstanceParentsState& prev);

#pragma GCC visibility pop
} // namespace mmx
